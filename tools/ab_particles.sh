#!/bin/bash
# A/B builds of the particle kernels only - the units particles.hip was cut into; the other objects are reused:
# tools/ab_particles.sh name "-DFLAGS" [name flags]... (CPU box: build;
# GPU box: MIDAS_HIP_LIB=midastouch_amd/csrc/build/variants/<name>.so python tools/bench_c5.py)
VFILES="particles tree front front_folded front_batch" exec "$(dirname "$0")/variants.sh" "$@"
