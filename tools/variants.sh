#!/bin/bash
# Build tuning variants of libmidas_hip.so:  tools/variants.sh name "-DMIDAS_NN_BATCH=16 ..." [name flags]...
# Outputs midastouch_amd/csrc/build/variants/<name>.so ; run one with MIDAS_HIP_LIB=<path>.
# VFILES="front front_folded" restricts the flags (and the recompilation) to the named translation units: the others are
# taken from the regular build.  The units and the link line are the Makefile's (its BUILD, LIB, EXTRA, EXTRA_UNITS).
set -e
cd "$(dirname "$0")/../midastouch_amd/csrc"
make -s -j"${JOBS:-16}"
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  dir=build/variants/$name
  rm -rf "$dir"  # (a name built before with other flags: its objects would count as up to date)
  mkdir -p "$dir"
  if [ -n "$VFILES" ]; then
    cp -p build/*.o "$dir"/
    for f in $VFILES; do rm -f "$dir/$f.o"; done
    make -s -j"${JOBS:-16}" BUILD="$dir" LIB="$dir.so" EXTRA="$flags" EXTRA_UNITS="$VFILES"
  else
    make -s -j"${JOBS:-16}" BUILD="$dir" LIB="$dir.so" EXTRA="$flags"
  fi
  echo built "$name"
done
