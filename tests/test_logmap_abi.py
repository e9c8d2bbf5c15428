"""The log-map cluster centres' C ABI on a machine without a GPU: midas_se3_log, midas_cluster_centers_logmap and the phase bit
MIDAS_LOOP_CENTERS_LOGMAP in the header, in the library's exports and in the ctypes table - in step in both directions - and the
host side of the keyword (`centers=`, `method=`)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "midas_hip.h")).read(), flags=re.S)


def _params(name):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _code())
    assert decl, name
    return [" ".join(p.split()) for p in decl.group(1).split(",")]


def test_entries_declared_bound_and_exported():
    from midastouch_amd import _lib
    # midas_cluster_centers' parameters, one for one
    assert _params("midas_cluster_centers_logmap") == _params("midas_cluster_centers")
    assert _lib.SIGNATURES["midas_cluster_centers_logmap"] == _lib.SIGNATURES["midas_cluster_centers"]
    assert _params("midas_se3_log") == ["midas_ctx* ctx", "int64_t N", "const float* poses_dev", "double* xi_dev"]
    assert _lib.SIGNATURES["midas_se3_log"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p])
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.build()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    lib = _lib.load()
    for entry in ("midas_se3_log", "midas_cluster_centers_logmap"):
        assert entry in exported and hasattr(lib, entry), entry


def test_header_and_ctypes_table_in_step():
    """Every function the header declares has a ctypes signature of as many parameters, and the table names nothing else."""
    from midastouch_amd import _lib
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(midas_\w+)\s*\(([^)]*)\)\s*;", _code())}
    new = lambda n: "logmap" in n or "se3_log" in n
    in_header, in_table = {n for n in declared if new(n)}, {n for n in _lib.SIGNATURES if new(n)}
    assert in_header == in_table == {"midas_se3_log", "midas_cluster_centers_logmap"}
    for name in in_table:
        assert len(_lib.SIGNATURES[name][1]) == declared[name], name


def test_phase_bit():
    from midastouch_amd import _lib, loop_engine
    m = re.search(r"#define\s+MIDAS_LOOP_CENTERS_LOGMAP\s+(\d+)", _code())
    assert m and int(m.group(1)) == _lib.LOOP_CENTERS_LOGMAP == 16
    phases = [_lib.LOOP_FRONT, _lib.LOOP_DBSCAN, _lib.LOOP_ANNEAL, _lib.LOOP_RESAMPLE, _lib.LOOP_CENTERS_LOGMAP]
    assert sorted(phases) == [1, 2, 4, 8, 16]
    assert loop_engine.ALL_PHASES == 15  # the bit is a form, not a phase
    assert loop_engine.CENTER_FORMS == {"quat_avg": 0, "logmap": 16}
    # the records the loop entries take do not change with it (their sizes are pinned elsewhere)
    assert "centers" not in {f for f, _ in _lib.LoopArgs._fields_} and "centers" not in {f for f, _ in _lib.LoopRowParams._fields_}


def test_phase_mask_carries_the_form_with_anneal_only():
    from types import SimpleNamespace

    from midastouch_amd import _lib
    from midastouch_amd.loop_engine import ALL_PHASES, _LoopBase
    for centers, bit in (("quat_avg", 0), ("logmap", 16)):
        eng = SimpleNamespace(cluster=True, cluster_every=50, step_count=0, centers=centers)
        assert _LoopBase._phase_mask(eng, ALL_PHASES, None) == 15 | bit
        assert _LoopBase._phase_mask(eng, ALL_PHASES, False) == 13 | bit
        assert _LoopBase._phase_mask(eng, _lib.LOOP_FRONT | _lib.LOOP_DBSCAN, None) == 3
        assert _LoopBase._phase_mask(eng, _lib.LOOP_RESAMPLE, None) == 8
        eng.cluster = False
        assert _LoopBase._phase_mask(eng, ALL_PHASES, None) == 9


def test_keywords_on_the_host():
    from midastouch_amd import filter as flt
    from midastouch_amd import ops
    from midastouch_amd._lib import MidasError
    from midastouch_amd.batch_loop_engine import DEFAULTS, BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    for fn in (LoopEngine.__init__, BatchLoopEngine.__init__, flt.filter, flt.filter_sweep):
        assert inspect.signature(fn).parameters["centers"].default == "quat_avg", fn
    assert DEFAULTS["centers"] == "quat_avg"
    assert inspect.signature(ops.cluster_centers).parameters["method"].default == "quat_avg"
    assert set(ops.CLUSTER_CENTER_ENTRIES) == {"quat_avg", "logmap"}
    # an unknown value raises before anything touches a device
    with pytest.raises(MidasError, match="centers"):
        LoopEngine(None, None, None, 100, centers="mean")
    with pytest.raises(MidasError, match="centers"):
        BatchLoopEngine(None, None, None, 2, 100, centers="mean")
    with pytest.raises(MidasError, match="method"):
        ops.cluster_centers(torch.zeros(1, 4, 4), torch.ones(1), torch.zeros(1), torch.zeros(1), method="mean")
