"""midas_loop_step_batch_wide on a machine without a GPU: the capacity the header states is the one the Python side holds, and
the entry is in the header, in the ctypes table and among the library's exports."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(REPO, "include", "midas_hip.h")).read()


def test_wide_capacity_matches_header():
    from midastouch_amd import _lib
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MIDAS_LOOP_BATCH\w*MAX_CAP) (\d+)", _header())}
    assert defines == {"MIDAS_LOOP_BATCH_MAX_CAP": _lib.LOOP_BATCH_MAX_CAP, "MIDAS_LOOP_BATCH_WIDE_MAX_CAP": _lib.LOOP_BATCH_WIDE_MAX_CAP}
    assert _lib.LOOP_BATCH_WIDE_MAX_CAP == 131072 == 32 * 4096  # 32 summation blocks: the reference's 50 000, the headline's 100 000
    assert _lib.LOOP_BATCH_MAX_CAP == 16384  # the small entries keep theirs


def test_wide_entry_declared_bound_and_exported():
    from midastouch_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+midas_loop_step_batch_wide\s*\(([^)]*)\)\s*;", code)
    small = re.search(r"\bint\s+midas_loop_step_batch\s*\(([^)]*)\)\s*;", code)
    assert decl and small and " ".join(decl.group(1).split()) == " ".join(small.group(1).split())  # midas_loop_step_batch's arguments
    assert _lib.SIGNATURES["midas_loop_step_batch_wide"] == _lib.SIGNATURES["midas_loop_step_batch"]
    path = _lib.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert "midas_loop_step_batch_wide" in {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert hasattr(_lib.load(), "midas_loop_step_batch_wide")


def test_wide_engine_refuses_before_any_device_work():
    """The constructor's bounds are checked before a context is asked for: the same errors with and without a GPU."""
    import pytest
    from midastouch_amd import BatchLoopEngine, _lib
    for B, cap in ((1, _lib.LOOP_BATCH_WIDE_MAX_CAP + 1), (129, _lib.LOOP_BATCH_WIDE_MAX_CAP), (1, 0)):
        with pytest.raises(_lib.MidasError, match="wide"):
            BatchLoopEngine(None, None, None, B, cap, wide=True)
    with pytest.raises(_lib.MidasError, match="larger sets: LoopEngine"):
        BatchLoopEngine(None, None, None, 1, _lib.LOOP_BATCH_MAX_CAP + 1)
