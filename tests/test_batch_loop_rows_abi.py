"""midas_loop_step_batch_rows and midas_loop_row_params on a machine without a GPU: the header, the library's exports and the ctypes
table agree on the entry point, the header's record, its ctypes mirror and the numpy dtype the engine fills agree on the layout, the
header cites the reference lines every field stands for, and the engine's host side - the squared threshold, the table, the
refusals that need no device - is what the header says."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "midas_loop_step_batch_rows"
CTYPES = {"float": C.c_float, "double": C.c_double, "int32_t": C.c_int32}


def _header():
    return open(os.path.join(REPO, "include", "midas_hip.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def test_entry_declared_bound_and_exported():
    from midastouch_amd import _lib
    code = _code()
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % ENTRY, code)
    assert decl, ENTRY
    params = " ".join(decl.group(1).split())
    # midas_loop_step_batch_objects' parameters with the table behind the argument record
    objects = " ".join(re.search(r"\bint\s+midas_loop_step_batch_objects\s*\(([^)]*)\)\s*;", code).group(1).split())
    assert params == objects.replace("args, ", "args, const midas_loop_row_params* rows_dev, ")
    res, args = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == len(params.split(",")) == 8
    assert args == [C.c_void_p, C.c_void_p, C.POINTER(_lib.LoopArgs), C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    path = _lib.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert ENTRY in {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert hasattr(_lib.load(), ENTRY)


def test_record_layout():
    """Field for field: the header's struct, _lib.LoopRowParams and _lib.LOOP_ROW_PARAMS_DTYPE - names, types, offsets, 40 bytes."""
    from midastouch_amd import _lib
    body = re.search(r"typedef struct midas_loop_row_params \{(.*?)\} midas_loop_row_params;", _code(), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), CTYPES[ty]) for n in names.split(",")]
    assert fields == [(n, t) for n, t in _lib.LoopRowParams._fields_]
    assert [n for n, _ in fields] == ["std_t", "std_r", "prune_thr", "prune_t2", "floor", "softmax", "unit_weights", "pad_"]
    dt = np.dtype(_lib.LOOP_ROW_PARAMS_DTYPE)
    assert dt.itemsize == C.sizeof(_lib.LoopRowParams) == 40 and C.alignment(_lib.LoopRowParams) == 8
    for name, ty in fields:
        assert dt.fields[name][1] == getattr(_lib.LoopRowParams, name).offset, name
        assert dt.fields[name][0].itemsize == C.sizeof(ty) and dt.fields[name][0].kind == ("f" if ty in (C.c_float, C.c_double) else "i")
    # midas_loop_args keeps its layout: the record is beside it, not in it
    args = re.search(r"typedef struct midas_loop_args \{(.*?)\} midas_loop_args;", _code(), re.S).group(1)
    assert "row" not in args and args.strip().endswith("dbscan_batched;")


def test_header_cites_the_reference():
    text = _header()
    start = text.index("typedef struct midas_loop_row_params {")
    comment = text[text.rindex("/*", 0, start):start]
    for cite in ("particle_filter.py:326-335", ":379-403", ":405-447", ":449-469", "filter_real.py:205-212"):
        assert cite in comment, cite
    decl = re.search(r"\bint\s+%s\s*\(" % ENTRY, text).start()
    entry = text[text.rindex("/*", 0, decl):decl]
    assert "bash/run_filter.sh" in entry and "ycb.yaml" in entry and "mcmaster.yaml" in entry and "filter_real.py" in entry


def test_squared_threshold_on_the_host():
    """batch_loop_engine.squared_threshold is csrc/midas_internal.hpp's (restated once more by tests/_recipes.py)."""
    from _recipes import PE_DEGENERATE, PE_ULP_THRS, pe_squared_threshold
    from midastouch_amd.batch_loop_engine import squared_threshold
    rng = np.random.default_rng(3)
    thrs = list(PE_ULP_THRS) + [131 * 2.0 ** -16, 113 * 2.0 ** -16, 1e-300, 1e150, 5e-324] + list(10.0 ** rng.uniform(-6, 1, 500))
    for thr in thrs:
        t2 = squared_threshold(thr)
        assert t2 == pe_squared_threshold(thr), thr
        assert np.sqrt(t2) <= thr < np.sqrt(np.nextafter(t2, np.inf)), thr
    for thr in PE_DEGENERATE:
        got, want = squared_threshold(thr), pe_squared_threshold(thr)
        assert got == want and type(got) is float, thr
    assert squared_threshold(float("nan")) == -1.0 and squared_threshold(-0.5) == -1.0 and squared_threshold(float("inf")) == float("inf")


def test_table_from_columns():
    from midastouch_amd import _lib
    from midastouch_amd.batch_loop_engine import row_params_table, squared_threshold
    std_t = (2.0 * np.asarray([2e-4, 1e-4, 3e-4])).astype(np.float32)
    tab = row_params_table(3, std_t, np.float32(0.5), [0.002, float("inf"), float("nan")], [1000, 1500, 1], [True, False, True], False)
    assert tab.dtype.itemsize == 40 and tab.shape == (3,)
    assert tab["std_t"].tolist() == [float(np.float32(2.0 * s)) for s in (2e-4, 1e-4, 3e-4)]  # float32(mul * sig), the product in float64
    assert tab["std_r"].tolist() == [0.5] * 3 and tab["floor"].tolist() == [1000, 1500, 1]
    assert tab["softmax"].tolist() == [1, 0, 1] and tab["unit_weights"].tolist() == [0, 0, 0] and tab["pad_"].tolist() == [0, 0, 0]
    assert tab["prune_t2"][0] == squared_threshold(0.002) and tab["prune_t2"][1] == np.inf and tab["prune_t2"][2] == -1.0
    assert np.isnan(tab["prune_thr"][2])
    rec = _lib.LoopRowParams.from_buffer_copy(tab.tobytes()[40:80])  # row 1 as the C side reads it
    assert (rec.std_t, rec.floor, rec.softmax, rec.prune_t2) == (tab["std_t"][1], 1500, 0, float("inf"))
    units = row_params_table(2, np.float32(0), np.float32(0), 0.002, 500, True, [True, False])
    assert units["unit_weights"].tolist() == [1, 0] and units["softmax"].tolist() == [1, 1]


def test_row_values_and_refusals_without_a_device():
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    from midastouch_amd.batch_loop_engine import ROW_PARAMS, row_values
    assert ROW_PARAMS == ("sig_t", "sig_r", "pen_max", "floor", "softmax")
    assert row_values("sig_t", 2e-4, 3) == (2e-4, None) and row_values("floor", [1, 2, 3], 3) == (None, [1, 2, 3])
    assert row_values("sig_r", np.asarray([0.5, 0.25]), 2) == (None, [0.5, 0.25]) and row_values("softmax", (1, 0), 2) == (None, [True, False])
    assert row_values("pen_max", [float("inf"), -1.0], 2)[1] == [float("inf"), -1.0]  # a threshold is taken as it stands
    assert row_values("sig_t", 0.0, 4) == (0.0, None)
    for name, bad, B in (("sig_t", [1e-4], 2), ("sig_t", -1e-9, 2), ("sig_r", [0.5, float("nan")], 2), ("floor", 0, 2), ("floor", [5, 0], 2),
                         ("unit_weights", [True], 2), ("softmax", [], 1), ("floor", [1, 2, 3], 2), ("sig_t", "much", 1)):
        with pytest.raises(MidasError):
            row_values(name, bad, B)
    # the constructors refuse before a context is asked for
    obj = lambda K, D: (np.tile(np.eye(4, dtype=np.float32), (K, 1, 1)), np.ones((K, D), dtype=np.float32), np.zeros((8, 3)))  # noqa: E731
    assert row_values("sig_t", torch.tensor(3e-4, dtype=torch.float64), 2) == (3e-4, None) and row_values("floor", np.int64(7), 2) == (7, None)
    for bad in (dict(sig_t=[1e-4]), dict(floor=[100, 0]), dict(sig_r=[-0.5, 0.5]), dict(softmax=[True, True, False]), dict(floor=0),
                dict(sig_t=np.float64(-1.0)), dict(sig_r=torch.tensor(float("nan")))):
        with pytest.raises(MidasError):
            BatchLoopEngine.for_objects([obj(4, 128)], [0, 0], 100, **bad)
        with pytest.raises(MidasError):
            BatchLoopEngine(*obj(4, 128), 2, 100, **bad)
    # step() takes a bool or B bools; the other per-frame values stay shared
    p = inspect.signature(BatchLoopEngine.step).parameters
    assert p["unit_weights"].default is False and "std_override" not in p and "set_row_params" in dir(BatchLoopEngine)
