"""midas_dbscan_batch and the batch engines' `batched_dbscan` switch, as far as a machine without a GPU can check them: the bound in
the header and in `_lib`, the entry declared, bound and exported, the field at the end of midas_loop_args, the refusals that need no
device - and that the clouds of tests/test_gpu_dbscan_batch.py have the properties its cases rely on (the oracle's cluster counts,
the cells per axis that decide between a dense and a hashed row)."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "midas_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_bound_in_header_and_lib():
    from midastouch_amd import _lib
    m = re.search(r"#define\s+MIDAS_DBSCAN_BATCH_MAX_POINTS\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.DBSCAN_BATCH_MAX_POINTS == 1 << 20


def test_entry_declared_bound_and_exported():
    from midastouch_amd import _lib
    m = re.search(r"int\s+midas_dbscan_batch\s*\(([^;]*)\)\s*;", _header())
    assert m, "midas_dbscan_batch is not declared in include/midas_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 11 and params[0].startswith("midas_ctx*") and params[-1] == "int32_t max_clusters"
    res, args = _lib.SIGNATURES["midas_dbscan_batch"]
    assert len(args) == len(params)
    lib = _lib.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT midas_dbscan_batch\b", out), "libmidas_hip.so does not export midas_dbscan_batch"


def test_loop_args_field_is_last():
    from midastouch_amd import _lib
    body = re.search(r"typedef struct midas_loop_args \{(.*?)\} midas_loop_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields[-1] == "dbscan_batched" and _lib.LoopArgs._fields_[-1][0] == "dbscan_batched"
    assert _lib.LoopArgs().dbscan_batched == 0  # a zero-initialised caller keeps the serial passes


def test_engine_refuses_batched_beyond_the_bound_before_any_device_work():
    """65 x 16 384 > 2^20 with batched_dbscan=True: MidasError from the constructor's checks, in front of the context (this machine
    has none to give) - with None codebook arguments nothing else could have raised it."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    with pytest.raises(MidasError, match="DBSCAN_BATCH_MAX_POINTS"):
        BatchLoopEngine(None, None, None, 65, 16384, batched_dbscan=True)
    with pytest.raises(MidasError, match="DBSCAN_BATCH_MAX_POINTS"):
        BatchLoopEngine(None, None, None, 9, 131072, wide=True, batched_dbscan=True)


def test_ops_entry_refuses_beyond_the_bound_without_a_device():
    torch = pytest.importorskip("torch")
    from midastouch_amd import ops
    from midastouch_amd._lib import MidasError
    assert callable(ops.dbscan_batch)
    with pytest.raises(MidasError, match="DBSCAN_BATCH_MAX_POINTS"):
        ops.dbscan_batch(torch.zeros((1, 1, 4, 4)).expand(2, (1 << 19) + 1, 4, 4))  # (a view: no memory behind the shape)
    with pytest.raises(MidasError, match=r"\(B,N,4,4\)"):
        ops.dbscan_batch(torch.zeros((8, 4, 4)))


def test_clouds_of_the_gpu_cases(oracle):
    """What tests/test_gpu_dbscan_batch.py states about its clouds, by the oracle on the CPU."""
    import test_gpu_dbscan_batch as T
    _, a, b = T.isolation_clouds()
    assert oracle.dbscan(a, T.EPS, 200)[1] == 0
    twice, ncl = oracle.dbscan(np.concatenate([a, a]), T.EPS, 200)
    assert ncl == 1 and (twice == 0).sum() == 380
    lab, ncl = oracle.dbscan(b, T.EPS, 200)
    assert ncl == 1 and (lab == 0).sum() == 210
    assert [oracle.dbscan(x, T.EPS, 5)[1] for x in T.many_cluster_rows()] == [80, 1, 3]
    for last, want in (("dense", [32, 32, 32]), ("hashed", [33, 32, 32])):
        rows = T.boundary_rows(last)
        assert T.cells_per_axis(rows[63]).tolist() == want
        assert T.cells_per_axis(rows[2]).tolist() == [36, 36, 36] and len(np.unique(np.floor(rows[2] / T.H), axis=0)) == 512
        assert all(len(x) <= 512 for x in rows)
