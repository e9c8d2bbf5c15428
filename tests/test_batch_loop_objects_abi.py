"""midas_object_set_create / _destroy and midas_loop_step_batch_objects on a machine without a GPU: the three entries are in the
header, in the ctypes table and among the library's exports, and BatchLoopEngine.for_objects refuses what it can before any
device work."""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("midas_object_set_create", "midas_object_set_destroy", "midas_loop_step_batch_objects")


def _header():
    return open(os.path.join(REPO, "include", "midas_hip.h")).read()


def test_entries_declared_bound_and_exported():
    from midastouch_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decls = {n: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, code) for n in ENTRIES}
    assert all(decls.values()), decls
    # one ctypes argument per declared parameter
    for n, m in decls.items():
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[n][1]), n
    # the step entry: the set in place of the codebook and the trees, then midas_loop_step_batch's arguments and the regime flag
    step = " ".join(decls["midas_loop_step_batch_objects"].group(1).split())
    small = " ".join(re.search(r"\bint\s+midas_loop_step_batch\s*\(([^)]*)\)\s*;", code).group(1).split())
    assert step == "midas_ctx* ctx, const midas_object_set* set, " + small.split("tree3, ", 1)[1] + ", int32_t wide"
    path = _lib.build()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    lib = _lib.load()
    for n in ENTRIES:
        assert n in exported and hasattr(lib, n), n


def test_entries_cite_the_reference():
    """Every entry's comment names the reference call site, as the header's other entries do."""
    text = _header()
    for n in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(" % n, text).start()
        comment = text[text.rindex("/*", 0, decl):decl]
        assert "bash/run_filter.sh" in comment and "filter/filter.py:82,89-93" in comment, n


def test_for_objects_refuses_before_any_device_work():
    """An empty object list, a row index out of range and codebooks of different D: MidasError with and without a GPU - nothing
    is built for the objects that were fine."""
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd._lib import MidasError
    obj = lambda K, D: (np.tile(np.eye(4, dtype=np.float32), (K, 1, 1)), np.ones((K, D), dtype=np.float32), np.zeros((8, 3)))  # noqa: E731
    with pytest.raises(MidasError, match="at least one object"):
        BatchLoopEngine.for_objects([], [0], 100)
    with pytest.raises(MidasError, match="at least one row"):
        BatchLoopEngine.for_objects([obj(4, 128)], [], 100)
    for rows in ([0, 2], [-1], [1, 0, 5]):
        with pytest.raises(MidasError, match="object index"):
            BatchLoopEngine.for_objects([obj(4, 128), obj(5, 128)], rows, 100)
    with pytest.raises(MidasError, match="one D"):
        BatchLoopEngine.for_objects([obj(4, 128), obj(5, 256)], [0, 1], 100)
    # the constructor's own bounds and keywords hold here too
    with pytest.raises(MidasError, match="larger sets: LoopEngine"):
        BatchLoopEngine.for_objects([obj(4, 128)], [0], 16385)
    with pytest.raises(MidasError, match="wide"):
        BatchLoopEngine.for_objects([obj(4, 128)], [0], 131073, wide=True)
    with pytest.raises(MidasError, match="for_objects"):
        BatchLoopEngine.for_objects([obj(4, 128)], [0], 100, no_such_keyword=1)


def test_for_objects_keywords_are_the_constructors():
    """for_objects takes the constructor's keywords with the constructor's defaults: the table it fills **kw from is __init__'s
    signature, and both go through the one initialiser."""
    import inspect
    from midastouch_amd.batch_loop_engine import DEFAULTS, BatchLoopEngine
    sig = inspect.signature(BatchLoopEngine.__init__)
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == DEFAULTS
    init = inspect.signature(BatchLoopEngine._init)
    assert {k for k, p in init.parameters.items() if p.kind is p.KEYWORD_ONLY} == set(DEFAULTS)
