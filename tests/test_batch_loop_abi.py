"""The batch loop's surface, checked without a device: `midas_loop_step_batch` and the capacity constant in include/midas_hip.h,
the entry in the binding table and in the built library with matching argument types, `midastouch_amd.BatchLoopEngine`."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type (whitespace removed) -> ctypes type of the binding table
CTYPES = {"midas_ctx*": ctypes.c_void_p, "constmidas_codebook*": ctypes.c_void_p, "constmidas_tree*": ctypes.c_void_p,
          "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


def _header():
    return open(os.path.join(REPO, "include", "midas_hip.h")).read()


def _declared_params(name):
    """[(type, name)] of a function's parameters as the header declares them (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/midas_hip.h"
    out = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        ty, nm = re.match(r"(.*?)(\w+)$", p).groups()
        out.append((ty.replace(" ", ""), nm))
    return out


def test_header_declares_the_batch_entry_and_its_capacity():
    from midastouch_amd import _lib
    params = _declared_params("midas_loop_step_batch")
    single = _declared_params("midas_loop_step")
    # midas_loop_step's arguments, then the batch size and the stride between two trajectories' log rows
    assert params[:len(single)] == single
    assert params[len(single):] == [("int32_t", "B"), ("int64_t", "log_stride")]
    m = re.search(r"^#define\s+MIDAS_LOOP_BATCH_MAX_CAP\s+(\d+)\s*$", _header(), flags=re.M)
    assert m, "MIDAS_LOOP_BATCH_MAX_CAP is not defined in include/midas_hip.h"
    assert int(m.group(1)) == 16384 == _lib.LOOP_BATCH_MAX_CAP
    # documented in the style of the other entries: the reference's call sites and the regime
    doc = _header()[:_header().index("#define MIDAS_LOOP_BATCH_MAX_CAP")].rsplit("/*", 1)[1]
    for word in ("filter/filter.py:150-190", "particle_filter.py", "grid.y", "seed + b", "MIDAS_ERR_INVALID", "score_stamps_dev"):
        assert word in doc, word


def test_binding_matches_the_declaration_and_the_library():
    from midastouch_amd import _lib
    assert "midas_loop_step_batch" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["midas_loop_step_batch"]
    assert res is ctypes.c_int
    params = _declared_params("midas_loop_step_batch")
    assert len(args) == len(params)
    for (ty, nm), got in zip(params, args):
        if ty == "constmidas_loop_args*":
            assert got._type_ is _lib.LoopArgs, nm
        else:
            assert got is CTYPES[ty], (nm, ty, got)
    single = _lib.SIGNATURES["midas_loop_step"][1]
    assert args[:len(single)] == single
    lib = ctypes.CDLL(_lib.build())
    assert hasattr(lib, "midas_loop_step_batch")


def test_batch_loop_engine_is_importable():
    import midastouch_amd
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    assert midastouch_amd.BatchLoopEngine is BatchLoopEngine
    sig = inspect.signature(BatchLoopEngine.__init__).parameters
    assert list(sig)[1:6] == ["cb_poses", "cb_embeddings", "mesh_vertices", "batch", "num_particles"]
    single = inspect.signature(LoopEngine.__init__).parameters
    for kw in ("sig_t", "sig_r", "pen_max", "seed", "softmax", "resample", "floor", "eps", "cluster", "cluster_every", "log_frames", "device"):
        assert sig[kw].kind is inspect.Parameter.KEYWORD_ONLY and sig[kw].default == single[kw].default, kw
    assert "topk_ties" not in sig  # (the ATen tie rule stays with LoopEngine)
    step = inspect.signature(BatchLoopEngine.step).parameters
    assert list(step)[1:] == ["odoms", "codes", "gts", "u32", "multiplier", "dbscan", "unit_weights"]
    for name in ("set_particles", "project_to_codebook", "read_log", "frame_view"):
        assert callable(getattr(BatchLoopEngine, name)), name
    assert isinstance(inspect.getattr_static(BatchLoopEngine, "n"), property)
