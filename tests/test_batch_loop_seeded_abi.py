"""The seeded batch loop's surface, checked without a device: `midas_mt19937_draws_counted_batch` and `midas_loop_step_batch_draws`
in include/midas_hip.h, in the binding table with matching argument types and in the built library; BatchLoopEngine's new methods
beside a step() whose parameters stay what they were."""
import ctypes
import inspect

from test_batch_loop_abi import CTYPES, _declared_params, _header

TYPES = dict(CTYPES, **{"uint32_t*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "constfloat*": ctypes.c_void_p,
                        "constmidas_mt_counted_segment*": ctypes.c_void_p})


def _check_binding(name):
    from midastouch_amd import _lib
    assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int
    params = _declared_params(name)
    assert len(args) == len(params)
    for (ty, nm), got in zip(params, args):
        if ty == "constmidas_loop_args*":
            assert got._type_ is _lib.LoopArgs, nm
        else:
            assert got is TYPES[ty], (name, nm, ty, got)
    assert hasattr(ctypes.CDLL(_lib.build()), name)
    return params


def test_counted_batch_entry():
    params = _check_binding("midas_mt19937_draws_counted_batch")
    assert [nm for _, nm in params] == ["ctx", "B", "states_dev", "skip_words", "nseg", "segs", "count_stride", "radius_dev", "cos_dev",
                                        "sin_dev", "status_dev", "status_stride"]
    doc = _header()[:_header().index("int midas_mt19937_draws_counted_batch")].rsplit("/*", 1)[1]
    for word in ("particle_filter.py:326-335", ":245", "count_stride", "status_stride", "grid.y", "B = 1"):
        assert word in doc, word


def test_batch_draws_entry():
    from midastouch_amd import _lib
    params = _check_binding("midas_loop_step_batch_draws")
    assert params == _declared_params("midas_loop_step_batch")
    assert _lib.SIGNATURES["midas_loop_step_batch_draws"] == _lib.SIGNATURES["midas_loop_step_batch"]
    doc = _header()[:_header().index("int midas_loop_step_batch_draws")].rsplit("/*", 1)[1]
    for word in ("particle_filter.py:326-335", ":245", ":433-441", "tn_dev", "rot_dev", "u_dev", "MIDAS_TOPK_TIES_ATEN_CPU",
                 "MIDAS_ERR_INVALID", "RESAMPLE"):
        assert word in doc, word


def test_engine_surface():
    from midastouch_amd import BatchLoopEngine
    from midastouch_amd.loop_engine import LoopEngine
    from midastouch_amd.torch_rng import TorchCpuStreams
    assert list(inspect.signature(BatchLoopEngine.seed_torch_streams).parameters) == ["self", "seeds"]
    assert list(inspect.signature(BatchLoopEngine.set_annealing_state).parameters) == ["self", "particle_vars", "init_particles"]
    assert list(inspect.signature(LoopEngine.set_annealing_state).parameters) == ["self", "particle_var", "init_particles"]
    sp = inspect.signature(BatchLoopEngine.set_particles).parameters
    assert list(sp) == ["self", "poses", "labels", "reset_annealing"] and sp["reset_annealing"].default is True
    step = inspect.signature(BatchLoopEngine.step).parameters
    assert list(step)[1:] == ["odoms", "codes", "gts", "u32", "multiplier", "dbscan", "unit_weights"]
    assert "topk_ties" not in inspect.signature(BatchLoopEngine.__init__).parameters
    assert isinstance(inspect.getattr_static(BatchLoopEngine, "topk_ties"), property)
    assert list(inspect.signature(TorchCpuStreams.draws_counted_async).parameters) == ["self", "spec", "outs", "status"]
    assert callable(TorchCpuStreams.counted_scratch_bytes)
