"""The per-frame pose estimate's surface, checked without a device: `midas_estimate_args` in include/midas_hip.h and its ctypes
mirror, the two new entries in the binding table and in the built library, the engines' `estimate` keyword."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_fields(cname):
    """Field names of a struct of include/midas_hip.h in declaration order (the parsing of test_abi.test_args_structs_match_header)."""
    text = open(os.path.join(REPO, "include", "midas_hip.h")).read()
    body = text[text.index("typedef struct %s {" % cname):text.index("} %s;" % cname)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.replace("*", " ").split(",")
        fields.append(names[0].split()[-1])
        fields.extend(n.strip() for n in names[1:])
    return fields


def test_estimate_args_mirror_follows_header():
    from midastouch_amd import _lib
    fields = _header_fields("midas_estimate_args")
    assert fields[:2] == ["N", "B"] and "tables_dev" in fields and "weights_dev" in fields
    assert [f.replace("_dev", "") for f in fields] == [f[0] for f in _lib.EstimateArgs._fields_]
    # the layout a C compiler gives the header's struct: int64, int32 (+4 pad), four pointers, int32 (+4 pad), two pointers
    assert ctypes.sizeof(_lib.EstimateArgs) == 8 + 8 + 4 * 8 + 8 + 2 * 8
    assert _lib.EstimateArgs.poses_prop.offset == 16 and _lib.EstimateArgs.softmax.offset == 48 and _lib.EstimateArgs.centers.offset == 56


def test_estimate_entries_bound_and_exported():
    from midastouch_amd import _lib
    path = _lib.build()
    lib = ctypes.CDLL(path)
    for name in ("midas_pose_estimate", "midas_lazy_run_estimate"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), f"{name} not exported by {path}"
    res, args = _lib.SIGNATURES["midas_pose_estimate"]
    assert res is ctypes.c_int and len(args) == 2 and args[1]._type_ is _lib.EstimateArgs
    # midas_lazy_run's arguments followed by the two estimate logs
    run, est = _lib.SIGNATURES["midas_lazy_run"][1], _lib.SIGNATURES["midas_lazy_run_estimate"][1]
    assert est[:len(run)] == run and len(est) == len(run) + 2
    text = open(os.path.join(REPO, "include", "midas_hip.h")).read()
    assert re.search(r"int\s+midas_pose_estimate\s*\(\s*midas_ctx\s*\*\s*ctx\s*,\s*const\s+midas_estimate_args\s*\*", text)
    assert re.search(r"int\s+midas_lazy_run_estimate\s*\(", text)


def test_engines_take_the_estimate_keyword():
    from midastouch_amd import engine, ops
    for name in ("FilterEngine", "PipelinedFilterEngine", "BatchFilterEngine", "PipelinedBatchFilterEngine"):
        cls = getattr(engine, name)
        init = next(c.__dict__["__init__"] for c in cls.__mro__ if "__init__" in c.__dict__ and
                    "estimate" in inspect.signature(c.__dict__["__init__"]).parameters)
        p = inspect.signature(init).parameters["estimate"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, name
        assert isinstance(inspect.getattr_static(cls, "estimate"), property), name
    assert "estimate" not in inspect.signature(engine.PipelinedFilterEngine.run).parameters  # (run()'s call does not change)
    assert list(inspect.signature(ops.pose_estimate).parameters) == ["poses_prop", "weights"]
