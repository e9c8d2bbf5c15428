"""midastouch_amd - MI355X-native particle-filter hot path of MidasTouch (gfx950 HIP kernels behind a C ABI)."""
__version__ = "0.1.0"


def __getattr__(name):  # the engines import torch: on first use, not with the package
    if name == "BatchLoopEngine":
        from .batch_loop_engine import BatchLoopEngine
        return BatchLoopEngine
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
