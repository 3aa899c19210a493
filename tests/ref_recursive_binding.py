"""ctypes binding of tests/ref_recursive/libref_recursive.so (TEST INFRASTRUCTURE).

The CPU checker for rt_settings::integrator 1 and 2 (Whitted, Ground Truth Recursive), which the oracle and
tests/ref_integrators refuse: a unity build over oracle/oracle.c plus restatements of RT/integrators.cpp:310-483
as plain C recursion.  Only tests/ loads it.  A plain shared object: nothing else is loaded with it.
"""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_recursive", "libref_recursive.so")

_lib = None


def _abi():
    import importlib
    import sys
    if "buas_pathtracer_amd" in sys.modules:
        return sys.modules["buas_pathtracer_amd"].abi
    return importlib.import_module("buas_pathtracer_amd").abi


def load():
    global _lib
    if _lib is not None:
        return _lib
    abi = _abi()
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_recursive (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fns = {
        "rr_render": (C.c_int, [P(abi.SceneDesc), P(abi.Camera), P(abi.Settings), P(abi.FilterCache),
                                P(abi.TileSet), P(abi.V3), C.c_uint32, C.c_uint32, P(abi.AccumulationBuffer),
                                P(abi.Stats)]),
        "rr_trace_samples": (C.c_int, [P(abi.SceneDesc), P(abi.Camera), P(abi.Settings), P(abi.V3), C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_float),
                                       P(abi.Stats)]),
        "rr_set_math_mode": (None, [C.c_int]),
    }
    for name, (res, args) in fns.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


def _ambient(ambient):
    if ambient is None:
        return None
    return C.byref(_abi().V3(*[float(c) for c in ambient]))


def render(desc, cam, st, fc, w, h, ambient=None, tile=64, shard_index=0, shard_count=1, frame_count=0,
           total_frame_index=0, accum=None, threads=1):
    """rr_render: one frame, RT_RNG_PER_SAMPLE, tiles total-1 .. 0 -> (accum, stats).  threads=1 is the
    reference's single-threaded splat order; more threads are for timing runs only."""
    import numpy as np
    abi = _abi()
    lib = load()
    if accum is None:
        accum = np.zeros((h, w, 4), np.float32)
    buf = abi.AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
    tiles = abi.TileSet(tile, tile, shard_index, shard_count)
    stats = abi.Stats()
    err = lib.rr_render(C.byref(desc), C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), _ambient(ambient),
                        total_frame_index, threads, C.byref(buf), C.byref(stats))
    assert err == 0, err
    return accum, stats


def trace_samples(desc, cam, st, w, h, xy, s, ambient=None, frame_count=0, total_frame_index=0, tile=64):
    """rr_trace_samples: per listed sample {r, g, b, jitter_x, jitter_y} -> (out, stats)."""
    import numpy as np
    abi = _abi()
    lib = load()
    xy = np.ascontiguousarray(xy, np.uint32).reshape(-1, 2)
    s = np.ascontiguousarray(s, np.uint32).reshape(-1)
    out = np.zeros((xy.shape[0], 5), np.float32)
    stats = abi.Stats()
    err = lib.rr_trace_samples(C.byref(desc), C.byref(cam), C.byref(st), _ambient(ambient), w, h, tile, tile,
                               frame_count, total_frame_index, xy.shape[0],
                               xy.ctypes.data_as(C.POINTER(C.c_uint32)), s.ctypes.data_as(C.POINTER(C.c_uint32)),
                               out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(stats))
    assert err == 0, err
    return out, stats
