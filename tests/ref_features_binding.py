"""ctypes binding of tests/ref_features/libref_features.so (TEST INFRASTRUCTURE).

The CPU checker of the feature frames (rt_render_feature) and of the denoise stage that uses them
(rt_denoise_features): a unity build over oracle/oracle.c with the feature walk, a frame driver of its own and
the filter restated in plain C.  Only tests/ loads it.  Also the random inputs the CPU and the GPU tests of the
filter share.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_features", "libref_features.so")

ADVANCED = -1                       # ref_features_render's `feature` for the driver pin
NORMAL, DISTANCE, ALBEDO = range(3)
END_MISS, END_EMITTER, END_DIFFUSE, END_BOUND = range(4)

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
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_features (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fns = {
        "ref_features_render": (C.c_int, [P(abi.SceneDesc), P(abi.Camera), P(abi.Settings), P(abi.FilterCache),
                                          P(abi.TileSet), C.c_uint32, C.c_int, P(abi.AccumulationBuffer),
                                          P(abi.Stats), P(C.c_uint64)]),
        "ref_features_trace_samples": (C.c_int, [P(abi.SceneDesc), P(abi.Camera), P(abi.Settings), C.c_uint32,
                                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                                 C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_float),
                                                 P(C.c_uint32), P(abi.Stats)]),
        "ref_denoise_features": (C.c_int, [C.c_int, P(abi.AccumulationBuffer), P(C.c_float), P(C.c_float),
                                           P(C.c_float), P(abi.DenoiseFeaturesParams), P(C.c_float)]),
        "ref_features_set_math_mode": (None, [C.c_int]),
    }
    for name, (res, args) in fns.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib
    return lib


def render(desc, cam, st, fc, w, h, feature, tile=64, shard_index=0, shard_count=1, frame_count=0,
           total_frame_index=0, accum=None):
    """ref_features_render: one frame on one thread, tiles total-1 .. 0 -> (accum, stats, specular bounces)."""
    abi = _abi()
    if accum is None:
        accum = np.zeros((h, w, 4), np.float32)
    buf = abi.AccumulationBuffer(w, h, frame_count, accum.ctypes.data_as(C.POINTER(C.c_float)))
    tiles = abi.TileSet(tile, tile, shard_index, shard_count)
    stats = abi.Stats()
    spec = C.c_uint64(0)
    err = load().ref_features_render(C.byref(desc), C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles),
                                     total_frame_index, int(feature), C.byref(buf), C.byref(stats), C.byref(spec))
    assert err == 0, err
    return accum, stats, int(spec.value)


def trace_samples(desc, cam, st, w, h, xy, s, feature, frame_count=0, total_frame_index=0, tile=64):
    """ref_features_trace_samples: per listed sample {r, g, b, jitter_x, jitter_y} and {end, specular bounces,
    T} -> (out (n, 5) f32, end (n,) u32, specular bounces (n,) u32, T (n,) f32, stats)."""
    abi = _abi()
    xy = np.ascontiguousarray(xy, np.uint32).reshape(-1, 2)
    s = np.ascontiguousarray(s, np.uint32).reshape(-1)
    out = np.zeros((xy.shape[0], 5), np.float32)
    walk = np.zeros((xy.shape[0], 3), np.uint32)
    stats = abi.Stats()
    u32 = C.POINTER(C.c_uint32)
    err = load().ref_features_trace_samples(C.byref(desc), C.byref(cam), C.byref(st), w, h, tile, tile, frame_count,
                                            total_frame_index, int(feature), xy.shape[0], xy.ctypes.data_as(u32),
                                            s.ctypes.data_as(u32), out.ctypes.data_as(C.POINTER(C.c_float)),
                                            walk.ctypes.data_as(u32), C.byref(stats))
    assert err == 0, err
    return out, walk[:, 0].copy(), walk[:, 1].copy(), walk[:, 2].copy().view(np.float32), stats


def params(iterations=3, sigma_color=1.0, sigma_guide=(0.1, 0.05), firefly_clamp=10.0, sigma_albedo=0.0,
           demodulate=0, albedo_floor=0.0):
    p = _abi().DenoiseFeaturesParams()
    p.base.iterations = iterations
    p.base.sigma_color = sigma_color
    p.base.sigma_guide[0], p.base.sigma_guide[1] = sigma_guide
    p.base.firefly_clamp = firefly_clamp
    p.sigma_albedo = sigma_albedo
    p.demodulate = demodulate
    p.albedo_floor = albedo_floor
    return p


def denoise(beauty, normal, distance, albedo, p, expect=0):
    """ref_denoise_features: float32 (h, w, 4) accumulation buffers (any frame but the beauty may be None) ->
    the filtered buffer."""
    abi = _abi()
    fp = C.POINTER(C.c_float)
    beauty = np.ascontiguousarray(beauty, np.float32)
    h, w, _ = beauty.shape
    gs = [None if g is None else np.ascontiguousarray(g, np.float32) for g in (normal, distance, albedo)]
    out = np.zeros((h, w, 4), np.float32)
    buf = abi.AccumulationBuffer(w, h, 0, beauty.ctypes.data_as(fp))
    err = load().ref_denoise_features(0, C.byref(buf), *[None if g is None else g.ctypes.data_as(fp) for g in gs],
                                      C.byref(p), out.ctypes.data_as(fp))
    assert err == expect, err
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_albedo(w, h, seed, invalid_fraction=0.02):
    """A random albedo accumulation buffer for ref_denoise_binding.random_frames' beauty and guides: two
    checker-like regions of 0..1 values, a tenth of the pixels below every floor the tests use (0 included), and
    `invalid_fraction` of the pixels invalid: weight 0, NaN, a negative weight, a resolved value that overflows."""
    rng = np.random.default_rng(seed + 7919)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((xx // 4) ^ (yy // 3)) & 1
    a = np.stack([0.8 - 0.6*region, 0.3 + 0.5*region, 0.6 + 0.0*region], axis=2) + rng.normal(0.0, 0.01, (h, w, 3))
    a[rng.random((h, w)) < 0.1] *= 0.004
    a[rng.random((h, w)) < 0.03] = 0.0
    wt = rng.uniform(1.0, 4.0, (h, w, 1))
    albedo = np.concatenate([a*wt, wt], axis=2).astype(np.float32)
    ys, xs = np.nonzero(rng.random((h, w)) < invalid_fraction)
    for k, (y, x) in enumerate(zip(ys, xs)):
        k %= 4
        if k == 0:
            albedo[y, x, 3] = 0.0
        elif k == 1:
            albedo[y, x, 0] = np.nan
        elif k == 2:
            albedo[y, x, 3] = -1.0
        else:
            albedo[y, x] = (3e38, 1.0, 1.0, 0.5)
    return albedo
