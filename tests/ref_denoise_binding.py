"""ctypes binding of tests/ref_denoise/libref_denoise.so (TEST INFRASTRUCTURE).

The CPU checker of the denoise stage (rt_denoise / rt_denoise_device): the filter of DESIGN.md ("The denoise
stage") restated in plain C over the oracle's expf.  Only tests/ loads it.  Also the random inputs the CPU and
the GPU tests of the stage share.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_denoise", "libref_denoise.so")

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
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_denoise (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    lib.ref_denoise.restype = C.c_int
    lib.ref_denoise.argtypes = [C.c_int, P(abi.AccumulationBuffer), P(C.c_float), P(C.c_float),
                                P(abi.DenoiseParams), P(C.c_float)]
    _lib = lib
    return lib


def params(iterations=3, sigma_color=1.0, sigma_guide=(0.1, 0.05), firefly_clamp=10.0):
    abi = _abi()
    p = abi.DenoiseParams()
    p.iterations = iterations
    p.sigma_color = sigma_color
    p.sigma_guide[0], p.sigma_guide[1] = sigma_guide
    p.firefly_clamp = firefly_clamp
    return p


def denoise(beauty, guide0, guide1, p):
    """ref_denoise: float32 (h, w, 4) accumulation buffers (guides may be None) -> the filtered buffer."""
    abi = _abi()
    fp = C.POINTER(C.c_float)
    beauty = np.ascontiguousarray(beauty, np.float32)
    h, w, _ = beauty.shape
    gs = [None if g is None else np.ascontiguousarray(g, np.float32) for g in (guide0, guide1)]
    out = np.zeros((h, w, 4), np.float32)
    buf = abi.AccumulationBuffer(w, h, 0, beauty.ctypes.data_as(fp))
    err = load().ref_denoise(0, C.byref(buf), *[None if g is None else g.ctypes.data_as(fp) for g in gs],
                             C.byref(p), out.ctypes.data_as(fp))
    assert err == 0, err
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_frames(w, h, seed, invalid_fraction=0.02):
    """A random HDR accumulation buffer and two guide buffers, weights included: radiance log-uniform over
    1e-3 .. 1e3 (fireflies), piecewise-smooth guides (a normals-like one in 0..1 with two regions, a
    distance-like one), and `invalid_fraction` of the pixels invalid in every way the definition names:
    NaN, +inf, weight 0, a negative weight, a resolved value that overflows, and an invalid guide pixel."""
    rng = np.random.default_rng(seed)
    wt = rng.uniform(0.5, 4.0, (h, w, 1)).astype(np.float32)
    rad = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (h, w, 3))).astype(np.float32)
    rad[rng.random((h, w)) < 0.1] *= np.float32(0.0)                  # black pixels too
    beauty = np.concatenate([rad*wt, wt], axis=2).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((xx*3 + yy*2) // 11) % 2
    n = np.stack([0.5 + 0.4*region, 0.5 - 0.3*region + 0.002*xx, 0.9 - 0.001*yy], axis=2)
    n = n + rng.normal(0.0, 0.02, (h, w, 3))
    gw0 = rng.uniform(1.0, 4.0, (h, w, 1))
    guide0 = np.concatenate([n*gw0, gw0], axis=2).astype(np.float32)
    d = 1.0 - np.clip((2.0 + 0.05*xx + 3.0*region)/15.0, 0.0, 1.0)
    d = np.repeat(d[:, :, None], 3, axis=2) + rng.normal(0.0, 0.01, (h, w, 3))
    gw1 = rng.uniform(1.0, 4.0, (h, w, 1))
    guide1 = np.concatenate([d*gw1, gw1], axis=2).astype(np.float32)
    kinds = 8
    pick = rng.random((h, w)) < invalid_fraction
    ys, xs = np.nonzero(pick)
    for k, (y, x) in enumerate(zip(ys, xs)):
        k %= kinds
        if k == 0:
            beauty[y, x, 1] = np.nan
        elif k == 1:
            beauty[y, x, 0] = np.inf
        elif k == 2:
            beauty[y, x, 3] = 0.0
        elif k == 3:
            beauty[y, x, 3] = -2.0
        elif k == 4:
            beauty[y, x] = (3e38, 1.0, 1.0, 0.5)       # finite in, the resolved value overflows
        elif k == 5:
            guide0[y, x, 3] = 0.0
        elif k == 6:
            guide1[y, x, 2] = np.nan
        else:
            beauty[y, x, 3] = np.nan
    return beauty, guide0, guide1
