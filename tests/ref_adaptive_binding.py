"""ctypes binding of tests/ref_adaptive/libref_adaptive.so (TEST INFRASTRUCTURE).

The CPU checker of the tile error estimate (rt_tile_error / rt_tile_error_device): the operation of DESIGN.md
("Adaptive sampling by tiles") restated in plain C.  Only tests/ loads it.  Also the synthetic half buffers the CPU
and the GPU tests of the estimate share, and a numpy float64 restatement of the metric.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_adaptive", "libref_adaptive.so")

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
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_adaptive (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    lib.ref_tile_error.restype = C.c_int
    lib.ref_tile_error.argtypes = [C.c_int, P(C.c_float), P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                   P(C.c_uint32), C.c_uint32, P(abi.TileErrorParams), P(C.c_float), P(C.c_uint32)]
    _lib = lib
    return lib


def params(floor=1e-4):
    p = _abi().TileErrorParams()
    p.floor = floor
    return p


def tile_grid(w, h, tw, th):
    return (w + tw - 1) // tw, (h + th - 1) // th


def tile_error(a, b, tw, th, ids=None, p=None):
    """ref_tile_error: two float32 (h, w, 4) half buffers -> (error float32, valid uint32) per listed tile."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    h, w, _ = a.shape
    tcx, tcy = tile_grid(w, h, tw, th)
    ids_a = None if ids is None else np.ascontiguousarray(ids, np.uint32).reshape(-1)
    count = tcx*tcy if ids_a is None else ids_a.size
    err = np.zeros(count, np.float32)
    valid = np.zeros(count, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    code = load().ref_tile_error(0, a.ctypes.data_as(fp), b.ctypes.data_as(fp), w, h, tw, th,
                                 None if ids_a is None else ids_a.ctypes.data_as(up), count,
                                 C.byref(p if p is not None else params()), err.ctypes.data_as(fp), valid.ctypes.data_as(up))
    assert code == 0, code
    return err, valid


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def numpy_tile_error(a, b, tw, th, ids=None, floor=1e-4):
    """The metric in float64, from the definition alone: no summation order, no f32 rounding -> (error, valid)."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    h, w, _ = a64.shape
    tcx, tcy = tile_grid(w, h, tw, th)
    ids = range(tcx*tcy) if ids is None else ids
    valid = (np.asarray(a)[..., 3] > np.float32(0.001)) & (np.asarray(b)[..., 3] > np.float32(0.001))
    valid &= np.isfinite(a64).all(axis=2) & np.isfinite(b64).all(axis=2)
    with np.errstate(all="ignore"):
        ra, rb = a64[..., :3]/a64[..., 3:], b64[..., :3]/b64[..., 3:]
        m = ((a64[..., :3] + b64[..., :3])/(a64[..., 3:] + b64[..., 3:])).sum(axis=2)
        e = np.abs(ra - rb).sum(axis=2)/np.sqrt(np.maximum(m, float(np.float32(floor))))
    errs, counts = [], []
    for t in ids:
        x0, y0 = tw*(t % tcx), th*(t // tcx)
        v = valid[y0:y0 + th, x0:x0 + tw]
        n = int(v.sum())
        counts.append(n)
        errs.append(float(e[y0:y0 + th, x0:x0 + tw][v].sum()/n) if n else np.inf)
    return np.array(errs), np.array(counts, np.uint32)


def half_buffers(w, h, seed, invalid_fraction=0.03, dead_tile=None):
    """Two random half buffers of one image: radiance log-uniform over 1e-3 .. 1e2 with per-half noise of up to 30 %,
    weights 0.5 .. 4, a tenth of the pixels black (m under the floor), a band of pixels where A equals B, and
    `invalid_fraction` of the pixels invalid in the ways the definition names (NaN, +inf, a zero weight, a
    negative weight, in either half).  dead_tile = (x0, y0, x1, y1): a rectangle with no valid pixel."""
    rng = np.random.default_rng(seed)
    rad = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (h, w, 3)))
    rad[rng.random((h, w)) < 0.1] = 0.0
    out = []
    for _ in range(2):
        wt = rng.uniform(0.5, 4.0, (h, w, 1))
        noisy = rad*rng.uniform(0.7, 1.3, (h, w, 3))
        out.append(np.concatenate([noisy*wt, wt], axis=2).astype(np.float32))
    a, b = out
    b[h // 2] = a[h // 2]                               # a row of equal halves: e = 0 there
    pick = rng.random((h, w)) < invalid_fraction
    for k, (y, x) in enumerate(zip(*np.nonzero(pick))):
        buf = a if (k // 4) % 2 == 0 else b
        if k % 4 == 0:
            buf[y, x, k % 3] = np.nan
        elif k % 4 == 1:
            buf[y, x, 1] = np.inf
        elif k % 4 == 2:
            buf[y, x, 3] = 0.0
        else:
            buf[y, x, 3] = -1.5
    if dead_tile is not None:
        x0, y0, x1, y1 = dead_tile
        a[y0:y1, x0:x1, 3] = 0.0
    return a, b


# (w, h, tile_w, tile_h): tiles of 1x1, 16x16 (exactly 256 pixels: one trip of the per-thread loop), 17x16 (the
# second trip), 64x64, and a ragged 130x70 frame of 64x64 tiles whose edge tiles are 2 wide and 6 tall
SHAPES = [(5, 3, 1, 1), (48, 32, 16, 16), (51, 32, 17, 16), (128, 64, 64, 64), (130, 70, 64, 64)]


def synthetic_case(w, h, tw, th):
    """The shared inputs of a shape: buffers with every kind of pixel, one tile without a valid pixel (the last),
    and a sub-list of the tiles (descending, to show the outputs follow the list)."""
    tcx, tcy = tile_grid(w, h, tw, th)
    last = tcx*tcy - 1
    x0, y0 = tw*(last % tcx), th*(last // tcx)
    a, b = half_buffers(w, h, seed=7*w + h, dead_tile=(x0, y0, w, h))
    sub = [last] + list(range(last - 1, -1, -2))
    return a, b, sub
