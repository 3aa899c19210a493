"""ctypes binding of tests/ref_robust/libref_robust.so (TEST INFRASTRUCTURE).

The CPU checker of the robust estimator (rt_robust_combine / rt_robust_combine_device): the operation of DESIGN.md
("The robust estimator") restated in plain C.  Only tests/ loads it.  Also the synthetic stacks the CPU and the GPU
tests of the estimator share, and an independent numpy float32 restatement of the definition.
"""
import ctypes as C
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_robust", "libref_robust.so")

_lib = None
F = np.float32


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
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_robust (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    lib.ref_robust_combine.restype = C.c_int
    lib.ref_robust_combine.argtypes = [C.c_int, P(C.c_float), C.c_uint32, C.c_uint32, C.c_uint32, P(abi.RobustParams),
                                       P(C.c_float), P(C.c_float)]
    _lib = lib
    return lib


def params(gini_scale=1.0, max_trim=15, buffers=8):
    p = _abi().RobustParams()
    p.buffers, p.gini_scale, p.max_trim = buffers, gini_scale, max_trim
    return p


def combine(stack, p=None, want_info=True):
    """ref_robust_combine: a float32 (K, h, w, 4) stack -> (out (h, w, 4), info (h, w, 4) or None)."""
    stack = np.ascontiguousarray(stack, np.float32)
    k, h, w, _ = stack.shape
    out = np.full((h, w, 4), -7.0, np.float32)
    info = np.full((h, w, 4), -7.0, np.float32) if want_info else None
    fp = C.POINTER(C.c_float)
    code = load().ref_robust_combine(0, stack.ctypes.data_as(fp), k, w, h, C.byref(p if p is not None else params()),
                                     out.ctypes.data_as(fp), info.ctypes.data_as(fp) if want_info else None)
    assert code == 0, code
    return out, info


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def numpy_combine(stack, gini_scale=1.0, max_trim=15):
    """The definition in numpy float32, every pixel at once: a stable argsort for the ranking, the Gini sums added
    in rank order, the pooled sums in buffer order -> (out, info, kept (K, h, w) bool); out and info are to match
    the checker bit for bit."""
    stack = np.ascontiguousarray(stack, np.float32)
    K, h, w, _ = stack.shape
    S = stack.reshape(K, h*w, 4)
    with np.errstate(all="ignore"):
        # 1. validity
        valid = (S[..., 3] > F(0.001)) & np.isfinite(S).all(axis=2)
        m = S[..., :3]/S[..., 3:]
        key = (m[..., 0] + m[..., 1]) + m[..., 2]
        valid &= np.isfinite(m).all(axis=2) & np.isfinite(key)
        key = np.where(key == 0, F(0), key).astype(np.float32)          # -0 counts as +0
        n = valid.sum(axis=0)
        nf = n.astype(np.float32)
        # 3. rank: a stable sort keeps equal keys in buffer order; invalid buffers go last
        order = np.argsort(np.where(valid, key, np.inf), axis=0, kind="stable")
        rank = np.argsort(order, axis=0, kind="stable")                  # the inverse permutation
        g = np.take_along_axis(np.where(valid & (key > 0), key, F(0)).astype(np.float32), order, axis=0)
        # 4. the Gini coefficient
        Ssum = np.zeros(h*w, np.float32)
        T = np.zeros(h*w, np.float32)
        for r in range(K):
            live = r < n
            Ssum = np.where(live, Ssum + g[r], Ssum)
            T = np.where(live, T + F(r + 1)*g[r], T)
        G = (F(2)*T)/(nf*Ssum) - (nf + F(1))/nf
        G = np.where((n >= 3) & np.isfinite(Ssum) & (Ssum > 0), G, F(0))
        G = np.where(G > 0, G, F(0)).astype(np.float32)
        # 5. the trim count (a NaN x, from 0*inf, trims nothing)
        cmax = np.minimum((np.maximum(n, 1) - 1)//2, max_trim)
        x = (F(gini_scale)*G)*(nf*F(0.5))
        c = np.where(x >= cmax.astype(np.float32), cmax, np.floor(np.nan_to_num(x, nan=0.0, posinf=0.0)).astype(np.int64))
        # 6. the kept ranks, pooled in buffer order
        kept = valid & (rank >= c) & (rank + c < n)
        num = np.zeros((h*w, 3), np.float32)
        den = np.zeros(h*w, np.float32)
        for k in range(K):
            num = np.where(kept[k][:, None], num + S[k, :, :3], num)
            den = np.where(kept[k], den + S[k, :, 3], den)
        out = np.concatenate([num/den[:, None], np.ones((h*w, 1), np.float32)], axis=1).astype(np.float32)
        info = np.stack([G, c.astype(np.float32), nf, den], axis=1).astype(np.float32)
    dead = n == 0
    out[dead] = S[0][dead]
    info[dead] = 0
    return out.reshape(h, w, 4), info.reshape(h, w, 4), kept.reshape(K, h, w)


SIZES = [(1, 1), (5, 3), (65, 33), (130, 7)]                             # (w, h)
COUNTS = [2, 3, 4, 5, 8, 9, 16, 17, 31, 32]


@functools.lru_cache(maxsize=None)
def _stack(w, h, K, seed):
    rng = np.random.default_rng(seed)
    rad = np.exp(rng.normal(0.0, 1.0, (1, h, w, 3)))                    # the pixel's radiance, log-normal
    noisy = rad*np.exp(rng.normal(0.0, 0.5, (K, h, w, 3)))              # each buffer's mean of it
    noisy[rng.random((K, h, w)) < 0.01] *= 1e3                          # sparse outliers
    wt = rng.uniform(0.5, 4.0, (K, h, w, 1))
    s = np.concatenate([noisy*wt, wt], axis=3).astype(np.float32)
    pick = rng.random((K, h, w)) < 0.05
    kind = rng.integers(0, 8, (K, h, w))
    above = np.nextafter(F(0.001), F(1))
    for k, y, x in zip(*np.nonzero(pick)):
        t = kind[k, y, x]
        if t == 0:
            s[k, y, x, 3] = 0.0                                         # weight 0
        elif t == 1:
            s[k, y, x, 3] = F(0.001)                                    # the threshold itself: not valid
        elif t == 2:
            s[k, y, x] = (1e38, 1e38, 1e38, above)                      # finite floats, a quotient that overflows
        elif t == 3:
            s[k, y, x, (k + x) % 4] = np.nan
        elif t == 4:
            s[k, y, x, (k + y) % 4] = np.inf if (k + x) % 2 else -np.inf
        elif t == 5:
            s[k, y, x, :3] *= -1.0                                      # a negative-sum radiance: valid, ranks first
        elif t == 6:
            s[k, y, x, :3] = -0.0 if k % 2 else 0.0                     # a key of -0 or +0
        else:
            s[k, y, x] = s[(k + K - 1) % K, y, x]*F(2)                  # the neighbour's key, another weight
    flat = s.reshape(K, h*w, 4)
    idx = np.arange(h*w)
    zeros = idx % 7 == 2                                                # -0.0 beside +0.0 in every buffer: S = 0
    flat[0::2, zeros, :3] = -0.0
    flat[1::2, zeros, :3] = 0.0
    flat[0, idx % 11 == 3, 3] = 0.0                                     # buffer 0 invalid
    dead = idx % 13 == 5                                                # no valid buffer
    flat[:, dead, 3] = 0.0
    flat[0, dead & (idx % 2 == 1), 1] = np.nan                          # ... and buffer 0 a NaN, which must pass through
    flat[0, dead & (idx % 4 == 0), 3] = -2.0                            # ... or a negative weight
    s.setflags(write=False)
    return s


def synthetic_stack(w, h, K):
    """The shared stack of a shape (read-only; K, h, w, 4): positive log-normal radiance with sparse 1e3x outliers;
    about 5 % of the (pixel, buffer) slots special in the ways the definition names; every 7th pixel all zeros of
    both signs, every 11th with buffer 0 invalid, every 13th with no valid buffer."""
    return _stack(w, h, K, 1000*K + 7*w + h)


@functools.lru_cache(maxsize=None)
def checked(w, h, K, gini_scale=1.0, max_trim=15):
    """The checker's (out, info) of synthetic_stack(w, h, K), computed once."""
    out, info = combine(synthetic_stack(w, h, K), params(gini_scale, max_trim))
    out.setflags(write=False)
    info.setflags(write=False)
    return out, info
