"""ctypes binding of tests/ref_motion/libref_motion.so (TEST INFRASTRUCTURE).

The CPU checker of the history that follows moving instances ("Moving instances"): the motion table and the
motion-aware accumulate stage restated in plain C.  Only tests/ loads it.  Also the seeded synthetic inputs the CPU and
the GPU tests share (tests/ref_temporal_binding's and tests/ref_svgf_binding's cases with a 6-entry table), the
transforms as numpy arrays and the float64 model of the carried point.
"""
import ctypes as C
import functools
import os

import numpy as np

import ref_svgf_binding as sb
import ref_temporal_binding as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_motion", "libref_motion.so")

_lib = None
MISS = tb.MISS
PLANE_BIT = tb.PLANE_BIT
_abi = tb._abi
dtype = tb.dtype
bits = tb.bits


def _rt():
    import sys
    return sys.modules["buas_pathtracer_amd"]


def load():
    global _lib
    if _lib is not None:
        return _lib
    abi = _abi()
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_motion (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fp, gp, mp, ep = P(C.c_float), P(abi.GBufferTexel), P(abi.M4x4Inv), P(abi.MotionEntry)
    lib.ref_motion_table.restype = None
    lib.ref_motion_table.argtypes = [C.c_uint32, mp, mp, ep]
    lib.ref_motion_carry.restype = None
    lib.ref_motion_carry.argtypes = [ep, C.c_uint32, fp, fp, fp, fp]
    lib.ref_temporal_accumulate_motion.restype = C.c_int
    lib.ref_temporal_accumulate_motion.argtypes = [fp, gp, fp, fp, gp, P(abi.Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                   P(abi.TemporalParams), fp, fp, ep, C.c_uint32, fp, fp, fp]
    _lib = lib
    return lib


def m4dtype():
    return np.dtype(_abi().M4X4INV_DTYPE)


def mdtype():
    return np.dtype(_abi().MOTION_DTYPE)


def transforms(*ts):
    """rt_m4x4inv structs (rt.translate(...) and the like) -> a structured array of abi.M4X4INV_DTYPE."""
    return np.concatenate([np.frombuffer(bytes(t), m4dtype()) for t in ts]) if ts else np.zeros(0, m4dtype())


def table(cur, prev):
    """ref_motion_table of two transform arrays -> a structured array of abi.MOTION_DTYPE."""
    abi = _abi()
    cur, prev = np.ascontiguousarray(cur, m4dtype()), np.ascontiguousarray(prev, m4dtype())
    out = np.zeros(cur.shape[0], mdtype())
    out["reserved"] = 7                      # the checker writes them
    mp = C.POINTER(abi.M4x4Inv)
    load().ref_motion_table(cur.shape[0], cur.ctypes.data_as(mp), prev.ctypes.data_as(mp),
                            out.ctypes.data_as(C.POINTER(abi.MotionEntry)))
    return out


def carry(entry, P, n):
    """The checker's new step alone: float32 points and normals (k, 3) under one table entry -> (Q, m)."""
    abi = _abi()
    P, n = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(n, np.float32)
    e = np.ascontiguousarray(entry, mdtype()).reshape(1)
    Q, m = np.zeros_like(P), np.zeros_like(n)
    fp = C.POINTER(C.c_float)
    load().ref_motion_carry(e.ctypes.data_as(C.POINTER(abi.MotionEntry)), P.shape[0], P.ctypes.data_as(fp), n.ctypes.data_as(fp),
                            Q.ctypes.data_as(fp), m.ctypes.data_as(fp))
    return Q, m


def accumulate_motion(current, gbuf, prev=None, prev_cam=None, prev_lens_distortion=0.0, p=None, motion=None,
                      want_moments=False, want_velocity=False):
    """ref_temporal_accumulate_motion: current (h, w, 4), its G-buffer (h, w), prev = (history, length, gbuffer[, moments])
    or None, motion a table or None -> (history, length, moments or None, velocity or None)."""
    abi = _abi()
    current = np.ascontiguousarray(current, np.float32)
    h, w, _ = current.shape
    gbuf = np.ascontiguousarray(gbuf, dtype())
    fp, gp = C.POINTER(C.c_float), C.POINTER(abi.GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph = np.ascontiguousarray(prev[0], np.float32)
        pl = np.ascontiguousarray(prev[1], np.float32)
        pg = np.ascontiguousarray(prev[2], dtype())
        if want_moments:
            pm = np.ascontiguousarray(prev[3], np.float32)
            assert pm.shape == (h, w, 2)
    count = 0
    if motion is not None:
        motion = np.ascontiguousarray(motion, mdtype())
        count = motion.shape[0]
    history = np.full((h, w, 4), -7.0, np.float32)
    length = np.full((h, w), -7.0, np.float32)
    moments = np.full((h, w, 2), -7.0, np.float32) if want_moments else None
    velocity = np.full((h, w, 2), -7.0, np.float32) if want_velocity else None
    cam = prev_cam if prev_cam is not None else abi.Camera()
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    code = load().ref_temporal_accumulate_motion(current.ctypes.data_as(fp), gbuf.ctypes.data_as(gp), opt(ph, fp), opt(pl, fp),
                                                 opt(pg, gp), C.byref(cam), prev_lens_distortion, w, h,
                                                 C.byref(p if p is not None else tb.params()), history.ctypes.data_as(fp),
                                                 length.ctypes.data_as(fp), opt(motion, C.POINTER(abi.MotionEntry)), count,
                                                 opt(pm, fp), opt(moments, fp), opt(velocity, fp))
    assert code == 0, code
    return history, length, moments, velocity


# ---- the seeded synthetic inputs

def six_transforms():
    """(cur, prev) of six primitives: 1 translated, 3 rotated about y, 4 rotated about z, the others where they were.
    The motions are small against the default plane tolerance at the synthetic case's distance, so taps of the moved
    primitives pass and fail in comparable numbers."""
    rt = _rt()
    still = rt.mul(rt.translate((0.2, -0.1, 0.3)), rt.scale(1.5))
    cur = transforms(rt.identity(), rt.translate((0.05, -0.03, 0.02)), still, rt.rotate_y(0.004), rt.rotate_z(0.01), still)
    prev = transforms(rt.identity(), rt.translate((-0.04, 0.02, -0.01)), still, rt.rotate_y(-0.003), rt.rotate_z(-0.006), still)
    return cur, prev


def _respread(g, rng):
    """A copy of a synthetic G-buffer whose hits on primitives 1 and 2 are spread over ids 1..7 (6 and 7 lie beyond a
    6-entry table)."""
    g = g.copy()
    ids = g["primitive"].reshape(-1)
    one = np.nonzero(ids == 1)[0]
    ids[one] = np.array([1, 1, 3, 3, 4, 4, 6], np.uint32)[rng.integers(0, 7, one.size)]
    two = np.nonzero(ids == 2)[0]
    ids[two] = np.array([2, 5, 7], np.uint32)[rng.integers(0, 3, two.size)]
    return g


@functools.lru_cache(maxsize=None)
def motion_case(w, h, amount=2.0):
    """ref_svgf_binding.moments_case with its primitive ids spread over a 6-entry table's and beyond ->
    (current, gbuffer, (history, length, gbuffer, moments), camera, table, unmoved table)."""
    cur, g, prev, cam = sb.moments_case(w, h, amount)
    rng = np.random.default_rng(31*w + h)
    g2, pg2 = _respread(g, rng), _respread(prev[2], rng)
    # the same ids more often than chance: a tap needs them equal
    same = rng.random((h, w)) < 0.5
    pg2["primitive"][same] = np.where(pg2["primitive"][same] < 8, g2["primitive"][same], pg2["primitive"][same])
    tc, tp = six_transforms()
    moving, unmoved = table(tc, tp), table(tc, tc)
    for a in (g2, pg2, moving, unmoved):
        a.setflags(write=False)
    return cur, g2, (prev[0], prev[1], pg2, prev[3]), cam, moving, unmoved


@functools.lru_cache(maxsize=None)
def checked(w, h, amount, moments, velocity):
    """The checker's outputs of motion_case(w, h, amount) with the moving table under the default parameters."""
    cur, g, prev, cam, moving, _ = motion_case(w, h, amount)
    out = accumulate_motion(cur, g, prev, cam, amount, tb.params(), moving, want_moments=moments, want_velocity=velocity)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


# ---- the float64 model of the carried point

def m64(kind, v):
    """A 4 x 4 forward matrix in float64: 't' translation by v (3,), 'ry' rotation about y by v, 's' uniform scale v."""
    m = np.eye(4)
    if kind == "t":
        m[:3, 3] = v
    elif kind == "ry":
        c, s = np.cos(v), np.sin(v)
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    else:
        m[0, 0] = m[1, 1] = m[2, 2] = v
    return m


def product_transform(kind, v):
    """The product's own transform of the same kind, from the value rounded to float32."""
    rt = _rt()
    if kind == "t":
        return rt.translate(tuple(float(np.float32(x)) for x in v))
    if kind == "ry":
        return rt.rotate_y(float(np.float32(v)))
    return rt.scale(float(np.float32(v)))
