"""ctypes binding of tests/ref_svgf/libref_svgf.so (TEST INFRASTRUCTURE).

The CPU checker of variance-guided filtering of the temporal history ("Variance-guided filtering"): the
accumulate stage with moments, the variance of the history and the variance-guided filter, restated in plain C.  Only
tests/ loads it.  Also the seeded synthetic inputs the CPU and the GPU tests share; the cameras and the float64 forward
projection are tests/ref_temporal_binding's.
"""
import ctypes as C
import functools
import os

import numpy as np

import ref_temporal_binding as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_svgf", "libref_svgf.so")

_lib = None
F = np.float32
MISS = tb.MISS
PLANE_BIT = tb.PLANE_BIT
SPATIAL_BELOW = 4.0

_abi = tb._abi
dtype = tb.dtype
bits = tb.bits


def load():
    global _lib
    if _lib is not None:
        return _lib
    abi = _abi()
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_svgf (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fp, gp = P(C.c_float), P(abi.GBufferTexel)
    lib.ref_temporal_accumulate_moments.restype = C.c_int
    lib.ref_temporal_accumulate_moments.argtypes = [fp, gp, fp, fp, gp, fp, P(abi.Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                    P(abi.TemporalParams), fp, fp, fp]
    lib.ref_temporal_variance.restype = C.c_int
    lib.ref_temporal_variance.argtypes = [fp, fp, gp, C.c_uint32, C.c_uint32, P(abi.TemporalParams), C.c_float, fp,
                                          P(C.c_uint32)]
    lib.ref_denoise_variance.restype = C.c_int
    lib.ref_denoise_variance.argtypes = [C.c_int, fp, fp, gp, C.c_uint32, C.c_uint32, P(abi.DenoiseVarianceParams), fp, fp]
    _lib = lib
    return lib


def filter_params(iterations=4, sigma_color=4.0, sigma_normal=0.2, sigma_plane=0.02, variance_epsilon=0.03,
                  firefly_clamp=10.0):
    p = _abi().DenoiseVarianceParams()
    p.iterations, p.sigma_color, p.sigma_normal, p.sigma_plane = iterations, sigma_color, sigma_normal, sigma_plane
    p.variance_epsilon, p.firefly_clamp = variance_epsilon, firefly_clamp
    return p


def accumulate_moments(current, gbuf, prev=None, prev_cam=None, prev_lens_distortion=0.0, p=None):
    """ref_temporal_accumulate_moments: current (h, w, 4), its G-buffer (h, w), prev = (history, length, gbuffer, moments)
    or None -> (history (h, w, 4), length (h, w), moments (h, w, 2))."""
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
        pm = np.ascontiguousarray(prev[3], np.float32)
        assert pm.shape == (h, w, 2)
    history = np.full((h, w, 4), -7.0, np.float32)
    length = np.full((h, w), -7.0, np.float32)
    moments = np.full((h, w, 2), -7.0, np.float32)
    cam = prev_cam if prev_cam is not None else abi.Camera()
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    code = load().ref_temporal_accumulate_moments(current.ctypes.data_as(fp), gbuf.ctypes.data_as(gp), opt(ph, fp), opt(pl, fp),
                                                  opt(pg, gp), opt(pm, fp), C.byref(cam), prev_lens_distortion, w, h,
                                                  C.byref(p if p is not None else tb.params()), history.ctypes.data_as(fp),
                                                  length.ctypes.data_as(fp), moments.ctypes.data_as(fp))
    assert code == 0, code
    return history, length, moments


def variance(moments, length, gbuf, p=None, spatial_below=SPATIAL_BELOW, want_counted=False):
    """ref_temporal_variance: moments (h, w, 2), length (h, w), the G-buffer (h, w) -> variance (h, w), and with
    want_counted the number of window taps that counted per pixel (0 where no window was taken)."""
    abi = _abi()
    moments = np.ascontiguousarray(moments, np.float32)
    h, w, _ = moments.shape
    length = np.ascontiguousarray(length, np.float32)
    gbuf = np.ascontiguousarray(gbuf, dtype())
    assert length.shape == (h, w) and gbuf.shape == (h, w)
    fp = C.POINTER(C.c_float)
    out = np.full((h, w), -7.0, np.float32)
    counted = np.zeros((h, w), np.uint32)
    code = load().ref_temporal_variance(moments.ctypes.data_as(fp), length.ctypes.data_as(fp),
                                        gbuf.ctypes.data_as(C.POINTER(abi.GBufferTexel)), w, h,
                                        C.byref(p if p is not None else tb.params()), spatial_below, out.ctypes.data_as(fp),
                                        counted.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert code == 0, code
    return (out, counted) if want_counted else out


def denoise_variance(color, var, gbuf, p=None):
    """ref_denoise_variance: colour (h, w, 4), variance (h, w), the G-buffer (h, w) -> (out (h, w, 4), variance (h, w))."""
    abi = _abi()
    color = np.ascontiguousarray(color, np.float32)
    h, w, _ = color.shape
    var = np.ascontiguousarray(var, np.float32)
    gbuf = np.ascontiguousarray(gbuf, dtype())
    assert var.shape == (h, w) and gbuf.shape == (h, w)
    fp = C.POINTER(C.c_float)
    out = np.full((h, w, 4), -7.0, np.float32)
    var_out = np.full((h, w), -7.0, np.float32)
    code = load().ref_denoise_variance(0, color.ctypes.data_as(fp), var.ctypes.data_as(fp),
                                       gbuf.ctypes.data_as(C.POINTER(abi.GBufferTexel)), w, h,
                                       C.byref(p if p is not None else filter_params()), out.ctypes.data_as(fp),
                                       var_out.ctypes.data_as(fp))
    assert code == 0, code
    return out, var_out


# ---- hand-made G-buffers

def plane_gbuffer(cam, w, h, depth, primitive=PLANE_BIT | 0):
    """The G-buffer a camera without distortion sees of the plane `depth` in front of it, facing it."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    P = tb.point_at(cam, 0.0, w, h, x, y, np.full((h, w), float(depth)))
    g = np.zeros((h, w), dtype())
    g["p"] = P
    g["t"] = np.linalg.norm(P - np.array([cam.p.x, cam.p.y, cam.p.z]), axis=2)
    g["n"] = (cam.z.x, cam.z.y, cam.z.z)
    g["primitive"] = primitive
    return g


def miss_gbuffer(cam, w, h):
    """An all-miss G-buffer: {the ray's direction, 0, 0, RT_HIT_MISS}."""
    g = plane_gbuffer(cam, w, h, 1.0, MISS)
    d = g["p"].astype(np.float64) - np.array([cam.p.x, cam.p.y, cam.p.z])
    g["p"] = d/np.linalg.norm(d, axis=2, keepdims=True)
    g["t"] = 0.0
    g["n"] = 0.0
    return g


# ---- the seeded synthetic inputs of the kernel tests

KERNEL_SIZES = [(1, 1), (5, 3), (65, 33), (130, 7)]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def synthetic_gbuffer(w, h, seed=0):
    """A frame's G-buffer (h, w): patches of four surfaces (two primitives, a plane, the sky) with a tenth of the
    pixels reassigned at random, so hit-and-miss borders run through every window; the hits lie near a plane 6 in
    front of the camera (seven in ten within 0.03 of it, the rest within 1: both sides of the plane tests), normals
    facing the camera but for 15 % turned at random and 5 % zero; a hit's t is > 0."""
    rng = np.random.default_rng(1000*w + h + 7919*seed)
    cam = tb.make_camera(p=(0.3, -0.2, 1.0), aspect=w/h)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    prims = np.array([1, 2, PLANE_BIT | 0, MISS], np.uint32)
    idx = ((x//7 + y//5) % 4).astype(np.int64)
    swap = rng.random((h, w)) < 0.1
    idx[swap] = rng.integers(0, 4, (h, w))[swap]
    depth = 6.0 + np.where(rng.random((h, w)) < 0.7, rng.uniform(-0.03, 0.03, (h, w)), rng.uniform(-1.0, 1.0, (h, w)))
    P = tb.point_at(cam, 0.0, w, h, x, y, depth)
    g = np.zeros((h, w), dtype())
    g["primitive"] = prims[idx]
    g["p"] = P
    o = np.array([cam.p.x, cam.p.y, cam.p.z])
    g["t"] = np.linalg.norm(P - o, axis=2)
    n = np.tile(np.array([0.0, 0.0, 1.0]), (h, w, 1))
    rnd = rng.normal(size=(h, w, 3))
    turned = rng.random((h, w)) < 0.15
    n[turned] = (rnd/np.linalg.norm(rnd, axis=2, keepdims=True))[turned]
    n[rng.random((h, w)) < 0.05] = 0.0
    g["n"] = n
    miss = g["primitive"] == MISS
    d = P - o
    g["p"][miss] = (d/np.linalg.norm(d, axis=2, keepdims=True))[miss]
    g["t"][miss] = 0.0
    g["n"][miss] = 0.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def moments_case(w, h, amount=2.0):
    """tests/ref_temporal_binding's synthetic accumulate case (snapped and bilinear taps, every tap rule, invalid current
    pixels) with previous moments beside it -> (current, gbuffer, (history, length, gbuffer, moments), camera)."""
    cur, g, prev, cam = tb.synthetic_case(w, h, amount)
    rng = np.random.default_rng(77*w + h)
    m1 = rng.uniform(0.0, 1.0, (h, w))
    pm = np.stack([m1, m1*m1 + rng.uniform(0.0, 0.05, (h, w))], axis=2).astype(np.float32)
    _frozen(pm)
    return cur, g, prev + (pm,), cam


@functools.lru_cache(maxsize=None)
def variance_case(w, h):
    """(moments (h, w, 2), length (h, w), gbuffer (h, w)): lengths on both sides of the default spatial_below (and the
    value itself), below 1, NaN and long; second moments a little above, at and below the first one's square."""
    rng = np.random.default_rng(31*w + h)
    g = synthetic_gbuffer(w, h)
    m1 = rng.uniform(0.0, 1.0, (h, w))
    m2 = m1*m1 + rng.uniform(-0.01, 0.05, (h, w))
    m = np.stack([m1, m2], axis=2).astype(np.float32)
    lens = np.array([0.0, 0.5, 1.0, 1.0, 2.0, 3.0, 3.5, 4.0, 4.0, 7.0, 32.0, np.nan], np.float32)
    length = lens[rng.integers(0, len(lens), (h, w))]
    return _frozen(m, length) + (g,)


@functools.lru_cache(maxsize=None)
def filter_case(w, h):
    """(colour (h, w, 4), variance (h, w), gbuffer (h, w)): a history {r, g, b, 1} on most pixels and an accumulation
    buffer's sums on the rest; invalid pixels as NaN, zero and negative weights, and as NaN, negative and infinite
    variances; variances log-uniform over six decades, and exactly 0."""
    rng = np.random.default_rng(53*w + h)
    g = synthetic_gbuffer(w, h, seed=1)
    wt = np.where(rng.random((h, w, 1)) < 0.7, 1.0, rng.uniform(0.5, 4.0, (h, w, 1)))
    col = np.concatenate([np.exp(rng.normal(-0.5, 1.2, (h, w, 3)))*wt, wt], axis=2).astype(np.float32)
    kind = rng.integers(0, 50, (h, w))
    col[kind == 0, 3] = 0.0
    col[kind == 1, 0] = np.nan
    col[kind == 2, 3] = -2.0
    col[kind == 3, 2] = np.inf
    col[kind == 4, :3] *= -1.0                                           # negative radiance: clamped to 0
    col[kind == 5, :3] *= 1000.0                                         # a firefly: clamped
    var = np.exp(rng.uniform(np.log(1e-7), np.log(1e-1), (h, w))).astype(np.float32)
    var[kind == 6] = np.nan
    var[kind == 7] = -1e-3
    var[kind == 8] = np.inf
    var[(kind >= 9) & (kind < 14)] = 0.0
    return _frozen(col, var) + (g,)


FILTER_PARAMS = [dict(), dict(iterations=1), dict(iterations=5), dict(iterations=5, sigma_color=0.0, variance_epsilon=1e-3), dict(iterations=2, sigma_normal=0.0),
                 dict(iterations=2, sigma_plane=0.0, firefly_clamp=0.0),
                 dict(iterations=3, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0)]


@functools.lru_cache(maxsize=None)
def checked_filter(w, h, k):
    """The checker's (out, variance) of filter_case(w, h) under FILTER_PARAMS[k], computed once."""
    col, var, g = filter_case(w, h)
    return _frozen(*denoise_variance(col, var, g, filter_params(**FILTER_PARAMS[k])))


# ---- the measurement set of the defaults: a camera path rendered by the oracle

def moved_along(cam, dx=0.0, dy=0.0, dz=0.0):
    """A copy of `cam` translated along its own axes."""
    abi = _abi()
    c = abi.Camera.from_buffer_copy(cam)
    c.p = abi.V3(*[getattr(cam.p, k) + dx*getattr(cam.x, k) + dy*getattr(cam.y, k) + dz*getattr(cam.z, k) for k in "xyz"])
    return c


@functools.lru_cache(maxsize=None)
def path_case(name, w, h, frames=16, standing=False, ref_spp=256, threads=16):
    """DESIGN.md's camera path ("Temporal accumulation": a flight of 3 units sideways and 2 forward over 16 frames) on a
    preset, 1 spp a frame by the oracle, or the same count of frames from the last camera when `standing`; the
    G-buffers by tests/ref_temporal; a `ref_spp` oracle frame at the last camera, of another total_frame_index
    -> (cameras, frames, gbuffers, reference, lens distortion)."""
    import sys
    import oracle_binding as ob
    rt = sys.modules["buas_pathtracer_amd"]
    scene, cam, st, fc, post = rt.load_preset(name, w, h)
    amount = st.lens_distortion
    last = frames - 1
    step = lambda k: moved_along(cam, dx=3.0*k/15.0, dz=-2.0*k/15.0)
    cams = [step(last if standing else k) for k in range(frames)]
    st.samples_per_pixel = 1
    frs = [ob.render(scene.desc(), cams[k], st, fc, w, h, rng_mode=0, threads=threads, frame_count=k, total_frame_index=0)[0]
           for k in range(frames)]
    if standing:
        g = tb.gbuffer(scene.desc(), cams[0], amount, w, h)
        gs = [g]*frames
    else:
        gs = [tb.gbuffer(scene.desc(), c, amount, w, h) for c in cams]
    st.samples_per_pixel = ref_spp
    ref = ob.render(scene.desc(), cams[last], st, fc, w, h, rng_mode=0, threads=threads, total_frame_index=7)[0]
    return cams, frs, gs, ref, amount


def run_path(case, p=None):
    """The accumulate stage with moments along path_case's frames -> the last (history, length, moments, gbuffer)."""
    cams, frs, gs, ref, amount = case
    prev, prev_cam = None, None
    for k in range(len(frs)):
        hist, length, mom = accumulate_moments(frs[k], gs[k], prev, prev_cam, amount, p)
        prev, prev_cam = (hist, length, gs[k], mom), cams[k]
    return hist, length, mom, gs[-1]


def tm_rmse(a, ref):
    """Tonemapped (1 - e^-c) RMSE of two accumulation buffers' resolved colours."""
    def tm(x):
        x = np.asarray(x, np.float64)
        with np.errstate(all="ignore"):
            c = np.maximum(x[..., :3]/x[..., 3:], 0.0)
        return 1.0 - np.exp(-np.nan_to_num(c, nan=0.0, posinf=1e30))
    return float(np.sqrt(np.mean((tm(a) - tm(ref))**2)))
