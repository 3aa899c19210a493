"""ctypes binding of tests/ref_clip/libref_clip.so (TEST INFRASTRUCTURE).

The CPU checker of neighbourhood clipping of the temporal history ("Neighbourhood clipping"): the statistics of
the current frame's windows and the accumulate stage with a clip, restated in plain C.  Only tests/ loads it.  Also what
the CPU and the GPU tests share: the seeded images of the statistics' tests and the checker's outputs of
tests/ref_deform_binding's case with a clip, computed once.
"""
import ctypes as C
import functools
import os

import numpy as np

import ref_deform_binding as db
import ref_motion_binding as mb
import ref_temporal_binding as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_clip", "libref_clip.so")

_lib = None
F = np.float32
_abi = tb._abi
bits = tb.bits

STAT_SIZES = [(65, 33), (130, 7), (1, 1), (3, 2), (200, 40)]     # straddle the 64-pixel and 16-row block edges
RADII = [1, 2, 3]
GAMMAS = [0.0, 1.0, 4.0]


def load():
    global _lib
    if _lib is not None:
        return _lib
    abi = _abi()
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_clip (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fp, gp = P(C.c_float), P(abi.GBufferTexel)
    lib.ref_temporal_neighbourhood.restype = C.c_int
    lib.ref_temporal_neighbourhood.argtypes = [fp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, fp]
    lib.ref_temporal_accumulate_clip.restype = C.c_int
    lib.ref_temporal_accumulate_clip.argtypes = [fp, gp, fp, fp, gp, P(abi.Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                 P(abi.TemporalParams), fp, fp, P(abi.MotionEntry), C.c_uint32, fp, fp, fp,
                                                 P(abi.SurfaceTexel), P(abi.DeformEntry), C.c_uint32, fp, C.c_float, C.c_float, fp]
    _lib = lib
    return lib


def ndtype():
    return np.dtype(_abi().NEIGHBOURHOOD_DTYPE)


def neighbourhood(current, radius, firefly_clamp=10.0):
    """ref_temporal_neighbourhood: an accumulation buffer (h, w, 4) -> (h, w) of abi.NEIGHBOURHOOD_DTYPE."""
    current = np.ascontiguousarray(current, F)
    h, w, _ = current.shape
    out = np.full((h, w), -7.0, F).repeat(8).reshape(h, w, 8).view(ndtype()).reshape(h, w)
    fp = C.POINTER(C.c_float)
    code = load().ref_temporal_neighbourhood(current.ctypes.data_as(fp), w, h, radius, firefly_clamp, out.ctypes.data_as(fp))
    assert code == 0, code
    return out


def accumulate_clip(current, gbuf, prev=None, prev_cam=None, prev_lens_distortion=0.0, p=None, motion=None, surf=None,
                    deform=None, nb=None, gamma=0.5, min_count=2.0, want_moments=False, want_velocity=False, want_amount=True):
    """ref_temporal_accumulate_clip: ref_deform_binding.accumulate_deform's arguments, the neighbourhood texels (h, w) or
    None, gamma and min_count -> (history, length, moments or None, velocity or None, clip amount or None)."""
    abi = _abi()
    current = np.ascontiguousarray(current, F)
    h, w, _ = current.shape
    gbuf = np.ascontiguousarray(gbuf, tb.dtype())
    fp, gp = C.POINTER(C.c_float), C.POINTER(abi.GBufferTexel)
    ph = pl = pg = pm = None
    if prev is not None:
        ph, pl = np.ascontiguousarray(prev[0], F), np.ascontiguousarray(prev[1], F)
        pg = np.ascontiguousarray(prev[2], tb.dtype())
        if want_moments:
            pm = np.ascontiguousarray(prev[3], F)
            assert pm.shape == (h, w, 2)
    count = dcount = 0
    if motion is not None:
        motion = np.ascontiguousarray(motion, mb.mdtype())
        count = motion.shape[0]
    if deform is not None:
        deform = np.ascontiguousarray(deform, db.ddtype())
        dcount = deform.shape[0]
    if surf is not None:
        surf = np.ascontiguousarray(surf, db.sdtype())
        assert surf.shape == (h, w)
    if nb is not None:
        nb = np.ascontiguousarray(nb, ndtype())
        assert nb.shape == (h, w)
    history = np.full((h, w, 4), -7.0, F)
    length = np.full((h, w), -7.0, F)
    moments = np.full((h, w, 2), -7.0, F) if want_moments else None
    velocity = np.full((h, w, 2), -7.0, F) if want_velocity else None
    amount = np.full((h, w), -7.0, F) if want_amount else None
    cam = prev_cam if prev_cam is not None else abi.Camera()
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    code = load().ref_temporal_accumulate_clip(current.ctypes.data_as(fp), gbuf.ctypes.data_as(gp), opt(ph, fp), opt(pl, fp),
                                               opt(pg, gp), C.byref(cam), prev_lens_distortion, w, h,
                                               C.byref(p if p is not None else tb.params()), history.ctypes.data_as(fp),
                                               length.ctypes.data_as(fp), opt(motion, C.POINTER(abi.MotionEntry)), count,
                                               opt(pm, fp), opt(moments, fp), opt(velocity, fp),
                                               opt(surf, C.POINTER(abi.SurfaceTexel)),
                                               opt(deform, C.POINTER(abi.DeformEntry)), dcount, opt(nb, fp), gamma, min_count,
                                               opt(amount, fp))
    assert code == 0, code
    return history, length, moments, velocity, amount


# ---- the seeded inputs

@functools.lru_cache(maxsize=None)
def stats_image(w, h):
    """A read-only accumulation buffer (h, w, 4): log-normal colours under weights of 0.5 to 4, and one pixel in eight
    invalid or at an edge of the rule: weight 0, the threshold 0.001 itself, a NaN and an infinite colour, a negative
    weight, negative radiance (clamped to 0), a quotient that overflows, a colour above the firefly clamp."""
    rng = np.random.default_rng(900*w + h)
    n = w*h
    wt = rng.uniform(0.5, 4.0, (n, 1))
    cur = np.concatenate([np.exp(rng.normal(0.0, 1.5, (n, 3)))*wt, wt], axis=1).astype(F)
    kind = rng.integers(0, 64, n)
    cur[kind == 0, 3] = 0.0
    cur[kind == 1, 3] = F(0.001)
    cur[kind == 2, 0] = np.nan
    cur[kind == 3, 3] = -2.0
    cur[kind == 4, 2] = np.inf
    cur[kind == 5, :3] *= -1.0
    cur[kind == 6] = (1e38, 1e38, 1e38, np.nextafter(F(0.001), F(1)))
    cur[kind == 7, 1] = 500.0
    cur = cur.reshape(h, w, 4)
    cur.setflags(write=False)
    return cur


@functools.lru_cache(maxsize=None)
def stats_checked(w, h, radius):
    out = neighbourhood(stats_image(w, h), radius, 10.0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clip_texels(w, h, amount):
    """The checker's radius-3 statistics of deform_case(w, h, amount)'s current frame under the default clamp."""
    out = neighbourhood(db.deform_case(w, h, amount)[0], 3, tb.params().firefly_clamp)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def checked(w, h, amount, moments, velocity, gamma, want_amount=True, min_count=2.0):
    """The checker's outputs of deform_case(w, h, amount) clipped to clip_texels under the default parameters."""
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    out = accumulate_clip(cur, g, prev, cam, amount, tb.params(), moving, surf, db.host_table(tp, arrays), clip_texels(w, h, amount),
                          gamma, min_count, want_moments=moments, want_velocity=velocity, want_amount=want_amount)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


# ---- the ghost the clip exists for: a box's shadow on a floor, and the box moved

# the box's centre in frames 0..7 and from frame 8 on: out of the picture, shadow and all, so that the mask is the old
# shadow alone (with both shadows in it the history is too dark in one and too bright in the other, and the mask's mean
# hides both)
GHOST_BOX_AT = [(-2.4, 2.0, 5.0), (14.0, 2.0, 5.0)]


def ghost_scene(rt, w, h):
    """A floor plane, a sphere light above it and a box between them, under a dim sky, seen by a standing camera from
    above; the box's shadow lies on the floor beside it, and GHOST_BOX_AT[1] takes box and shadow out of the picture
    -> (scene, the box's primitive id, camera, settings at one sample per pixel, filter)."""
    s = rt.Scene()
    floor = s.add_diffuse_material((0.7, 0.7, 0.7), 1.5)
    red = s.add_diffuse_material((0.7, 0.3, 0.2), 1.5)
    light = s.add_emissive_material((30.0, 28.0, 26.0))
    s.add_plane(floor, (0.0, 1.0, 0.0), 0.0)
    s.add_sphere(light, 0.7, rt.translate((0.0, 9.0, 5.0)))
    box = s.add_box(red, (1.2, 0.4, 1.2), rt.translate(GHOST_BOX_AT[0]))
    s.set_sky((0.05, 0.06, 0.08), (0.03, 0.03, 0.03))
    s.create_scene_bvh()
    cam = rt.abi.Camera()
    cam.vfov, cam.aspect_ratio, cam.lens_radius, cam.focus_distance = rt.DEG_TO_RAD*50.0, w/h, 0.0, 10.0
    cam.p = rt.v3(0.0, 6.0, -4.0)
    rt.aim_camera_at(cam, (0.0, 0.0, 5.0))
    rt.recompute_camera(cam)
    st, _ = rt.default_settings()
    st.lens_distortion, st.samples_per_pixel = 0.0, 1
    return s, box, cam, st, rt.load_reconstruction_kernel("Box")


def luminance(rgb):
    return 0.2126*rgb[..., 0] + 0.7152*rgb[..., 1] + 0.0722*rgb[..., 2]


def ghost_mask(ref_old, ref_new, floor):
    """The floor pixels whose luminance differs between the two configurations' reference frames (h, w, 3, resolved) by
    more than half of the larger of the two."""
    a, b = luminance(ref_old), luminance(ref_new)
    return floor & (np.abs(a - b) > 0.5*np.maximum(a, b))
