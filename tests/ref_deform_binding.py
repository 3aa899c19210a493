"""ctypes binding of tests/ref_deform/libref_deform.so (TEST INFRASTRUCTURE).

The CPU checker of the history that follows deforming meshes ("Deforming meshes keep their history"): the
point and the shading normal of a surface record, and the deform-aware accumulate stage, restated in plain C.  Only
tests/ loads it.  Also what the CPU and the GPU tests share: the seeded synthetic inputs (tests/ref_motion_binding's
case with surface records and a deform table whose vertices put most carried points where the motion case has them),
the table as a numpy array over host or device pointers, and the flat sheet.
"""
import ctypes as C
import functools
import os

import numpy as np

import ref_motion_binding as mb
import ref_temporal_binding as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_deform", "libref_deform.so")

_lib = None
F = np.float32
NONE = 0xFFFFFFFF
_abi = tb._abi
bits = tb.bits


def load():
    global _lib
    if _lib is not None:
        return _lib
    abi = _abi()
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_deform (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    P = C.POINTER
    fp, gp, up = P(C.c_float), P(abi.GBufferTexel), P(C.c_uint32)
    lib.ref_deform_surface.restype = None
    lib.ref_deform_surface.argtypes = [fp, fp, fp, fp, C.c_uint32, up, fp, fp, fp]
    lib.ref_temporal_accumulate_deform.restype = C.c_int
    lib.ref_temporal_accumulate_deform.argtypes = [fp, gp, fp, fp, gp, P(abi.Camera), C.c_float, C.c_uint32, C.c_uint32,
                                                   P(abi.TemporalParams), fp, fp, P(abi.MotionEntry), C.c_uint32, fp, fp, fp,
                                                   P(abi.SurfaceTexel), P(abi.DeformEntry), C.c_uint32]
    _lib = lib
    return lib


def sdtype():
    return np.dtype(_abi().SURFACE_DTYPE)


def ddtype():
    return np.dtype(_abi().DEFORM_DTYPE)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def surface(triangles, normals, fwd, inv, triangle, v, w):
    """ref_deform_surface: records (triangle, v, w) under vertices [n,3,3], normals [n,3,3] or None, and the rows 0..2
    of a forward and an inverse matrix -> (Q (k, 3), n (k, 3))."""
    t = np.ascontiguousarray(triangles, F).reshape(-1, 9)
    nn = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 9)
    f = np.ascontiguousarray(np.asarray(fwd, F)[:3, :4])
    iv = np.ascontiguousarray(np.asarray(inv, F)[:3, :4])
    tri = np.ascontiguousarray(triangle, np.uint32).reshape(-1)
    assert tri.size == 0 or int(tri.max()) < t.shape[0]
    vw = np.ascontiguousarray(np.stack([np.asarray(v, F).reshape(-1), np.asarray(w, F).reshape(-1)], axis=1))
    Q, n = np.full((tri.size, 3), -7.0, F), np.full((tri.size, 3), -7.0, F)
    load().ref_deform_surface(_fp(t), _fp(nn), _fp(f), _fp(iv), tri.size, tri.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(vw),
                              _fp(Q), _fp(n))
    return Q, n


def table(prev, meshes):
    """The deform table as rt_scene_deform_table lays it out, from the previous transforms (abi.M4X4INV_DTYPE) and
    {primitive: (address of the vertices, address of the normals or 0, triangle count)}: host addresses for the
    checker, device addresses for the product."""
    prev = np.ascontiguousarray(prev, mb.m4dtype())
    out = np.zeros(prev.shape[0], ddtype())
    out["inv_prev"], out["fwd_prev"] = prev["inverse"][:, :3, :], prev["forward"][:, :3, :]
    for k, (t, n, count) in meshes.items():
        out["d_prev_triangles"][k], out["d_prev_normals"][k] = t, n
        out["triangle_count"][k], out["deformed"][k], out["has_normals"][k] = count, 1, 1 if n else 0
    return out


def host_table(prev, arrays):
    """table() over host arrays {primitive: (triangles, normals or None)}; the arrays must outlive its use."""
    return table(prev, {k: (t.ctypes.data, 0 if n is None else n.ctypes.data, t.reshape(-1, 9).shape[0])
                        for k, (t, n) in arrays.items()})


def accumulate_deform(current, gbuf, prev=None, prev_cam=None, prev_lens_distortion=0.0, p=None, motion=None, surf=None,
                      deform=None, want_moments=False, want_velocity=False):
    """ref_temporal_accumulate_deform: ref_motion_binding.accumulate_motion's arguments, the surface records (h, w) and a
    deform table over host pointers -> (history, length, moments or None, velocity or None)."""
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
        deform = np.ascontiguousarray(deform, ddtype())
        dcount = deform.shape[0]
    if surf is not None:
        surf = np.ascontiguousarray(surf, sdtype())
        assert surf.shape == (h, w)
    history = np.full((h, w, 4), -7.0, F)
    length = np.full((h, w), -7.0, F)
    moments = np.full((h, w, 2), -7.0, F) if want_moments else None
    velocity = np.full((h, w, 2), -7.0, F) if want_velocity else None
    cam = prev_cam if prev_cam is not None else abi.Camera()
    opt = lambda a, t: None if a is None else a.ctypes.data_as(t)
    code = load().ref_temporal_accumulate_deform(current.ctypes.data_as(fp), gbuf.ctypes.data_as(gp), opt(ph, fp), opt(pl, fp),
                                                 opt(pg, gp), C.byref(cam), prev_lens_distortion, w, h,
                                                 C.byref(p if p is not None else tb.params()), history.ctypes.data_as(fp),
                                                 length.ctypes.data_as(fp), opt(motion, C.POINTER(abi.MotionEntry)), count,
                                                 opt(pm, fp), opt(moments, fp), opt(velocity, fp),
                                                 opt(surf, C.POINTER(abi.SurfaceTexel)),
                                                 opt(deform, C.POINTER(abi.DeformEntry)), dcount)
    assert code == 0, code
    return history, length, moments, velocity


# ---- the seeded synthetic inputs

DEFORMED = {3: False, 4: True, 5: True}     # primitive -> its mesh has normals.  3 and 4 also move (4 about z), 5 stands;
                                            # 1 moves without deforming, 0 and 2 do neither, 6 and 7 lie beyond the table


def _quirk(inv):
    """xform_normal's 3 x 3 matrix of an inverse's rows: r = M n."""
    e = np.asarray(inv, np.float64)
    return np.array([[e[0, 0], e[0, 1], e[2, 0]], [e[0, 1], e[1, 1], e[2, 1]], [e[0, 2], e[1, 2], e[2, 2]]])


@functools.lru_cache(maxsize=None)
def deform_case(w, h, amount=2.0):
    """ref_motion_binding.motion_case with a surface record per pixel and last frame's vertices for primitives 3, 4 and
    5: one triangle per pixel, placed so that the record's point under the previous transform lies where the motion
    case carries the pixel's point, slid along the surface by up to a few pixels (its normal the carried one), so taps
    pass and fail in the motion case's proportions at other pixels of the previous frame.  A twelfth of the records name a triangle out of range; records on other primitives hold
    indices the stage must not look at.
    -> (current, gbuffer, prev, camera, motion table, surface, {primitive: (triangles, normals or None)}, prev transforms)."""
    cur, g, prev, cam, moving, _ = mb.motion_case(w, h, amount)
    _, tp = mb.six_transforms()
    rng = np.random.default_rng(77*w + h)
    n = w*h
    ids = g["primitive"].reshape(-1)
    P, N = g["p"].reshape(-1, 3), g["n"].reshape(-1, 3)
    surf = np.zeros(n, sdtype())
    surf["triangle"] = NONE
    arrays = {}
    for k, has_normals in DEFORMED.items():
        if moving["moved"][k]:
            Q, m = mb.carry(moving[k], P, N)
        else:
            Q, m = P.copy(), N.copy()
        # the deformation itself: up to half a unit along the surfaces (they lie near a plane z = const; a pixel is
        # about 0.2 units there), so the record's pixel of the previous frame is another one than the motion case's
        slide = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.zeros((n, 1))], axis=1)
        Q = Q.astype(np.float64) + slide + rng.normal(0.0, 3e-4, (n, 3))
        inv, fwd = tp["inverse"][k].astype(np.float64), tp["forward"][k].astype(np.float64)
        po = Q @ inv[:3, :3].T + inv[:3, 3]
        no = np.linalg.solve(_quirk(inv), m.astype(np.float64).T).T
        no /= np.maximum(np.linalg.norm(no, axis=1, keepdims=True), 1e-9)
        v = rng.uniform(0.0, 0.9, n)
        wv = rng.uniform(0.0, 0.9, n)*(1.0 - v)
        helper = np.where(np.abs(no[:, :1]) < 0.7, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
        e1 = np.cross(no, helper)
        e1 /= np.maximum(np.linalg.norm(e1, axis=1, keepdims=True), 1e-9)
        e2 = np.cross(no, e1)                                   # cross(e1, e2) = no
        e1, e2 = e1*rng.uniform(0.1, 0.4, (n, 1)), e2*rng.uniform(0.1, 0.4, (n, 1))
        a = po - v[:, None]*e1 - wv[:, None]*e2
        tris = np.stack([a, a + e1, a + e2], axis=1).astype(F)
        nrm = None
        if has_normals:
            nrm = (no[:, None, :] + rng.normal(0.0, 0.01, (n, 3, 3))).astype(F)
            nrm.setflags(write=False)
        tris.setflags(write=False)
        arrays[k] = (tris, nrm)
        here = ids == k
        surf["triangle"][here] = np.arange(n, dtype=np.uint32)[here]
        surf["v"][here], surf["w"][here] = v[here], wv[here]
    off = rng.random(n) < 1.0/12.0
    surf["triangle"][off] = np.array([n, n + 5, 0x7FFFFFFF, NONE], np.uint32)[rng.integers(0, 4, int(off.sum()))]
    other = ~np.isin(ids, list(DEFORMED)) & (ids < 8)
    surf["triangle"][other] = rng.integers(0, n, int(other.sum()))
    surf["v"][other], surf["w"][other] = 0.25, 0.5
    surf = surf.reshape(h, w)
    surf.setflags(write=False)
    return cur, g, prev, cam, moving, surf, arrays, tp


@functools.lru_cache(maxsize=None)
def checked(w, h, amount, moments, velocity):
    """The checker's outputs of deform_case(w, h, amount) under the default parameters."""
    cur, g, prev, cam, moving, surf, arrays, tp = deform_case(w, h, amount)
    out = accumulate_deform(cur, g, prev, cam, amount, tb.params(), moving, surf, host_table(tp, arrays), want_moments=moments,
                            want_velocity=velocity)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def sheet(cells=8, size=3.0, z=0.0, y0=0.0, tilt=0.2):
    """A flat sheet of cells x cells quads (two triangles each), `size` wide and high, its lower edge at y0, centred
    in x and facing -z (cross(b - a, c - a) points along (0, tilt, -1)).  Its plane is z + tilt*(y - the middle height): a
    sheet in a plane z = const would have boxes without depth, which no ray enters (the slab test's tn < tf)
    -> triangles [2 cells^2, 3, 3]."""
    s = np.linspace(0.0, 1.0, cells + 1)
    at = lambda x, y: [x, y, z + tilt*(y - (y0 + 0.5*size))]
    out = []
    for j in range(cells):
        for i in range(cells):
            x0, x1 = (s[i] - 0.5)*size, (s[i + 1] - 0.5)*size
            ya, yb = y0 + s[j]*size, y0 + s[j + 1]*size
            out.append([at(x0, ya), at(x0, yb), at(x1, ya)])
            out.append([at(x1, ya), at(x0, yb), at(x1, yb)])
    return np.array(out, F)
