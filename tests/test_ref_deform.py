"""Deforming meshes keep their history, on the CPU: the checker of the deform-aware accumulate stage (tests/ref_deform)
against the checker it extends, the surface point against float64 for rigid motions written as deformations, the normal
of a surface record against the oracle's own hit, rt_scene_deform_table's layout, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import ref_deform_binding as db
import ref_motion_binding as mb
import ref_refit_binding as rb
import ref_temporal_binding as tb

F = np.float32


def same(a, b):
    return np.array_equal(tb.bits(a), tb.bits(b))


# ---- 1. no deformed entry: the motion stage

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_no_deformed_entry_equals_the_motion_checker(rt, w, h, amount):
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p = tb.params()
    still = db.host_table(tp, arrays)
    still["deformed"] = 0                                   # the pointers and counts stay: nothing may look at them
    for moments in (False, True):
        for velocity in (False, True):
            want = mb.accumulate_motion(cur, g, prev, cam, amount, p, moving, want_moments=moments, want_velocity=velocity)
            for table, s in ((None, None), (None, surf), (still, surf), (still[:0], surf)):
                got = db.accumulate_deform(cur, g, prev, cam, amount, p, moving, s, table, want_moments=moments,
                                           want_velocity=velocity)
                for a, b in zip(got, want):
                    assert (a is None) == (b is None) and (a is None or same(a, b))
    # and the deforming table is another stage: the case can tell them apart, and its deformed pixels keep a history
    want = mb.accumulate_motion(cur, g, prev, cam, amount, p, moving)
    got = db.checked(w, h, amount, False, False)
    ids = g["primitive"]
    deformed = np.isin(ids, list(db.DEFORMED)) & (surf["triangle"] < w*h)
    changed = int(np.count_nonzero(tb.bits(got[1]) != tb.bits(want[1])))
    kept = int(np.count_nonzero(got[1][deformed] > 1.0))
    print(f"{w}x{h}: {int(deformed.sum())} deformed pixels, {kept} with a history; lengths that differ from the motion stage's: {changed}")
    assert changed >= 10 and kept > 20
    assert same(got[1][~deformed], want[1][~deformed]) and same(got[0][~deformed], want[0][~deformed])
    # without history: velocity is NaN everywhere, whatever the table
    _, length, _, vel = db.accumulate_deform(cur, g, None, None, 0.0, p, moving, surf, db.host_table(tp, arrays), want_velocity=True)
    assert (tb.bits(vel) == 0x7FC00000).all() and set(np.unique(length)) <= {0.0, 1.0}


def test_velocity_of_a_deformed_pixel_is_the_projection_of_its_surface_point(rt):
    w, h, amount = tb.SIZES[0]
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    _, _, _, vel = db.checked(w, h, amount, False, True)
    ids = g["primitive"]
    for k, (tris, nrm) in arrays.items():
        here = (ids == k) & (surf["triangle"] < w*h) & ~np.isnan(vel).any(axis=2)
        Q, _ = db.surface(tris, nrm, tp["forward"][k], tp["inverse"][k], surf["triangle"][here], surf["v"][here], surf["w"][here])
        ok, fx, fy = tb.project_many(cam, amount, Q, w, h)
        ys, xs = np.nonzero(here)
        assert here.sum() > 20 and ok.all() and same(vel[here][:, 0], fx - xs.astype(F)) and same(vel[here][:, 1], fy - ys.astype(F))


# ---- 2. a rigid motion written as a deformation, against float64

def test_rigid_deformation_against_float64(rt):
    """Vertices x moved by T (an identity instance): the current frame holds T_cur x, the previous one T_prev x, each
    rounded to float32.  Q of the checker (the kernel's, bit for bit) for the surface point P = (v, w) of the current
    triangle against T_prev . T_cur^-1 . P in float64 from the unrounded parameters.  The bound is 4 x the largest error
    the float64 model shows for rounding the inputs alone: the same barycentric sum in float64 arithmetic from the
    float32 vertices and barycentrics.  Measured (this seed; |Q| reaches 560 under the 56-fold scales): observed 3.15e-5,
    the inputs' own 1.72e-5, so the bound is 6.88e-5 ("Deforming meshes keep their history")."""
    rng = np.random.default_rng(2024)
    observed = inputs = 0.0
    ident = np.eye(4, dtype=F)
    for kind in ("t", "ry", "s"):
        for _ in range(40):
            if kind == "t":
                vc, vp = rng.uniform(-8.0, 8.0, 3), rng.uniform(-8.0, 8.0, 3)
            elif kind == "ry":
                vc, vp = rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi)
            else:
                vc, vp = rng.uniform(0.25, 14.0), rng.uniform(0.25, 14.0)
            x = rng.uniform(-10.0, 10.0, (64, 1, 3)) + rng.uniform(-1.0, 1.0, (64, 3, 3))      # 64 triangles, object space
            Tc, Tp = mb.m64(kind, vc), mb.m64(kind, vp)
            now = (x @ Tc[:3, :3].T + Tc[:3, 3]).astype(F)
            before = (x @ Tp[:3, :3].T + Tp[:3, 3]).astype(F)
            v = rng.uniform(0.0, 1.0, 64).astype(F)
            w = (rng.uniform(0.0, 1.0, 64)*(1.0 - v)).astype(F)
            tri = np.arange(64, dtype=np.uint32)
            P, _ = db.surface(now, None, ident, ident, tri, v, w)                                # the current frame's point
            exact = (Tp @ np.linalg.inv(Tc))[:3]
            want = P.astype(np.float64) @ exact[:, :3].T + exact[:, 3]
            b64, v64, w64 = before.astype(np.float64), v.astype(np.float64)[:, None], w.astype(np.float64)[:, None]
            rounded = b64[:, 0] + v64*(b64[:, 1] - b64[:, 0]) + w64*(b64[:, 2] - b64[:, 0])
            Q, _ = db.surface(before, None, ident, ident, tri, v, w)
            inputs = max(inputs, float(np.abs(rounded - want).max()))
            observed = max(observed, float(np.abs(Q.astype(np.float64) - want).max()))
    bound = 4.0*inputs
    print(f"rigid deformation: observed max |Q - Q64| {observed:.3e}, the inputs' own rounding {inputs:.3e}, bound {bound:.3e}")
    assert inputs > 0.0 and observed <= bound


# ---- 3. the normal of a surface record is hit_geometry's

def oracle_records(desc, prim, tris, rays, hits):
    """(triangle, v, w) of the oracle's hits on mesh primitive `prim`: ray_intersect_triangle (oracle.c) restated in
    float32 numpy over every triangle of the mesh in its original order, for the object-space ray the oracle makes.  A
    ray is kept when exactly one triangle gives the oracle's t, bit for bit."""
    inv = np.frombuffer(bytes(desc.transforms[desc.primitives[prim].transform_index].inverse), F).reshape(4, 4)
    a, b, c = (np.ascontiguousarray(tris[:, k, :], F) for k in range(3))
    e1, e2 = b - a, c - a
    dot = lambda p, q: p[..., 0]*q[..., 0] + p[..., 1]*q[..., 1] + p[..., 2]*q[..., 2]
    cross = lambda p, q: np.stack([p[..., 1]*q[..., 2] - p[..., 2]*q[..., 1], p[..., 2]*q[..., 0] - p[..., 0]*q[..., 2],
                                   p[..., 0]*q[..., 1] - p[..., 1]*q[..., 0]], axis=-1)
    out = []
    with np.errstate(all="ignore"):
        for r, hit in zip(rays, hits):
            if hit.primitive != prim:
                continue
            ro = np.array([r.o.x, r.o.y, r.o.z], F)
            rd = np.array([r.d.x, r.d.y, r.d.z], F)
            xf = lambda p, pw: np.array([p[0]*inv[k, 0] + p[1]*inv[k, 1] + p[2]*inv[k, 2] + F(pw)*inv[k, 3] for k in range(3)], F)
            o, d = xf(ro, 1.0), xf(rd, 0.0)
            pvec = cross(np.broadcast_to(d, e2.shape), e2)
            det = dot(e1, pvec)
            inv_det = F(1.0)/det
            tvec = o - a
            v = dot(tvec, pvec)*inv_det
            qvec = cross(tvec, e1)
            w = dot(np.broadcast_to(d, qvec.shape), qvec)*inv_det
            t = dot(e2, qvec)*inv_det
            ok = (np.abs(det) >= F(1e-9)) & (v >= 0) & (v <= 1) & (w >= 0) & (v + w <= 1) & (tb.bits(t) == tb.bits(F(hit.t)))
            at = np.nonzero(ok)[0]
            if at.size == 1:
                out.append((int(at[0]), v[at[0]], w[at[0]], hit))
    return out


@pytest.mark.parametrize("second_normals", [True, False], ids=["normals", "no-normals"])
def test_surface_normal_is_the_oracles(rt, second_normals):
    """Mesh 0 (with normals, two instances, one rotated about y) and mesh 1 with or without normals: for every oracle
    hit whose triangle and barycentrics the float32 restatement pins, the checker's normal from the mesh's original-
    order arrays and the primitive's inverse equals the oracle's, bit for bit."""
    W, H = 128, 96
    tris, nrm = rb.generated(1)
    t2, n2 = rb.generated(1, seed=5)
    s = rt.Scene()
    grey = s.add_diffuse_material((0.7, 0.6, 0.5), 1.5)
    s.add_plane(grey, (0.0, 1.0, 0.0), -0.5)
    m0 = s.create_mesh(tris, nrm, rt.abi.RTH_BVH_SAH_BINNED)
    m1 = s.create_mesh(t2, n2 if second_normals else None)
    prims = {s.add_mesh(grey, m0, rt.translate((-2.2, 0.0, 6.0))*rt.scale(2.0)): (tris, nrm),
             s.add_mesh(grey, m0, rt.translate((0.8, 0.2, 7.0))*rt.rotate_y(0.7)*rt.scale(2.0)): (tris, nrm),
             s.add_mesh(grey, m1, rt.translate((-0.5, 2.2, 8.0))*rt.scale(1.5)): (t2, n2 if second_normals else None)}
    s.create_scene_bvh()
    cam = rt.abi.Camera()
    cam.vfov, cam.aspect_ratio, cam.lens_radius, cam.focus_distance = rt.DEG_TO_RAD*28.0, W/H, 0.0, 8.0
    cam.p = rt.v3(0.0, 1.5, -3.0)
    rt.aim_camera_at(cam, (0.0, 1.0, 7.0))
    rt.recompute_camera(cam)
    d = tb.gbuffer_rays(cam, 0.0, W, H).reshape(-1, 3)
    rays = [rt.abi.RayQuery(cam.p, rt.v3(*[float(v) for v in d[i]]), 3.0e38, 0) for i in range(len(d))]
    desc = s.desc()
    hits = ob.intersect(desc, rays)
    total = 0
    for prim, (t, n) in prims.items():
        recs = oracle_records(desc, prim, t, rays, hits)
        inv = np.frombuffer(bytes(desc.transforms[desc.primitives[prim].transform_index].inverse), F).reshape(4, 4)
        _, got = db.surface(t, n, np.eye(4, dtype=F), inv, [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
        want = np.array([[r[3].n.x, r[3].n.y, r[3].n.z] for r in recs], F)
        print(f"primitive {prim}: {len(recs)} pinned hits")
        assert len(recs) >= 40 and same(got, want) and np.abs(np.linalg.norm(want, axis=1) - 1.0).max() < 1e-5
        total += len(recs)
    assert total > 300


# ---- 4. layouts and refusals that need no device

def test_layouts(rt):
    abi = rt.abi
    assert C.sizeof(abi.SurfaceTexel) == 16 == np.dtype(abi.SURFACE_DTYPE).itemsize
    assert C.sizeof(abi.DeformEntry) == 128 == np.dtype(abi.DEFORM_DTYPE).itemsize
    assert C.sizeof(abi.DeformMesh) == 24
    for name, _ in abi.DeformEntry._fields_:
        assert getattr(abi.DeformEntry, name).offset == np.dtype(abi.DEFORM_DTYPE).fields[name][1]
    motion, surf, table = (rt.temporal_motion_workspace_bytes(130, 70, 5), 16*130*70, 128*5)
    assert rt.temporal_deform_workspace_bytes(130, 70, 5) == (motion + 15)//16*16 + surf + table
    assert rt.temporal_deform_workspace_bytes(3, 3, 0) >= rt.temporal_motion_workspace_bytes(3, 3, 0) + 16*9


def refused(rt, code, text):
    assert code == rt.abi.RT_ERROR_INVALID
    message = rt.lib().rt_last_error().decode()
    assert text in message, message


def test_refusals_by_name(rt):
    lib, abi = rt.lib(), rt.abi
    w, h = 4, 3
    p = tb.params()
    buf, other, third = ((C.c_float*(w*h*8))() for _ in range(3))
    cam = tb.make_camera()
    motion, entries = (abi.MotionEntry*2)(), (abi.DeformEntry*2)()
    ptr = lambda a: C.cast(a, C.c_void_p)

    def stage(**kw):
        a = dict(current=ptr(buf), gbuffer=ptr(buf), ph=None, pl=None, pg=None, cam=C.byref(cam), p=C.byref(p), hist=ptr(other),
                 length=ptr(other), motion=None, count=0, pm=None, moments=None, vel=None, w=w, h=h, surf=None, deform=None,
                 dcount=0)
        a.update(kw)
        return lib.rt_temporal_accumulate_deform_device(0, a["current"], a["gbuffer"], a["ph"], a["pl"], a["pg"], a["cam"], 0.0,
                                                        a["w"], a["h"], a["p"], a["hist"], a["length"], None, a["motion"],
                                                        a["count"], a["pm"], a["moments"], a["vel"], a["surf"], a["deform"],
                                                        a["dcount"])
    e = "rt_temporal_accumulate_deform_device: "
    # the motion stage's
    refused(rt, stage(current=None), e + "null d_current")
    refused(rt, stage(gbuffer=None), e + "null d_gbuffer")
    refused(rt, stage(hist=None), e + "null d_history")
    refused(rt, stage(length=None), e + "null d_length")
    refused(rt, stage(w=0), e + "w is 0")
    refused(rt, stage(h=0), e + "h is 0")
    refused(rt, stage(p=None), e + "null rt_temporal_params")
    refused(rt, stage(ph=ptr(buf)), e + "null d_prev_length beside other previous buffers")
    refused(rt, stage(ph=ptr(other), pl=ptr(buf), pg=ptr(buf)), e + "d_history aliases d_prev_history")
    refused(rt, stage(ph=ptr(buf), pl=ptr(buf), pg=ptr(buf), cam=None), e + "null prev_camera with a history")
    refused(rt, stage(count=2), e + "null d_motion with a motion_count")
    refused(rt, stage(motion=ptr(motion), count=0x80000000), e + "motion_count must be below 2^31")
    refused(rt, stage(pm=ptr(buf)), e + "d_prev_moments without d_moments")
    refused(rt, stage(ph=ptr(buf), pl=ptr(buf), pg=ptr(buf), moments=ptr(third)),
            e + "null d_prev_moments beside other previous buffers")
    refused(rt, stage(p=C.byref(tb.params(snap=-1.0))), e + "rt_temporal_params: snap must be finite and >= 0")
    # its own
    refused(rt, stage(dcount=2), e + "null d_deform with a deform_count")
    refused(rt, stage(deform=ptr(entries), dcount=0x80000000, surf=ptr(buf)), e + "deform_count must be below 2^31")
    refused(rt, stage(deform=ptr(entries), dcount=2), e + "null d_surface with a deform table")
    fp, gp = C.POINTER(C.c_float), C.POINTER(abi.GBufferTexel)
    code = lib.rt_temporal_accumulate_deform(0, C.cast(buf, fp), C.cast(buf, gp), None, None, None, C.byref(cam), 0.0, w, h,
                                             C.byref(p), C.cast(other, fp), C.cast(other, fp), None, 0, None, None, None, None,
                                             entries, 2)
    refused(rt, code, "rt_temporal_accumulate_deform: null surface with a deform table")
    # the surface G-buffer and the table without a scene
    refused(rt, lib.rt_gbuffer_surface_device(None, C.byref(cam), 0.0, w, h, ptr(buf), ptr(other), None),
            "rt_gbuffer_surface_device: null scene")
    refused(rt, lib.rt_gbuffer_surface_device(None, C.byref(cam), 0.0, w, h, None, ptr(other), None),
            "rt_gbuffer_surface_device: null d_out")
    refused(rt, lib.rt_gbuffer_surface_device(None, None, 0.0, w, h, ptr(buf), ptr(other), None),
            "rt_gbuffer_surface_device: null camera")
    refused(rt, lib.rt_gbuffer_surface_device(None, C.byref(cam), 0.0, 0, h, ptr(buf), ptr(other), None),
            "rt_gbuffer_surface_device: w is 0")
    refused(rt, lib.rt_gbuffer_surface(None, C.byref(cam), 0.0, w, h, None, None), "rt_gbuffer_surface: null out")
    one = (abi.M4x4Inv*1)()
    refused(rt, lib.rt_scene_deform_table(None, 0, None, 1, one, entries), "rt_scene_deform_table: null scene")
    # the driver: rt_render_temporal_motion_device's order, the parameters first and the scene last
    state = abi.TemporalMotionState()
    st, _ = rt.default_settings()
    fc = rt.load_reconstruction_kernel("Box")
    tiles = abi.TileSet(64, 64, 0, 1)

    def driver(**kw):
        a = dict(p=C.byref(p), state=C.byref(state), st=C.byref(st), cam=C.byref(cam), fc=C.byref(fc), tiles=C.byref(tiles),
                 out=ptr(buf), w=w, h=h)
        a.update(kw)
        return lib.rt_render_temporal_deform_device(None, a["cam"], a["st"], a["fc"], a["tiles"], 0, a["w"], a["h"], 0, a["p"],
                                                    a["state"], 0, None, a["out"], None, None, None)
    e = "rt_render_temporal_deform_device: "
    refused(rt, driver(p=None), e + "null rt_temporal_params")
    refused(rt, driver(state=None), e + "null rt_temporal_motion_state")
    refused(rt, driver(), e + "rt_temporal_motion_state: null d_workspace")
    state.d_workspace = C.addressof(buf)
    refused(rt, driver(), e + "rt_temporal_motion_state: null transforms")
    state.transforms = C.cast(one, C.POINTER(abi.M4x4Inv))
    state.parity = 2
    refused(rt, driver(), e + "rt_temporal_motion_state: parity must be 0 or 1")
    state.parity = 0
    refused(rt, driver(st=None), e + "null settings")
    refused(rt, driver(w=0), e + "w is 0")
    refused(rt, driver(cam=None), e + "null camera")
    refused(rt, driver(fc=None), e + "null filter")
    refused(rt, driver(tiles=None), e + "null tiles")
    refused(rt, driver(out=None), e + "null d_out")
    refused(rt, driver(), e + "null scene")
    code = lib.rt_render_temporal_deform(None, C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), 0, w, h, 0, C.byref(p),
                                         C.byref(state), 0, None, None, None, None)
    refused(rt, code, "rt_render_temporal_deform: null out_pixels")
