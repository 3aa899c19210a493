"""Moving instances on the CPU: the checker of the motion table and of the motion-aware accumulate stage
(tests/ref_motion) against the checkers it extends, the product's table and host model, the float64 model of the
carried point, and every refusal of the new entries that needs no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import ref_motion_binding as mb
import ref_svgf_binding as sb
import ref_temporal_binding as tb

F = np.float32


def same(a, b):
    return np.array_equal(tb.bits(a), tb.bits(b))


# ---- 1. an unmoved table is the stage that was

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_unmoved_table_equals_the_plain_checkers(rt, w, h, amount):
    cur, g, prev, cam, _, unmoved = mb.motion_case(w, h, amount)
    p = tb.params()
    want_hist, want_len = tb.accumulate(cur, g, prev[:3], cam, amount, p)
    mh, ml, mm = sb.accumulate_moments(cur, g, prev, cam, amount, p)
    assert same(mh, want_hist) and same(ml, want_len)
    for table in (None, unmoved):
        hist, length, none, vel = mb.accumulate_motion(cur, g, prev[:3], cam, amount, p, table, want_velocity=True)
        assert none is None and same(hist, want_hist) and same(length, want_len)
        hist, length, mom, _ = mb.accumulate_motion(cur, g, prev, cam, amount, p, table, want_moments=True)
        assert same(hist, want_hist) and same(length, want_len) and same(mom, mm)
    # and the moving table is another stage: the case can tell them apart
    hist, length, _, _ = mb.checked(w, h, amount, False, False)
    changed = int(np.count_nonzero(tb.bits(length) != tb.bits(want_len)))
    print(f"{w}x{h}: pixels whose length differs under the moving table: {changed}")
    assert changed > 20
    # without history: velocity is NaN everywhere, whatever the table
    _, length, _, vel = mb.accumulate_motion(cur, g, None, None, 0.0, p, unmoved, want_velocity=True)
    assert (tb.bits(vel) == 0x7FC00000).all() and set(np.unique(length)) <= {0.0, 1.0}


def test_velocity_is_the_projection_minus_the_pixel(rt):
    w, h, amount = tb.SIZES[0]
    cur, g, prev, cam, moving, _ = mb.motion_case(w, h, amount)
    _, length, _, vel = mb.checked(w, h, amount, False, True)
    nan = np.isnan(vel).all(axis=2)
    assert (np.isnan(vel).any(axis=2) == nan).all() and (tb.bits(vel[nan]) == 0x7FC00000).all()
    assert nan[length == 0.0].all() and 0.02 < nan.mean() < 0.6
    # an unmoved hit's velocity is the plain projection of its point
    ids = g["primitive"]
    plain = (ids == 2) & ~nan
    ok, fx, fy = tb.project_many(cam, amount, g["p"][plain], w, h)
    ys, xs = np.nonzero(plain)
    assert ok.all() and same(vel[plain][:, 0], fx - xs.astype(F)) and same(vel[plain][:, 1], fy - ys.astype(F))
    # a moved hit's is the projection of the carried point
    moved = (ids == 3) & ~nan
    Q, _ = mb.carry(moving[3], g["p"][moved], g["n"][moved])
    ok, fx, fy = tb.project_many(cam, amount, Q, w, h)
    ys, xs = np.nonzero(moved)
    assert moved.sum() > 20 and ok.all() and same(vel[moved][:, 0], fx - xs.astype(F))


# ---- 2. rt_motion_table

def test_motion_table_against_the_checker(rt):
    cur, prev = mb.six_transforms()
    got, want = rt.motion_table(cur, prev), mb.table(cur, prev)
    assert got.dtype.itemsize == 112 == C.sizeof(rt.abi.MotionEntry)
    assert got.tobytes() == want.tobytes()
    assert list(got["moved"]) == [0, 1, 0, 1, 1, 0] and not got["reserved"].any()
    assert same(got["inv_cur"], cur["inverse"][:, :3, :]) and same(got["fwd_prev"], prev["forward"][:, :3, :])
    assert not rt.motion_table(cur, cur)["moved"].any()
    # one ulp in any single word of the 24 moves the entry; row 3 is not looked at
    one = cur[4:5]
    for field in ("forward", "inverse"):
        for r in range(4):
            for c in range(4):
                other = one.copy()
                word = other[field][0, r:r + 1, c].view(np.uint32)
                word += 1
                got = rt.motion_table(other, one)
                assert got.tobytes() == mb.table(other, one).tobytes()
                assert got["moved"][0] == (1 if r < 3 else 0), (field, r, c)
    assert rt.motion_table(cur[:0], prev[:0]).shape == (0,)


# ---- 3. the carried point against float64

def test_carried_point_against_float64(rt):
    """Q of the checker (the kernel's, bit for bit) against F_prev . F_cur^-1 . P in float64 from the unrounded
    parameters.  The bound is 4 x the largest error that the float64 model shows for rounding the inputs alone: the
    same product in float64 arithmetic from the float32 table.  Measured (this seed; |Q| reaches 560 under the 56-fold scales):
    observed 3.85e-5, the inputs' own 1.83e-5, so the bound is 7.30e-5 ("Moving instances")."""
    rng = np.random.default_rng(2024)
    observed = inputs = 0.0
    for kind in ("t", "ry", "s"):
        for _ in range(40):
            if kind == "t":
                vc, vp = rng.uniform(-8.0, 8.0, 3), rng.uniform(-8.0, 8.0, 3)
            elif kind == "ry":
                vc, vp = rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi)
            else:
                vc, vp = rng.uniform(0.25, 14.0), rng.uniform(0.25, 14.0)
            P = rng.uniform(-10.0, 10.0, (64, 3)).astype(F)
            n = rng.normal(size=(64, 3)).astype(F)
            exact = (mb.m64(kind, vp) @ np.linalg.inv(mb.m64(kind, vc)))[:3]
            want = P.astype(np.float64) @ exact[:, :3].T + exact[:, 3]
            cur, prev = mb.transforms(mb.product_transform(kind, vc)), mb.transforms(mb.product_transform(kind, vp))
            entry = rt.motion_table(cur, prev)[0]
            assert entry["moved"] == 1
            a, b = entry["inv_cur"].astype(np.float64), entry["fwd_prev"].astype(np.float64)
            po = P.astype(np.float64) @ a[:, :3].T + a[:, 3]
            rounded = po @ b[:, :3].T + b[:, 3]
            Q, m = mb.carry(entry, P, n)
            inputs = max(inputs, float(np.abs(rounded - want).max()))
            observed = max(observed, float(np.abs(Q.astype(np.float64) - want).max()))
            # a rigid motion or a uniform scale keeps the normal's direction up to the rotation
            r = exact[:, :3]/np.cbrt(np.linalg.det(exact[:, :3]))
            wn = n.astype(np.float64) @ r.T
            wn /= np.linalg.norm(wn, axis=1, keepdims=True)
            assert np.abs(m - wn).max() < 1e-5 and np.abs(np.linalg.norm(m.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    bound = 4.0*inputs
    print(f"carried point: observed max |Q - Q64| {observed:.3e}, the inputs' own rounding {inputs:.3e}, bound {bound:.3e}")
    assert inputs > 0.0 and observed <= bound
    # a normal that the 3 x 3 parts send to zero is kept
    e = rt.motion_table(mb.transforms(rt.translate((1.0, 0.0, 0.0))), mb.transforms(rt.identity()))
    e["fwd_prev"][0, :, :3] = 0.0
    Q, m = mb.carry(e[0], np.zeros((1, 3), F), np.array([[0.0, 0.6, 0.8]], F))
    assert same(m, np.array([[0.0, 0.6, 0.8]], F))


# ---- 4. a face translated toward the camera, in closed form

def test_translated_front_face_finds_its_previous_pixel(rt):
    """A face z = const facing a camera at the origin that looks along -z moves from depth d0 to d1 < d0.  The point
    seen at pixel x now was at w/2 - (w/2 - x) * d1/d0 then (similar triangles; no lens distortion), and the face's
    history follows although it moved by far more than the plane tolerance allows."""
    w, h, d0, d1 = 64, 36, 6.0, 5.0
    cam = tb.make_camera(aspect=w/h)
    qx, qy = np.meshgrid(np.arange(w), np.arange(h))

    def face(depth):
        g = np.zeros((h, w), tb.dtype())
        g["p"] = tb.point_at(cam, 0.0, w, h, qx.reshape(-1), qy.reshape(-1), np.full(w*h, depth)).reshape(h, w, 3)
        g["t"] = np.linalg.norm(g["p"], axis=2)
        g["n"] = (0.0, 0.0, 1.0)
        g["primitive"] = 1
        return g
    g0, g1 = face(d0), face(d1)
    # the object's own frame has the face at z = -1; the translations put it at -d0, then -d1
    cur = mb.transforms(rt.identity(), rt.translate((0.0, 0.0, 1.0 - d1)))
    prev = mb.transforms(rt.identity(), rt.translate((0.0, 0.0, 1.0 - d0)))
    motion = rt.motion_table(cur, prev)
    current = np.ones((h, w, 4), F)
    ph = np.concatenate([np.full((h, w, 3), 3.0, F), np.ones((h, w, 1), F)], axis=2)
    pl = np.full((h, w), 5.0, F)
    p = tb.params()
    assert (d0 - d1) > p.plane_tolerance*g1["t"].max()
    hist, length, _, vel = mb.accumulate_motion(current, g1, (ph, pl, g0), cam, 0.0, p, motion, want_velocity=True)
    want_x = w/2 - (w/2 - qx)*d1/d0
    want_y = h/2 - (h/2 - qy)*d1/d0
    err = max(float(np.abs(vel[..., 0] + qx - want_x).max()), float(np.abs(vel[..., 1] + qy - want_y).max()))
    print(f"translated face: previous pixel against the closed form, max error {err:.3e} pixels (snap {p.snap})")
    assert err <= p.snap
    # every tap counts: the history is the previous one's 3 blended with the current 1 at length 5 + 1 (the four
    # bilinear weights sum to 1 within an ulp or two)
    assert np.abs(length - 6.0).max() < 1e-5 and np.abs(hist[..., :3] - (3.0 - 2.0/6.0)).max() < 1e-5
    # the stage without the table looks where the point is now and finds the face 1 unit behind it: no history
    _, plain, _, _ = mb.accumulate_motion(current, g1, (ph, pl, g0), cam, 0.0, p, None)
    assert (plain == 1.0).all()


# ---- 5. the host model

def rebuilt(rt, scene, moved_id, transform):
    """A scene built through the public builder from `scene`'s desc (spheres, boxes and planes only), primitive
    `moved_id` with `transform` from the start."""
    d = scene.desc()
    assert d.mesh_count == 0
    s = rt.Scene()
    for i in range(1, d.material_count):
        assert lib_add_material(rt, s, d.materials[i]) == i
    for i in range(d.plane_count):
        q = d.planes[i]
        s.add_plane(q.material_id, (q.p[0], q.p[1], q.p[2]), q.p[3])
    for i in range(1, d.primitive_count):
        q = d.primitives[i]
        t = transform if i == moved_id else (None if q.transform_index == 0 else
                                             rt.abi.M4x4Inv.from_buffer_copy(d.transforms[q.transform_index]))
        if q.type == rt.abi.RT_PRIMITIVE_SPHERE:
            pid = s.add_sphere(q.material_id, q.p[0], t)
        else:
            assert q.type == rt.abi.RT_PRIMITIVE_BOX
            pid = s.add_box(q.material_id, (q.p[0], q.p[1], q.p[2]), t)
        assert pid == i
    s.set_sky(tuple(d.top_sky_color), tuple(d.bot_sky_color))
    s.create_scene_bvh()
    return s


def lib_add_material(rt, s, m):
    return rt.lib().rth_add_material(s.handle, C.byref(m))


def test_host_model_moves_a_primitive(rt, oracle):
    w = h = 64
    scene, cam, st, fc, _ = rt.load_preset("c1", w, h)
    st.samples_per_pixel = 1
    before = scene.desc()
    count, moved_id = before.transform_count, 3
    t = rt.translate((1.5, 3.0, -6.0))
    first, _ = ob.render(before, cam, st, fc, w, h, rng_mode=0, threads=4)
    scene.set_primitive_transform(moved_id, t)
    scene.create_scene_bvh()
    d = scene.desc()
    assert d.transform_count == count                      # the sphere had a slot of its own
    assert bytes(d.transforms[d.primitives[moved_id].transform_index]) == bytes(t)
    got, _ = ob.render(d, cam, st, fc, w, h, rng_mode=0, threads=4)
    fresh = rebuilt(rt, scene, moved_id, t)
    want, _ = ob.render(fresh.desc(), cam, st, fc, w, h, rng_mode=0, threads=4)
    assert same(got, want) and not same(got, first)
    # a primitive on the shared identity slot gets one of its own; the others keep the identity
    s = rt.Scene()
    m = s.add_diffuse_material((0.5, 0.5, 0.5), 1.0)
    a, b = s.add_sphere(m, 1.0), s.add_sphere(m, 1.0)
    s.set_primitive_transform(a, t)
    s.create_scene_bvh()
    d = s.desc()
    assert d.transform_count == 2 and d.primitives[a].transform_index == 1 and d.primitives[b].transform_index == 0
    assert bytes(d.transforms[0]) == bytes(rt.identity()) and bytes(d.transforms[1]) == bytes(t)
    for bad in (0, 3, 99):
        with pytest.raises(ValueError, match="primitive id out of range"):
            s.set_primitive_transform(bad, t)


# ---- 6. refusals by name, none of which needs a device

def refused(rt, code, text):
    assert code == rt.abi.RT_ERROR_INVALID
    message = rt.lib().rt_last_error().decode()
    assert text in message, message


def test_refusals_by_name(rt):
    lib, abi = rt.lib(), rt.abi
    w, h = 4, 3
    p = tb.params()
    buf = (C.c_float*(w*h*8))()
    other = (C.c_float*(w*h*8))()
    third = (C.c_float*(w*h*8))()
    cam = tb.make_camera()
    entries = (abi.MotionEntry*2)()
    ptr = lambda a: C.cast(a, C.c_void_p)

    def stage(**kw):
        a = dict(current=ptr(buf), gbuffer=ptr(buf), ph=None, pl=None, pg=None, cam=C.byref(cam), p=C.byref(p), hist=ptr(other),
                 length=ptr(other), motion=None, count=0, pm=None, moments=None, vel=None, w=w, h=h)
        a.update(kw)
        return lib.rt_temporal_accumulate_motion_device(0, a["current"], a["gbuffer"], a["ph"], a["pl"], a["pg"], a["cam"], 0.0,
                                                        a["w"], a["h"], a["p"], a["hist"], a["length"], None, a["motion"],
                                                        a["count"], a["pm"], a["moments"], a["vel"])
    e = "rt_temporal_accumulate_motion_device: "
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
    refused(rt, stage(motion=ptr(entries), count=0x80000000), e + "motion_count must be below 2^31")
    refused(rt, stage(pm=ptr(buf)), e + "d_prev_moments without d_moments")
    refused(rt, stage(pm=ptr(buf), moments=ptr(third)), e + "null d_prev_history beside other previous buffers")
    refused(rt, stage(ph=ptr(buf), pl=ptr(buf), pg=ptr(buf), moments=ptr(third)),
            e + "null d_prev_moments beside other previous buffers")
    refused(rt, stage(ph=ptr(buf), pl=ptr(buf), pg=ptr(buf), moments=ptr(third), pm=ptr(third)),
            e + "d_moments aliases d_prev_moments")
    bad = tb.params(snap=-1.0)
    refused(rt, stage(p=C.byref(bad)), e + "rt_temporal_params: snap must be finite and >= 0")
    # the host twin names its buffers without the prefix
    fp, gp = C.POINTER(C.c_float), C.POINTER(abi.GBufferTexel)
    code = lib.rt_temporal_accumulate_motion(0, None, C.cast(buf, gp), None, None, None, C.byref(cam), 0.0, w, h, C.byref(p),
                                             C.cast(other, fp), C.cast(other, fp), None, 0, None, None, None)
    refused(rt, code, "rt_temporal_accumulate_motion: null current")
    code = lib.rt_temporal_accumulate_motion(0, C.cast(buf, fp), C.cast(buf, gp), None, None, None, C.byref(cam), 0.0, w, h,
                                             C.byref(p), C.cast(other, fp), C.cast(other, fp), None, 3, None, None, None)
    refused(rt, code, "rt_temporal_accumulate_motion: null motion with a motion_count")
    # the table, the transforms and the update
    one = (abi.M4x4Inv*1)()
    refused(rt, lib.rt_motion_table(1, None, one, entries), "rt_motion_table: null cur")
    refused(rt, lib.rt_motion_table(1, one, None, entries), "rt_motion_table: null prev")
    refused(rt, lib.rt_motion_table(1, one, one, None), "rt_motion_table: null out")
    assert lib.rt_motion_table(0, None, None, None) == 0
    n = C.c_uint32()
    refused(rt, lib.rt_scene_primitive_transforms(None, 0, None, C.byref(n)), "rt_scene_primitive_transforms: null scene")
    refused(rt, lib.rt_scene_update_instances(None, None), "rt_scene_update_instances: null scene")
    # the driver: the existing driver's order, the parameters first and the scene last
    state = abi.TemporalMotionState()
    st, _ = rt.default_settings()
    fc = rt.load_reconstruction_kernel("Box")
    tiles = abi.TileSet(64, 64, 0, 1)

    def driver(**kw):
        a = dict(p=C.byref(p), state=C.byref(state), st=C.byref(st), cam=C.byref(cam), fc=C.byref(fc), tiles=C.byref(tiles),
                 out=ptr(buf), w=w, h=h)
        a.update(kw)
        return lib.rt_render_temporal_motion_device(None, a["cam"], a["st"], a["fc"], a["tiles"], 0, a["w"], a["h"], 0, a["p"],
                                                    a["state"], a["out"], None, None, None)
    e = "rt_render_temporal_motion_device: "
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
    refused(rt, driver(h=0), e + "h is 0")
    refused(rt, driver(cam=None), e + "null camera")
    refused(rt, driver(fc=None), e + "null filter")
    refused(rt, driver(tiles=None), e + "null tiles")
    refused(rt, driver(out=None), e + "null d_out")
    refused(rt, driver(), e + "null scene")
    code = lib.rt_render_temporal_motion(None, C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), 0, w, h, 0, C.byref(p),
                                         C.byref(state), None, None, None)
    refused(rt, code, "rt_render_temporal_motion: null out_pixels")
    # sizes
    assert rt.temporal_motion_workspace_bytes(130, 70, 5) >= rt.temporal_workspace_bytes(130, 70) + 5*112
    assert rt.temporal_motion_workspace_bytes(3, 3, 0) >= rt.temporal_workspace_bytes(3, 3)
    assert C.sizeof(abi.TemporalMotionState) == rt_state_size(rt)


def rt_state_size(rt):
    """sizeof(rt_temporal_motion_state) as the C header lays it out: four words, the camera, three words, padding to
    8, two pointers."""
    head = 16 + C.sizeof(rt.abi.Camera) + 12
    return (head + 7)//8*8 + 16
