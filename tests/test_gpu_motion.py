"""Moving instances on the GPU: the motion-aware accumulate stage against its plain-C checker, rt_scene_update_instances
against a fresh upload, refused updates, the driver against the loop it is defined as, and a box that walks toward a
standing camera by more than the plane tolerance per frame."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import ref_motion_binding as mb
import ref_temporal_binding as tb
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 3          # total_frame_index of every frame here


def rays(s):
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def mismatches(a, b):
    return int(np.count_nonzero(tb.bits(host(a)) != tb.bits(host(b))))


def to_device(torch, a):
    """A host array (structured arrays as their 32-bit words) -> a device tensor."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.float32).reshape(a.shape + (a.dtype.itemsize//4,))
    d = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize(0)
    return d


def garbage(torch, *shape):
    d = torch.full(shape, -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    return d


def device_stage(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h, d_table, count, moments, velocity):
    """rt_temporal_accumulate_motion_device into outputs that start as garbage -> (history, length, moments, velocity)."""
    d_hist, d_len = garbage(torch, h, w, 4), garbage(torch, h, w)
    d_mom = garbage(torch, h, w, 2) if moments else None
    d_vel = garbage(torch, h, w, 2) if velocity else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    ph, pl, pg, pm = d_prev if d_prev is not None else (None, None, None, None)
    rt.temporal_accumulate_motion_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                         d_hist.data_ptr(), d_len.data_ptr(), d_motion=ptr(d_table), motion_count=count,
                                         d_prev_moments=ptr(pm) if moments else None, d_moments=ptr(d_mom),
                                         d_velocity=ptr(d_vel))
    return d_hist, d_len, d_mom, d_vel


# ---- 1. the stage against the checker

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_stage_matches_the_checker(rt, w, h, amount):
    import torch
    cur, g, prev, cam, moving, unmoved = mb.motion_case(w, h, amount)
    p = tb.params()
    d_cur, d_g = to_device(torch, cur), to_device(torch, g)
    d_prev = tuple(to_device(torch, a) for a in prev)
    d_moving, d_unmoved = to_device(torch, moving), to_device(torch, unmoved)
    bad = {}
    for moments in (False, True):
        for velocity in (False, True):
            got = device_stage(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), moments, velocity)
            want = mb.checked(w, h, amount, moments, velocity)
            assert (got[2] is None) == (want[2] is None) and (got[3] is None) == (want[3] is None)
            bad[(moments, velocity)] = sum(mismatches(a, b) for a, b in zip(got, want) if b is not None)
    print(f"{w}x{h}: words that differ from the checker", bad)
    REPORT[f"motion_stage_{w}x{h}"] = {str(k): v for k, v in bad.items()}
    assert not any(bad.values())
    # an unmoved table, no table and a table shorter than every id: rt_temporal_accumulate_device's output
    d_hist, d_len = garbage(torch, h, w, 4), garbage(torch, h, w)
    rt.temporal_accumulate_device(d_cur.data_ptr(), d_g.data_ptr(), d_prev[0].data_ptr(), d_prev[1].data_ptr(),
                                  d_prev[2].data_ptr(), cam, amount, w, h, p, d_hist.data_ptr(), d_len.data_ptr())
    for table, count in ((d_unmoved, len(unmoved)), (None, 0), (d_moving, 1)):
        got = device_stage(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h, table, count, False, True)
        assert mismatches(got[0], d_hist) == 0 and mismatches(got[1], d_len) == 0
    # and the moving table does change it
    got = device_stage(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), False, False)
    assert mismatches(got[1], d_len) > 20
    # without history: lengths 0 or 1, velocity NaN, the moments the current frame's
    got = device_stage(rt, torch, d_cur, d_g, None, None, 0.0, p, w, h, d_moving, len(moving), True, True)
    want = mb.accumulate_motion(cur, g, None, None, 0.0, p, moving, want_moments=True, want_velocity=True)
    assert sum(mismatches(a, b) for a, b in zip(got, want)) == 0
    # the host twin
    hh, hl, hm, hv = rt.temporal_accumulate_motion(cur, g, prev, cam, amount, p, moving, want_moments=True, want_velocity=True)
    want = mb.checked(w, h, amount, True, True)
    assert sum(mismatches(a, b) for a, b in zip((hh, hl, hm, hv), want)) == 0


# ---- 2. an update against a fresh upload

def stripped(rt, d):
    """A copy of a desc as rt_scene_update_instances may be given it: no material, sky or mesh array."""
    c = rt.abi.SceneDesc.from_buffer_copy(d)
    c.materials = None
    c.skydome = None
    meshes = (rt.abi.Mesh*max(1, d.mesh_count))()
    for m in range(d.mesh_count):
        meshes[m].triangle_count = d.meshes[m].triangle_count
        meshes[m].has_normals = d.meshes[m].has_normals
        meshes[m].node_count = d.meshes[m].node_count
    c.meshes = C.cast(meshes, C.POINTER(rt.abi.Mesh))
    c._keep = (meshes, d)
    return c


class Padded:
    """A desc with `extra` unused identity transforms behind its own; anything with desc() uploads."""

    def __init__(self, rt, d, extra):
        self.d = rt.abi.SceneDesc.from_buffer_copy(d)
        n = d.transform_count
        self.transforms = (rt.abi.M4x4Inv*(n + extra))(*([rt.abi.M4x4Inv.from_buffer_copy(d.transforms[i]) for i in range(n)] +
                                                        [rt.identity() for _ in range(extra)]))
        self.d.transforms, self.d.transform_count = C.cast(self.transforms, C.POINTER(rt.abi.M4x4Inv)), n + extra
        self.keep = d

    def desc(self):
        return self.d


def query_rays(rt, cam, w, h, count=256):
    d = tb.gbuffer_rays(cam, 0.0, w, h).reshape(-1, 3)
    step = max(1, len(d)//count)
    return [rt.abi.RayQuery(cam.p, rt.v3(*[float(v) for v in d[i]]), 3.0e38, 0) for i in range(0, len(d), step)]


def everything(rt, dev, cam, st, fc, w, h, queries):
    """What the two scenes must agree on: a frame and its ray counts, the G-buffer, closest hits and occlusion of a
    batch of rays, the stack depth and the resolved transforms."""
    frame, stats = dev.render(cam, st, fc, w, h, total_frame_index=TFI)
    return {"frame": frame, "rays": rays(stats), "gbuffer": dev.gbuffer(cam, w, h, st.lens_distortion).tobytes(),
            "hits": b"".join(bytes(r) for r in dev.intersect(queries)),
            "occluded": [r.primitive == rt.abi.RT_HIT_MISS for r in dev.intersect(queries, occlusion=True)],
            "depth": dev.stack_depth(), "transforms": dev.primitive_transforms().tobytes()}


def disagreements(a, b):
    return [k for k in a if not (np.array_equal(tb.bits(a[k]), tb.bits(b[k])) if k == "frame" else a[k] == b[k])]


UPDATES = {
    "c1": (130, 70, lambda rt: [
        {3: rt.translate((1.0, 2.0, -6.0))},
        {3: rt.translate((-1.0, 4.5, -2.0)), 2: rt.translate((-3.5, 2.3, -6.5))},
        {3: rt.translate((5.0, 2.0, 3.0))}]),
    "c4": (192, 108, lambda rt: [
        {2: rt.translate((-5.0, 3.7, 2.0))*rt.scale(6.0)},
        {2: rt.translate((-6.0, 4.2, 1.0))*rt.scale(6.0), 3: rt.translate((-5.0, 3.7, -7.0))*rt.rotate_y(0.6)*rt.scale(6.0)},
        {3: rt.translate((-5.0, 3.7, -7.0))*rt.rotate_y(-1.1)*rt.scale(6.0)}]),
}


@pytest.mark.parametrize("preset", ["c1", "c4"])
def test_update_equals_a_fresh_upload(rt, preset):
    w, h, moves = UPDATES[preset]
    scene, cam, st, fc, _ = rt.load_preset(preset, w, h)
    st.samples_per_pixel = 1
    d0 = scene.desc()
    original = {i: rt.abi.M4x4Inv.from_buffer_copy(d0.transforms[d0.primitives[i].transform_index]) for i in (2, 3)}
    queries = query_rays(rt, cam, w, h)
    dev = rt.DeviceScene(scene, 0)
    dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
    config = bytes(dev.config())
    try:
        first = everything(rt, dev, cam, st, fc, w, h, queries)
        steps = moves(rt) + [original]
        for k, step in enumerate(steps):
            for pid, t in step.items():
                scene.set_primitive_transform(pid, t)
            scene.create_scene_bvh()
            dev.update_instances(stripped(rt, scene.desc()))
            assert bytes(dev.config()) == config
            got = everything(rt, dev, cam, st, fc, w, h, queries)
            if k == len(steps) - 1:
                assert disagreements(got, first) == []          # back where it was: the first upload's frame
                break
            fresh = rt.DeviceScene(scene, 0)
            fresh.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
            try:
                want = everything(rt, fresh, cam, st, fc, w, h, queries)
            finally:
                fresh.close()
            assert disagreements(got, want) == [], (preset, k)
            assert disagreements(got, first) != []
            if k == 0:
                # a desc with more transforms than the tables on the device have room for: they are allocated anew
                wider = Padded(rt, scene.desc(), 5)
                dev.update_instances(stripped(rt, wider.desc()))
                fresh = rt.DeviceScene(wider, 0)
                fresh.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
                try:
                    want = everything(rt, fresh, cam, st, fc, w, h, queries)
                finally:
                    fresh.close()
                assert disagreements(everything(rt, dev, cam, st, fc, w, h, queries), want) == [], (preset, "wider")
            if k == 1:
                # and the oracle's frame of that desc: the exact splat sums in the reference's order
                cpu, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, total_frame_index=TFI)
                share = float(np.all(tb.bits(got["frame"]) == tb.bits(cpu), axis=2).mean())
                print(f"{preset}: updated scene against the oracle: pixels bit-identical {share:.5f}")
                REPORT[f"motion_update_oracle_{preset}"] = {"pixels_bit_identical": share}
                assert np.array_equal(tb.bits(got["frame"]), tb.bits(cpu))
    finally:
        dev.close()


# ---- 3. a refused update leaves the scene as it was

def copied(rt, d):
    """A desc whose primitive and top-level arrays are copies that a test may spoil."""
    c = rt.abi.SceneDesc.from_buffer_copy(d)
    prims = (rt.abi.Primitive*d.primitive_count)(*[rt.abi.Primitive.from_buffer_copy(d.primitives[i])
                                                    for i in range(d.primitive_count)])
    idx = (C.c_uint32*d.bvh_index_count)(*[d.bvh_indices[i] for i in range(d.bvh_index_count)])
    c.primitives = C.cast(prims, C.POINTER(rt.abi.Primitive))
    c.bvh_indices = C.cast(idx, C.POINTER(C.c_uint32))
    c._keep = (prims, idx, d)
    return c, prims, idx


def chain(rt, levels, index_count):
    """A top-level BVH2 that is one long chain: every interior node has a leaf and the next interior node."""
    nodes = (rt.abi.BvhNode*(2*levels + 2))()
    at = 0
    for k in range(levels):
        nodes[at].left_first, nodes[at].count = 2*k + 2, 0
        nodes[2*k + 2].left_first, nodes[2*k + 2].count = k % index_count, 1
        at = 2*k + 3
    nodes[at].left_first, nodes[at].count = 0, 1
    return nodes


def test_refused_update_leaves_the_scene_alone(rt):
    w, h = 130, 70
    scene, cam, st, fc, _ = rt.load_preset("c1", w, h)
    st.samples_per_pixel = 1
    queries = query_rays(rt, cam, w, h, 64)
    dev = rt.DeviceScene(scene, 0)
    dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
    try:
        before = everything(rt, dev, cam, st, fc, w, h, queries)
        d = scene.desc()
        cases = []
        c, prims, _ = copied(rt, d)
        prims[3].type = rt.abi.RT_PRIMITIVE_BOX
        cases.append((c, "primitive 3: type differs from the uploaded scene's"))
        c, _, idx = copied(rt, d)
        idx[d.bvh_index_count - 1] = d.primitive_count
        cases.append((c, "bvh index out of range"))
        c, _, _ = copied(rt, d)
        nodes = chain(rt, 70, d.bvh_index_count)
        c.bvh_nodes, c.bvh_node_count = C.cast(nodes, C.POINTER(rt.abi.BvhNode)), len(nodes)
        c._nodes = nodes
        cases.append((c, "rt_scene_update_instances: BVH too deep for the device's BVH4 traversal stack"))
        c, prims, _ = copied(rt, d)
        prims[2].p[0] = 2.5
        cases.append((c, "primitive 2: p differs from the uploaded scene's"))
        c, _, _ = copied(rt, d)
        c.plane_count -= 1
        cases.append((c, "plane_count differs from the uploaded scene's"))
        for c, text in cases:
            with pytest.raises(rt.RenderError) as e:
                dev.update_instances(c)
            assert e.value.code == rt.abi.RT_ERROR_INVALID and text in str(e.value), str(e.value)
            assert disagreements(everything(rt, dev, cam, st, fc, w, h, queries), before) == [], text
    finally:
        dev.close()


# ---- 4. the driver against the loop it is defined as

class Loop:
    """A scene on the device in the exact splat mode, with what a temporal loop needs."""

    def __init__(self, rt, scene, cam, st, fc, w, h):
        import torch
        self.rt, self.torch, self.scene, self.cam, self.st, self.fc, self.w, self.h = rt, torch, scene, cam, st, fc, w, h
        self.dev = rt.DeviceScene(scene, 0)
        self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        self.count = len(self.dev.primitive_transforms())

    def full(self, fill, *shape):
        d = self.torch.full(shape, fill, dtype=self.torch.float32, device="cuda:0")
        self.torch.cuda.synchronize(0)
        return d

    def frame(self, frame_count):
        d = self.full(0.0, self.h, self.w, 4)
        s = self.dev.render_device(self.cam, self.st, self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI,
                                   frame_count=frame_count)
        return d, s

    def gbuffer(self):
        d = self.full(float("nan"), self.h, self.w, 8)
        self.dev.gbuffer_device(self.cam, self.w, self.h, d.data_ptr(), lens_distortion=self.st.lens_distortion)
        return d

    def motion_state(self):
        """A fresh rt_temporal_motion_state over a workspace that starts as garbage -> (state, what it points at)."""
        n = self.rt.temporal_motion_workspace_bytes(self.w, self.h, self.count)
        ws = self.full(float("nan"), (n + 3)//4)
        store = (self.rt.abi.M4x4Inv*self.count)()
        st = self.rt.TemporalMotionState()
        st.d_workspace, st.transforms, st.transform_cap = ws.data_ptr(), C.cast(store, C.POINTER(self.rt.abi.M4x4Inv)), self.count
        return st, (ws, store)

    def plain_state(self):
        ws = self.full(float("nan"), self.rt.temporal_workspace_bytes(self.w, self.h)//4)
        st = self.rt.TemporalState()
        st.d_workspace = ws.data_ptr()
        return st, ws

    def motion_driver(self, frame_count, p, state):
        d_out, d_len = self.full(9.0, self.h, self.w, 4), self.full(9.0, self.h, self.w)
        s = self.dev.render_temporal_motion_device(self.cam, self.st, self.fc, self.w, self.h, p, state, d_out.data_ptr(),
                                                   d_length_out=d_len.data_ptr(), frame_count=frame_count,
                                                   total_frame_index=TFI)
        return d_out, d_len, s

    def plain_driver(self, frame_count, p, state):
        d_out, d_len = self.full(9.0, self.h, self.w, 4), self.full(9.0, self.h, self.w)
        self.dev.render_temporal_device(self.cam, self.st, self.fc, self.w, self.h, p, state, d_out.data_ptr(),
                                        d_length_out=d_len.data_ptr(), frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_len

    def move(self, step):
        for pid, t in step.items():
            self.scene.set_primitive_transform(pid, t)
        self.scene.create_scene_bvh()
        self.dev.update_instances()

    def close(self):
        self.dev.close()


def test_driver_equals_the_loop_on_the_public_entries(rt):
    import torch
    w, h = 130, 70
    scene, cam, st, fc, _ = rt.load_preset("c1", w, h)
    st.samples_per_pixel = 1
    loop = Loop(rt, scene, cam, st, fc, w, h)
    steps = [{3: rt.translate((3.0 - 0.3*k, 2.0 + 0.1*k, -4.0 - 0.2*k)), 1: rt.translate((-3.0, 3.0, 1.0))*rt.rotate_y(-0.39 + 0.02*k)}
             for k in (1, 2, 3)]
    try:
        p = tb.params()
        amount = st.lens_distortion
        state, keep = loop.motion_state()
        prev, prev_tr, bad, shares, moved = None, None, 0, [], []
        for k in range(4):
            if k:
                loop.move(steps[k - 1])
            # rt_render_temporal_motion_device's definition, on the public entries below it
            f, want_stats = loop.frame(k)
            g = loop.gbuffer()
            tr = loop.dev.primitive_transforms()
            if prev is None:
                want = device_stage(rt, torch, f, g, None, None, amount, p, w, h, None, 0, False, False)
            else:
                table = rt.motion_table(tr, prev_tr)
                moved.append(int(table["moved"].sum()))
                want = device_stage(rt, torch, f, g, prev + (None,), cam, amount, p, w, h, to_device(torch, table), len(table),
                                    False, False)
            got_hist, got_len, stats = loop.motion_driver(k, p, state)
            bad += mismatches(got_hist, want[0]) + mismatches(got_len, want[1])
            assert rays(stats) == rays(want_stats) and stats.samples == w*h
            assert (state.frames, state.parity, state.w, state.h, state.primitive_count) == (k + 1, (k + 1) % 2, w, h, loop.count)
            assert bytes(state.camera) == bytes(cam) and bytes(keep[1]) == tr.tobytes()
            prev, prev_tr = (want[0], want[1], g), tr
            shares.append(float((host(got_len) > 1).mean()))
        print("C1 motion driver: share of pixels with a history per frame", shares, "moved entries", moved)
        REPORT["motion_driver_c1"] = {"mismatches": bad, "share_with_history": shares, "moved": moved}
        assert bad == 0 and shares[0] == 0.0 and min(shares[1:]) > 0.5 and moved == [2, 2, 2]
        # a state of another primitive count restarts; the host entry
        state.primitive_count = loop.count + 1
        out, length, _ = loop.dev.render_temporal_motion(cam, st, fc, w, h, state, p, frame_count=4, total_frame_index=TFI)
        assert (length[np.isfinite(out).all(axis=2)] == 1.0).all() and state.frames == 5 and state.primitive_count == loop.count
        # too small a transform array is refused by name, and the state stays
        state.transform_cap = loop.count - 1
        with pytest.raises(rt.RenderError, match="transform_cap is below the scene's primitive count"):
            loop.dev.render_temporal_motion(cam, st, fc, w, h, state, p, frame_count=5, total_frame_index=TFI)
        assert state.frames == 5
        del keep
    finally:
        loop.close()


# ---- 5. a box that walks toward a standing camera

def box_scene(rt, z):
    """A wall facing the camera and a box in front of it, its front face at z - 0.5."""
    s = rt.Scene()
    m = s.add_diffuse_material((0.6, 0.5, 0.4), 1.5)
    s.add_plane(m, (0.0, 0.0, -1.0), -3.0)           # z = 3, facing -z
    box = s.add_box(m, (1.5, 1.0, 0.5), rt.translate((0.0, 1.0, z)))
    s.set_sky((0.6, 0.7, 0.9), (0.1, 0.1, 0.1))
    s.create_scene_bvh()
    return s, box


def eroded(mask):
    """The pixels whose 3 x 3 neighbourhood lies in the mask."""
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out &= np.roll(np.roll(mask, dy, 0), dx, 1)
    out[0, :] = out[-1, :] = False
    out[:, 0] = out[:, -1] = False
    return out


def texels(d):
    a = d.cpu().numpy()
    return a.view(tb.dtype()).reshape(a.shape[0], a.shape[1])


@pytest.mark.parametrize("snap", [0.5, None], ids=["nearest", "bilinear"])
def test_box_walking_toward_the_camera_keeps_its_history(rt, snap):
    """Four frames, the box 0.2 nearer in each: twice the plane tolerance at its distance (0.02 x 5.5).  The motion
    driver's history of the front face grows by one per frame; rt_render_temporal_device's restarts every frame, since
    it looks for the face where it is now.  With snap = 0.5 every position snaps to its nearest previous pixel, a
    single tap of weight 1, and the lengths are whole numbers exactly.  Under the default snap a length is
    sum(w L)/sum(w) over four bilinear taps, at most 8 roundings of 2^-24 each: within 4 x 8 x 2^-24 = 1.9e-6 of
    frame + 1 (the checker gives 3.9999998 to 4.0000005 at the fourth frame)."""
    w, h, zs = 96, 64, [1.0, 0.8, 0.6, 0.4]
    cam = rt.abi.Camera()
    cam.vfov, cam.aspect_ratio, cam.lens_radius, cam.focus_distance = rt.DEG_TO_RAD*50.0, w/h, 0.0, 10.0
    cam.p = rt.v3(0.0, 1.0, -5.0)
    rt.aim_camera_at(cam, (0.0, 1.0, 0.0))
    rt.recompute_camera(cam)
    st, _ = rt.default_settings()
    st.lens_distortion, st.samples_per_pixel, st.integrator = 0.0, 1, rt.abi.RT_INTEGRATOR_NORMALS
    fc = rt.load_reconstruction_kernel("Box")
    scene, box = box_scene(rt, zs[0])
    loop = Loop(rt, scene, cam, st, fc, w, h)
    try:
        p = tb.params() if snap is None else tb.params(snap=snap)
        mstate, keep = loop.motion_state()
        pstate, pws = loop.plain_state()
        g_prev, sizes = None, []
        for k, z in enumerate(zs):
            if k:
                loop.move({box: rt.translate((0.0, 1.0, z))})
            mh, ml, _ = loop.motion_driver(k, p, mstate)
            ph, pl = loop.plain_driver(k, p, pstate)
            g = texels(loop.gbuffer())
            face = (g["primitive"] == box) & (g["n"][..., 2] == -1.0)
            mask = eroded(face) & (eroded(g_prev) if g_prev is not None else True)
            if k:
                assert 0.2 > p.plane_tolerance*float(g["t"][mask].max())
            sizes.append(int(mask.sum()))
            ml, pl = host(ml), host(pl)
            print(f"frame {k}: mask {sizes[-1]} pixels, motion lengths {np.unique(ml[mask])}, plain {np.unique(pl[mask])}")
            assert sizes[-1] >= 200
            if snap is not None:
                assert (ml[mask] == k + 1).all()
            else:
                assert np.abs(ml[mask] - (k + 1)).max() <= 32*2.0**-24
            assert (pl[mask] == 1.0).all()
            wall = g["primitive"] == tb.PLANE_BIT
            assert wall.sum() > 1000 and mismatches(host(mh)[wall], host(ph)[wall]) == 0 and mismatches(ml[wall], pl[wall]) == 0
            assert (ml[wall] == k + 1).all()
            g_prev = face
        REPORT[f"motion_box_{'nearest' if snap else 'bilinear'}"] = {"mask_pixels": sizes}
        del keep, pws
    finally:
        loop.close()
