"""Deforming meshes keep their history, on the GPU: the surface record beside the G-buffer against the checker's normal,
the deform-aware accumulate stage against its plain-C checker, the driver against the loop it is defined as, a sheet that
walks toward a standing camera by more than the plane tolerance per frame, a sheet sheared in its own plane, and the
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the product library's first HIP call: a process has room for one HIP runtime, torch's own

import ref_deform_binding as db
import ref_refit_binding as rb
import ref_temporal_binding as tb
from parity_report import REPORT

pytestmark = pytest.mark.gpu

F = np.float32
TFI = 3          # total_frame_index of every frame here
NONE = db.NONE


def rays(s):
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def mismatches(a, b):
    return int(np.count_nonzero(tb.bits(host(a)) != tb.bits(host(b))))


def to_device(a):
    """A host array (structured arrays as their 32-bit words) -> a device tensor."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.float32).reshape(a.shape + (a.dtype.itemsize//4,))
    d = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize(0)
    return d


def full(fill, *shape):
    d = torch.full(shape, fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    return d


def texels(d):
    a = host(d)
    return a.view(tb.dtype()).reshape(a.shape[0], a.shape[1])


def records(d):
    a = host(d)
    return a.view(db.sdtype()).reshape(a.shape[0], a.shape[1])


def device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_motion, count, d_surf, d_deform, dcount, moments, velocity,
                 motion_entry=False):
    """rt_temporal_accumulate_deform_device (or the motion stage) into outputs that start as garbage
    -> (history, length, moments, velocity)."""
    d_hist, d_len = full(-5.0, h, w, 4), full(-5.0, h, w)
    d_mom = full(-5.0, h, w, 2) if moments else None
    d_vel = full(-5.0, h, w, 2) if velocity else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    ph, pl, pg, pm = d_prev if d_prev is not None else (None, None, None, None)
    common = dict(d_motion=ptr(d_motion), motion_count=count, d_prev_moments=ptr(pm) if moments else None, d_moments=ptr(d_mom),
                  d_velocity=ptr(d_vel))
    if motion_entry:
        rt.temporal_accumulate_motion_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                             d_hist.data_ptr(), d_len.data_ptr(), **common)
    else:
        rt.temporal_accumulate_deform_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                             d_hist.data_ptr(), d_len.data_ptr(), d_surface=ptr(d_surf), d_deform=ptr(d_deform),
                                             deform_count=dcount, **common)
    return d_hist, d_len, d_mom, d_vel


# ---- 1. the surface record beside the G-buffer

W, H, SPP = 64, 48, 2
CASES = {"24": (lambda: rb.generated(1), "RTH_BVH_SAH_BINNED"), "3024-binned": (lambda: rb.generated(3000), "RTH_BVH_SAH_BINNED")}


class World:
    """tests/test_gpu_refit.py's world: a floor plane, an emissive sphere, two instances of mesh 0 (one translated, one
    rotated about y) and mesh 1 with or without normals."""

    def __init__(self, rt, case="24", second_normals=True):
        make, how = CASES[case]
        self.tris, self.normals = make()
        s = rt.Scene()
        grey = s.add_diffuse_material((0.7, 0.6, 0.5), 1.5)
        red = s.add_diffuse_material((0.8, 0.25, 0.2), 1.4, checkers=True)
        light = s.add_emissive_material((14.0, 13.0, 12.0))
        s.add_plane(grey, (0.0, 1.0, 0.0), -0.5)
        s.add_sphere(light, 1.0, rt.translate((0.5, 5.0, 5.0)))
        self.mesh = s.create_mesh(self.tris, self.normals, getattr(rt.abi, how))
        t2, n2 = rb.generated(1, seed=5)
        self.other = s.create_mesh(t2, n2 if second_normals else None)
        self.arrays = {self.mesh: (self.tris, self.normals), self.other: (t2, n2 if second_normals else None)}
        self.first = s.add_mesh(red, self.mesh, rt.translate((-2.2, 0.0, 6.0))*rt.scale(2.0))
        self.second = s.add_mesh(grey, self.mesh, rt.translate((0.8, 0.2, 7.0))*rt.rotate_y(0.7)*rt.scale(2.0))
        self.third = s.add_mesh(grey, self.other, rt.translate((-0.5, 2.2, 8.0))*rt.scale(1.5))
        s.set_sky((0.6, 0.7, 0.9), (0.2, 0.2, 0.2))
        s.create_scene_bvh()
        self.scene = s
        cam = rt.abi.Camera()
        cam.vfov = rt.DEG_TO_RAD*28.0
        cam.aspect_ratio = W/H
        cam.lens_radius = 0.0
        cam.focus_distance = 8.0
        cam.p = rt.v3(0.0, 1.5, -3.0)
        rt.aim_camera_at(cam, (0.0, 1.0, 7.0))
        rt.recompute_camera(cam)
        self.cam = cam
        self.st, _ = rt.default_settings()
        self.st.samples_per_pixel = SPP
        self.fc = rt.load_reconstruction_kernel()

    def upload(self, rt):
        dev = rt.DeviceScene(self.scene, 0)
        dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        return dev

    def mesh_of(self, primitive):
        return int(self.scene.desc().primitives[primitive].mesh_index)


def check_surface(rt, wd, dev, label):
    """The texels are rt_gbuffer's; a record is {NONE, 0, 0, 0} off the meshes and, on them, names a triangle and a place
    whose normal under the checker is the texel's, bit for bit."""
    plain = dev.gbuffer(wd.cam, W, H, wd.st.lens_distortion)
    g, s = dev.gbuffer_surface(wd.cam, W, H, wd.st.lens_distortion)
    assert g.tobytes() == plain.tobytes()
    d_g, d_s = full(float("nan"), H, W, 8), full(float("nan"), H, W, 4)
    dev.gbuffer_surface_device(wd.cam, W, H, d_g.data_ptr(), d_s.data_ptr(), lens_distortion=wd.st.lens_distortion)
    assert texels(d_g).tobytes() == plain.tobytes() and records(d_s).tobytes() == s.tobytes()
    tr = dev.primitive_transforms()
    ids = g["primitive"]
    on_mesh = np.zeros((H, W), bool)
    counts = {}
    for prim in (wd.first, wd.second, wd.third):
        tris, nrm = wd.arrays[wd.mesh_of(prim)]
        here = ids == prim
        on_mesh |= here
        counts[prim] = int(here.sum())
        assert counts[prim] >= 12 and int(s["triangle"][here].max()) < len(tris) and not s["reserved"][here].any()
        _, n = db.surface(tris, nrm, np.eye(4, dtype=F), tr["inverse"][prim], s["triangle"][here], s["v"][here], s["w"][here])
        assert mismatches(n, g["n"][here]) == 0, (label, prim)
        assert (s["v"][here] >= 0).all() and (s["w"][here] >= 0).all() and (s["v"][here] + s["w"][here] <= 1).all()
    off = ~on_mesh
    assert off.sum() > 500 and (s["triangle"][off] == NONE).all()
    assert not tb.bits(s["v"][off]).any() and not tb.bits(s["w"][off]).any() and not s["reserved"][off].any()
    assert (ids[off] == tb.PLANE_BIT).any() and (ids[off] == tb.MISS).any()
    print(label, "mesh pixels per instance", counts, "triangles named", len(np.unique(s["triangle"][on_mesh])))
    return counts


@pytest.mark.parametrize("second_normals", [True, False], ids=["normals", "no-normals"])
@pytest.mark.parametrize("case", list(CASES))
def test_surface_record_names_the_hit(rt, case, second_normals):
    wd = World(rt, case, second_normals)
    dev = wd.upload(rt)
    try:
        check_surface(rt, wd, dev, f"{case} upload")
        # deformed and moved: the records follow the new arrays in their original order
        moved = rb.displaced(wd.tris, 0.15, 0.4)
        new_n = np.ascontiguousarray(wd.normals[:, ::-1, :])
        dev.update_mesh(wd.mesh, moved, new_n)
        wd.scene.update_mesh(wd.mesh, moved, new_n)
        wd.scene.set_primitive_transform(wd.third, rt.translate((-0.3, 2.0, 7.5))*rt.rotate_z(0.3)*rt.scale(1.5))
        wd.scene.create_scene_bvh()
        dev.update_instances()
        wd.arrays[wd.mesh] = (moved, new_n)
        check_surface(rt, wd, dev, f"{case} updated")
    finally:
        dev.close()


def test_surface_record_off_the_meshes(rt):
    """C1 has spheres, boxes and planes and no mesh: every record is {NONE, 0, 0, 0}."""
    scene, cam, st, fc, _ = rt.load_preset("c1", W, H)
    dev = rt.DeviceScene(scene, 0)
    try:
        g, s = dev.gbuffer_surface(cam, W, H, st.lens_distortion)
        assert g.tobytes() == dev.gbuffer(cam, W, H, st.lens_distortion).tobytes()
        d = scene.desc()
        ids = g["primitive"]
        kinds = {int(d.primitives[i].type) for i in np.unique(ids[ids < d.primitive_count])}
        assert {rt.abi.RT_PRIMITIVE_SPHERE, rt.abi.RT_PRIMITIVE_BOX} <= kinds and (ids & tb.PLANE_BIT).any()
        assert (s["triangle"] == NONE).all() and not s.view(np.uint32).reshape(H, W, 4)[..., 1:].any()
    finally:
        dev.close()


# ---- 2. the stage against the checker

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_stage_matches_the_checker(rt, w, h, amount):
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p = tb.params()
    d_cur, d_g, d_surf, d_moving = to_device(cur), to_device(g), to_device(surf), to_device(moving)
    d_prev = tuple(to_device(a) for a in prev)
    d_arrays = {k: (to_device(t), None if n is None else to_device(n)) for k, (t, n) in arrays.items()}
    table = db.table(tp, {k: (t.data_ptr(), 0 if n is None else n.data_ptr(), w*h) for k, (t, n) in d_arrays.items()})
    assert list(table["deformed"]) == [0, 0, 0, 1, 1, 1] and list(table["has_normals"]) == [0, 0, 0, 0, 1, 1]
    assert moving["moved"][1] == 1 and int(g["primitive"][g["primitive"] < 8].max()) == 7        # moved, not deformed; beyond
    assert (surf["triangle"][np.isin(g["primitive"], list(db.DEFORMED))] >= w*h).sum() > 10      # out of range
    d_table = to_device(table)
    bad = {}
    for moments in (False, True):
        for velocity in (False, True):
            got = device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), d_surf, d_table, len(table),
                               moments, velocity)
            want = db.checked(w, h, amount, moments, velocity)
            assert (got[2] is None) == (want[2] is None) and (got[3] is None) == (want[3] is None)
            bad[(moments, velocity)] = sum(mismatches(a, b) for a, b in zip(got, want) if b is not None)
    print(f"{w}x{h}: words that differ from the checker", bad)
    REPORT[f"deform_stage_{w}x{h}"] = {str(k): v for k, v in bad.items()}
    assert not any(bad.values())
    # no table (with and without a surface buffer), a table without a deformed entry, an empty one: the motion stage
    still = table.copy()
    still["deformed"] = 0
    d_still = to_device(still)
    for moments in (False, True):
        want = device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), None, None, 0, moments, True,
                            motion_entry=True)
        for s, t, count in ((None, None, 0), (d_surf, None, 0), (d_surf, d_still, len(still))):
            got = device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), s, t, count, moments, True)
            assert sum(mismatches(a, b) for a, b in zip(got, want) if b is not None) == 0
    # and the deforming table does change it
    got = device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), d_surf, d_table, len(table), False, False)
    assert mismatches(got[1], want[1]) >= 10
    # without history
    got = device_stage(rt, d_cur, d_g, None, None, 0.0, p, w, h, d_moving, len(moving), d_surf, d_table, len(table), True, True)
    want = db.accumulate_deform(cur, g, None, None, 0.0, p, moving, surf, db.host_table(tp, arrays), want_moments=True,
                                want_velocity=True)
    assert sum(mismatches(a, b) for a, b in zip(got, want)) == 0
    # the host twin: host buffers, a table on the host whose vertex pointers are the device's
    got = rt.temporal_accumulate_deform(cur, g, prev, cam, amount, p, moving, surf, table, want_moments=True, want_velocity=True)
    assert sum(mismatches(a, b) for a, b in zip(got, db.checked(w, h, amount, True, True))) == 0
    del d_arrays


# ---- 3. the driver against the loop it is defined as

class Loop:
    """A scene on the device in the exact splat mode, with what a temporal loop over deforming meshes needs."""

    def __init__(self, rt, scene, cam, st, fc, w, h):
        self.rt, self.scene, self.cam, self.st, self.fc, self.w, self.h = rt, scene, cam, st, fc, w, h
        self.dev = rt.DeviceScene(scene, 0)
        self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        self.count = len(self.dev.primitive_transforms())

    def frame(self, frame_count):
        d = full(0.0, self.h, self.w, 4)
        s = self.dev.render_device(self.cam, self.st, self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI,
                                   frame_count=frame_count)
        return d, s

    def gbuffer_surface(self):
        d, s = full(float("nan"), self.h, self.w, 8), full(float("nan"), self.h, self.w, 4)
        self.dev.gbuffer_surface_device(self.cam, self.w, self.h, d.data_ptr(), s.data_ptr(), lens_distortion=self.st.lens_distortion)
        return d, s

    def state(self, deform=True):
        """A fresh rt_temporal_motion_state over a workspace that starts as garbage -> (state, what it points at)."""
        size = self.rt.temporal_deform_workspace_bytes if deform else self.rt.temporal_motion_workspace_bytes
        ws = full(float("nan"), (size(self.w, self.h, self.count) + 3)//4)
        store = (self.rt.abi.M4x4Inv*self.count)()
        st = self.rt.TemporalMotionState()
        st.d_workspace, st.transforms, st.transform_cap = ws.data_ptr(), C.cast(store, C.POINTER(self.rt.abi.M4x4Inv)), self.count
        return st, (ws, store)

    def deform_driver(self, frame_count, p, state, meshes):
        d_out, d_len = full(9.0, self.h, self.w, 4), full(9.0, self.h, self.w)
        s = self.dev.render_temporal_deform_device(self.cam, self.st, self.fc, self.w, self.h, p, state, meshes, d_out.data_ptr(),
                                                   d_length_out=d_len.data_ptr(), frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_len, s

    def motion_driver(self, frame_count, p, state):
        d_out, d_len = full(9.0, self.h, self.w, 4), full(9.0, self.h, self.w)
        self.dev.render_temporal_motion_device(self.cam, self.st, self.fc, self.w, self.h, p, state, d_out.data_ptr(),
                                               d_length_out=d_len.data_ptr(), frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_len

    def deform(self, mesh, triangles, normals=None, moves=None):
        """One frame's update in the caller's order: the mesh on the device from a fresh device buffer, the host model,
        the top-level BVH, the instances -> the device buffers, which the next frame names as the previous ones."""
        d_t = to_device(triangles)
        d_n = None if normals is None else to_device(normals)
        self.dev.update_mesh_device(mesh, d_t, d_n)
        self.scene.update_mesh(mesh, triangles, normals)
        for pid, t in (moves or {}).items():
            self.scene.set_primitive_transform(pid, t)
        self.scene.create_scene_bvh()
        self.dev.update_instances()
        return d_t, d_n

    def close(self):
        self.dev.close()


def test_driver_equals_the_loop_on_the_public_entries(rt):
    wd = World(rt, "24")
    loop = Loop(rt, wd.scene, wd.cam, wd.st, wd.fc, W, H)
    try:
        p = tb.params()
        amount = wd.st.lens_distortion
        state, keep = loop.state()
        d_normals = to_device(wd.normals)
        buffers = (to_device(wd.tris), d_normals)            # what the frame before was rendered with
        prev, prev_tr, bad, shares, deformed_px = None, None, 0, [], []
        for k in range(4):
            if k:
                latest = loop.deform(wd.mesh, rb.displaced(wd.tris, 0.04*k, 0.3*k), None,
                                     {wd.third: rt.translate((-0.5 + 0.05*k, 2.2, 8.0 - 0.1*k))*rt.scale(1.5)})
            meshes = [(wd.mesh, buffers[0], buffers[1])]
            # rt_render_temporal_deform_device's definition, on the public entries below it
            f, want_stats = loop.frame(k)
            g, s = loop.gbuffer_surface()
            tr = loop.dev.primitive_transforms()
            if prev is None:
                loop.dev.deform_table(meshes, tr)              # the list is checked all the same
                want = device_stage(rt, f, g, None, None, amount, p, W, H, None, 0, s, None, 0, False, False)
            else:
                motion, table = rt.motion_table(tr, prev_tr), loop.dev.deform_table(meshes, prev_tr)
                assert list(table["deformed"]) == [0, 0, 1, 1, 0] and list(motion["moved"]) == [0, 0, 0, 0, 1]
                assert table["d_prev_triangles"][wd.first] == buffers[0].data_ptr() and table["d_prev_normals"][wd.second] == d_normals.data_ptr()
                assert list(table["triangle_count"]) == [0, 0, 24, 24, 0] and list(table["has_normals"]) == [0, 0, 1, 1, 0]
                assert mismatches(table["inv_prev"], prev_tr["inverse"][:, :3]) == 0
                want = device_stage(rt, f, g, prev + (None,), wd.cam, amount, p, W, H, to_device(motion), len(motion), s,
                                    to_device(table), len(table), False, False)
                ids = texels(g)["primitive"]
                deformed_px.append(int(((ids == wd.first) | (ids == wd.second)).sum()))
            got_hist, got_len, stats = loop.deform_driver(k, p, state, meshes)
            bad += mismatches(got_hist, want[0]) + mismatches(got_len, want[1])
            assert rays(stats) == rays(want_stats) and stats.samples == W*H*SPP
            assert (state.frames, state.parity, state.w, state.h, state.primitive_count) == (k + 1, (k + 1) % 2, W, H, loop.count)
            assert bytes(state.camera) == bytes(wd.cam) and bytes(keep[1]) == tr.tobytes()
            prev, prev_tr = (want[0], want[1], g), tr
            shares.append(float((host(got_len) > 1).mean()))
            if k:
                buffers = (latest[0], d_normals)
        print("deform driver: share of pixels with a history per frame", shares, "pixels on the deformed mesh", deformed_px)
        REPORT["deform_driver"] = {"mismatches": bad, "share_with_history": shares}
        assert bad == 0 and shares[0] == 0.0 and min(shares[1:]) > 0.5 and min(deformed_px) > 100
        # the host entry, on a state of another primitive count: it restarts, and the list is still checked
        state.primitive_count = loop.count + 1
        with pytest.raises(rt.RenderError, match=r"rt_scene_deform_table: meshes\[0\]: mesh_index 7 is out of range"):
            loop.dev.render_temporal_deform(wd.cam, wd.st, wd.fc, W, H, state, [(7, buffers[0], None)], p, frame_count=4,
                                            total_frame_index=TFI)
        assert state.frames == 4
        out, length, _ = loop.dev.render_temporal_deform(wd.cam, wd.st, wd.fc, W, H, state, [(wd.mesh, buffers[0], buffers[1])], p,
                                                         frame_count=4, total_frame_index=TFI)
        assert (length[np.isfinite(out).all(axis=2)] == 1.0).all() and state.frames == 5 and state.primitive_count == loop.count
        del keep
    finally:
        loop.close()


# ---- 4. a sheet that walks toward a standing camera, and one sheared in its own plane

SW, SH = 96, 64


def sheet_scene(rt, triangles, normals=None):
    """A wall facing the camera and a sheet in front of it, on an instance transform nobody touches."""
    s = rt.Scene()
    m = s.add_diffuse_material((0.6, 0.5, 0.4), 1.5)
    s.add_plane(m, (0.0, 0.0, -1.0), -3.0)           # z = 3, facing -z
    mesh = s.create_mesh(triangles, normals)
    prim = s.add_mesh(m, mesh, rt.identity())
    s.set_sky((0.6, 0.7, 0.9), (0.1, 0.1, 0.1))
    s.create_scene_bvh()
    return s, mesh, prim


def sheet_camera(rt):
    cam = rt.abi.Camera()
    cam.vfov, cam.aspect_ratio, cam.lens_radius, cam.focus_distance = rt.DEG_TO_RAD*50.0, SW/SH, 0.0, 10.0
    cam.p = rt.v3(0.0, 1.0, -5.0)
    rt.aim_camera_at(cam, (0.0, 1.0, 0.0))
    rt.recompute_camera(cam)
    st, _ = rt.default_settings()
    st.lens_distortion, st.samples_per_pixel, st.integrator = 0.0, 1, rt.abi.RT_INTEGRATOR_NORMALS
    return cam, st, rt.load_reconstruction_kernel("Box")


def eroded(mask):
    """The pixels whose 3 x 3 neighbourhood lies in the mask."""
    out = mask.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out &= np.roll(np.roll(mask, dy, 0), dx, 1)
    out[0, :] = out[-1, :] = False
    out[:, 0] = out[:, -1] = False
    return out


@pytest.mark.parametrize("snap", [0.5, None], ids=["nearest", "bilinear"])
def test_sheet_walking_toward_the_camera_keeps_its_history(rt, snap):
    """Four frames, the sheet's vertices 0.2 nearer in each: twice the plane tolerance at its distance (0.02 x 5.5).  The
    instance transform is the identity throughout, so the motion driver sees nothing move: it looks for the sheet where
    it is now, finds last frame's 0.2 behind, and restarts every frame.  The deform driver's history grows by one per
    frame.  With snap = 0.5 every position snaps to its nearest previous pixel, a single tap of weight 1, and the lengths
    are whole numbers exactly; under the default snap a length is sum(w L)/sum(w) over four bilinear taps, at most 8
    roundings of 2^-24 each: within 4 x 8 x 2^-24 of frame + 1 (the motion test's own bound)."""
    zs = [1.0, 0.8, 0.6, 0.4]
    cam, st, fc = sheet_camera(rt)
    scene, mesh, prim = sheet_scene(rt, db.sheet(8, 3.0, zs[0], -0.5))
    loop = Loop(rt, scene, cam, st, fc, SW, SH)
    try:
        p = tb.params() if snap is None else tb.params(snap=snap)
        dstate, keep = loop.state()
        mstate, mkeep = loop.state(deform=False)
        buffers = (to_device(db.sheet(8, 3.0, zs[0], -0.5)), None)
        g_prev, sizes = None, []
        for k, z in enumerate(zs):
            if k:
                latest = loop.deform(mesh, db.sheet(8, 3.0, z, -0.5))
            dh, dl, _ = loop.deform_driver(k, p, dstate, [(mesh, buffers[0], None)])
            mh, ml = loop.motion_driver(k, p, mstate)
            g = texels(loop.gbuffer_surface()[0])
            face = g["primitive"] == prim
            mask = eroded(face) & (eroded(g_prev) if g_prev is not None else True)
            if k:
                assert 0.2 > p.plane_tolerance*float(g["t"][mask].max())
                buffers = latest
            sizes.append(int(mask.sum()))
            dl, ml = host(dl), host(ml)
            print(f"frame {k}: mask {sizes[-1]} pixels, deform lengths {np.unique(dl[mask])}, motion {np.unique(ml[mask])}")
            assert sizes[-1] >= 200
            if snap is not None:
                assert (dl[mask] == k + 1).all()
            else:
                assert np.abs(dl[mask] - (k + 1)).max() <= 32*2.0**-24
            assert (ml[mask] == 1.0).all()
            wall = g["primitive"] == tb.PLANE_BIT
            assert wall.sum() > 1000 and mismatches(host(dh)[wall], host(mh)[wall]) == 0 and mismatches(dl[wall], ml[wall]) == 0
            g_prev = face
        REPORT[f"deform_sheet_{'nearest' if snap else 'bilinear'}"] = {"mask_pixels": sizes}
        assert bytes(keep[1]) == bytes(mkeep[1])                # the transforms never moved
        del keep, mkeep
    finally:
        loop.close()


def project64(cam, P, w, h):
    """The pinhole projection of the stage (no lens distortion) in float64 from the camera's float32 fields."""
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)
    d = P - v(cam.p)
    z = -(d @ v(cam.z))
    u = ((d @ v(cam.x))*float(cam.film_distance))/(z*float(cam.half_film_w))
    t = ((d @ v(cam.y))*float(cam.film_distance))/(z*float(cam.half_film_h))
    return (1.0 - u)*(w*0.5), (1.0 - t)*(h*0.5)


def barycentric64(tris, rec):
    t = np.asarray(tris, np.float64)[rec["triangle"]]
    v, w = rec["v"].astype(np.float64)[:, None], rec["w"].astype(np.float64)[:, None]
    return t[:, 0] + v*(t[:, 1] - t[:, 0]) + w*(t[:, 2] - t[:, 0])


def test_sheared_sheet_velocity_is_the_surface_points_shift(rt):
    """The sheet sheared in its own plane, x += 0.15 y between two frames: no rigid motion takes one to the other.  The
    velocity the stage writes at an interior sheet pixel against the screen shift of that surface point in float64, from
    the record and the two vertex sets: proj(previous point) - proj(current point).  The float64 model attributes one
    error to the float32 inputs: the record's barycentrics are rounded, so the current point's own projection misses the
    pixel centre it was seen through.  The bound is 4 x the largest such miss.  Measured (584 pixels, shifts of 0.04 to
    2.9 pixels): observed 8.26e-6 pixels, the inputs' own 5.89e-6, so the bound is 2.36e-5 ("Deforming meshes
    keep their history")."""
    cam, st, fc = sheet_camera(rt)
    flat = db.sheet(8, 3.0, 1.0, -0.5)
    nrm = np.tile((np.array([0.0, 0.2, -1.0])/np.sqrt(1.04)).astype(F), (len(flat), 3, 1))      # the sheet's own tilt
    sheared = flat.copy()
    sheared[..., 0] += F(0.15)*flat[..., 1]
    scene, mesh, prim = sheet_scene(rt, flat, nrm)
    loop = Loop(rt, scene, cam, st, fc, SW, SH)
    try:
        p = tb.params()
        d_flat, d_nrm = to_device(flat), to_device(nrm)
        f0, _ = loop.frame(0)
        g0, s0 = loop.gbuffer_surface()
        tr0 = loop.dev.primitive_transforms()
        first = device_stage(rt, f0, g0, None, None, 0.0, p, SW, SH, None, 0, s0, None, 0, False, False)
        loop.deform(mesh, sheared, nrm)
        f1, _ = loop.frame(1)
        g1, s1 = loop.gbuffer_surface()
        table = loop.dev.deform_table([(mesh, d_flat, d_nrm)], tr0)
        got = device_stage(rt, f1, g1, (first[0], first[1], g0, None), cam, 0.0, p, SW, SH, None, 0, s1, to_device(table),
                           len(table), False, True)
        vel, length = host(got[3]), host(got[1])
        ids0, ids1, rec = texels(g0)["primitive"], texels(g1)["primitive"], records(s1)
        mask = eroded(ids1 == prim) & eroded(ids0 == prim)
        ys, xs = np.nonzero(mask)
        r = rec[mask]
        px, py = project64(cam, barycentric64(flat, r), SW, SH)
        cx, cy = project64(cam, barycentric64(sheared, r), SW, SH)
        inputs = max(float(np.abs(cx - xs).max()), float(np.abs(cy - ys).max()))
        observed = max(float(np.abs(vel[mask][:, 0] - (px - cx)).max()), float(np.abs(vel[mask][:, 1] - (py - cy)).max()))
        bound = 4.0*inputs
        print(f"sheared sheet: {int(mask.sum())} pixels, shifts of {np.abs(px - cx).min():.3f} to {np.abs(px - cx).max():.3f} pixels; "
              f"observed max |velocity - shift64| {observed:.3e}, the inputs' own rounding {inputs:.3e}, bound {bound:.3e}")
        REPORT["deform_sheared_sheet"] = {"pixels": int(mask.sum()), "observed": observed, "inputs": inputs, "bound": bound}
        assert mask.sum() >= 200 and np.abs(px - cx).max() > 2.0 and np.abs(py - cy).max() < 1e-3
        assert inputs > 0.0 and observed <= bound
        assert (np.abs(length[mask] - 2.0) <= 32*2.0**-24).mean() > 0.9     # and the history follows the shear
    finally:
        loop.close()


# ---- 5. refusals, each by name and leaving the outputs untouched

def test_refusals_leave_the_outputs_untouched(rt):
    wd = World(rt, "24", second_normals=False)
    loop = Loop(rt, wd.scene, wd.cam, wd.st, wd.fc, W, H)
    dev = loop.dev
    try:
        d_t, d_n = to_device(wd.tris), to_device(wd.normals)
        d_g, d_s = full(7.0, H, W, 8), full(7.0, H, W, 4)
        untouched = lambda *ts: all(bool((t == t.flatten()[0]).all()) for t in ts)

        def refused(call, text):
            with pytest.raises(rt.RenderError, match=text) as info:
                call()
            assert info.value.code == rt.abi.RT_ERROR_INVALID

        # the surface G-buffer
        refused(lambda: dev.gbuffer_surface_device(wd.cam, W, H, d_g.data_ptr(), None), "rt_gbuffer_surface_device: null d_surface")
        assert untouched(d_g, d_s)
        # the stage: a table without a surface buffer
        f, _ = loop.frame(0)
        g, s = loop.gbuffer_surface()
        tr = dev.primitive_transforms()
        table = dev.deform_table([(wd.mesh, d_t, d_n)], tr)
        d_table, d_hist, d_len = to_device(table), full(7.0, H, W, 4), full(7.0, H, W)
        refused(lambda: rt.temporal_accumulate_deform_device(f.data_ptr(), g.data_ptr(), None, None, None, None, 0.0, W, H, tb.params(),
                                                             d_hist.data_ptr(), d_len.data_ptr(), d_deform=d_table.data_ptr(),
                                                             deform_count=len(table)),
                "rt_temporal_accumulate_deform_device: null d_surface with a deform table")
        assert untouched(d_hist, d_len)
        # rt_scene_deform_table
        t = "rt_scene_deform_table: "
        refused(lambda: dev.deform_table([(wd.mesh, d_t, d_n)], tr[:3]), t + "primitive_count 3 is not the scene's 5")
        refused(lambda: dev.deform_table([(2, d_t, d_n)], tr), t + r"meshes\[0\]: mesh_index 2 is out of range")
        refused(lambda: dev.deform_table([(wd.mesh, d_t, d_n), (wd.other, d_t, None), (wd.mesh, d_t, d_n)], tr),
                t + r"meshes\[2\]: mesh 0 is listed twice")
        refused(lambda: dev.deform_table([(wd.mesh, None, d_n)], tr), t + r"meshes\[0\]: null d_prev_triangles")
        refused(lambda: dev.deform_table([(wd.mesh, d_t, None)], tr),
                t + r"meshes\[0\]: null d_prev_normals for mesh 0, which was uploaded with normals")
        refused(lambda: dev.deform_table([(wd.other, d_t, d_n)], tr),
                t + r"meshes\[0\]: d_prev_normals for mesh 1, which was uploaded without normals")
        lib, abi = rt.lib(), rt.abi
        one = (abi.DeformMesh*1)(abi.DeformMesh(0, 0, d_t.data_ptr(), d_n.data_ptr()))
        out = (abi.DeformEntry*5)()
        trp = tr.ctypes.data_as(C.POINTER(abi.M4x4Inv))
        for args, text in (((dev._h, 1, None, 5, trp, out), "null meshes with a mesh_count"), ((dev._h, 1, one, 5, None, out), "null prev"),
                           ((dev._h, 1, one, 5, trp, None), "null out")):
            assert lib.rt_scene_deform_table(*args) == abi.RT_ERROR_INVALID and (t + text) in lib.rt_last_error().decode()
        # an entry of a mesh nobody listed, and of no mesh at all
        assert list(table["deformed"]) == [0, 0, 1, 1, 0] and not table["d_prev_triangles"][[0, 1, 4]].any()
        # a stale scene: the driver and the surface G-buffer refuse, the outputs and the state stay
        state, keep = loop.state()
        d_out, d_lo = full(9.0, H, W, 4), full(9.0, H, W)
        dev.update_mesh(wd.mesh, rb.displaced(wd.tris, 0.15, 0.4))
        named = r"mesh 0 .*rt_scene_update_instances with a top-level BVH over the new bounds"
        refused(lambda: dev.gbuffer_surface_device(wd.cam, W, H, d_g.data_ptr(), d_s.data_ptr()), "rt_gbuffer_surface_device: .*" + named)
        refused(lambda: dev.render_temporal_deform_device(wd.cam, wd.st, wd.fc, W, H, tb.params(), state, [(wd.mesh, d_t, d_n)],
                                                          d_out.data_ptr(), d_length_out=d_lo.data_ptr()), named)
        assert untouched(d_g, d_s, d_out, d_lo) and state.frames == 0
        del keep
    finally:
        loop.close()
