"""Deforming meshes on the device ("Deforming meshes"): rt_scene_update_mesh against a fresh upload of the
rth_update_mesh-ed host scene and against the plain-C checker, table for table and byte for byte, then everything
downstream of the tables, the staleness rule and the refusals.  No tolerance appears anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch        # before the product library's first HIP call: a process has room for one HIP runtime, torch's own

import deep_bvh
import ref_refit_binding as rb
import ref_temporal_binding as tb

pytestmark = pytest.mark.gpu

W, H, SPP, TFI = 64, 48, 4, 3
SIX = ("TRIANGLES", "NORMALS", "NODES_SRC", "NODES", "NODES4", "MID4")


def one_triangle():
    return np.array([[[0.1, 0.2, 0.5], [0.9, 0.25, 0.45], [0.4, 0.95, 0.6]]], np.float32), None


def forty_identical():
    return np.tile(np.array([[[0.1, 0.1, 0.5], [0.9, 0.1, 0.5], [0.1, 0.9, 0.6]]], np.float32), (40, 1, 1)), None


CASES = {
    "one": (one_triangle, "RTH_BVH_SAH_BINNED"),
    "forty": (forty_identical, "RTH_BVH_SAH_BINNED"),
    "24": (lambda: rb.generated(1), "RTH_BVH_SAH_BINNED"),
    "3024-midpoint": (lambda: rb.generated(3000), "RTH_BVH_MIDPOINT_SPLIT"),
    "3024-binned": (lambda: rb.generated(3000), "RTH_BVH_SAH_BINNED"),
}


class World:
    """A floor plane, an emissive sphere, two instances of mesh 0 (one translated, one rotated about y) and mesh 1,
    which no test updates."""

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
        s.add_mesh(red, self.mesh, rt.translate((-2.2, 0.0, 6.0))*rt.scale(2.0))
        s.add_mesh(grey, self.mesh, rt.translate((0.8, 0.2, 7.0))*rt.rotate_y(0.7)*rt.scale(2.0))
        s.add_mesh(grey, self.other, rt.translate((-0.5, 2.2, 8.0))*rt.scale(1.5))
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

    def upload(self, rt, scene=None):
        dev = rt.DeviceScene(scene if scene is not None else self.scene, 0)
        dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        return dev

    def queries(self, rt, count=192):
        d = tb.gbuffer_rays(self.cam, 0.0, W, H).reshape(-1, 3)
        step = max(1, len(d)//count)
        return [rt.abi.RayQuery(self.cam.p, rt.v3(*[float(v) for v in d[i]]), 3.0e38, 0) for i in range(0, len(d), step)]


def six(rt, dev, m):
    return {name: dev.mesh_table(m, getattr(rt.abi, "RT_MESH_TABLE_" + name)).tobytes() for name in SIX}


def differing(a, b):
    return [k for k in a if a[k] != b[k]]


def plan(rt, dev, m):
    c = dev.mesh_table(m, rt.abi.RT_MESH_TABLE_REFIT_PLAN).view(np.uint32)
    return dict(zip(("rounds", "subtrees", "first_round", "reachable", "largest", "levels", "bvh4", "launches"), map(int, c)))


def checker_tables(rt, dev, m, before, host_before, triangles, normals):
    """The six tables the checker gives: the refit of the host arrays as they were, and the device's own tables as
    they were with the checker's boxes put in."""
    _, idx, _, nodes0 = host_before
    nodes, recs, slot_n = rb.refit(triangles, normals, idx, nodes0)
    want = dict(before)
    want["TRIANGLES"] = recs.tobytes()
    if normals is not None:
        want["NORMALS"] = slot_n.tobytes()
    want["NODES_SRC"] = nodes.tobytes()
    trav = np.frombuffer(before["NODES"], rb.NODE_DTYPE).copy()
    trav["bv_p"], trav["bv_r"] = nodes["bv_p"], nodes["bv_r"]
    want["NODES"] = trav.tobytes()
    src = dev.mesh_table(m, rt.abi.RT_MESH_TABLE_BVH4_SOURCES).view(np.uint32)
    n4 = np.frombuffer(before["NODES4"], np.float32).reshape(-1, 32)
    m4 = np.frombuffer(before["MID4"], np.float32).reshape(-1, 12)
    assert len(src) == len(n4) == len(m4)
    a, b = rb.bvh4(nodes, src, n4, m4)
    want["NODES4"], want["MID4"] = a.tobytes(), b.tobytes()
    return want


def moved_vertices(case, tris, step=1):
    if case == "forty":
        out = tris.copy()
        out[7] += np.float32(0.5*step)
        return out
    return rb.displaced(tris, 0.15*step, 0.4*step)


# ---- 1. the tables

@pytest.mark.parametrize("case", list(CASES))
def test_tables_equal_a_fresh_upload_and_the_checker(rt, case):
    wd = World(rt, case)
    dev = wd.upload(rt)
    try:
        before = six(rt, dev, wd.mesh)
        other = six(rt, dev, wd.other)
        host_before = rb.mesh_arrays(wd.scene.desc(), wd.mesh)
        p = plan(rt, dev, wd.mesh)
        print(case, p)
        reach = int(np.count_nonzero(np.arange(len(host_before[3])) != 1))
        assert p["reachable"] == reach and p["largest"] <= 1024
        if case.startswith("3024"):
            # several workgroup subtrees, and what is left above them in a later launch
            assert p["rounds"] >= 2 and p["first_round"] >= 2 and p["subtrees"] > p["first_round"]
        else:
            assert p["rounds"] == 1 and p["subtrees"] == 1
        assert p["bvh4"] == (0 if case in ("one", "forty") else len(before["NODES4"])//128)
        moved = moved_vertices(case, wd.tris)
        new_n = None if wd.normals is None else np.ascontiguousarray(wd.normals[:, ::-1, :])
        root = dev.update_mesh(wd.mesh, moved, new_n)
        got = six(rt, dev, wd.mesh)
        assert differing(got, checker_tables(rt, dev, wd.mesh, before, host_before, moved, new_n)) == []
        wd.scene.update_mesh(wd.mesh, moved, new_n)
        fresh = wd.upload(rt)
        try:
            assert differing(got, six(rt, fresh, wd.mesh)) == []
            assert differing(other, six(rt, fresh, wd.other)) == []
        finally:
            fresh.close()
        assert differing(six(rt, dev, wd.other), other) == []           # the second mesh's slices
        assert "NODES_SRC" in differing(got, before) and "TRIANGLES" in differing(got, before)
        assert bytes(root) == got["NODES_SRC"][:32]
    finally:
        dev.close()


def test_hand_made_tree_with_children_before_parents(rt):
    """tests/deep_bvh.py's caterpillar, renumbered so that every pair of children precedes its parent: the plan walks
    from node 0, whatever the order of the array."""
    ds = deep_bvh.DeepScene(rt, 7, "tight")
    flipped = rb.children_first(np.frombuffer(bytes(ds._nodes), rb.NODE_DTYPE))
    kids = [(i, int(e["left_first"])) for i, e in enumerate(flipped) if i >= 2 and e["count"] == 0 and e["left_first"]]
    assert kids and all(c < i for i, c in kids)
    ds._nodes = (rt.abi.BvhNode*len(flipped)).from_buffer_copy(flipped.tobytes())
    ds._meshes[0].nodes = ds._nodes
    dev = rt.DeviceScene(ds, 0)
    try:
        before = six(rt, dev, 0)
        assert before["NODES_SRC"] == flipped.tobytes()
        p = plan(rt, dev, 0)
        assert p["rounds"] == 1 and p["reachable"] == len(flipped) - 1 and p["bvh4"] == len(before["NODES4"])//128 == 7
        idx = np.arange(len(ds.tris), dtype=np.uint32)
        moved = (ds.tris*np.float32(1.25) + np.float32(0.5)).astype(np.float32)
        dev.update_mesh(0, moved)
        got = six(rt, dev, 0)
        assert differing(got, checker_tables(rt, dev, 0, before, (None, idx, None, flipped), moved, None)) == []
        assert {"TRIANGLES", "NODES_SRC", "NODES", "NODES4", "MID4"} <= set(differing(got, before))
        assert got["NODES_SRC"][32:64] == before["NODES_SRC"][32:64]        # the padding entry keeps its bytes
    finally:
        dev.close()


# ---- 2. everything downstream

def everything(rt, wd, dev, queries):
    frame, stats = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)
    with dev.configured(traversal_ref=1):                                # the reference's units: reads mid4
        frame_ref, stats_ref = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)
    return {"frame": frame,
            "rays": (stats.closest_hit_rays, stats.shadow_rays, stats.samples),
            "traversal": (stats.traversal[0].as_dict(), stats.traversal[1].as_dict()),
            "frame_ref": frame_ref,
            "traversal_ref": (stats_ref.traversal_ref[0].as_dict(), stats_ref.traversal_ref[1].as_dict()),
            "gbuffer": dev.gbuffer(wd.cam, W, H, wd.st.lens_distortion).tobytes(),
            "hits": b"".join(bytes(r) for r in dev.intersect(queries)),
            "occluded": [r.primitive == rt.abi.RT_HIT_MISS for r in dev.intersect(queries, occlusion=True)],
            "depth": dev.stack_depth()}


def disagreements(a, b):
    return [k for k in a if not (np.array_equal(tb.bits(a[k]), tb.bits(b[k])) if k.startswith("frame") else a[k] == b[k])]


def test_update_equals_a_fresh_upload(rt):
    wd = World(rt, "3024-binned")
    queries = wd.queries(rt)
    dev = wd.upload(rt)
    try:
        first = everything(rt, wd, dev, queries)
        assert sum(first["traversal"][0].values()) > 0
        steps = [moved_vertices("x", wd.tris, 1), moved_vertices("x", moved_vertices("x", wd.tris, 1), 2), wd.tris]
        for k, vertices in enumerate(steps):
            before = dev.mesh_table(wd.mesh, rt.abi.RT_MESH_TABLE_NODES_SRC)[:24].tobytes()
            dev.update_mesh(wd.mesh, vertices)
            assert dev.mesh_table(wd.mesh, rt.abi.RT_MESH_TABLE_NODES_SRC)[:24].tobytes() != before      # the root box moved
            wd.scene.update_mesh(wd.mesh, vertices)
            wd.scene.create_scene_bvh()
            dev.update_instances()
            got = everything(rt, wd, dev, queries)
            if k == len(steps) - 1:
                assert disagreements(got, first) == []          # back where it was: the very first frame
                break
            fresh = wd.upload(rt)
            try:
                want = everything(rt, wd, fresh, queries)
            finally:
                fresh.close()
            assert disagreements(got, want) == [], k
            assert "frame" in disagreements(got, first) and "gbuffer" in disagreements(got, first)
    finally:
        dev.close()


# ---- 3. device input

def test_device_input_equals_host_input(rt):
    wd = World(rt, "3024-midpoint")
    moved = moved_vertices("x", wd.tris)
    new_n = np.ascontiguousarray(wd.normals[:, ::-1, :])
    a, b = wd.upload(rt), wd.upload(rt)
    try:
        a.update_mesh(wd.mesh, moved, new_n)
        d_t, d_n = torch.from_numpy(moved).to("cuda:0"), torch.from_numpy(new_n).to("cuda:0")
        torch.cuda.synchronize(0)
        root = b.update_mesh_device(wd.mesh, d_t, d_n)
        assert differing(six(rt, a, wd.mesh), six(rt, b, wd.mesh)) == []
        assert bytes(root) == six(rt, b, wd.mesh)["NODES_SRC"][:32]
        # pointers, and NULL normals: the stored ones stay
        b.update_mesh_device(wd.mesh, d_t.data_ptr())
        assert differing(six(rt, a, wd.mesh), six(rt, b, wd.mesh)) == []
    finally:
        a.close()
        b.close()


# ---- 4. identity, staleness

def test_identity_update_changes_nothing(rt):
    wd = World(rt, "3024-binned")
    dev = wd.upload(rt)
    try:
        before = six(rt, dev, wd.mesh)
        frame, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)
        dev.update_mesh(wd.mesh, wd.tris, wd.normals)
        assert differing(six(rt, dev, wd.mesh), before) == []
        again, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)    # not stale: no update_instances
        assert np.array_equal(tb.bits(again), tb.bits(frame))
    finally:
        dev.close()


def test_stale_scene_refuses_to_trace(rt):
    wd = World(rt, "24")
    queries = wd.queries(rt, 16)
    dev = wd.upload(rt)
    try:
        dev.update_mesh(wd.mesh, moved_vertices("x", wd.tris))
        named = r"mesh 0 .*rt_scene_update_instances with a top-level BVH over the new bounds"
        for call in (lambda: dev.render(wd.cam, wd.st, wd.fc, W, H), lambda: dev.gbuffer(wd.cam, W, H),
                     lambda: dev.intersect(queries), lambda: dev.intersect(queries, occlusion=True)):
            with pytest.raises(rt.RenderError, match=named) as info:
                call()
            assert info.value.code == rt.abi.RT_ERROR_INVALID
        # an identity update on top does not clear the mark
        dev.update_mesh(wd.mesh, moved_vertices("x", wd.tris))
        with pytest.raises(rt.RenderError, match=named):
            dev.render(wd.cam, wd.st, wd.fc, W, H)
        wd.scene.update_mesh(wd.mesh, moved_vertices("x", wd.tris))
        wd.scene.create_scene_bvh()
        dev.update_instances()
        frame, stats = dev.render(wd.cam, wd.st, wd.fc, W, H)
        assert stats.samples == W*H*SPP and np.isfinite(frame).all()
        assert dev.gbuffer(wd.cam, W, H).shape == (H, W) and len(dev.intersect(queries)) == len(queries)
    finally:
        dev.close()


# ---- 5. refusals leave the scene alone

def test_refused_updates_leave_the_scene_alone(rt):
    wd = World(rt, "3024-binned", second_normals=False)
    dev = wd.upload(rt)
    try:
        dev.update_mesh(wd.mesh, wd.tris)                                # the plan exists: a refusal frees nothing of it
        before = [six(rt, dev, m) for m in (wd.mesh, wd.other)]
        frame, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)
        nan = wd.tris.copy()
        nan[-1, 2, 1] = np.nan
        far = wd.tris.copy()
        far[5, 1, 0] = np.float32(2.0**41)
        t2, n2 = rb.generated(1, seed=5)
        for args, why in (((wd.mesh, nan), "rt_scene_update_mesh: mesh 0: a vertex is not finite"),
                          ((wd.mesh, far), r"rt_scene_update_mesh: mesh 0: .*within 2\^40"),
                          ((wd.other, t2, n2), "rt_scene_update_mesh: normals for mesh 1, which was uploaded without normals"),
                          ((2, wd.tris), "rt_scene_update_mesh: mesh_index 2 is out of range")):
            with pytest.raises(rt.RenderError, match=why) as info:
                dev.update_mesh(*args)
            assert info.value.code == rt.abi.RT_ERROR_INVALID
            assert [six(rt, dev, m) for m in (wd.mesh, wd.other)] == before
            again, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)     # and not stale
            assert np.array_equal(tb.bits(again), tb.bits(frame))
        with pytest.raises(rt.RenderError, match="rt_scene_update_mesh_device: null d_triangles"):
            dev.update_mesh_device(wd.mesh, None)
        assert [six(rt, dev, m) for m in (wd.mesh, wd.other)] == before
    finally:
        dev.close()


# ---- 6. a mesh without a BVH

class WithoutBvh:
    """The world's desc with mesh 0's BVH taken away (node_count 0), as tests/test_gpu_edges.py makes one."""

    def __init__(self, rt, scene):
        self.scene = scene
        d = scene.desc()
        self._meshes = (rt.abi.Mesh*d.mesh_count)(*[d.meshes[i] for i in range(d.mesh_count)])
        self._meshes[0].node_count = 0
        self._meshes[0].nodes = None
        self._desc = rt.abi.SceneDesc.from_buffer_copy(d)
        self._desc.meshes = self._meshes

    def desc(self):
        return self._desc


def test_mesh_without_a_bvh(rt):
    wd = World(rt, "24")
    dev = wd.upload(rt, WithoutBvh(rt, wd.scene))
    try:
        before = six(rt, dev, wd.mesh)
        other = six(rt, dev, wd.other)
        assert before["NODES_SRC"] == before["NODES"] == before["NODES4"] == before["MID4"] == b""
        frame, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)
        moved = moved_vertices("x", wd.tris)
        dev.update_mesh(wd.mesh, moved)
        got = six(rt, dev, wd.mesh)
        idx = rb.mesh_arrays(wd.scene.desc(), wd.mesh)[1]
        recs = rb.refit(moved, None, idx, np.zeros(0, rb.NODE_DTYPE))[1]
        assert got["TRIANGLES"] == recs.tobytes()
        assert differing(got, before) == ["TRIANGLES"]
        assert differing(six(rt, dev, wd.other), other) == []
        again, _ = dev.render(wd.cam, wd.st, wd.fc, W, H, total_frame_index=TFI)    # no box: not stale, nothing to see
        assert np.array_equal(tb.bits(again), tb.bits(frame))
    finally:
        dev.close()
