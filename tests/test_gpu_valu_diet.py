"""Bit identity of the walks whose instruction count was cut: the ray prologue's reuse of the world ray's 1/d at
translate-only leaves, and the BVH4 node's pushes by rank (push_children4, rt_kernels.hip).

Both changes claim the same bits by construction.  The frames below hold them to it on a scene that has every
kind of top-level leaf the prologue tells apart -- a translate-only box, a rotated box, a translate-only
instance of a mesh, a scaled and rotated instance of the same mesh, a sphere light, two planes -- from a camera
whose rays are plain (every component of origin and direction finite and non-zero: the reuse is taken) and
from a camera on an axis (an origin component is exactly 0: it is not).  The push order is held against the
hand-made trees of tests/deep_bvh.py, whose stack occupancy is known in closed form, with rays in all eight
direction octants: every order of the two pairs and within each pair, loose boxes (all four children pushed)
and tight ones (partial hit masks), past the LDS levels (L = 6) and up to the 64-entry limit (L = 20).

Comparisons are exact.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import deep_bvh as db
import oracle_binding as ob

W, H, SPP = 96, 64, 4
OCTANTS = list(itertools.product((1, -1), repeat=3))


def diet_scene(rt):
    s = rt.Scene()
    grey = s.add_diffuse_material((0.7, 0.7, 0.65), 1.5)
    red = s.add_diffuse_material((0.8, 0.3, 0.25), 1.4, checkers=True)
    light = s.add_emissive_material((14.0, 13.0, 11.0))
    s.add_plane(grey, (0.0, 1.0, 0.0), -1.0)                         # a floor
    s.add_plane(red, (0.0, 0.0, -1.0), -16.0)                        # a back wall
    s.add_box(red, (0.9, 1.2, 0.7), rt.translate((-3.1, 0.4, 6.3)))
    s.add_box(grey, (0.8, 0.9, 1.1), rt.translate((3.3, 0.2, 7.9)) * rt.rotate_y(0.6) * rt.rotate_x(0.2))
    n = rt.lib().rth_generate_mesh(400, 11, None, None)
    tris = np.zeros((n, 3, 3), np.float32)
    nn = np.zeros((n, 3, 3), np.float32)
    rt.lib().rth_generate_mesh(400, 11, tris.ctypes.data_as(C.POINTER(rt.abi.V3)), nn.ctypes.data_as(C.POINTER(rt.abi.V3)))
    tris *= np.float32(4.0)                                          # radius about 1.2: a good part of the frame
    mesh = s.create_mesh(tris, nn)
    s.add_mesh(grey, mesh, rt.translate((-0.9, 0.7, 8.2)))
    s.add_mesh(red, mesh, rt.translate((1.4, 1.1, 5.1)) * rt.rotate_y(1.1) * rt.rotate_x(-0.3) * rt.scale((0.6, 0.8, 0.7)))
    s.add_sphere(light, 0.8, rt.translate((0.7, 6.2, 4.4)))
    s.set_sky((0.5, 0.6, 0.8), (0.15, 0.15, 0.15))
    s.create_scene_bvh()
    return s


def camera(rt, p, at):
    cam = rt.abi.Camera()
    cam.vfov = rt.DEG_TO_RAD * 50.0
    cam.aspect_ratio = W / H
    cam.lens_radius = 0.0
    cam.focus_distance = 10.0
    cam.p = rt.v3(*p)
    rt.aim_camera_at(cam, at)
    rt.recompute_camera(cam)
    return cam


_scene = {}


def scene_and_settings(rt):
    if not _scene:
        st, _ = rt.default_settings()
        st.samples_per_pixel = SPP
        _scene["v"] = (diet_scene(rt), st, rt.load_reconstruction_kernel("Mitchell Netravali"))
    return _scene["v"]


VIEWS = {"plain": ((0.37, 2.5, -9.0), (0.1, 1.0, 6.0)), "on_axis": ((0.0, 2.5, -9.0), (0.0, 1.0, 6.0))}
_oracle = {}


def oracle_frame(rt, view):
    """(camera, frame, stats, the restated device walk's counts), rendered once per view and left unchanged."""
    if view not in _oracle:
        s, st, fc = scene_and_settings(rt)
        cam = camera(rt, *VIEWS[view])
        with ob.gpu_walk() as walk:
            frame, cs = ob.render(s.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
        _oracle[view] = (cam, frame, cs, walk.result)
    return _oracle[view]


def test_scene_has_every_leaf_kind(rt):
    """CPU: the scene is what the GPU test needs, and the oracle renders it deterministically."""
    s, st, fc = scene_and_settings(rt)
    d = s.desc()
    assert d.plane_count == 2 and d.mesh_count == 1
    kinds = {}
    for i in range(d.primitive_count):
        p = d.primitives[i]
        e = d.transforms[p.transform_index].inverse.e
        lin = np.array([[e[r][c] for c in range(3)] for r in range(3)])
        kinds.setdefault((p.type, bool(np.array_equal(lin, np.eye(3)))), 0)
        kinds[(p.type, bool(np.array_equal(lin, np.eye(3))))] += 1
    a = rt.abi
    for key in ((a.RT_PRIMITIVE_BOX, True), (a.RT_PRIMITIVE_BOX, False), (a.RT_PRIMITIVE_MESH, True),
                (a.RT_PRIMITIVE_MESH, False), (a.RT_PRIMITIVE_SPHERE, True)):
        assert kinds.get(key) == 1, (key, kinds)
    for view in VIEWS:
        cam, x, sx, walk = oracle_frame(rt, view)
        assert (cam.p.x == 0.0) == (view == "on_axis") and cam.p.y != 0.0 and cam.p.z != 0.0
        assert np.isfinite(x).all() and sx.shadow_rays > 1000
        # both ray kinds reach the meshes' nodes and leaves in numbers
        assert min(walk["calls"]) > 1000 and min(walk["nodes"]) > 1000 and min(walk["leaves"]) > 300, walk
    cam, x, sx, _ = oracle_frame(rt, "on_axis")
    y, sy = ob.render(d, cam, st, fc, W, H, rng_mode=0, threads=1)
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and sx.shadow_rays == sy.shadow_rays


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["plain", "on_axis"])
def test_frame_is_the_oracles(rt, view):
    """The exact-splat 96x64, 4 spp frame is the oracle's bit for bit, with its ray counts, and the TraversalStats
    are those of the oracle's restatement of the device's walk.  `plain`: no component of the camera's position
    is 0, so its rays take the translate-only leaves' shortcut; `on_axis`: x = 0 exactly, so none does."""
    from parity_report import REPORT
    s, st, fc = scene_and_settings(rt)
    cam, cframe, cs, restated = oracle_frame(rt, view)
    dev = rt.DeviceScene(s, 0)
    try:
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
            frame, gs = dev.render(cam, st, fc, W, H)
        assert gs.splat_mode == rt.abi.RT_SPLAT_EXACT
    finally:
        dev.close()
    same = np.array_equal(np.ascontiguousarray(frame).view(np.uint32), np.ascontiguousarray(cframe).view(np.uint32))
    got = {"calls": [int(gs.traversal[k].mesh_intersection_count) for k in range(2)],
           "leaves": [int(gs.traversal[k].mesh_leaf_traversals) for k in range(2)],
           "nodes": [int(gs.traversal[k].mesh_node_traversals) for k in range(2)],
           "bvh": [int(gs.traversal[k].mesh_bvh_traversals) for k in range(2)]}
    want = {k: [int(v) for v in restated[k]] for k in got}
    REPORT[f"valu_diet_frame_{view}"] = {
        "identical_to_oracle": bool(same), "pixels_identical": float(np.all(frame == cframe, axis=2).mean()),
        "rays": [int(gs.closest_hit_rays), int(gs.shadow_rays)], "oracle_rays": [int(cs.closest_hit_rays), int(cs.shadow_rays)],
        "traversal": got, "restated": want}
    print(REPORT[f"valu_diet_frame_{view}"])
    assert (gs.closest_hit_rays, gs.shadow_rays, gs.samples) == (cs.closest_hit_rays, cs.shadow_rays, W*H*SPP)
    assert same, REPORT[f"valu_diet_frame_{view}"]
    assert got == want


def octant_rays(rt, sc):
    """Per triangle one ray from every direction octant, aimed at its centroid (deep_bvh.DeepScene.rays' form),
    then rays through the gaps; the count is no multiple of 128."""
    out = []

    def ray(at, sign):
        d = db.DIR*np.array(sign, np.float64)
        d = (d/np.linalg.norm(d)).astype(np.float32)
        o = (at - db.START*d.astype(np.float64)).astype(np.float32)
        out.append(rt.abi.RayQuery(rt.abi.V3(*o), rt.abi.V3(*d), 3.0e38, 0))

    n = len(sc.tris)
    for k in range(n):
        for sign in OCTANTS:
            ray(sc.centroid(k), sign)
    for j in range(16):
        k = (j*5) % n
        ray(sc.tris[k][0].astype(np.float64) + [0.9, 0.9, 0.0], OCTANTS[j % 8])
    if len(out) % 128 == 0:
        ray(sc.tris[0][0].astype(np.float64) + [0.9, 0.9, 0.0], OCTANTS[0])
    return out


def test_octant_rays_cover_every_order(rt):
    """CPU: eight sign patterns per triangle, and through the oracle every aimed ray hits the mesh."""
    sc = db.DeepScene(rt, 4)
    q = octant_rays(rt, sc)
    assert len(q) % 128 != 0
    signs = {tuple(np.sign([r.d.x, r.d.y, r.d.z]).astype(int)) for r in q}
    assert signs == set(OCTANTS)
    hits = ob.intersect(sc.desc(), q, False)
    assert sum(h.primitive == sc.mesh_prim for h in hits) >= 8*len(sc.tris)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["loose", "tight"])
@pytest.mark.parametrize("L", [4, 6, 20])
def test_push_order_in_every_octant(rt, L, variant):
    """rt_debug_intersect against the oracle, every field bit for bit (occlusion: hit or miss), for rays in all
    eight octants: 0 mismatches.  L = 4 stays in the LDS levels, L = 6 spills three, L = 20 reaches the 64-entry
    limit's neighbourhood (61 entries), where the rank form must spill and drop exactly as the sequential one."""
    from parity_report import REPORT
    sc = db.DeepScene(rt, L, variant)
    q = octant_rays(rt, sc)
    want = {occ: ob.intersect(sc.desc(), q, occ) for occ in (False, True)}
    dev = rt.DeviceScene(sc, 0)
    try:
        got = {occ: dev.intersect(q, occ) for occ in (False, True)}
    finally:
        dev.close()
    mism = {occ: sum(not db.same_hit(a, b, occ) for a, b in zip(got[occ], want[occ])) for occ in (False, True)}
    REPORT[f"valu_diet_push_order_L{L}_{variant}"] = {"rays": len(q), "mismatches_closest": mism[False],
                                                      "mismatches_occlusion": mism[True]}
    assert sum(h.primitive == sc.mesh_prim for h in want[False]) >= 8*len(sc.tris)
    assert mism == {False: 0, True: 0}, f"{mism} of {len(q)} differ"
