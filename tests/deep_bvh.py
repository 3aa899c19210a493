"""A mesh whose BVH2 is made by hand, so that a traversal's stack occupancy is known in closed form.

The host builders stay shallow on request (graded triangle fans end at depth <= 12), but rt_mesh::nodes comes
from the caller: any valid BVH2 may be handed to rt_scene_upload.  `caterpillar(L)` is the tree that costs the
device's BVH4 walk the most stack per BVH2 level:

    R_i (interior) -> A_i (interior) -> R_{i+1}, leaf
                      B_i (interior) -> leaf, leaf            i = 0 .. L-1;  R_L is a leaf

The BVH4 collapse (build_bvh4, rt_kernels.hip) merges R_i with A_i and B_i: L BVH4 levels, each with the slots
{R_{i+1}, leaf, leaf, leaf}.  A ray that visits slot 0 first leaves 3 entries behind per level and pushes 4 at the
last: 3L + 1 entries, which is exactly the upload's bound (mesh_depth = need + 1 = 3L + 1; 4L + 1 with the
markers of rt_scene_config::traversal_ref).  The BVH2's own depth is 2L + 1, which the reference's and the
oracle's node_stack[64] walk for every L used here (L <= 21: depth 43).

    L    tree nodes   BVH2 depth   3L + 1
    4        25            9         13      just past the LDS-only fast path (sp > 16 - 4)
    5        31           11         16      the last LDS level
    6        37           13         19      three spilled levels
    20      121           41         61      1 + 61 + 2 = 64: the deepest scene the upload accepts
    21      127           43         64      refused (67 > 64)

(The node array has one entry more: index 1 is the BVHStorage_Scalar padding entry, RT/bvh.h.)

Each leaf holds one triangle, in creation order: leaf of A_i = 3i, leaves of B_i = 3i + 1 and 3i + 2, R_L = 3L, so
triangle k hangs off BVH4 level min(k // 3, L - 1) and, for a slot-0-first ray, waits at stack level >= 3*(k // 3).
Triangle k is [[x, y, z], [x + 0.8, y, z], [x, y + 0.8, z]] with x = k % 8, y = k // 8, z = 0.05 k: the z values
differ, so t, hit_p and n identify the triangle, and the mesh's box has thickness.

Two box variants:
* loose: every node's box is the mesh's bounds padded by 0.5.  A valid BVH; a ray that enters the box has every
  child pushed.  The split axes cycle i % 3, (i+1) % 3, (i+2) % 3 over R_i, A_i, B_i, and a child pair is visited
  left first when the ray's direction is positive on the pair's axis: a ray with every component > 0 goes down
  slot 0 first at every level (3L + 1 entries), one with every component < 0 takes the leaves first (never more
  than 4), mixed signs fall in between.
* tight: boxes computed bottom-up from the triangles.  For hit / miss parity only, no occupancy claim.  A leaf's
  box is its triangle's, with a half extent of 0.01 where the triangle has none (z): the reference's slab test
  needs tn < tf strictly (RT/intersection.cpp:128), so a one-triangle leaf of zero thickness is never entered.
"""
import ctypes as C

import numpy as np

DIR = np.array([0.02, 0.03, 1.0])
SIGNS = {"deep": (1, 1, 1), "leaf": (-1, -1, -1), "ppn": (1, 1, -1), "pnp": (1, -1, 1), "npp": (-1, 1, 1)}
START = 7.0          # a ray starts this far before the point it is aimed at


def triangles(L):
    k = np.arange(3*L + 1)
    x, y, z = (k % 8).astype(np.float64), (k // 8).astype(np.float64), 0.05*k
    a = np.stack([x, y, z], 1)
    return np.stack([a, a + [0.8, 0.0, 0.0], a + [0.0, 0.8, 0.0]], 1).astype(np.float32)


def caterpillar(L):
    """The BVH2 as a list of dicts {left, count, axis} in node-array order (index 1 is padding): interior nodes
    have count 0 and left = the left child (right = left + 1); leaves have count 1 and left = their triangle."""
    assert L >= 1
    nodes = [None, {"left": 0, "count": 0, "axis": 0, "pad": True}]
    tri = [0]

    def leaf():
        tri[0] += 1
        return {"left": tri[0] - 1, "count": 1, "axis": 0}

    r = {"left": 0, "count": 0, "axis": 0}
    nodes[0] = r
    for i in range(L):
        a = {"left": 0, "count": 0, "axis": (i + 1) % 3}
        b = {"left": 0, "count": 0, "axis": (i + 2) % 3}
        r["left"], r["axis"] = len(nodes), i % 3
        nodes += [a, b]
        nxt = {"left": 0, "count": 0, "axis": 0}
        a["left"] = len(nodes)
        nodes += [nxt, leaf()]
        b["left"] = len(nodes)
        nodes += [leaf(), leaf()]
        r = nxt
    r.update(leaf())
    assert tri[0] == 3*L + 1 and len(nodes) == 6*L + 2
    return nodes


def interior(nodes, i):
    n = nodes[i]
    return n["count"] == 0 and n["left"] != 0 and n["left"] + 1 < len(nodes)


def bvh2_depth(nodes, i=0):
    if not interior(nodes, i):
        return 1
    return 1 + max(bvh2_depth(nodes, nodes[i]["left"]), bvh2_depth(nodes, nodes[i]["left"] + 1))


def bvh4_need(nodes, i=0):
    """build_bvh4's bound restated: (need, levels) below the BVH4 node made from BVH2 interior node i -- the
    stack entries a walk below it can hold, and its BVH4 levels.  The upload takes mesh_depth = need + 1 and,
    for a reference-unit walk (a marker per level), need + 1 + levels."""
    slots = []
    for c in (nodes[i]["left"], nodes[i]["left"] + 1):
        slots += [nodes[c]["left"], nodes[c]["left"] + 1] if interior(nodes, c) else [c]
    below = [bvh4_need(nodes, m) for m in slots if interior(nodes, m)]
    return (len(slots) - 1 + max([b[0] for b in below], default=0), 1 + max([b[1] for b in below], default=0))


def mesh_depth(nodes):
    """(mesh_depth, mesh_depth_ref) as rt_scene_upload computes them for this BVH2."""
    if not interior(nodes, 0):
        return 1, 0                                # a one-leaf mesh: one entry, no BVH4 level
    need, levels = bvh4_need(nodes)
    return need + 1, need + 1 + levels


def boxes(nodes, tris, variant):
    """Per node (centre, half extent), float32."""
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    if variant == "loose":
        p, r = 0.5*(lo + hi), 0.5*(hi - lo) + 0.5
        return [(p.astype(np.float32), r.astype(np.float32))]*len(nodes)
    assert variant == "tight"
    out = [None]*len(nodes)

    def rec(i):
        n = nodes[i]
        if n["count"]:
            t = tris[n["left"]:n["left"] + n["count"]].reshape(-1, 3).astype(np.float64)
            a, b = t.min(0), t.max(0)
            c, h = 0.5*(a + b), np.maximum(0.5*(b - a), 0.01)
            a, b = c - h, c + h
        else:
            (a0, b0), (a1, b1) = rec(n["left"]), rec(n["left"] + 1)
            a, b = np.minimum(a0, a1), np.maximum(b0, b1)
        out[i] = (a, b)
        return a, b
    rec(0)
    out[1] = out[0]
    res = []
    for a, b in out:
        p = (0.5*(a + b)).astype(np.float32)
        r = (0.5*(b - a)).astype(np.float32)
        # float32 rounding of centre and half extent must not lose a corner
        while np.any(p.astype(np.float64) - r > a) or np.any(p.astype(np.float64) + r < b):
            r = np.nextafter(r, np.float32(np.inf))
        res.append((p, r))
    return res


def node_array(rt, nodes, bx):
    arr = (rt.abi.BvhNode * len(nodes))()
    for i, n in enumerate(nodes):
        p, r = bx[i]
        arr[i].bv_p = rt.abi.V3(*[float(v) for v in p])
        arr[i].bv_r = rt.abi.V3(*[float(v) for v in r])
        if n.get("pad"):
            continue                               # padding: a zeroed entry but for its box
        arr[i].left_first, arr[i].count, arr[i].split_axis = n["left"], n["count"], n["axis"]
    return arr


class DeepScene:
    """One diffuse material, a sky, a diffuse plane behind the mesh (z = 12), a sphere light between the two and
    the mesh.  The triangles face +z and a surface seen from behind is left into air (RT/integrators.cpp:619-638),
    so a camera whose rays are deep-first (below) shades none of them: its rays reach the plane, whose bounces
    come back onto the triangles' fronts, and the shadow rays from there to the light (towards +x, +y, +z from
    every triangle) are deep-first again.  The mesh is made through create_mesh / add_mesh so that the host model and the top level are real; desc() is
    a copy of the host scene's rt_scene_desc whose mesh has the hand-made BVH2 instead (nodes, node_count,
    triangles in leaf order, identity indices).  host_desc() is the host builder's own BVH over the same
    triangles.  Anything with desc() uploads (DeviceScene)."""

    def __init__(self, rt, L, variant="loose", spheres=0):
        self.rt, self.L, self.variant = rt, L, variant
        self.tris = triangles(L)
        s = rt.Scene()
        m = s.add_diffuse_material((0.7, 0.6, 0.5), 1.5)
        light = s.add_emissive_material((30.0, 28.0, 25.0))
        self.sphere_ids = [s.add_sphere(m, 0.15, rt.translate((-1.0 - 0.4*(i % 8), 0.5*(i // 8), 0.3*(i % 5))))
                           for i in range(spheres)]
        self.mesh_prim = s.add_mesh(m, s.create_mesh(self.tris), rt.identity())
        self.light_prim = s.add_sphere(light, 0.5, rt.translate((10.0, 10.0, 5.0)))
        s.add_plane(m, (0.0, 0.0, -1.0), -12.0)      # z = 12, facing the mesh and the camera; behind every ray origin
        s.set_sky((0.6, 0.7, 0.9), (0.2, 0.2, 0.2))
        s.set_ambient_light((0.05, 0.1, 0.15))       # the Whitted integrator reads it
        s.create_scene_bvh()
        self.scene = s
        self.nodes = caterpillar(L)
        d = s.desc()
        assert d.mesh_count == 1 and d.meshes[0].triangle_count == len(self.tris)
        self._nodes = node_array(rt, self.nodes, boxes(self.nodes, self.tris, variant))
        self._tris = np.ascontiguousarray(self.tris)
        self._indices = (C.c_uint32 * len(self.tris))(*range(len(self.tris)))
        self._meshes = (rt.abi.Mesh * 1)(d.meshes[0])
        self._meshes[0].nodes = self._nodes
        self._meshes[0].node_count = len(self.nodes)
        self._meshes[0].triangles = self._tris.ctypes.data_as(C.POINTER(rt.abi.V3))
        self._meshes[0].indices = self._indices
        self._desc = rt.abi.SceneDesc.from_buffer_copy(d)
        self._desc.meshes = self._meshes

    def desc(self):
        return self._desc

    def host_desc(self):
        return self.scene.desc()

    def ambient_light(self):
        return self.scene.ambient_light()

    def comb_top_level(self):
        """Replace the top-level BVH by a hand-made comb: T_i (interior) -> T_{i+1}, a leaf of two of the small
        spheres; the last T is a leaf of the mesh and the light.  Every box is the scene's bounds (a valid BVH,
        every child pushed); split axes cycle, so a ray with every component > 0 goes down the chain first and
        enters the mesh with one pending entry per comb level.  Returns the comb's depth."""
        rt = self.rt
        assert len(self.sphere_ids) >= 2 and len(self.sphere_ids) % 2 == 0
        d = self.scene.desc()
        p, r = np.array(list(d.bvh_nodes[0].bv_p)), np.array(list(d.bvh_nodes[0].bv_r))
        levels = len(self.sphere_ids) // 2
        n = 2 + 2*levels
        arr = (rt.abi.BvhNode * n)()
        order = list(self.sphere_ids) + [self.mesh_prim, self.light_prim]
        assert sorted(order) == sorted(d.bvh_indices[i] for i in range(d.bvh_index_count))
        for i in range(n):
            arr[i].bv_p, arr[i].bv_r = rt.abi.V3(*p), rt.abi.V3(*(r + 0.25))
        cur = 0
        for i in range(levels):
            arr[cur].left_first, arr[cur].count, arr[cur].split_axis = 2 + 2*i, 0, i % 3
            leaf = 3 + 2*i
            arr[leaf].left_first, arr[leaf].count = 2*i, 2
            cur = 2 + 2*i
        arr[cur].left_first, arr[cur].count = 2*levels, 2
        self._top = arr
        self._top_indices = (C.c_uint32 * len(order))(*order)
        self._desc.bvh_nodes, self._desc.bvh_node_count = arr, n
        self._desc.bvh_indices, self._desc.bvh_index_count = self._top_indices, len(order)
        return levels + 1

    # ---- rays

    def centroid(self, k):
        return self.tris[k].astype(np.float64).mean(0)

    def rays(self):
        """[(kind, k, RayQuery)]: per triangle k a deep-first ray (+,+,+) and a leaf-first ray (-,-,-), lane by
        lane, so that a wave holds lanes at sp ~ 3L beside lanes at sp ~ 3; then the mixed-sign directions; then
        rays through the gaps between the triangles (they cross the box and miss).  kind "miss" has k = -1.
        The list fills more than two of rt_debug_intersect's blocks of 128 (for small L it is repeated whole) and
        its count is no multiple of 128."""
        rt = self.rt
        out = []

        def ray(kind, k, at, sign):
            d = DIR*np.array(sign, np.float64)
            d = (d/np.linalg.norm(d)).astype(np.float32)
            o = (at - START*d.astype(np.float64)).astype(np.float32)
            out.append((kind, k, rt.abi.RayQuery(rt.abi.V3(*o), rt.abi.V3(*d), 3.0e38, 0)))

        n = len(self.tris)
        for k in range(n):
            ray("deep", k, self.centroid(k), SIGNS["deep"])
            ray("leaf", k, self.centroid(k), SIGNS["leaf"])
        for kind in ("ppn", "pnp", "npp"):
            for k in range(n):
                ray(kind, k, self.centroid(k), SIGNS[kind])
        for j in range(16):                          # the gap right of and above triangle k's cell
            k = (j*5) % n
            ray("miss", -1, self.tris[k][0].astype(np.float64) + [0.9, 0.9, 0.0], list(SIGNS.values())[j % 5])
        out = out*(-(-257 // len(out)))              # small L: the whole list again, until it fills two blocks
        if len(out) % 128 == 0:
            ray("miss", -1, self.tris[0][0].astype(np.float64) + [0.9, 0.9, 0.0], SIGNS["deep"])
        return out

    def camera(self, w, h):
        """Looks along (+,+,+)-ish at the mesh with a narrow field of view: primary rays are deep-first."""
        rt = self.rt
        cam = rt.abi.Camera()
        cam.vfov = rt.DEG_TO_RAD * 24.0
        cam.aspect_ratio = w / h
        cam.lens_radius = 0.0
        cam.focus_distance = 10.0
        cam.p = rt.v3(-6.0, -8.0, -14.0)
        lo, hi = self.tris.reshape(-1, 3).min(0), self.tris.reshape(-1, 3).max(0)
        rt.aim_camera_at(cam, tuple(float(v) for v in 0.5*(lo + hi)))
        rt.recompute_camera(cam)
        return cam


def same_hit(a, b, occlusion):
    """test_intersect_bit_exact's comparison (tests/test_gpu_parity.py): every field of a closest hit bit for
    bit; an occlusion query is a b32, hit or miss only."""
    if occlusion:
        return (a.primitive == 0xFFFFFFFF) == (b.primitive == 0xFFFFFFFF)
    if a.primitive != b.primitive:
        return False
    return a.primitive == 0xFFFFFFFF or (a.t == b.t and tuple(a.n) == tuple(b.n) and tuple(a.hit_p) == tuple(b.hit_p))
