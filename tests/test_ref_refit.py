"""The mesh refit on the CPU ("Deforming meshes"): rth_update_mesh against the builder, against the plain-C
checker (tests/ref_refit) and on the hand-made cases.  Every comparison is bit for bit; against the builder `==` per
float (zeros of either sign are equal), among the refits bytes."""
import itertools

import numpy as np
import pytest

import deep_bvh
import ref_refit_binding as rb

METHODS = ["RTH_BVH_MIDPOINT_SPLIT", "RTH_BVH_SAH_BINNED", "RTH_BVH_SAH_FULL"]


def method(rt, name):
    return getattr(rt.abi, name)


def mesh_scene(rt, tris, normals=None, how="RTH_BVH_SAH_BINNED"):
    s = rt.Scene()
    m = s.create_mesh(tris, normals, method(rt, how))
    return s, m


def quantised(tris):
    """Multiples of 2^-10: a translation by a power of two is then exact, and so is every box of the builder."""
    return (np.round(np.asarray(tris, np.float64)*1024.0)/1024.0).astype(np.float32)


@pytest.mark.parametrize("how", METHODS)
@pytest.mark.parametrize("target", [1, 3000])
def test_identity_refit_reproduces_the_builder(rt, target, how):
    tris, nrm = rb.generated(target)
    assert tris.shape[0] == {1: 24, 3000: 3024}[target]
    s, m = mesh_scene(rt, tris, nrm, how)
    t0, idx, n0, nodes0 = rb.mesh_arrays(s.desc(), m)
    s.update_mesh(m, tris)
    t1, idx1, n1, nodes1 = rb.mesh_arrays(s.desc(), m)
    assert rb.boxes_equal(nodes1, nodes0)
    assert t1.tobytes() == t0.tobytes() and idx1.tobytes() == idx.tobytes() and n1.tobytes() == n0.tobytes()
    # and the checker on the builder's nodes
    nodes2, recs, sn = rb.refit(tris, nrm, idx, nodes0)
    assert rb.node_bytes(nodes2) == rb.node_bytes(nodes1)


@pytest.mark.parametrize("how", METHODS)
@pytest.mark.parametrize("target", [1, 3000])
def test_moved_vertices_equal_the_checker(rt, target, how):
    tris, nrm = rb.generated(target)
    s, m = mesh_scene(rt, tris, nrm, how)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    moved = rb.displaced(tris, 0.4, 0.3)
    new_n = np.ascontiguousarray(nrm[:, ::-1, :])
    s.update_mesh(m, moved, new_n)
    t1, idx1, n1, nodes1 = rb.mesh_arrays(s.desc(), m)
    want_nodes, recs, slot_n = rb.refit(moved, new_n, idx, nodes0)
    assert rb.node_bytes(nodes1) == rb.node_bytes(want_nodes)
    assert not rb.boxes_equal(nodes1, nodes0)
    assert idx1.tobytes() == idx.tobytes()
    assert t1.tobytes() == moved[idx].tobytes() and n1.tobytes() == new_n.tobytes()
    # the checker's records against the definition, in numpy's float32
    a, b, c = moved[idx][:, 0], moved[idx][:, 1], moved[idx][:, 2]
    z = np.zeros((len(idx), 1), np.float32)
    assert recs.tobytes() == np.concatenate([a, z, b - a, z, c - a, z], 1).astype(np.float32).tobytes()
    assert slot_n.tobytes() == new_n[idx].reshape(-1, 9).tobytes()
    # NULL normals keep the stored ones
    s.update_mesh(m, tris)
    assert rb.mesh_arrays(s.desc(), m)[2].tobytes() == new_n.tobytes()


@pytest.mark.parametrize("how", METHODS)
@pytest.mark.parametrize("target", [1, 3000])
def test_translated_mesh_equals_a_fresh_build(rt, target, how):
    tris = quantised(rb.generated(target)[0])
    shift = np.array([8.0, -16.0, 32.0], np.float32)
    s, m = mesh_scene(rt, tris, None, how)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    s.update_mesh(m, tris + shift)
    refitted = rb.mesh_arrays(s.desc(), m)[3]
    built_scene, bm = mesh_scene(rt, tris + shift, None, how)
    _, bidx, _, built = rb.mesh_arrays(built_scene.desc(), bm)
    assert bidx.tobytes() == idx.tobytes()                  # the build kept the topology
    assert rb.boxes_equal(refitted, built)
    reach = refitted["bv_r"].any(1)
    assert np.array_equal(refitted["bv_p"][reach], nodes0["bv_p"][reach] + shift)
    assert np.array_equal(refitted["bv_r"], nodes0["bv_r"])


def numpy_refit(tris, idx, nodes):
    """The definition once more, in numpy's float32 (min and max on values that hold no zero of either sign)."""
    out = nodes.copy()
    n = len(nodes)
    h = np.float32(0.5)

    def rec(i):
        e = nodes[i]
        if e["count"]:
            t = tris[idx[e["left_first"]:e["left_first"] + e["count"]]]
            lo, hi = t.min(1), t.max(1)
            p, r = h*(lo + hi), h*(hi - lo)
            mn, mx = (p - r).min(0), (p + r).max(0)
        elif e["left_first"] != 0 and e["left_first"] + 1 < n:
            (a0, b0), (a1, b1) = rec(e["left_first"]), rec(e["left_first"] + 1)
            mn, mx = np.minimum(a0, a1), np.maximum(b0, b1)
        else:
            return None
        out[i]["bv_p"], out[i]["bv_r"] = h*(mn + mx), h*(mx - mn)
        return mn, mx
    rec(0)
    return out


def test_one_triangle_is_a_root_leaf(rt):
    tri = np.array([[[0.5, 1.0, 2.0], [1.5, 1.25, 2.0], [0.75, 3.0, 2.5]]], np.float32)
    s, m = mesh_scene(rt, tri)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    assert nodes0[0]["count"] == 1
    moved = tri*np.float32(1.5) + np.float32(0.1)
    s.update_mesh(m, moved)
    nodes1 = rb.mesh_arrays(s.desc(), m)[3]
    assert rb.node_bytes(nodes1) == rb.node_bytes(rb.refit(moved, None, idx, nodes0)[0])
    assert rb.node_bytes(nodes1) == rb.node_bytes(numpy_refit(moved, idx, nodes0))
    assert nodes1[1:].tobytes() == nodes0[1:].tobytes()     # the padding entry keeps its bytes


def test_forty_identical_triangles_are_one_leaf(rt):
    tri = np.tile(np.array([[[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.5]]], np.float32), (40, 1, 1))
    s, m = mesh_scene(rt, tri)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    assert len(nodes0) == 2 and nodes0[0]["count"] == 40
    moved = tri.copy()
    moved[7] += np.float32(2.0)                             # one of them leaves the rest
    s.update_mesh(m, moved)
    nodes1 = rb.mesh_arrays(s.desc(), m)[3]
    assert rb.node_bytes(nodes1) == rb.node_bytes(rb.refit(moved, None, idx, nodes0)[0])
    assert rb.node_bytes(nodes1) == rb.node_bytes(numpy_refit(moved, idx, nodes0))
    assert tuple(nodes1[0]["bv_p"]) == (1.5, 1.5, 2.25) and tuple(nodes1[0]["bv_r"]) == (1.5, 1.5, 1.25)


def test_zeros_of_either_sign_do_not_depend_on_the_order(rt):
    pz, nz = np.float32(0.0), np.float32(-0.0)
    tris = np.array([[[pz, 0.0, 1.0], [pz, 1.0, 1.0], [pz, 0.0, 2.0]],          # flat in x = +0
                     [[nz, 0.5, 1.0], [nz, 1.5, 1.0], [nz, 0.5, 2.0]],          # flat in x = -0
                     [[nz, nz, 1.0], [pz, pz, 1.5], [nz, 0.25, pz]]], np.float32)
    s, m = mesh_scene(rt, tris)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    seen = set()
    for perm in itertools.permutations(range(3)):
        t = tris[list(perm)]
        s.update_mesh(m, t)
        host = rb.node_bytes(rb.mesh_arrays(s.desc(), m)[3])
        assert host == rb.node_bytes(rb.refit(t, None, idx, nodes0)[0])
        seen.add(host[:24])
    assert len(seen) == 1                                   # the root box, whatever slot a triangle is in


@pytest.mark.parametrize("L", [2, 7])
def test_hand_made_tree_with_children_before_parents(rt, L):
    tris = deep_bvh.triangles(L)
    tree = deep_bvh.caterpillar(L)
    arr = deep_bvh.node_array(rt, tree, deep_bvh.boxes(tree, tris, "loose"))
    nodes = np.frombuffer(bytes(arr), rb.NODE_DTYPE).copy()
    flipped = rb.children_first(nodes)
    kids = [(i, flipped[i]["left_first"]) for i in range(2, len(flipped)) if flipped[i]["count"] == 0 and flipped[i]["left_first"]]
    assert kids and all(c < i for i, c in kids)
    idx = np.arange(len(tris), dtype=np.uint32)
    moved = (tris*np.float32(1.25) + np.float32(0.5)).astype(np.float32)
    for tree_nodes in (nodes, flipped):
        got = rb.refit(moved, None, idx, tree_nodes)[0]
        assert rb.node_bytes(got) == rb.node_bytes(numpy_refit(moved, idx, tree_nodes))
        assert got[1].tobytes() == tree_nodes[1].tobytes()  # the padding entry
    # the same boxes under either numbering
    a, b = rb.refit(moved, None, idx, nodes)[0], rb.refit(moved, None, idx, flipped)[0]
    reach = [0] + list(range(2, len(a)))
    box = lambda e: tuple(e["bv_p"]) + tuple(e["bv_r"])
    assert sorted(box(e) for e in a[reach]) == sorted(box(e) for e in b[reach])


def test_collapsed_mesh_has_no_extent(rt):
    tris, _ = rb.generated(1)
    s, m = mesh_scene(rt, tris)
    _, idx, _, nodes0 = rb.mesh_arrays(s.desc(), m)
    point = np.broadcast_to(np.array([0.75, -1.5, 3.0], np.float32), tris.shape).copy()
    s.update_mesh(m, point)
    nodes1 = rb.mesh_arrays(s.desc(), m)[3]
    assert rb.node_bytes(nodes1) == rb.node_bytes(rb.refit(point, None, idx, nodes0)[0])
    reach = [0] + list(range(2, len(nodes1)))
    assert not nodes1["bv_r"][reach].any() and np.all(nodes1["bv_p"][reach] == point[0, 0])
    assert not np.signbit(nodes1["bv_r"][reach]).any()


def test_refusals_change_nothing(rt):
    tris, nrm = rb.generated(1)
    s, m = mesh_scene(rt, tris)                             # without normals
    before = [a.tobytes() for a in rb.mesh_arrays(s.desc(), m) if a is not None]
    bad = tris.copy()
    bad[-1, 2, 1] = np.nan
    far = tris.copy()
    far[3, 0, 0] = np.float32(2.0**41)
    for args, why in (((m, bad), "finite"), ((m, far), "2^40"), ((m, tris, nrm), "without normals"), ((m + 1, tris), "out of range")):
        with pytest.raises(ValueError, match="rth_update_mesh.*" + why.replace("^", r"\^")):
            s.update_mesh(*args)
        assert [a.tobytes() for a in rb.mesh_arrays(s.desc(), m) if a is not None] == before
