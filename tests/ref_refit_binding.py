"""ctypes binding of tests/ref_refit/libref_refit.so (TEST INFRASTRUCTURE).

The CPU checker of the mesh refit ("Deforming meshes"): triangle records, slot-order normals, BVH2 boxes and
the BVH4's child and skipped-level boxes restated in plain C.  Only tests/ loads it.  Also what the CPU and the GPU
tests share: a mesh's arrays out of an rt_scene_desc, the generated meshes, the displacements and the hand-made cases.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "ref_refit", "libref_refit.so")

NODE_DTYPE = np.dtype([("bv_p", "<f4", (3,)), ("bv_r", "<f4", (3,)), ("left_first", "<u4"), ("count", "<u2"),
                       ("split_axis", "<u2")])
assert NODE_DTYPE.itemsize == 32

_lib = None


def _rt():
    import sys
    return sys.modules["buas_pathtracer_amd"]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} missing: run make -C tests/ref_refit (or __graft_entry__.build())")
    lib = C.CDLL(LIB)
    fp, up, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_void_p
    lib.ref_refit.restype = C.c_int
    lib.ref_refit.argtypes = [C.c_uint32, fp, fp, up, C.c_uint32, vp, fp, fp]
    lib.ref_refit_bvh4.restype = None
    lib.ref_refit_bvh4.argtypes = [C.c_uint32, vp, C.c_uint32, up, fp, fp]
    _lib = lib
    return lib


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def refit(triangles, normals, indices, nodes):
    """ref_refit: triangles [n,3,3] and normals (or None) in the original order, indices slot -> original, nodes a
    NODE_DTYPE array -> (refitted nodes, triangle records [n,12], slot-order normals [n,9] or None)."""
    t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
    nn = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
    idx = np.ascontiguousarray(indices, np.uint32)
    out_nodes = np.array(nodes, NODE_DTYPE, copy=True)
    recs = np.full((idx.size, 12), -7.0, np.float32)
    out_n = None if nn is None else np.full((idx.size, 9), -7.0, np.float32)
    code = load().ref_refit(idx.size, _fp(t), _fp(nn), idx.ctypes.data_as(C.POINTER(C.c_uint32)), out_nodes.size,
                            out_nodes.ctypes.data_as(C.c_void_p), _fp(recs), _fp(out_n))
    assert code == 0, "the checker found no tree"
    return out_nodes, recs, out_n


def bvh4(nodes, src, nodes4, mid4):
    """ref_refit_bvh4: the BVH4 tables (copies of nodes4 [k,32] and mid4 [k,12]) reboxed from `nodes`."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    src = np.ascontiguousarray(src, np.uint32)
    n4 = np.array(nodes4, np.float32, copy=True).reshape(-1, 32)
    m4 = np.array(mid4, np.float32, copy=True).reshape(-1, 12)
    assert n4.shape[0] == src.size == m4.shape[0]
    load().ref_refit_bvh4(nodes.size, nodes.ctypes.data_as(C.c_void_p), src.size, src.ctypes.data_as(C.POINTER(C.c_uint32)),
                          _fp(n4), _fp(m4))
    return n4, m4


def mesh_arrays(desc, m):
    """Copies of mesh m's arrays in an rt_scene_desc: (triangles in slot order [n,3,3], indices, normals in the original
    order or None, nodes)."""
    M = desc.meshes[m]
    n = M.triangle_count
    tris = np.ctypeslib.as_array(C.cast(M.triangles, C.POINTER(C.c_float)), (n, 3, 3)).copy() if n else np.zeros((0, 3, 3), np.float32)
    idx = np.ctypeslib.as_array(M.indices, (n,)).copy() if n else np.zeros(0, np.uint32)
    nrm = None
    if M.has_normals and M.normals and n:
        nrm = np.ctypeslib.as_array(C.cast(M.normals, C.POINTER(C.c_float)), (n, 3, 3)).copy()
    nodes = np.zeros(M.node_count, NODE_DTYPE)
    if M.node_count:
        C.memmove(nodes.ctypes.data, M.nodes, 32*M.node_count)
    return tris, idx, nrm, nodes


def original_order(tris_slot, indices):
    """The triangles in the order create_mesh took them in, from the slot-order array."""
    out = np.zeros_like(tris_slot)
    out[indices] = tris_slot
    return out


def generated(target, seed=3):
    """rth_generate_mesh -> (triangles [n,3,3], normals [n,3,3])."""
    rt = _rt()
    n = rt.lib().rth_generate_mesh(target, seed, None, None)
    tris, nrm = np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3), np.float32)
    vp = C.POINTER(rt.abi.V3)
    rt.lib().rth_generate_mesh(target, seed, tris.ctypes.data_as(vp), nrm.ctypes.data_as(vp))
    return tris, nrm


def displaced(tris, amount, phase=0.0):
    """A sinusoidal displacement along y and x that grows the mesh's bounds: the same function of a vertex's position
    wherever it occurs, so shared vertices stay shared."""
    t = np.asarray(tris, np.float64)
    out = t.copy()
    out[..., 1] += amount*(1.0 + np.sin(3.0*t[..., 0] + phase))
    out[..., 0] += 0.5*amount*np.cos(2.0*t[..., 2] - phase)
    return out.astype(np.float32)


def node_bytes(nodes):
    return np.ascontiguousarray(nodes, NODE_DTYPE).tobytes()


def boxes_equal(a, b):
    """== per float (zeros of either sign are equal), and the topology byte for byte."""
    return (np.array_equal(a["bv_p"], b["bv_p"]) and np.array_equal(a["bv_r"], b["bv_r"]) and
            np.array_equal(a["left_first"], b["left_first"]) and np.array_equal(a["count"], b["count"]) and
            np.array_equal(a["split_axis"], b["split_axis"]))


def children_first(nodes):
    """A hand-made tree's node array renumbered so that every pair of children precedes its parent: node 0 and the
    padding entry stay, the other pairs take the reverse of their order.  -> the renumbered NODE_DTYPE array."""
    nodes = np.asarray(nodes, NODE_DTYPE)
    n = nodes.size
    assert n % 2 == 0
    new = np.arange(n)
    for i in range(2, n):
        new[i] = 2 + (n - 2 - 2) - 2*((i - 2)//2) + (i % 2)      # pair k of (n - 2)/2 -> pair (last - k)
    out = np.zeros(n, NODE_DTYPE)
    for i in range(n):
        e = nodes[i].copy()
        if e["count"] == 0 and e["left_first"] != 0 and e["left_first"] + 1 < n:
            e["left_first"] = new[e["left_first"]]
        out[new[i]] = e
    return out
