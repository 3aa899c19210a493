"""What tests/test_gpu_layout_matrix.py shares between its GPU half and its CPU half (TEST INFRASTRUCTURE).

The matrix renders every frame kind of the device library under the five upload-time layouts of its scene tables
(parity section).  This module holds what does not need a GPU: the layouts, the size of the LDS blob restated
from an rt_scene_desc, the three scenes with the updates applied to them, the CPU side's answer for every kind (the
oracle and the plain-C checkers), and the comparisons.  The CPU-only tests at the top of the test module run all of it.
"""
import ctypes as C

import numpy as np

import oracle_binding as ob
import random_scenes
import recursive_cases as rc
import ref_binding as rb
import ref_deform_binding as db
import ref_features_binding as rf
import ref_recursive_binding as rr
import ref_refit_binding as rfit
import ref_temporal_binding as tb

# ---- the layouts: what rt_scene_upload reads from the environment

SWITCHES = ("RT_LDS_SCENE", "RT_MLIST_MAX", "RT_TOP_PROLOGUE")
LAYOUTS = {
    "L0": {},
    "L1": {"RT_LDS_SCENE": "0"},
    "L2": {"RT_MLIST_MAX": "0"},
    "L3": {"RT_TOP_PROLOGUE": "0"},
    "L4": {"RT_LDS_SCENE": "0", "RT_MLIST_MAX": "0"},
}
SAME_WALK = {"L1": "L0", "L4": "L2"}          # residency does not change the walk: rt_stats::traversal is the same
LDS_BYTES = 32768                             # 16 * LDS_SCENE_Q (rt_kernels.hip)

W, H, SPP, TFI = 64, 48, 4, 3
ADVANCED, WHITTED, GT_RECURSIVE, GT_ITERATIVE, NORMALS, DISTANCES = range(6)
INTEGRATORS = {"gt_iterative": GT_ITERATIVE, "normals": NORMALS, "distances": DISTANCES}
FEATURES = ("normal", "distance", "albedo")
RECURSIVE = {"whitted": WHITTED, "gt_recursive": GT_RECURSIVE}
RECURSIVE_SCENES = ("lights", "c4")           # no mesh (listed_only whatever RT_MLIST_MAX says), and four mesh instances
RECURSIVE_DEPTH = 4
LATE_FUSE = dict(path_pool=1024, fuse_paths=16)     # tests/test_gpu_ramp_shade.py's: the ramp runs the frame's tail


def blob_bytes(rt, desc):
    """The size of the blob build_tables makes (rt_kernels.hip): the seven tables, each padded to 16 bytes.  The
    materials table carries the integrator's `air` entry after the scene's; a transform is two M34 (the rows 0..2 of
    the inverse and of the forward matrix), one in each of two tables; a mesh header is four 32-bit words."""
    a = rt.abi
    pad = lambda n: (n + 15) & ~15
    m34 = 3*C.sizeof(a.M4x4)//4
    assert (C.sizeof(a.Material), C.sizeof(a.Primitive), m34) == (68, 32, 48)
    return (pad((desc.material_count + 1)*C.sizeof(a.Material)) + pad(desc.primitive_count*C.sizeof(a.Primitive)) +
            pad(desc.plane_count*C.sizeof(a.Primitive)) + 2*pad(desc.transform_count*m34) + pad(desc.light_count*4) +
            pad(desc.mesh_count*16))


def mesh_instances(rt, desc):
    return [i for i in range(desc.primitive_count) if desc.primitives[i].type == rt.abi.RT_PRIMITIVE_MESH]


# ---- the scenes

def matrix_scene(rt, stage=0):
    """The matrix scene (seed 1: an environment map, three meshes, one without normals, at most MLIST_MAX mesh slots)
    with NEE on, after `stage` of its two updates -> (scene, cam, st, fc)."""
    scene, cam, st, fc = random_scenes.random_scene(rt, 1, W, H, spp=SPP, mesh_instances=3)
    st.next_event_estimation = 1
    for k in range(stage):
        UPDATES[k](rt, scene, None)
    return scene, cam, st, fc


def moved_primitives(rt, desc):
    """One mesh instance, one box and the first light."""
    kind = lambda t: next(i for i in range(desc.primitive_count) if desc.primitives[i].type == t)
    return kind(rt.abi.RT_PRIMITIVE_MESH), kind(rt.abi.RT_PRIMITIVE_BOX), int(desc.lights[0])


def move_instances(rt, scene, dev):
    mesh, box, light = moved_primitives(rt, scene.desc())
    # (the generated meshes are 0.6 units across and cover five pixels as uploaded: this one comes to the camera)
    scene.set_primitive_transform(mesh, rt.translate((3.0, 2.5, 0.0))*rt.rotate_y(0.9)*rt.scale((8.0, 10.0, 6.0)))
    scene.set_primitive_transform(box, rt.translate((-2.0, 1.5, 6.0))*rt.rotate_x(0.4)*rt.rotate_y(1.1))
    scene.set_primitive_transform(light, rt.translate((3.0, 9.0, 10.0)))
    scene.create_scene_bvh()
    if dev is not None:
        dev.update_instances()


def deform_mesh(rt, scene, dev):
    tris, idx, _, _ = rfit.mesh_arrays(scene.desc(), 0)
    moved = rfit.displaced(rfit.original_order(tris, idx), 0.15, 0.4)
    if dev is not None:
        dev.update_mesh(0, moved)
    scene.update_mesh(0, moved)
    scene.create_scene_bvh()
    if dev is not None:
        dev.update_instances()


UPDATES = (move_instances, deform_mesh)


def overflow_scene(rt):
    """400 mesh instances: more than 400 transforms at 96 bytes each pass 32 KB with no switch set."""
    return random_scenes.random_scene(rt, 31, 80, 60, spp=8, mesh_instances=400)


def edge_scene(rt, n):
    """One plane, one light and n diffuse spheres, each with a translate of its own, on a 16-wide grid."""
    import analytic_scenes as an
    s = rt.Scene()
    mats = [s.add_diffuse_material(c, 1.4) for c in ((0.8, 0.3, 0.2), (0.2, 0.6, 0.8), (0.7, 0.7, 0.3))]
    floor = s.add_diffuse_material((0.6, 0.6, 0.6), 1.5, checkers=True)
    lamp = s.add_emissive_material((30.0, 28.0, 25.0))
    s.add_plane(floor, (0.0, 1.0, 0.0), 0.0)
    s.add_sphere(lamp, 1.5, rt.translate((0.0, 12.0, 9.0)))
    for i in range(n):
        s.add_sphere(mats[i % 3], 0.45, rt.translate((1.2*(i % 16) - 9.0, 0.45, 1.2*(i // 16))))
    s.set_sky((0.5, 0.6, 0.8), (0.2, 0.2, 0.2))
    s.create_scene_bvh()
    cam = an.camera(rt, W, H, (0.0, 9.0, -9.0), (0.0, 0.0, 9.0), 55.0)
    st = an.settings(rt, spp=SPP, bounces=4)
    return s, cam, st, rt.load_reconstruction_kernel("Mitchell Netravali")


def edge_count(rt):
    """The n whose blob is the largest that is still at most 32 KB -> (n, its size, the size of n + 1)."""
    per = 32 + 2*48                                       # an rt_primitive and a transform
    at = lambda n: blob_bytes(rt, edge_scene(rt, n)[0].desc())
    base = at(200)
    n = 200 + (LDS_BYTES - base)//per
    while at(n) > LDS_BYTES:                              # (the padding of each table can take the estimate one off)
        n -= 1
    while at(n + 1) <= LDS_BYTES:
        n += 1
    return n, at(n), at(n + 1)


def recursive_scene(rt, name):
    scene, cam, st, fc = rc.build(rt, name, W, H)
    return scene, cam, st, fc


def recursive_settings(st, integ):
    return rc.case_settings(st, integ, RECURSIVE_DEPTH, rc.UNIFORM, SPP)


# ---- inputs every side shares

def with_settings(st, **fields):
    return rc.with_settings(st, **fields)


def sample_list(w=W, h=H, spp=SPP, n=6000, seed=17):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.uint32)
    return xy, rng.integers(0, spp, n).astype(np.uint32)


def query_rays(n=512):
    from test_gpu_parity import random_rays
    return random_rays(np.random.default_rng(7), n, np.array([0.0, 3.0, 10.0]), np.array([30.0, 12.0, 40.0]))


def hit_arrays(records, occlusion):
    """rt_hit_record list -> what two walks of the same rays must agree on: the hit flags of an occlusion query (any hit
    ends it, so which one is the walk's business), the whole record of a closest hit and the primitive word of a miss."""
    prim = np.array([r.primitive for r in records], np.uint32)
    if occlusion:
        return {"occluded": (prim != 0xFFFFFFFF).astype(np.uint32)}
    hit = prim != 0xFFFFFFFF
    rest = np.array([[r.t, *r.hit_p, *r.n] for r in records], np.float32)
    rest[~hit] = 0.0
    return {"primitive": prim, "record": rest}


def counts(s):
    return {"samples": int(s.samples), "closest_hit_rays": int(s.closest_hit_rays), "shadow_rays": int(s.shadow_rays)}


def walk(s, field="traversal"):
    """The walk's own figures: the TraversalStats of both query kinds and, for rt_stats::traversal, the rays the trace
    kernels took from the queues (a prologue that proves a miss queues none)."""
    out = tuple(tuple(sorted(getattr(s, field)[k].as_dict().items())) for k in range(2))
    return out + ((int(s.traced_rays[0]), int(s.traced_rays[1])),) if field == "traversal" else out


# ---- comparisons

def words(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names or a.dtype.itemsize != 4:
        return np.frombuffer(a.tobytes(), np.uint8)
    return a.view(np.uint32)


def differences(got, want, skip=()):
    """{key: how many 32-bit words (or bytes of a structured array) differ, or 1 for an unequal count}: two results of
    one kind, compared as bits so NaNs count as equal bits.  Empty when they are identical."""
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    out = {}
    for k in got:
        if k in skip:
            continue
        if isinstance(got[k], np.ndarray):
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
            n = int(np.count_nonzero(words(got[k]) != words(want[k])))
        else:
            n = int(got[k] != want[k])
        if n:
            out[k] = n
    return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b)/max(np.linalg.norm(b), 1e-30))


def same_or_nan(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def advanced_figures(samples, sample_counts, frame, frame_counts, cpu):
    """tests/test_gpu_scenes._compare's figures for a device result against cpu_advanced()'s."""
    fig = {"bit_exact_fraction": float(np.all(same_or_nan(samples, cpu["samples"]), axis=1).mean()),
           "frame_pixels_identical": float(np.all(frame == cpu["frame"], axis=2).mean()),
           "frame_rel_l2": rel_l2(frame, cpu["frame"]),
           "sample_counts_equal": all(sample_counts[k] == cpu["sample_counts"][k] for k in ("closest_hit_rays", "shadow_rays")),
           "frame_counts_equal": all(frame_counts[k] == cpu["frame_counts"][k] for k in ("closest_hit_rays", "shadow_rays"))}
    return fig


def advanced_bars(fig):
    """The bars of tests/test_gpu_scenes._compare."""
    assert fig["bit_exact_fraction"] >= 0.999, fig
    assert fig["frame_pixels_identical"] >= 0.999, fig
    assert fig["frame_rel_l2"] <= 1e-6, fig
    assert fig["sample_counts_equal"] and fig["frame_counts_equal"], fig


# ---- the CPU side of every kind (the oracle and the checkers; no device)

def cpu_counts(s):
    return {"samples": int(s.samples), "closest_hit_rays": int(s.closest_hit_rays), "shadow_rays": int(s.shadow_rays)}


def cpu_advanced(scene, cam, st, fc, w=W, h=H, env=False, tfi=TFI):
    xy, so = sample_list(w, h, st.samples_per_pixel)
    with ob.env_sampling(1 if env else 0):
        samples, ss = ob.trace_samples(scene.desc(), cam, st, w, h, xy, so, total_frame_index=tfi)
        frame, fs = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, total_frame_index=tfi)
    return {"samples": samples, "sample_counts": cpu_counts(ss), "frame": frame, "frame_counts": cpu_counts(fs)}


def cpu_integrator(scene, cam, st, fc, integ, w=W, h=H, tfi=TFI):
    st = with_settings(st, integrator=integ)
    xy, so = sample_list(w, h, st.samples_per_pixel)
    samples, ss = rb.trace_samples(scene.desc(), cam, st, w, h, xy, so, total_frame_index=tfi)
    frame, fs = rb.render(scene.desc(), cam, st, fc, w, h, total_frame_index=tfi)
    return {"samples": samples, "sample_counts": cpu_counts(ss), "frame": frame, "frame_counts": cpu_counts(fs)}


def cpu_recursive(scene, cam, st0, fc, integ, tfi=TFI):
    st = recursive_settings(st0, integ)
    xy, so = rc.all_samples(W, H, SPP)
    amb = scene.ambient_light()
    samples, ss = rr.trace_samples(scene.desc(), cam, st, W, H, xy, so, ambient=amb, total_frame_index=tfi)
    frame, fs = rr.render(scene.desc(), cam, st, fc, W, H, ambient=amb, total_frame_index=tfi)
    return {"samples": samples, "sample_counts": cpu_counts(ss), "frame": frame, "frame_counts": cpu_counts(fs)}


def cpu_features(scene, cam, st, fc, w=W, h=H, tfi=TFI):
    """-> ([the three frames], the counts they share, the specular bounces followed)."""
    frames, stats, spec = [], None, None
    for f in range(3):
        frame, stats, spec = rf.render(scene.desc(), cam, st, fc, w, h, f, total_frame_index=tfi)
        frames.append(frame)
    return frames, cpu_counts(stats), int(spec)


def cpu_gbuffer(scene, cam, st, w=W, h=H):
    return tb.gbuffer(scene.desc(), cam, st.lens_distortion, w, h)


def surface_mismatches(rt, scene, g, s):
    """tests/test_gpu_deform.py's check of a surface record against the checker: off the meshes {NONE, 0, 0, 0}; on a
    mesh a triangle and a place whose normal under ref_deform_surface is the texel's, bit for bit -> (words that
    differ, pixels on a mesh)."""
    d = scene.desc()
    ids = g["primitive"]
    bad, on_mesh = 0, np.zeros(ids.shape, bool)
    arrays = {}
    for prim in mesh_instances(rt, d):
        here = ids == prim
        if not here.any():
            continue
        on_mesh |= here
        m = int(d.primitives[prim].mesh_index)
        if m not in arrays:
            tris, idx, nrm, _ = rfit.mesh_arrays(d, m)
            arrays[m] = (rfit.original_order(tris, idx), nrm)
        tris, nrm = arrays[m]
        inv = np.ctypeslib.as_array(d.transforms[d.primitives[prim].transform_index].inverse.e).astype(np.float32)
        if int(s["triangle"][here].max()) >= len(tris):
            bad += int((s["triangle"][here] >= len(tris)).sum())
            continue
        _, n = db.surface(tris, nrm, np.eye(4, dtype=np.float32), inv, s["triangle"][here], s["v"][here], s["w"][here])
        bad += int(np.count_nonzero(tb.bits(n) != tb.bits(np.ascontiguousarray(g["n"][here]))))
        bad += int(((s["v"][here] < 0) | (s["w"][here] < 0) | (s["v"][here] + s["w"][here] > 1)).sum())
        bad += int(np.count_nonzero(s["reserved"][here]))
    off = ~on_mesh
    bad += int((s["triangle"][off] != db.NONE).sum())
    bad += int(np.count_nonzero(np.ascontiguousarray(s[off]).view(np.uint32).reshape(-1, 4)[:, 1:]))
    return bad, int(on_mesh.sum())


def gbuffer_mismatches(got, want):
    return int(sum(np.count_nonzero(tb.bits(np.ascontiguousarray(got[f])) != tb.bits(np.ascontiguousarray(want[f])))
                   for f in ("p", "t", "n", "primitive")))


def intersect_mismatches(got, want, occlusion):
    """tests/test_gpu_parity.test_intersect_bit_exact's count."""
    bad = 0
    for a, b in zip(got, want):
        if occlusion:
            bad += (a.primitive == 0xFFFFFFFF) != (b.primitive == 0xFFFFFFFF)
        elif a.primitive != b.primitive or (a.primitive != 0xFFFFFFFF and (
                a.t != b.t or tuple(a.n) != tuple(b.n) or tuple(a.hit_p) != tuple(b.hit_p))):
            bad += 1
    return int(bad)
