"""The traversal stack's spill levels and its 64-entry limit (StackT, rt_kernels.hip), on purpose.

Every traversal on the device keeps a per-lane stack: 16 levels in LDS, levels 16..63 in a global spill area
addressed spill[(level - 16)*nthreads + gtid], where each kernel (k_trace, k_drain, k_recurse, the separate
shadow launch, k_debug_intersect) takes gtid and nthreads from its own grid and block size.  A wave leaves the
LDS-only fast path once a lane holds more than 12 entries (11 in reference units), push drops an entry at 64,
and rt_scene_upload refuses any scene whose bound top_depth + mesh_depth + 2 exceeds 64.  The presets' static
bounds are 34-38, so their rays may reach level 16, but nothing says whether they do.

tests/deep_bvh.py hands the library a BVH2 whose occupancy is known in closed form: a deep-first ray through
the loose caterpillar of L levels holds exactly 3L + 1 entries, a leaf-first ray at most 4.  L = 4, 5, 6, 20
give 13, 16, 19 and 61: past the fast path's threshold, the last LDS level, three spilled levels, and the
deepest scene the upload accepts.  The sensitivity of these tests rests on that closed form and on the rays
aimed at single triangles of known stack level (a wrong spill index loses exactly those), never on a broken
kernel run on a GPU.

No tolerance here is new: comparisons are exact, or reuse the margin of the test named beside them.
"""
import numpy as np
import pytest

import deep_bvh as db
import oracle_binding as ob
from parity_report import REPORT

W, H, SPP = 48, 36, 8
MISS = 0xFFFFFFFF

_scenes = {}


def deep_scene(rt, L, variant="loose"):
    """One DeepScene per (L, variant) for the whole module: scenes and their oracle answers are never changed."""
    if (L, variant) not in _scenes:
        _scenes[(L, variant)] = db.DeepScene(rt, L, variant)
    return _scenes[(L, variant)]


_answers = {}


def oracle_hits(rt, L, variant, occlusion):
    key = (L, variant, occlusion)
    if key not in _answers:
        sc = deep_scene(rt, L, variant)
        _answers[key] = ob.intersect(sc.desc(), [r[2] for r in sc.rays()], occlusion)
    return _answers[key]


def frame_setup(rt, sc, spp=SPP):
    st, _ = rt.default_settings()
    st.samples_per_pixel = spp
    return sc.camera(W, H), st, rt.load_reconstruction_kernel("Mitchell Netravali")


def top_depth(desc):
    """tree_depth of the top-level BVH2 (rt_kernels.hip): a lone leaf has depth 1."""
    def rec(i):
        n = desc.bvh_nodes[i]
        if n.count or (i == 0 and n.left_first == 0):
            return 1
        return 1 + max(rec(n.left_first), rec(n.left_first + 1))
    return rec(0) if desc.bvh_node_count else 0


def nodes_of(mesh):
    """An rt_mesh's BVH2 in tests/deep_bvh.py's form."""
    return [{"left": mesh.nodes[i].left_first, "count": mesh.nodes[i].count, "axis": mesh.nodes[i].split_axis}
            for i in range(mesh.node_count)]


def modelled_depth(desc):
    """(bvh_depth, bvh_depth_ref) as rt_scene_upload computes them, restated in Python."""
    md = [db.mesh_depth(nodes_of(desc.meshes[m])) for m in range(desc.mesh_count) if desc.meshes[m].node_count]
    d = max([x[0] for x in md], default=0)
    r = max([x[1] for x in md], default=0)
    top = top_depth(desc)
    return top + d, top + max(d, r)


# ---------------------------------------------------------------------------------------------------- CPU

def test_bound_model(rt):
    """build_bvh4's `need`, restated: the caterpillar's bound is 3L + 1 (4L + 1 in reference units), its BVH2
    depth 2L + 1 and it has 6L + 1 nodes and 3L + 1 triangles, for every L up to the first refused one."""
    for L in range(1, 22):
        nodes = db.caterpillar(L)
        assert db.mesh_depth(nodes) == (3*L + 1, 4*L + 1)
        assert db.bvh2_depth(nodes) == 2*L + 1 < 64
        assert len(nodes) - 1 == 6*L + 1 and len(db.triangles(L)) == 3*L + 1
    table = {L: (len(db.caterpillar(L)) - 1, db.bvh2_depth(db.caterpillar(L)), db.mesh_depth(db.caterpillar(L))[0])
             for L in (5, 19, 20, 21)}
    assert table == {5: (31, 11, 16), 19: (115, 39, 58), 20: (121, 41, 61), 21: (127, 43, 64)}
    sc = deep_scene(rt, 20)
    assert top_depth(sc.desc()) == 1                       # the mesh and the light share the root leaf
    assert modelled_depth(sc.desc()) == (1 + 61, 1 + 81)
    assert 1 + 61 + 2 == 64                                # the deepest scene the upload accepts


def test_ray_set_shape(rt):
    """The ray list is what the GPU tests need: no multiple of 128, more than two blocks, deep-first and
    leaf-first rays lane by lane, every mixed sign, and rays that cross the box and hit no triangle."""
    for L in (4, 5, 6, 20):
        sc = deep_scene(rt, L)
        rays = sc.rays()
        kinds = [r[0] for r in rays]
        n = 3*L + 1
        assert len(rays) % 128 != 0 and len(rays) > 2*128
        reps = kinds.count("deep") // n
        assert kinds[:2*n] == ["deep", "leaf"]*n and reps == -(-257 // (5*n + 16))
        assert {k: kinds.count(k) for k in ("ppn", "pnp", "npp")} == {"ppn": reps*n, "pnp": reps*n, "npp": reps*n}
        assert kinds.count("miss") >= 16
        for kind, k, q in rays:
            want = db.SIGNS[kind] if kind != "miss" else None
            if want:
                assert tuple(np.sign([q.d.x, q.d.y, q.d.z]).astype(int)) == want


@pytest.mark.parametrize("variant", ["loose", "tight"])
def test_fixture_against_the_oracle(rt, variant):
    """The hand-made tree is a valid BVH of its triangles: the oracle's closest hits through it are, bit for
    bit, those through the host builder's own BVH of the same triangles; every aimed ray hits its triangle
    (hit_p.z = 0.05 k names it) at t = 7 to float rounding, every gap ray misses the mesh, and as shadow
    queries all aimed rays are occluded."""
    sc = deep_scene(rt, 20, variant)
    rays = sc.rays()
    q = [r[2] for r in rays]
    mine = oracle_hits(rt, 20, variant, False)
    host = ob.intersect(sc.host_desc(), q, False)
    assert sum(not db.same_hit(a, b, False) for a, b in zip(mine, host)) == 0
    aimed = 0
    for (kind, k, _), h in zip(rays, mine):
        if k >= 0:
            aimed += 1
            assert h.primitive == sc.mesh_prim and round(h.hit_p.z / 0.05) == k, (kind, k, h.t, h.primitive)
            assert abs(h.t - db.START) <= 1e-6, (kind, k, h.t)          # two float32 ulps of 7: o = c - 7 d is rounded
        else:
            assert h.primitive != sc.mesh_prim
    assert aimed == 5*61
    occ = oracle_hits(rt, 20, variant, True)
    occ_host = ob.intersect(sc.host_desc(), q, True)
    assert [h.primitive == MISS for h in occ] == [h.primitive == MISS for h in occ_host]
    assert all(h.primitive != MISS for (kind, k, _), h in zip(rays, occ) if k >= 0)


def test_comb_top_level_against_the_oracle(rt):
    """The hand-made comb top level (40 spheres, depth 21) over the L = 5 mesh answers every ray as the host's
    own top level does, and its modelled bound is 21 + 16."""
    sc = db.DeepScene(rt, 5, "loose", spheres=40)
    host = sc.host_desc()
    rays = comb_rays(rt, sc)
    before = ob.intersect(host, rays, False)
    depth = sc.comb_top_level()
    assert depth == 21 and top_depth(sc.desc()) == 21
    assert modelled_depth(sc.desc()) == (21 + 16, 21 + 21)
    after = ob.intersect(sc.desc(), rays, False)
    assert sum(not db.same_hit(a, b, False) for a, b in zip(before, after)) == 0
    hit = {h.primitive for h in after}
    assert sc.mesh_prim in hit and len(hit & set(sc.sphere_ids)) == 40


def comb_rays(rt, sc):
    """The fixture's rays, and per small sphere one ray of every sign pattern through its centre."""
    rays = [r[2] for r in sc.rays()]
    d = sc.host_desc()
    for pid in sc.sphere_ids:
        f = d.transforms[d.primitives[pid].transform_index].forward.e
        c = np.array([f[0][3], f[1][3], f[2][3]], np.float64)
        for sign in db.SIGNS.values():
            dd = np.array([0.3, 0.4, 1.0])*sign
            dd = (dd/np.linalg.norm(dd)).astype(np.float32)
            o = (c - 3.0*dd.astype(np.float64)).astype(np.float32)
            rays.append(rt.abi.RayQuery(rt.abi.V3(*o), rt.abi.V3(*dd), 3.0e38, 0))
    if len(rays) % 128 == 0:
        rays.pop()
    return rays


def test_oracle_frames(rt):
    """The oracle renders the L = 20 scene deterministically, frames and sample lists, and sends shadow rays
    that reach the mesh."""
    sc = deep_scene(rt, 20)
    cam, st, fc = frame_setup(rt, sc)
    a, sa = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
    b, sb = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=2)
    assert (sa.closest_hit_rays, sa.shadow_rays) == (sb.closest_hit_rays, sb.shadow_rays)
    assert sa.shadow_rays > 1000 and sa.traversal[1].mesh_intersection_count > 1000
    a2, _ = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32)) and np.isfinite(a).all()
    from test_gpu_parity import _sample_list
    xy, s = _sample_list(np.random.default_rng(23), W, H, 4000, SPP)
    x, sx = ob.trace_samples(sc.desc(), cam, st, W, H, xy, s)
    y, sy = ob.trace_samples(sc.desc(), cam, st, W, H, xy, s)
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and sx.shadow_rays == sy.shadow_rays > 0


# ---------------------------------------------------------------------------------------------------- GPU

def _mismatches(got, want, occlusion):
    return sum(not db.same_hit(a, b, occlusion) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("top", ["prologue", "kernel"])
@pytest.mark.parametrize("variant", ["loose", "tight"])
@pytest.mark.parametrize("L", [4, 5, 6, 20])
def test_intersect_at_every_occupancy(rt, monkeypatch, L, variant, top):
    """rt_debug_intersect against the oracle, every field bit for bit (occlusion: hit or miss, as
    test_intersect_bit_exact): loose occupancies 13, 16, 19 and 61.  `kernel`: RT_TOP_PROLOGUE=0, as
    test_top_level_paths.  The scene's reported depth is the modelled 1 + 3L + 1."""
    if top == "kernel":
        monkeypatch.setenv("RT_TOP_PROLOGUE", "0")
    sc = deep_scene(rt, L, variant)
    rays = sc.rays()
    q = [r[2] for r in rays]
    dev = rt.DeviceScene(sc, 0)
    try:
        depth = dev.stack_depth()
        got = {occ: dev.intersect(q, occ) for occ in (False, True)}
    finally:
        dev.close()
    mism = {occ: _mismatches(got[occ], oracle_hits(rt, L, variant, occ), occ) for occ in (False, True)}
    REPORT[f"deep_bvh_intersect_L{L}_{variant}_{top}"] = {
        "rays": len(q), "stack_depth": list(depth), "mismatches_closest": mism[False], "mismatches_occlusion": mism[True]}
    assert depth == (1 + 3*L + 1, 1 + 4*L + 1), f"this scene needs {depth} levels"
    assert depth == modelled_depth(sc.desc())
    assert mism[False] == 0, f"{mism[False]} of {len(q)} hit records differ (scene needs {depth[0]} levels)"
    assert mism[True] == 0, f"{mism[True]} of {len(q)} occlusion answers differ (scene needs {depth[0]} levels)"
    if L == 20 and variant == "loose":
        # a deep-first ray holds the leaves of BVH4 level j at stack levels 3j .. 3j + 2 (one higher under the
        # top level's entry): from j = 6 on they wait in the spill area, which a wrong index would lose
        want = oracle_hits(rt, L, variant, False)
        lost = []
        for (kind, k, _), g, o in zip(rays, got[False], want):
            if kind == "deep" and k // 3 >= 6:
                assert o.primitive == sc.mesh_prim and round(o.hit_p.z / 0.05) == k
                if g.primitive != sc.mesh_prim or g.t != o.t:
                    lost.append((k, k // 3, g.t, o.t))
        REPORT[f"deep_bvh_intersect_L{L}_{variant}_{top}"]["spilled_level_targets_lost"] = len(lost)
        assert not lost, f"triangles (k, BVH4 level, t, want) lost from the spilled levels: {lost[:8]}"


def _exact(rt, dev, cam, st, fc, **cfg):
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT, **cfg):
        frame, stats = dev.render(cam, st, fc, W, H)
    assert stats.splat_mode == rt.abi.RT_SPLAT_EXACT
    return frame, stats


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("top", ["prologue", "kernel"])
def test_frames_and_samples(rt, monkeypatch, top):
    """L = 20 loose (61 entries) through every kernel that owns a spill index.  First as every scene of
    tests/test_gpu_scenes.py (`_compare`); then, on one DeviceScene, the exact-splat frame must be the oracle's
    byte for byte under every schedule: one and four partitions (each partition's own spill area; four need a
    pool small enough to split this frame), the fused drain off and forced at once (k_drain and k_drain_list,
    DTB lanes on the trace grid's area; fuse_paths values of test_fused_drain_matches_separate_kernels), the
    drain kernels on every and every third iteration, the shadow rays in their own launch (the connect grid) and
    merged, and a pool of 1024 paths, whose grids are far smaller than the spill area's.  rt_stats::traversal
    against the oracle's restatement of the device's walk, with test_top_level_paths's margins."""
    from test_gpu_scenes import _compare
    if top == "kernel":
        monkeypatch.setenv("RT_TOP_PROLOGUE", "0")
    sc = deep_scene(rt, 20)
    cam, st, fc = frame_setup(rt, sc)
    _compare(rt, f"deep_bvh_L20_{top}", sc, cam, st, fc, W, H)
    with ob.gpu_walk(top_prologue=top == "prologue") as walk:
        cframe, cs = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
    a = rt.abi
    big = 1000000000
    schedules = {
        "default": {},
        "partitions_1": {"partitions": 1},
        "partitions_4_pool_1024": {"partitions": 4, "path_pool": 1024},
        "drain_off": {"fuse_paths": 0},
        "drain_at_once": {"fuse_paths": big},
        "drain_every_1": {"fuse_paths": big, "drain_every": 1, "path_pool": 1024},
        "drain_every_3": {"fuse_paths": big, "drain_every": 3, "path_pool": 1024},
        "shadow_separate": {"shadow_launch": a.RT_SHADOW_LAUNCH_SEPARATE},
        "shadow_merged": {"shadow_launch": a.RT_SHADOW_LAUNCH_MERGED},
        "shadow_separate_drain_4_partitions": {"shadow_launch": a.RT_SHADOW_LAUNCH_SEPARATE, "fuse_paths": big,
                                               "partitions": 4, "path_pool": 1024},
        "shadow_merged_drain_4_partitions": {"shadow_launch": a.RT_SHADOW_LAUNCH_MERGED, "fuse_paths": big,
                                             "partitions": 4, "path_pool": 1024},
        "pool_1024": {"path_pool": 1024},
    }
    out = {}
    dev = rt.DeviceScene(sc, 0)
    try:
        assert dev.stack_depth() == (62, 82)
        for name, cfg in schedules.items():
            out[name] = _exact(rt, dev, cam, st, fc, **cfg)
    finally:
        dev.close()
    report = {}
    for name, (frame, stats) in out.items():
        report[name] = {"identical_to_oracle": _same_bits(frame, cframe),
                        "pixels_identical": float(np.all(frame == cframe, axis=2).mean()),
                        "rays": [int(stats.closest_hit_rays), int(stats.shadow_rays)],
                        "shadow_launch": int(stats.shadow_launch), "iterations": int(stats.iterations)}
    gs = out["default"][1]
    calls = [int(gs.traversal[k].mesh_intersection_count) for k in range(2)]
    report["traversal"] = {"gpu": [gs.traversal[k].as_dict() for k in range(2)], "restated": walk.result}
    REPORT[f"deep_bvh_frames_L20_{top}"] = report
    for name, (frame, stats) in out.items():
        assert (stats.closest_hit_rays, stats.shadow_rays) == (cs.closest_hit_rays, cs.shadow_rays), name
        assert _same_bits(frame, cframe), (name, report[name])
    assert out["shadow_separate"][1].shadow_launch == a.RT_SHADOW_LAUNCH_SEPARATE
    assert out["shadow_merged"][1].shadow_launch == a.RT_SHADOW_LAUNCH_MERGED
    assert cs.shadow_rays > 1000
    # the walk's own counts, as test_top_level_paths holds them
    assert calls == walk.result["calls"]
    for k in range(2):
        g, r = int(gs.traversal[k].mesh_leaf_traversals), walk.result["leaves"][k]
        assert abs(g - r) <= max(2, 1e-5 * r), (k, "leaves", g, r)
        for f, key in (("mesh_node_traversals", "nodes"), ("mesh_bvh_traversals", "bvh")):
            g, r = int(getattr(gs.traversal[k], f)), walk.result[key][k]
            assert abs(g - r) <= max(4, 1e-5 * r), (k, f, g, r)


@pytest.mark.gpu
@pytest.mark.parametrize("integ,tag", [(1, "whitted"), (2, "gtr")])
def test_recursive_integrators(rt, integ, tag):
    """k_recurse (DTB lanes per block on the trace grid's spill area) on L = 20 loose, max_bounce_count 4,
    against tests/ref_recursive exactly as test_gpu_recursive.py::test_parity: every listed sample and every
    pixel of the exact-splat frame bit-identical, equal ray counts, the streaming frame within that file's
    STREAM_BOUND of the exact one."""
    import recursive_cases as rc
    import ref_recursive_binding as rr
    from test_gpu_parity import _sample_list
    from test_gpu_recursive import STREAM_BOUND, rel_l2
    sc = deep_scene(rt, 20)
    amb = sc.ambient_light()
    assert max(amb) > 0.0                                      # Whitted reads it
    cam, st0, fc = frame_setup(rt, sc)
    st = rc.case_settings(st0, integ, 4, rc.STRATIFIED, SPP)
    xy, so = _sample_list(np.random.default_rng(29), W, H, 4000, SPP)
    dev = rt.DeviceScene(sc, 0)
    try:
        dev.set_recursive_integrators(True)
        dev.configure(path_pool=rc.POOL)
        gpu, gstats = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=2)
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
            frame, fstats = dev.render(cam, st, fc, W, H, total_frame_index=2)
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM):
            stream, sstats = dev.render(cam, st, fc, W, H, total_frame_index=2)
    finally:
        dev.close()
    cpu, cstats = rr.trace_samples(sc.desc(), cam, st, W, H, xy, so, ambient=amb, total_frame_index=2)
    cframe, cfstats = rr.render(sc.desc(), cam, st, fc, W, H, ambient=amb, total_frame_index=2)
    same, fsame = rc.same_samples(gpu, cpu), rc.same_samples(frame, cframe)
    err = rel_l2(stream, frame)
    REPORT[f"deep_bvh_recursive_L20_{tag}"] = {
        "samples": len(xy), "samples_differing": int((~same.all(axis=1)).sum()),
        "pixels_differing": int((~fsame.all(axis=2)).sum()), "stream_rel_l2": err,
        "rays": [int(fstats.closest_hit_rays), int(fstats.shadow_rays)]}
    assert np.isfinite(cpu).all() and np.isfinite(cframe).all()
    assert same.all(), f"{int((~same.all(axis=1)).sum())} of {len(xy)} samples differ"
    assert (gstats.closest_hit_rays, gstats.shadow_rays) == (cstats.closest_hit_rays, cstats.shadow_rays)
    assert gstats.samples == len(xy)
    assert fstats.splat_mode == rt.abi.RT_SPLAT_EXACT
    assert fsame.all(), f"{int((~fsame.all(axis=2)).sum())} of {W*H} pixels differ"
    assert (fstats.closest_hit_rays, fstats.shadow_rays, fstats.samples) == (
        cfstats.closest_hit_rays, cfstats.shadow_rays, cfstats.samples) and fstats.samples == W*H*SPP
    assert sstats.splat_mode == rt.abi.RT_SPLAT_STREAM and err <= STREAM_BOUND
    assert (sstats.closest_hit_rays, sstats.shadow_rays) == (fstats.closest_hit_rays, fstats.shadow_rays)
    if integ == 1:
        assert fstats.shadow_rays > 0


@pytest.mark.gpu
def test_reference_units_at_their_limit(rt):
    """rt_scene_config::traversal_ref adds a marker per BVH4 level: 4L + 1.  L = 15 needs 1 + 61 + 2 = 64: it
    renders, its reference-unit counts meet the oracle's reference walk (check_traversal_ref,
    tests/test_gpu_fullscale.py) and its frame is the one without traversal_ref."""
    from test_gpu_fullscale import check_traversal_ref
    sc = deep_scene(rt, 15)
    cam, st, fc = frame_setup(rt, sc)
    dev = rt.DeviceScene(sc, 0)
    try:
        assert dev.stack_depth() == (1 + 46, 1 + 61)
        plain, ps = _exact(rt, dev, cam, st, fc)
        ref, rs = _exact(rt, dev, cam, st, fc, traversal_ref=1)
    finally:
        dev.close()
    cframe, cs = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
    REPORT["deep_bvh_traversal_ref_L15"] = {"units": check_traversal_ref(rs, cs),
                                            "frame_unchanged": _same_bits(plain, ref),
                                            "identical_to_oracle": _same_bits(ref, cframe)}
    assert (rs.closest_hit_rays, rs.shadow_rays) == (cs.closest_hit_rays, cs.shadow_rays)
    assert cs.traversal[0].mesh_leaf_traversals > 0 and cs.traversal[1].mesh_intersection_count > 0
    assert _same_bits(plain, ref) and _same_bits(ref, cframe)
    assert all(ps.traversal_ref[k].mesh_bvh_traversals == 0 for k in range(2))


@pytest.mark.gpu
def test_reference_units_refused_past_their_limit(rt, monkeypatch):
    """L = 16 needs 1 + 65 + 2 = 68 entries in reference units: refused by configure(traversal_ref=1) on the
    uploaded scene and by an upload under RT_TRAVERSAL_REF=1, RT_ERROR_INVALID both; without traversal_ref
    (1 + 49 + 2) the same scene renders the oracle's frame, before and after the refusals."""
    sc = deep_scene(rt, 16)
    cam, st, fc = frame_setup(rt, sc)
    cframe, cs = ob.render(sc.desc(), cam, st, fc, W, H, rng_mode=0, threads=1)
    dev = rt.DeviceScene(sc, 0)
    try:
        assert dev.stack_depth() == (1 + 49, 1 + 65)
        before, _ = _exact(rt, dev, cam, st, fc)
        with pytest.raises(rt.RenderError) as e:
            dev.configure(traversal_ref=1)
        assert e.value.code == rt.abi.RT_ERROR_INVALID and "traversal_ref" in str(e.value)
        assert dev.config().traversal_ref == 0
        after, stats = _exact(rt, dev, cam, st, fc)
    finally:
        dev.close()
    monkeypatch.setenv("RT_TRAVERSAL_REF", "1")
    with pytest.raises(rt.RenderError) as e:
        rt.DeviceScene(sc, 0)
    assert e.value.code == rt.abi.RT_ERROR_INVALID and "traversal_ref" in str(e.value)
    monkeypatch.delenv("RT_TRAVERSAL_REF")
    REPORT["deep_bvh_traversal_ref_L16"] = {"identical_to_oracle": [_same_bits(before, cframe), _same_bits(after, cframe)]}
    assert _same_bits(before, cframe) and _same_bits(after, cframe)
    assert (stats.closest_hit_rays, stats.shadow_rays) == (cs.closest_hit_rays, cs.shadow_rays)
    assert all(stats.traversal_ref[k].mesh_bvh_traversals == 0 for k in range(2))


@pytest.mark.gpu
def test_the_limit(rt):
    """L = 21 needs 1 + 64 + 2 = 67 entries: rt_scene_upload refuses it with RT_ERROR_INVALID and says how many
    it needs, how many there are and that the bound is the device's BVH4 one -- the oracle (the reference's
    node_stack[64], BVH2 depth 43) answers every ray of the same scene.  The refusal leaves the library usable:
    L = 20 (64 of 64) uploads right after it, again after several refusals, and intersects bit for bit."""
    deep = db.DeepScene(rt, 21)
    rays = deep.rays()
    hits = ob.intersect(deep.desc(), [r[2] for r in rays], False)
    assert all(h.primitive == deep.mesh_prim and round(h.hit_p.z / 0.05) == k
               for (kind, k, _), h in zip(rays, hits) if k >= 0)
    assert modelled_depth(deep.desc()) == (1 + 64, 1 + 85)
    sc = deep_scene(rt, 20)
    q = [r[2] for r in sc.rays()]
    mism = []
    for n in (1, 4):
        for _ in range(n):
            with pytest.raises(rt.RenderError) as e:
                rt.DeviceScene(deep, 0)
            assert e.value.code == rt.abi.RT_ERROR_INVALID
            msg = str(e.value)
            assert "needs 67 entries" in msg and "64 available" in msg and "BVH4" in msg, msg
            assert "RT/intersection.cpp" not in msg            # not the reference's limit
        dev = rt.DeviceScene(sc, 0)
        try:
            assert dev.stack_depth() == (62, 82)
            mism.append(_mismatches(dev.intersect(q, False), oracle_hits(rt, 20, "loose", False), False))
        finally:
            dev.close()
    REPORT["deep_bvh_limit"] = {"refused_L21_message": msg, "L20_mismatches_after_refusals": mism}
    assert mism == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("top", ["prologue", "kernel"])
def test_deep_top_level(rt, monkeypatch, top):
    """A deep top level over the L = 5 mesh: 40 small spheres under a hand-made comb of depth 21.  Where the
    trace kernels walk the top level themselves (RT_TOP_PROLOGUE=0, or a prologue that does not take this top
    level), its pending entries lie under the mesh's 16, so the mesh's walk starts at mesh_base > 0 and ends in
    the spill levels.  Intersections bit for bit; frames and samples as `_compare` holds every scene."""
    from test_gpu_scenes import _compare
    if top == "kernel":
        monkeypatch.setenv("RT_TOP_PROLOGUE", "0")
    sc = db.DeepScene(rt, 5, "loose", spheres=40)
    rays = comb_rays(rt, sc)
    assert sc.comb_top_level() == 21
    want = {occ: ob.intersect(sc.desc(), rays, occ) for occ in (False, True)}
    dev = rt.DeviceScene(sc, 0)
    try:
        depth = dev.stack_depth()
        got = {occ: dev.intersect(rays, occ) for occ in (False, True)}
    finally:
        dev.close()
    mism = {occ: _mismatches(got[occ], want[occ], occ) for occ in (False, True)}
    REPORT[f"deep_bvh_comb_top_{top}"] = {"rays": len(rays), "stack_depth": list(depth),
                                          "mismatches_closest": mism[False], "mismatches_occlusion": mism[True]}
    assert depth == (21 + 16, 21 + 21) == modelled_depth(sc.desc())
    assert mism == {False: 0, True: 0}, f"{mism} of {len(rays)} differ (scene needs {depth[0]} levels)"
    cam, st, fc = frame_setup(rt, sc)
    _compare(rt, f"deep_bvh_comb_top_{top}", sc, cam, st, fc, W, H)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["c3", "c4"])
def test_preset_stack_depth(rt, preset):
    """The accessor on builder-made trees: rt_scene_stack_depth equals the Python restatement of the upload's
    bound (EMPTY4 slots, leaves of several triangles, several meshes).  The values are static bounds: whether
    a preset's own rays reach level 16 on the device stays unmeasured."""
    scene, cam, st, fc, post = rt.load_preset(preset, 96, 54)
    want = modelled_depth(scene.desc())
    dev = rt.DeviceScene(scene, 0)
    try:
        depth = dev.stack_depth()
    finally:
        dev.close()
    REPORT[f"deep_bvh_stack_depth_{preset}"] = {"stack_depth": depth[0], "stack_depth_ref": depth[1],
                                                "top_depth": top_depth(scene.desc())}
    assert depth == want
    assert depth[0] - top_depth(scene.desc()) == {"c3": 38, "c4": 37}[preset]
