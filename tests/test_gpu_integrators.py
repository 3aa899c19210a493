"""rt_settings::integrator on the device: Ground Truth Iterative (3), Normals (4) and Distances (5) against
the CPU checker of tests/ref_integrators (tests/ref_binding.py), the rejection of Whitted (1) and Ground Truth
Recursive (2), and Ground Truth as an independent estimator against the Advanced integrator's shade_bounce.

Bars (the project's, tests/test_gpu_parity.py): per-sample radiance >= 99.9 % bit-exact; the RT_SPLAT_EXACT
frame >= 99.9 % of pixels identical to the checker's single-threaded frame and rel L2 <= 1e-6; ray counts equal.
Shapes are small: what can go wrong is the one-bounce life, the record ring, ragged tiles and mesh normals.
"""
import numpy as np
import pytest

import oracle_binding as ob
import ref_binding as rb
from random_scenes import random_scene

pytestmark = pytest.mark.gpu

from parity_report import REPORT      # noqa: E402

ADVANCED, WHITTED, GT_RECURSIVE, GT_ITERATIVE, NORMALS, DISTANCES = range(6)
INTEG_NAME = {GT_ITERATIVE: "ground_truth", NORMALS: "normals", DISTANCES: "distances"}
SCENES = ["c1", "c3", "c4", "random21", "random22", "random23"]


def rel_l2(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def with_integrator(st, integ, **fields):
    c = type(st).from_buffer_copy(st)
    c.integrator = integ
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def build(rt, name):
    if name.startswith("random"):
        w, h = 67, 35                                    # two ragged 64-pixel tiles
        scene, cam, st, fc = random_scene(rt, int(name[6:]), w, h, spp=8)
    else:
        w, h = 96, 64
        scene, cam, st, fc, post = rt.load_preset(name, w, h)
        st.samples_per_pixel = 8
    return scene, cam, st, fc, w, h


@pytest.fixture(scope="module")
def scenes(rt):
    """Scene name -> (scene, cam, st, fc, w, h, dev), built and uploaded on first use."""
    made = {}

    def get(name):
        if name not in made:
            scene, cam, st, fc, w, h = build(rt, name)
            made[name] = (scene, cam, st, fc, w, h, rt.DeviceScene(scene, 0))
        return made[name]
    yield get
    for v in made.values():
        v[-1].close()


# ---- 5. per-sample and frame parity

@pytest.mark.parametrize("integ", [GT_ITERATIVE, NORMALS, DISTANCES])
@pytest.mark.parametrize("name", SCENES)
def test_parity(rt, scenes, name, integ):
    scene, cam, st0, fc, w, h, dev = scenes(name)
    st = with_integrator(st0, integ)
    rng = np.random.default_rng(11)
    n = 8000
    xy = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], axis=1).astype(np.uint32)
    so = rng.integers(0, st.samples_per_pixel, n).astype(np.uint32)
    gpu, gstats = dev.trace_samples(cam, st, w, h, xy, so)
    cpu, cstats = rb.trace_samples(scene.desc(), cam, st, w, h, xy, so)
    exact = np.all((gpu == cpu) | (np.isnan(gpu) & np.isnan(cpu)), axis=1)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        frame, fstats = dev.render(cam, st, fc, w, h)
    cframe, cfstats = rb.render(scene.desc(), cam, st, fc, w, h)
    same = np.all(frame == cframe, axis=2).mean()
    err = rel_l2(frame, cframe)
    key = f"integrator_{INTEG_NAME[integ]}_{name}"
    REPORT[key] = {"samples_bit_exact": float(exact.mean()), "pixels_identical": float(same), "frame_rel_l2": err,
                   "gpu_closest": int(fstats.closest_hit_rays), "cpu_closest": int(cfstats.closest_hit_rays)}
    print(key, REPORT[key])
    assert exact.mean() >= 0.999, f"only {exact.mean():.5f} of samples bit-exact"
    assert gstats.closest_hit_rays == cstats.closest_hit_rays and gstats.shadow_rays == 0
    assert gstats.traced_rays[1] == 0
    assert fstats.splat_mode == rt.abi.RT_SPLAT_EXACT
    assert same >= 0.999 and err <= 1e-6, (same, err)
    assert fstats.closest_hit_rays == cfstats.closest_hit_rays and fstats.samples == cfstats.samples == w*h*8
    assert fstats.shadow_rays == 0 and fstats.traced_rays[1] == 0
    if integ != GT_ITERATIVE:
        assert fstats.closest_hit_rays == fstats.samples and gstats.closest_hit_rays == n


# ---- 6. Normals and Distances never read max_bounce_count

@pytest.mark.parametrize("integ", [NORMALS, DISTANCES])
def test_first_hit_without_bounces(rt, integ):
    w = h = 32
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    st = with_integrator(st, integ, samples_per_pixel=2, max_bounce_count=0)
    dev = rt.DeviceScene(scene, 0)
    try:
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
            frame, stats = dev.render(cam, st, fc, w, h)
        stream, sstats = dev.render(cam, st, fc, w, h)
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_ATOMIC):
            atomic, astats = dev.render(cam, st, fc, w, h)
    finally:
        dev.close()
    assert astats.splat_mode == rt.abi.RT_SPLAT_ATOMIC and rel_l2(atomic, frame) <= 1e-5
    cframe, cstats = rb.render(scene.desc(), cam, st, fc, w, h)
    assert np.array_equal(frame.view(np.uint32), cframe.view(np.uint32))
    assert np.abs(frame[..., :3]).max() > 0.01                       # not black
    assert stats.closest_hit_rays == cstats.closest_hit_rays == w*h*2 and stats.shadow_rays == 0
    assert sstats.closest_hit_rays == w*h*2 and rel_l2(stream, frame) <= 2e-6


# ---- 7. the schedule does not enter a Ground Truth frame

def test_ground_truth_schedule_independence(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c3")
    st = with_integrator(st0, GT_ITERATIVE)
    E = rt.abi.RT_SPLAT_EXACT
    frames = {}
    for fuse in (-1, 0):
        for every in (1, 3):
            for parts in (1, 4):
                with dev.configured(splat_mode=E, fuse_paths=fuse, drain_every=every, partitions=parts):
                    frames[(fuse, every, parts)] = dev.render(cam, st, fc, w, h)
    base, bstats = frames[(-1, 1, 1)]
    for k, (f, s) in frames.items():
        assert np.array_equal(f.view(np.uint32), base.view(np.uint32)), k
        assert (s.closest_hit_rays, s.shadow_rays, s.samples) == (bstats.closest_hit_rays, 0, bstats.samples), k
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM):
        stream, sstats = dev.render(cam, st, fc, w, h)
        tiles = [dev.render(cam, st, fc, w, h, shard_index=r, shard_count=2) for r in range(2)]
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM, shard_mode=rt.abi.RT_SHARD_PASSES):
        passes = [dev.render(cam, st, fc, w, h, shard_index=r, shard_count=2) for r in range(2)]
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_ATOMIC):
        atomic, astats = dev.render(cam, st, fc, w, h)
    REPORT["integrator_ground_truth_schedule"] = {
        "stream_vs_exact": rel_l2(stream, base), "atomic_vs_exact": rel_l2(atomic, base),
        "tile_shards": rel_l2(sum(p[0].astype(np.float64) for p in tiles), base),
        "pass_shards": rel_l2(sum(p[0].astype(np.float64) for p in passes), base)}
    print(REPORT["integrator_ground_truth_schedule"])
    assert sstats.splat_mode == rt.abi.RT_SPLAT_STREAM and rel_l2(stream, base) <= 2e-6
    assert rel_l2(atomic, base) <= 1e-5 and astats.closest_hit_rays == bstats.closest_hit_rays
    for shards in (tiles, passes):
        assert rel_l2(sum(p[0].astype(np.float64) for p in shards), base) <= 1e-5
        assert sum(p[1].closest_hit_rays for p in shards) == bstats.closest_hit_rays
        assert sum(p[1].samples for p in shards) == bstats.samples
        assert all(p[1].shadow_rays == 0 for p in shards)
    # the environment NEE switch has nothing to act on
    with rt.env_sampling(1):
        with dev.configured(splat_mode=E):
            env, estats = dev.render(cam, st, fc, w, h)
    assert np.array_equal(env.view(np.uint32), base.view(np.uint32)) and estats.shadow_rays == 0


# ---- 8. a frame of another integrator leaves the Advanced schedule alone

def test_no_leak_into_advanced(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c3")
    adv = with_integrator(st0, ADVANCED)
    nrm = with_integrator(st0, NORMALS)
    a = rt.abi
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT, shadow_launch=a.RT_SHADOW_LAUNCH_AUTO):
        f0, s0 = dev.render(cam, adv, fc, w, h)
        fn, sn = dev.render(cam, nrm, fc, w, h)
        f1, s1 = dev.render(cam, adv, fc, w, h)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert s0.shadow_launch == s1.shadow_launch
    assert (s0.closest_hit_rays, s0.shadow_rays) == (s1.closest_hit_rays, s1.shadow_rays) and s0.shadow_rays > 0
    assert sn.shadow_rays == 0 and sn.traced_rays[1] == 0
    # no connect launch is made for it, whatever the scene's shadow_launch says (timed launches are counted)
    connect, shade = a.RT_KERNEL_NAMES.index("connect"), a.RT_KERNEL_NAMES.index("shade")
    rt.lib().rt_set_profiling(1)
    try:
        with dev.configured(shadow_launch=a.RT_SHADOW_LAUNCH_SEPARATE):
            _, pa = dev.render(cam, adv, fc, w, h)
            _, pn = dev.render(cam, nrm, fc, w, h)
    finally:
        rt.lib().rt_set_profiling(0)
    assert pa.kernel_launches[connect] > 0 and pa.kernel_launches[shade] > 0
    assert pn.kernel_launches[connect] == 0 and pn.kernel_launches[shade] > 0


def test_no_leak_into_advanced_auto_schedule(rt, scenes):
    """The AUTO shadow launch of a whole frame on a pool of 4M paths or more follows the shadow rays per
    extension ray the scene's previous frame traced (merged from 0.15; C3 traces ~0.26).  A Normals frame
    traces none: were it recorded, the Advanced frame after it would fall back to the separate launch."""
    scene, cam, st0, fc, w, h, dev = scenes("c3")
    spp = 700                                            # 96 x 64 x 700 samples fill a 4M-path pool
    adv = with_integrator(st0, ADVANCED, samples_per_pixel=spp)
    nrm = with_integrator(st0, NORMALS, samples_per_pixel=spp)
    a = rt.abi
    with dev.configured(path_pool=4 << 20, partitions=1, shadow_launch=a.RT_SHADOW_LAUNCH_AUTO):
        dev.render(cam, adv, fc, w, h)                   # the scene's share of shadow rays becomes known
        f0, s0 = dev.render(cam, adv, fc, w, h)
        fn, sn = dev.render(cam, nrm, fc, w, h)
        f1, s1 = dev.render(cam, adv, fc, w, h)
    REPORT["integrator_no_leak_auto"] = {"shadow_per_extension": s0.traced_rays[1]/max(s0.traced_rays[0], 1),
                                         "launch_before": int(s0.shadow_launch), "launch_after": int(s1.shadow_launch)}
    print(REPORT["integrator_no_leak_auto"])
    assert s0.traced_rays[1] >= 0.15*s0.traced_rays[0]
    assert s0.shadow_launch == a.RT_SHADOW_LAUNCH_MERGED
    assert sn.shadow_rays == 0 and sn.traced_rays[1] == 0 and sn.closest_hit_rays == w*h*spp
    assert s1.shadow_launch == s0.shadow_launch
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))


# ---- 9. what is refused

def test_rejections(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c1")
    xy = np.zeros((4, 2), np.uint32)
    so = np.arange(4, dtype=np.uint32)
    good = with_integrator(st0, DISTANCES)
    for integ, word in ((WHITTED, "Whitted"), (GT_RECURSIVE, "Ground Truth Recursive"), (6, "bad integrator"),
                        (-1, "bad integrator")):
        st = with_integrator(st0, integ)
        for call in (lambda: dev.render(cam, st, fc, w, h), lambda: dev.trace_samples(cam, st, w, h, xy, so)):
            with pytest.raises(rt.RenderError) as e:
                call()
            assert e.value.code == rt.abi.RT_ERROR_INVALID
            assert word in str(e.value), str(e.value)
            if integ in (WHITTED, GT_RECURSIVE):
                assert "recursion stack" in str(e.value)
        frame, stats = dev.render(cam, good, fc, w, h)          # the scene still renders
        assert stats.samples == w*h*8 and np.isfinite(frame).all()
    # the names the error carries are the table's
    assert rt.integrator_name(WHITTED) == "Whitted" and not rt.integrator_supported(GT_RECURSIVE)


# ---- every entry point

def test_picture_entry(rt, scenes):
    """rt_render_picture takes the integrator like rt_render (which is rt_render_device on a buffer of its own)."""
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_integrator(st0, NORMALS)
    post = rt.default_settings()[1]
    out = np.zeros((h, w), np.uint32)
    import ctypes as C
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    stats = rt.abi.Stats()
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        err = rt.lib().rt_render_picture(dev._h, C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), 5, w, h,
                                         C.byref(post), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats))
        assert err == 0, rt.lib().rt_last_error()
        frame, fstats = dev.render(cam, st, fc, w, h, total_frame_index=5)
    assert np.array_equal(out, ob.postprocess(frame, post, total_frame_index=6))
    assert stats.closest_hit_rays == fstats.closest_hit_rays == w*h*8 and len(np.unique(out)) > 16


# ---- 10. Ground Truth against the Advanced integrator: two estimators of one integral

def estimator_scene(rt, w, h):
    """Opaque diffuse surfaces (ior 1.5, no metal, no roughness) seen from outside, a uniform sky, one
    emissive sphere, no media, a pinhole camera: Ground Truth's fixed eta_i = 1 and missing inside flip never
    come into play, so it and the Advanced integrator estimate the same integral."""
    import analytic_scenes as an
    s = rt.Scene()
    floor = s.add_diffuse_material((0.7, 0.7, 0.7), 1.5)
    red = s.add_diffuse_material((0.8, 0.3, 0.2), 1.5)
    blue = s.add_diffuse_material((0.2, 0.4, 0.8), 1.5)
    lamp = s.add_emissive_material((6.0, 5.0, 4.0))
    s.add_plane(floor, (0.0, 1.0, 0.0), 0.0)
    s.add_sphere(red, 1.5, rt.translate((-2.2, 1.5, 0.5)))
    s.add_sphere(blue, 1.0, rt.translate((1.8, 1.0, -1.0)))
    s.add_sphere(lamp, 1.5, rt.translate((0.5, 5.0, 1.0)))
    s.set_sky((0.3, 0.35, 0.4), (0.3, 0.35, 0.4))
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 3.5, -10.0), (0.0, 1.5, 0.0), 40.0)
    st, post = rt.default_settings()
    st.samples_per_pixel = 256
    st.max_bounce_count = 12
    st.russian_roulette = 1
    st.vignette_strength = 0.0
    st.lens_distortion = 0.0
    return s, cam, st


@pytest.mark.parametrize("nee", [1, 0])
def test_ground_truth_agrees_with_advanced(rt, nee):
    """Image-mean luminance of every sample of 64 x 48 x 256 spp, depth 12: |m_gt - m_adv| within 4 standard
    errors of the difference, both computed from the samples.  The seed is fixed.  The CPU restatements (the
    checker's Ground Truth against the oracle's Advanced) give z = +1.26 with NEE and MIS, -0.50 without NEE
    at total_frame_index 0."""
    w, h, spp = 64, 48, 256
    s, cam, st = estimator_scene(rt, w, h)
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32)
    so = ss.ravel().astype(np.uint32)
    dev = rt.DeviceScene(s, 0)
    try:
        gt, gstats = dev.trace_samples(cam, with_integrator(st, GT_ITERATIVE), w, h, xy, so)
        adv, astats = dev.trace_samples(cam, with_integrator(st, ADVANCED, next_event_estimation=nee), w, h, xy, so)
    finally:
        dev.close()
    lum = np.array([0.2126, 0.7152, 0.0722])
    lg, la = gt[:, :3].astype(np.float64) @ lum, adv[:, :3].astype(np.float64) @ lum
    se_g, se_a = lg.std(ddof=1)/np.sqrt(len(lg)), la.std(ddof=1)/np.sqrt(len(la))
    z = (lg.mean() - la.mean())/np.hypot(se_g, se_a)
    REPORT[f"integrator_estimator_cross_check_nee{nee}"] = {
        "mean_ground_truth": float(lg.mean()), "se_ground_truth": float(se_g), "mean_advanced": float(la.mean()),
        "se_advanced": float(se_a), "z": float(z)}
    print(REPORT[f"integrator_estimator_cross_check_nee{nee}"])
    assert np.isfinite(lg).all() and np.isfinite(la).all() and se_g > 0 and se_a > 0
    assert gstats.shadow_rays == 0 and (astats.shadow_rays > 0) == bool(nee)
    assert abs(lg.mean() - la.mean()) <= 4.0*np.hypot(se_g, se_a), z
