"""The CPU checker of the two recursive integrators (tests/ref_recursive, tests/ref_recursive_binding.py), the
opt-in functions that need no device, and the finiteness of every case the GPU file compares.  No GPU.

1. The checker's driver (camera, seed, tile loop, splat) is the oracle's: with integrator = Advanced its
   samples and frames equal the oracle's bit for bit, so its restatements of RT/integrators.cpp:310-483 are the
   only text the oracle does not pin.
2. Whitted against closed forms.
3. Ground Truth Recursive against closed forms.
4. Ray counts: the light loop and the two children of a medium hit.
5. rt_scene_integrator_supported(NULL, i), the ambient light through rth_scene.
6. Every case of tests/recursive_cases.py is finite under the checker alone.
"""
import numpy as np
import pytest

import analytic_scenes as an
import oracle_binding as ob
import pyref
import recursive_cases as rc
import ref_recursive_binding as rr
from random_scenes import random_scene

ADVANCED, WHITTED, GT_RECURSIVE = 0, 1, 2
PI_32 = float(np.float32(3.14159265359))
SKY = (0.5, 0.25, 0.75)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera_rays(cam, w, h, xy, jitter):
    """The pinhole camera ray of each sample in float64 (RT/raytracer.cpp:381-401, :443-466; lens radius 0)."""
    v = lambda a: np.array([a.x, a.y, a.z], np.float64)
    fd = cam.focus_distance
    film_center = v(cam.p) - fd*cam.film_distance*v(cam.z)
    u = 1.0 - 2.0*xy[:, 0].astype(np.float64)/w + jitter[:, 0].astype(np.float64)/w
    vv = 1.0 - 2.0*xy[:, 1].astype(np.float64)/h + jitter[:, 1].astype(np.float64)/h
    film_p = film_center + (u*cam.half_film_w*fd)[:, None]*v(cam.x) + (vv*cam.half_film_h*fd)[:, None]*v(cam.y)
    d = film_p - v(cam.p)
    return v(cam.p), d/np.linalg.norm(d, axis=1, keepdims=True)


# ---- 1. the driver

def _driver_cases(rt):
    scene, cam, st, fc, post = rt.load_preset("c1", 48, 32)
    st.samples_per_pixel = 4
    yield "c1", scene, cam, st, fc, 48, 32
    for seed in (11, 12):                     # one with the sky colours, one with an environment map
        s, cam, st, fc = random_scene(rt, seed, 40, 24, spp=2)
        yield f"random{seed}", s, cam, st, fc, 40, 24


def test_driver_is_the_oracles(rt):
    for name, scene, cam, st, fc, w, h in _driver_cases(rt):
        assert st.integrator == ADVANCED
        xy, s = rc.all_samples(w, h, st.samples_per_pixel)
        a, sa = ob.trace_samples(scene.desc(), cam, st, w, h, xy, s, total_frame_index=3)
        b, sb = rr.trace_samples(scene.desc(), cam, st, w, h, xy, s, total_frame_index=3)
        assert np.array_equal(bits(a), bits(b)), name
        assert (sa.closest_hit_rays, sa.shadow_rays) == (sb.closest_hit_rays, sb.shadow_rays), name
        # tile 16: several tiles, ragged at 40 x 24
        fa, ta = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, total_frame_index=3)
        fb, tb = rr.render(scene.desc(), cam, st, fc, w, h, tile=16, total_frame_index=3)
        assert np.array_equal(bits(fa), bits(fb)), name
        assert (ta.closest_hit_rays, ta.shadow_rays, ta.samples) == (tb.closest_hit_rays, tb.shadow_rays, tb.samples), name
        # a tile shard is the same subset of tiles
        fa, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, shard_index=1, shard_count=2)
        fs, _ = rr.render(scene.desc(), cam, st, fc, w, h, tile=16, shard_index=1, shard_count=2)
        assert np.array_equal(bits(fa), bits(fs)), name
        # the timing runs' worker threads trace the same samples (the frame's float sums differ in order only)
        fc_, tc = rr.render(scene.desc(), cam, st, fc, w, h, tile=16, total_frame_index=3, threads=3)
        assert (tc.closest_hit_rays, tc.shadow_rays, tc.samples) == (tb.closest_hit_rays, tb.shadow_rays, tb.samples), name
        assert np.allclose(fc_, fb, rtol=1e-4, atol=1e-5), name


# ---- 2. Whitted

def test_whitted_diffuse_plane_under_ambient_pi(rt):
    """A diffuse plane of ior 1 (reflectance 0: the :406 branch), no lights, ambient pi: the sample is
    (1/pi) colour pi = the albedo, or the checker colour where floor(x/4) ^ floor(z/4) is odd."""
    w, h = 48, 32
    albedo, checker = (0.25, 0.5, 0.75), (0.9, 0.1, 0.3)
    s = rt.Scene()
    s.add_plane(s.add_diffuse_material(albedo, 1.0, checkers=True, checker_color=checker), (0.0, 1.0, 0.0), 0.0)
    s.set_sky(SKY, SKY)
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 10.0, -2.0), (0.0, 0.0, 0.5), 60.0)
    st = rc.with_settings(an.settings(rt, spp=2, bounces=3), integrator=WHITTED)
    xy, so = rc.all_samples(w, h, 2)
    out, stats = rr.trace_samples(s.desc(), cam, st, w, h, xy, so, ambient=(PI_32,)*3)
    o, d = camera_rays(cam, w, h, xy, out[:, 3:])
    assert np.all(d[:, 1] < 0)                                   # every ray meets the plane
    p = o + (-o[1]/d[:, 1])[:, None]*d
    cx, cz = 0.25*p[:, 0], 0.25*p[:, 2]
    clear = (np.abs(cx - np.round(cx)) > 1e-3) & (np.abs(cz - np.round(cz)) > 1e-3)   # off the checker's edges
    odd = ((np.floor(cx).astype(np.int64) ^ np.floor(cz).astype(np.int64)) & 1) == 1
    want = np.where(odd[:, None], np.array(checker), np.array(albedo))
    assert clear.sum() > 0.9*len(xy) and 100 < odd[clear].sum() < clear.sum() - 100
    assert np.max(np.abs(out[clear, :3] - want[clear])) <= 1e-6
    assert stats.closest_hit_rays == len(xy) and stats.shadow_rays == 0
    # without the ambient light the plane is black
    dark, _ = rr.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert np.all(dark[:, :3] == 0.0)


def test_whitted_metal_sky_miss_and_depth_zero(rt):
    w, h = 32, 32
    albedo = (0.6, 0.5, 0.4)
    s = rt.Scene()
    s.add_sphere(s.add_material(0, albedo, 0.0, 0.0, 1.5, 1.0, 0.0), 2.0, rt.translate((0.0, 0.0, 0.0)))
    s.set_environment_map(np.broadcast_to(np.array(SKY, np.float32), (32, 64, 3)))   # the texel fetch is exact
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -7.0), (0.0, 0.0, 0.0), 40.0)
    st = rc.with_settings(an.settings(rt, spp=1, bounces=4), integrator=WHITTED)
    xy, so = rc.all_samples(w, h, 1)
    out, stats = rr.trace_samples(s.desc(), cam, st, w, h, xy, so, ambient=(0.3, 0.2, 0.1))
    o, d = camera_rays(cam, w, h, xy, out[:, 3:])
    b = -(d @ o)
    disc = b*b - (o @ o - 4.0)
    hit, miss = disc > 0.05, disc < -0.05
    assert hit.sum() > 100 and miss.sum() > 100
    # metallic 1: reflectance 1, the mirror ray leaves the convex sphere for the sky: albedo . c
    want = np.array(albedo)*np.array(SKY)
    assert np.max(np.abs(out[hit, :3] - want)) <= 1e-6
    # a camera ray that misses: the sky exactly
    assert np.array_equal(out[miss, :3], np.broadcast_to(np.array(SKY, np.float32), (miss.sum(), 3)))
    # one camera ray per sample and one mirror ray per hit (the samples on the silhouette may go either way)
    assert stats.shadow_rays == 0
    assert abs(int(stats.closest_hit_rays) - len(xy) - int((disc > 0).sum())) <= int((~hit & ~miss).sum())
    # max_bounce_count 0: exactly 0 and no rays
    out0, stats0 = rr.trace_samples(s.desc(), cam, rc.with_settings(st, max_bounce_count=0), w, h, xy, so,
                                    ambient=(0.3, 0.2, 0.1))
    assert np.all(out0[:, :3] == 0.0) and stats0.closest_hit_rays == 0 and stats0.shadow_rays == 0
    frame, fstats = rr.render(s.desc(), cam, rc.with_settings(st, max_bounce_count=0), rt.load_reconstruction_kernel("Box"), w, h)
    assert np.all(frame[..., :3] == 0.0) and np.all(frame[..., 3] == 1.0) and fstats.closest_hit_rays == 0


# ---- 3. Ground Truth Recursive

def test_gtr_emitter_and_depth_zero(rt):
    w, h = 24, 24
    le = (2.0, 3.0, 4.0)
    s = rt.Scene()
    s.add_sphere(s.add_emissive_material(le), 2.0, rt.translate((0.0, 0.0, 0.0)))
    s.set_environment_map(np.broadcast_to(np.array(SKY, np.float32), (32, 64, 3)))
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -7.0), (0.0, 0.0, 0.0), 40.0)
    st = rc.with_settings(an.settings(rt, spp=2, bounces=6), integrator=GT_RECURSIVE)
    xy, so = rc.all_samples(w, h, 2)
    out, stats = rr.trace_samples(s.desc(), cam, st, w, h, xy, so)
    o, d = camera_rays(cam, w, h, xy, out[:, 3:])
    b = -(d @ o)
    disc = b*b - (o @ o - 4.0)
    hit, miss = disc > 0.05, disc < -0.05
    assert hit.sum() > 50 and miss.sum() > 50 and stats.closest_hit_rays == len(xy) and stats.shadow_rays == 0
    # an emitter seen directly: exactly Le, no throughput; elsewhere the sky
    assert np.array_equal(out[hit, :3], np.broadcast_to(np.array(le, np.float32), (hit.sum(), 3)))
    assert np.array_equal(out[miss, :3], np.broadcast_to(np.array(SKY, np.float32), (miss.sum(), 3)))
    # max_bounce_count 0: the sky, with no ray traced (:470 is reached without :433)
    out0, stats0 = rr.trace_samples(s.desc(), cam, rc.with_settings(st, max_bounce_count=0), w, h, xy, so)
    assert np.array_equal(out0[:, :3], np.broadcast_to(np.array(SKY, np.float32), (len(xy), 3)))
    assert stats0.closest_hit_rays == 0 and stats0.shadow_rays == 0


def _tangents(n):
    """get_tangents (RT/integrators.cpp:58-66) in float64."""
    sign = np.copysign(1.0, n[2])
    a = -1.0/(sign + n[2])
    b = n[0]*n[1]*a
    return (np.array([1.0 + sign*n[0]*n[0]*a, sign*b, -sign*n[0]]), np.array([b, sign + n[1]*n[1]*a, -n[1]]))


def test_gtr_depth_one_sphere(rt):
    """An albedo-a sphere under a uniform sky c at depth 1: the one hit draws r (:442); r.x below the Fresnel
    reflectance passes the sky through (:453), else the sample is 2 a c max(0, N . R) with R the hemisphere
    direction of (r.y, r.z) (:460-466), recomputed here from the same draw of an independent RandomSeries."""
    w, h, R, D = 16, 16, 2.0, 7.0
    a_, ior = (0.6, 0.5, 0.4), 1.5
    s = rt.Scene()
    s.add_sphere(s.add_diffuse_material(a_, ior), R, rt.translate((0.0, 0.0, 0.0)))
    s.set_sky(SKY, SKY)
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -D), (0.0, 0.0, 0.0), 40.0)
    st = rc.with_settings(an.settings(rt, spp=2, bounces=1), integrator=GT_RECURSIVE, sampling_strategy=0)
    xy, so = rc.all_samples(w, h, 2)
    out, stats = rr.trace_samples(s.desc(), cam, st, w, h, xy, so, total_frame_index=2, tile=64)
    o, d = camera_rays(cam, w, h, xy, out[:, 3:])
    b = -(d @ o)
    disc = b*b - (o @ o - R*R)
    checked = mirrored = 0
    for i in np.nonzero(disc > 0.5)[0]:
        x, y = int(xy[i, 0]), int(xy[i, 1])
        e = pyref.RandomSeries(pyref.sample_seed(2, 0, 0, y*w + x, int(so[i])))
        e.unilaterals()                                         # the AA jitter
        e.unilaterals()                                         # the lens sample
        r = e.unilaterals()
        t = b[i] - np.sqrt(disc[i])
        n = (o + t*d[i])/R
        ci = -float(d[i] @ n)
        si = np.sqrt(max(0.0, 1.0 - ci*ci))/ior
        ct = np.sqrt(max(0.0, 1.0 - si*si))
        refl = 0.5*(((ior*ci - ct)/(ior*ci + ct))**2 + ((ci - ior*ct)/(ci + ior*ct))**2)
        if abs(r[0] - refl) < 1e-4:
            continue
        if r[0] < refl:
            want = np.array(SKY)
            mirrored += 1
        else:
            T, B = _tangents(n)
            az, yy = 2.0*np.pi*r[1], r[2]
            hx, hz = np.cos(az)*np.sqrt(1.0 - yy*yy), np.sin(az)*np.sqrt(1.0 - yy*yy)
            Rd = hx*B + yy*n + hz*T
            want = 2.0*np.array(a_)*np.array(SKY)*max(0.0, float(n @ Rd))
        assert np.max(np.abs(out[i, :3] - want)) <= 1e-5, (i, out[i, :3], want)
        checked += 1
    assert checked > 100 and 0 < mirrored < checked
    assert stats.closest_hit_rays == len(xy) and stats.shadow_rays == 0


# ---- 4. ray counts

def test_whitted_light_loop_ray_counts(rt):
    """One hit on a non-emissive surface with L lights facing it casts L shadow rays: a floor under three
    small, far sphere lights, depth 1.  A light sample whose point faces away from the hit (the rim of the
    hemisphere towards it, a ~r/d share) casts none."""
    L = 3
    s = rt.Scene()
    s.add_plane(s.add_diffuse_material((0.5, 0.5, 0.5), 1.0), (0.0, 1.0, 0.0), 0.0)
    for k in range(L):
        s.add_sphere(s.add_emissive_material((50.0, 40.0, 30.0)), 0.05, rt.translate((4.0*k - 4.0, 30.0, 2.0)))
    s.create_scene_bvh()
    assert s.desc().light_count == L
    st = rc.with_settings(an.settings(rt, spp=1, bounces=1), integrator=WHITTED)
    cam = an.camera(rt, 1, 1, (0.0, 10.0, -2.0), (0.0, 0.0, 0.5), 30.0)
    out, stats = rr.trace_samples(s.desc(), cam, st, 1, 1, [[0, 0]], [0])
    assert (stats.closest_hit_rays, stats.shadow_rays) == (1, L) and np.all(out[0, :3] > 0.0)
    w, h = 32, 24
    cam = an.camera(rt, w, h, (0.0, 10.0, -2.0), (0.0, 0.0, 0.5), 30.0)
    xy, so = rc.all_samples(w, h, 4)
    out, stats = rr.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert stats.closest_hit_rays == len(xy)
    assert 0.98*L*len(xy) <= stats.shadow_rays <= L*len(xy)
    # deeper: the same hit casts the same rays (reflectance 0: no child)
    deep, dstats = rr.trace_samples(s.desc(), cam, rc.with_settings(st, max_bounce_count=5), w, h, xy, so)
    assert np.array_equal(bits(deep), bits(out)) and dstats.shadow_rays == stats.shadow_rays


def test_whitted_medium_hit_spawns_two_children(rt):
    """A glass sphere filling the view, no lights: depth 1 traces the camera ray; depth 2 its two children, the
    refracted one meeting the sphere from inside and the reflected one the sky; depth 3 the two children of
    that inside hit as well: n, 3 n and 5 n closest rays."""
    w, h = 16, 16
    s = rt.Scene()
    s.add_sphere(s.add_translucent_material((0.1, 0.2, 0.3), 1.5), 5.0, rt.translate((0.0, 0.0, 0.0)))
    s.set_sky(SKY, SKY)
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -7.0), (0.0, 0.0, 0.0), 30.0)
    st = rc.with_settings(an.settings(rt, spp=1, bounces=1), integrator=WHITTED)
    xy, so = rc.all_samples(w, h, 1)
    n = len(xy)
    counts = []
    for depth in (1, 2, 3):
        out, stats = rr.trace_samples(s.desc(), cam, rc.with_settings(st, max_bounce_count=depth), w, h, xy, so)
        assert np.isfinite(out).all() and stats.shadow_rays == 0
        counts.append(int(stats.closest_hit_rays))
    assert counts == [n, 3*n, 5*n]


# ---- 5. the opt-in functions that need no device

def test_scene_integrator_supported_without_a_scene(rt):
    lib = rt.lib()
    for i in range(-1, 7):
        assert lib.rt_scene_integrator_supported(None, i) == lib.rt_integrator_supported(i)
        assert rt.scene_integrator_supported(None, i) == rt.integrator_supported(i)
    assert lib.rt_abi_version() == 8
    # NULL arguments are refused, not dereferenced
    assert lib.rt_scene_set_recursive_integrators(None, 1) == rt.abi.RT_ERROR_INVALID
    assert lib.rt_scene_set_ambient_light(None, None) == rt.abi.RT_ERROR_INVALID


def test_ambient_light_round_trip(rt):
    s = rt.Scene()
    assert s.ambient_light() == (0.0, 0.0, 0.0)
    s.set_ambient_light((0.25, 0.5, 2.0))
    assert s.ambient_light() == (0.25, 0.5, 2.0)
    s.set_ambient_light(0.0)
    assert s.ambient_light() == (0.0, 0.0, 0.0)
    # the presets set what the reference's scene descriptions set (RT/raytracer.cpp:812, :832, :908)
    pi = float(np.float32(PI_32))
    for name, want in (("week_1", (pi,)*3), ("week_2", (pi,)*3), ("week_3", (0.0,)*3), ("c1", (0.0,)*3)):
        scene = rt.load_preset(name, 16, 16)[0]
        assert scene.ambient_light() == want, name
    w5 = rt.load_preset("week_5", 16, 16)[0].ambient_light()
    assert w5 == tuple(float(np.float32(c)) for c in (0.1, 0.7, 2.0))


# ---- 6. every case the GPU file compares is finite under the checker alone

@pytest.fixture(scope="module")
def cache(rt):
    return rc.SceneCache(rt)


@pytest.mark.parametrize("case", rc.cases(), ids=[c[0] for c in rc.cases()])
def test_checker_is_finite_on_every_gpu_case(rt, cache, case):
    cid, name, integ, depth, sampler, (w, h), spp = case
    scene, cam, st0, fc = cache.get(name, w, h)
    st = rc.case_settings(st0, integ, depth, sampler, spp)
    xy, so = rc.all_samples(w, h, spp)
    out, stats = rr.trace_samples(scene.desc(), cam, st, w, h, xy, so, ambient=scene.ambient_light())
    assert np.isfinite(out).all(), cid
    frame, fstats = rr.render(scene.desc(), cam, st, fc, w, h, ambient=scene.ambient_light())
    assert np.isfinite(frame).all(), cid
    assert (fstats.closest_hit_rays, fstats.shadow_rays) == (stats.closest_hit_rays, stats.shadow_rays)
    if depth == 0:
        assert stats.closest_hit_rays == 0 and (integ == GT_RECURSIVE or np.all(out[:, :3] == 0.0))
    elif name != "c1" or integ == WHITTED:
        assert np.count_nonzero(out[:, :3]) > 0, cid              # (c1's sky is black: depth 1 sees the lamp only)
