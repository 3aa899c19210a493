"""The CPU checker of the integrators besides the Advanced one (tests/ref_integrators, tests/ref_binding.py)
and the ABI's integrator table.  No GPU.

1. The helper's driver (camera, seed, tile loop, splat) is the oracle's: with integrator = Advanced its
   samples and frames equal the oracle's bit for bit, so its restatements of RT/integrators.cpp:486-579 are
   the only text the oracle does not pin.
2. Normals and Distances against closed forms: a sphere on the optical axis of a pinhole camera.
3. Ground Truth Iterative's exact cases: no bounces, nothing hit, an emitter hit.
4. rt_integrator_name / rt_find_integrator / rt_integrator_supported.
"""
import numpy as np
import pytest

import analytic_scenes as an
import oracle_binding as ob
import ref_binding as rb
from random_scenes import random_scene

ADVANCED, WHITTED, GT_RECURSIVE, GT_ITERATIVE, NORMALS, DISTANCES = range(6)
NAMES = ["Advanced Pathtracer", "Whitted", "Ground Truth Recursive", "Ground Truth Iterative", "Normals", "Distances"]


def all_samples(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32), ss.ravel().astype(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
        xy, s = all_samples(w, h, st.samples_per_pixel)
        a, sa = ob.trace_samples(scene.desc(), cam, st, w, h, xy, s, total_frame_index=3)
        b, sb = rb.trace_samples(scene.desc(), cam, st, w, h, xy, s, total_frame_index=3)
        assert np.array_equal(bits(a), bits(b)), name
        assert (sa.closest_hit_rays, sa.shadow_rays) == (sb.closest_hit_rays, sb.shadow_rays), name
        # tile 16: several tiles, ragged at 40 x 24
        fa, ta = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, total_frame_index=3)
        fb, tb = rb.render(scene.desc(), cam, st, fc, w, h, tile=16, total_frame_index=3)
        assert np.array_equal(bits(fa), bits(fb)), name
        assert (ta.closest_hit_rays, ta.shadow_rays, ta.samples) == (tb.closest_hit_rays, tb.shadow_rays, tb.samples), name
        # a tile shard is the same subset of tiles
        fa, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, shard_index=1, shard_count=2)
        fb, _ = rb.render(scene.desc(), cam, st, fc, w, h, tile=16, shard_index=1, shard_count=2)
        assert np.array_equal(bits(fa), bits(fb)), name


# ---- 2. closed forms

R, D = 2.0, 7.0
SKY = (0.5, 0.25, 0.75)


def sphere_scene(rt, w, h, material="diffuse", env=False, look_away=False):
    """A sphere of radius R at the origin, the pinhole camera at distance D on its axis, a uniform sky: the
    two sky colours equal, or (env) a constant environment map, whose texel fetch is exact."""
    s = rt.Scene()
    m = s.add_emissive_material((2.0, 3.0, 4.0)) if material == "emissive" else s.add_diffuse_material((0.6, 0.5, 0.4), 1.5)
    s.add_sphere(m, R, rt.translate((0.0, 0.0, 0.0)))
    if env:
        s.set_environment_map(np.broadcast_to(np.array(SKY, np.float32), (32, 64, 3)))
    else:
        s.set_sky(SKY, SKY)
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -D), (0.0, 0.0, -2*D) if look_away else (0.0, 0.0, 0.0), 40.0)
    st = an.settings(rt, spp=1, bounces=8)
    return s, cam, st


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


@pytest.mark.parametrize("bounces", [8, 0])
@pytest.mark.parametrize("env", [False, True])
def test_first_hit_closed_forms(rt, bounces, env):
    w, h = 32, 32
    s, cam, st = sphere_scene(rt, w, h, env=env)
    st.max_bounce_count = bounces               # never read by these two integrators
    xy, so = all_samples(w, h, 1)
    st.integrator = DISTANCES
    dist, sd = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    st.integrator = NORMALS
    nrm, sn = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert sd.closest_hit_rays == sn.closest_hit_rays == len(xy) and sd.shadow_rays == sn.shadow_rays == 0
    assert np.array_equal(dist[:, 3:], nrm[:, 3:])
    o, d = camera_rays(cam, w, h, xy, dist[:, 3:])
    b = -(d @ o)                                # the sphere is at the origin
    disc = b*b - (o @ o - R*R)
    hit = disc > 0
    # away from the silhouette, where the root is well conditioned in float32
    solid = disc > 0.5
    assert solid.sum() > 100 and (~hit).sum() > 100
    t = b - np.sqrt(np.where(hit, disc, 0.0))
    n = (o + t[:, None]*d)/R
    assert np.max(np.abs(dist[solid, :3] - (1.0 - t[solid]/15.0)[:, None])) <= 1e-5
    assert np.max(np.abs(nrm[solid, :3] - 0.5*(1.0 + n[solid]))) <= 1e-5
    # the sphere's nearest point: no sample is nearer, and the sample nearest the axis is within the
    # sagitta of its offset of 1 - (D - R)/15; its normal points back at the camera
    near = 1.0 - (D - R)/15.0
    assert np.all(dist[hit, 0] <= np.float32(near) + 1e-6)
    k = int(np.argmax(d[:, 2]))
    assert abs(dist[k, 0] - near) <= 1e-3 and np.max(np.abs(nrm[k, :3] - (0.5, 0.5, 0.0))) <= 5e-2
    # every miss is the sky: exactly the texel of the constant map; within an ulp of lerp(c, c, |d.y|)
    clear = disc < -0.5
    sky = np.array(SKY, np.float32)
    for out in (dist, nrm):
        if env:
            assert np.array_equal(out[clear, :3], np.broadcast_to(sky, (clear.sum(), 3)))
        else:
            assert np.max(np.abs(out[clear, :3] - sky)/np.spacing(sky)) <= 1.0
    # the frame: box filter, 1 spp, every pixel its one sample
    fc = rt.load_reconstruction_kernel("Box")
    frame, fs = rb.render(s.desc(), cam, st, fc, w, h)
    assert fs.closest_hit_rays == w*h and np.all(frame[..., 3] == 1.0)
    assert np.array_equal(bits(frame[..., :3].reshape(-1, 3)), bits(nrm[:, :3]))


# ---- 3. Ground Truth Iterative

def test_ground_truth_exact_cases(rt):
    w, h = 24, 24
    xy, so = all_samples(w, h, 2)
    # no bounces: nothing is traced, every sample is 0
    s, cam, st = sphere_scene(rt, w, h)
    st.integrator = GT_ITERATIVE
    st.max_bounce_count = 0
    out, stats = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert np.all(out[:, :3] == 0.0) and stats.closest_hit_rays == 0
    # nothing in view: the sky, the bits Normals returns for the same ray
    s, cam, st = sphere_scene(rt, w, h, look_away=True)
    st.integrator = GT_ITERATIVE
    out, stats = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    st.integrator = NORMALS
    sky, _ = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert np.array_equal(bits(out), bits(sky)) and stats.closest_hit_rays == len(xy) and stats.shadow_rays == 0
    assert np.max(np.abs(out[:, :3] - np.array(SKY, np.float32))) <= 1e-6
    s, cam, st = sphere_scene(rt, w, h, env=True, look_away=True)
    st.integrator = GT_ITERATIVE
    out, _ = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    assert np.array_equal(out[:, :3], np.broadcast_to(np.array(SKY, np.float32), (len(xy), 3)))
    # an emitter: its emission where the camera ray hits it, the sky elsewhere, one ray per sample
    s, cam, st = sphere_scene(rt, w, h, material="emissive", env=True)
    st.integrator = GT_ITERATIVE
    out, stats = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    st.integrator = DISTANCES
    dist, _ = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    hit = dist[:, 0] != np.float32(SKY[0])       # Distances is grey (>= 1 - 7/15) on the sphere
    assert 50 < hit.sum() < len(xy) - 50 and stats.closest_hit_rays == len(xy)
    assert np.array_equal(out[hit, :3], np.broadcast_to(np.array((2.0, 3.0, 4.0), np.float32), (hit.sum(), 3)))
    assert np.array_equal(out[~hit, :3], np.broadcast_to(np.array(SKY, np.float32), ((~hit).sum(), 3)))


def test_ground_truth_diffuse_sphere_is_a_furnace(rt):
    """An albedo-1 diffuse sphere under a uniform sky: a Ground Truth path leaves the convex sphere after
    one event, a mirror reflection (weight 1) or a uniform bounce of weight 2 dot(R, N) (mean 1).  The
    image mean over many samples is the sky within 4 standard errors (seed fixed)."""
    w, h = 24, 24
    s = rt.Scene()
    s.add_sphere(s.add_diffuse_material((1.0, 1.0, 1.0), 1.5), 2.0, rt.translate((0.0, 0.0, 0.0)))
    s.set_sky(SKY, SKY)
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, -7.0), (0.0, 0.0, 0.0), 40.0)
    st = an.settings(rt, spp=16, bounces=8)
    st.integrator = GT_ITERATIVE
    xy, so = all_samples(w, h, 16)
    out, stats = rb.trace_samples(s.desc(), cam, st, w, h, xy, so)
    g = out[:, 1].astype(np.float64)
    se = g.std(ddof=1)/np.sqrt(len(g))
    assert g.std() > 0.01 and abs(g.mean() - SKY[1]) <= 4*se, (g.mean(), se)
    assert stats.shadow_rays == 0 and len(xy) < stats.closest_hit_rays <= 2*len(xy)


# ---- 4. the ABI's integrator table (no device)

def test_integrator_table(rt):
    lib = rt.lib()
    assert lib.rt_abi_version() == 8
    a = rt.abi
    assert [a.RT_INTEGRATOR_ADVANCED, a.RT_INTEGRATOR_WHITTED, a.RT_INTEGRATOR_GROUND_TRUTH_RECURSIVE,
            a.RT_INTEGRATOR_GROUND_TRUTH_ITERATIVE, a.RT_INTEGRATOR_NORMALS, a.RT_INTEGRATOR_DISTANCES] == list(range(6))
    assert [rt.integrator_name(i) for i in range(6)] == NAMES
    assert rt.integrator_name(6) is None and rt.integrator_name(-1) is None
    assert [rt.find_integrator(n) for n in NAMES] == list(range(6))
    assert rt.find_integrator("Bidirectional") == 0 and rt.find_integrator("normals") == 0 and rt.find_integrator("") == 0
    assert [int(rt.integrator_supported(i)) for i in range(6)] == [1, 0, 0, 1, 1, 1]
    assert not rt.integrator_supported(6) and not rt.integrator_supported(-1)
    assert [lib.rt_integrator_supported(i) for i in range(-1, 7)] == [0, 1, 0, 0, 1, 1, 1, 0]


def test_helper_refuses_the_recursive_integrators(rt):
    s, cam, st = sphere_scene(rt, 8, 8)
    import ctypes as C
    for integ in (WHITTED, GT_RECURSIVE, 6, -1):
        st.integrator = integ
        out = np.zeros((1, 5), np.float32)
        xy = np.zeros(2, np.uint32)
        so = np.zeros(1, np.uint32)
        err = rb.load().ref_trace_samples(C.byref(s.desc()), C.byref(cam), C.byref(st), 8, 8, 64, 64, 0, 0, 1,
                                          xy.ctypes.data_as(C.POINTER(C.c_uint32)), so.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          out.ctypes.data_as(C.POINTER(C.c_float)), None)
        assert err == rt.abi.RT_ERROR_INVALID
