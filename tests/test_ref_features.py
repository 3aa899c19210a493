"""The CPU checker of the feature frames and of the denoise stage that uses them (tests/ref_features,
tests/ref_features_binding.py), and what the new entries do without a device.  No GPU.

1. The checker's driver is the oracle's: with the Advanced integrator in the walk's place its frames and
   samples equal the oracle's bit for bit, so the walk is the only text the oracle does not pin.
2. The walk against closed forms: a mirror facing a checkered wall, a medium slab in front of a wall, an emitter
   in a mirror, misses before and after a reflection, two facing mirrors at depth 63.
3. The anchor: with max_bounce_count 0 and 1 the NORMAL and DISTANCE frames are tests/ref_integrators' integrator
   4 and 5 frames.
4. The prefix identity with the Advanced integrator of the oracle.
5. The filter: the stage's invariants, equality with tests/ref_denoise when nothing new is on, demodulation.
6. Defaults, workspace, refusals by name, no device.
7. Usefulness of the new defaults (DESIGN.md has the table).
"""
import ctypes as C
import math
import re

import numpy as np
import pytest

import analytic_scenes as an
import oracle_binding as ob
import ref_binding as rb
import ref_denoise_binding as rd
import ref_features_binding as rf
from random_scenes import random_scene
from recursive_cases import all_samples, mirrors_scene

F = np.float32
NORMAL, DISTANCE, ALBEDO = range(3)
NORMALS, DISTANCES = 4, 5
EPSILON = 1e-3
bits = rf.bits


def with_settings(st, **fields):
    c = type(st).from_buffer_copy(st)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


# ---- 1. the driver

def test_driver_is_the_oracles(rt):
    cases = []
    scene, cam, st, fc, post = rt.load_preset("c1", 48, 32)
    st.samples_per_pixel = 4
    cases.append(("c1", scene, cam, st, fc, 48, 32))
    s, cam, st, fc = random_scene(rt, 11, 40, 24, spp=2)
    cases.append(("random11", s, cam, st, fc, 40, 24))
    for name, scene, cam, st, fc, w, h in cases:
        xy, so = all_samples(w, h, st.samples_per_pixel)
        a, sa = ob.trace_samples(scene.desc(), cam, st, w, h, xy, so, total_frame_index=3)
        b = rf.trace_samples(scene.desc(), cam, st, w, h, xy, so, rf.ADVANCED, total_frame_index=3)
        assert np.array_equal(bits(a), bits(b[0])), name
        assert (sa.closest_hit_rays, sa.shadow_rays) == (b[4].closest_hit_rays, b[4].shadow_rays), name
        fa, ta = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, total_frame_index=3)
        fb, tb, _ = rf.render(scene.desc(), cam, st, fc, w, h, rf.ADVANCED, tile=16, total_frame_index=3)
        assert np.array_equal(bits(fa), bits(fb)), name
        assert (ta.closest_hit_rays, ta.shadow_rays, ta.samples) == (tb.closest_hit_rays, tb.shadow_rays, tb.samples), name
        fa, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=1, tile=16, shard_index=1, shard_count=2)
        fb, _, _ = rf.render(scene.desc(), cam, st, fc, w, h, rf.ADVANCED, tile=16, shard_index=1, shard_count=2)
        assert np.array_equal(bits(fa), bits(fb)), name


# ---- 2. closed forms

A, B = (0.25, 0.5, 0.75), (0.75, 0.5, 0.125)           # the environment map's two halves; exact in f32
WALL, CHECK = (0.6, 0.5, 0.4), (0.1, 0.2, 0.3)


def two_sided_sky(s):
    """u < 0.5 (directions with d.z < 0) is A, u >= 0.5 (d.z > 0) is B: a texel fetch, exact."""
    env = np.zeros((32, 64, 3), F)
    env[:, :32] = A
    env[:, 32:] = B
    s.set_environment_map(env)


def pinhole(rt, w, h, bounces=8, at=(0.0, 0.0, 5.0)):
    cam = an.camera(rt, w, h, (0.0, 0.0, 0.0), at, 40.0)
    st = an.settings(rt, spp=1, bounces=bounces)
    st.vignette_strength = 0.0
    st.lens_distortion = 0.0
    return cam, st


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


def walk(s, cam, st, w, h, feature):
    xy, so = all_samples(w, h, 1)
    out, end, spec, T, stats = rf.trace_samples(s.desc(), cam, st, w, h, xy, so, feature)
    o, d = camera_rays(cam, w, h, xy, out[:, 3:])
    return out[:, :3], end, spec, T, stats, o, d


def test_a_mirror_facing_a_checkered_wall(rt):
    """The camera at the origin looks at a perfect mirror at z = 2; behind it a diffuse wall (ior 1: no Fresnel
    reflection) at z = -3 with checkers.  Every walk: mirror, wall.  NORMAL is the wall's, DISTANCE is of
    t0 + t1 = 7 / d.z (less the reflected ray's offset), ALBEDO the wall's colour under the reflected ray."""
    w, h = 32, 24
    s = rt.Scene()
    mirror = s.add_material(0, (0.9, 0.9, 0.9), 0.0, 0.0, 1.5, 1.0, 0.0)
    wall = s.add_diffuse_material(WALL, 1.0, checkers=True, checker_color=CHECK)
    s.add_plane(mirror, (0.0, 0.0, -1.0), -2.0)
    s.add_plane(wall, (0.0, 0.0, 1.0), -3.0)
    two_sided_sky(s)
    s.create_scene_bvh()
    cam, st = pinhole(rt, w, h)
    nrm, end, spec, T, stats, o, d = walk(s, cam, st, w, h, NORMAL)
    assert np.all(end == rf.END_DIFFUSE) and np.all(spec == 1)
    assert stats.closest_hit_rays == 2*w*h and stats.shadow_rays == 0
    assert np.array_equal(nrm, np.broadcast_to(np.array((0.5, 0.5, 1.0), F), nrm.shape))
    dist = walk(s, cam, st, w, h, DISTANCE)[0]
    t = 7.0/d[:, 2]
    assert np.all(dist[:, 0] == dist[:, 1]) and np.all(dist[:, 0] == dist[:, 2])
    assert np.max(np.abs(dist[:, 0] - (1.0 - t/15.0))) <= (EPSILON + 1e-4)/15.0
    assert np.max(np.abs(T - t)) <= EPSILON + 1e-4
    alb = walk(s, cam, st, w, h, ALBEDO)[0]
    x = t*d[:, 0]                                        # the reflection keeps the ray's x and y components
    clear = np.abs(x/4.0 - np.round(x/4.0)) > 1e-3       # away from a checker edge
    odd =(np.floor(0.25*x).astype(np.int64) ^ int(math.floor(0.25*-3.0))) & 1
    want = np.where(odd[:, None] == 1, np.array(CHECK, F), np.array(WALL, F))
    assert clear.sum() > 0.95*len(x) and 0.1 < odd.mean() < 0.9
    assert np.array_equal(alb[clear], want[clear])


def test_a_medium_slab_in_front_of_a_wall(rt):
    """A glass box (ior 1.5) from z = 2.5 to 3.5 in front of a diffuse wall at z = 6.  A walk that refracts in
    and out reaches the wall along a parallel ray: NORMAL is the wall's, ALBEDO the wall's, and
    T = 5 / cos i + 1 / cos t with sin t = sin i / 1.5.  A walk reflected at the front face misses."""
    w, h = 32, 24
    s = rt.Scene()
    glass = s.add_translucent_material((0.1, 0.2, 0.3), 1.5)
    wall = s.add_diffuse_material(WALL, 1.0)
    s.add_box(glass, (50.0, 50.0, 0.5), rt.translate((0.0, 0.0, 3.0)))
    s.add_plane(wall, (0.0, 0.0, -1.0), -6.0)
    two_sided_sky(s)
    s.create_scene_bvh()
    cam, st = pinhole(rt, w, h)
    nrm, end, spec, T, stats, o, d = walk(s, cam, st, w, h, NORMAL)
    through = (end == rf.END_DIFFUSE) & (spec == 2)
    back = (end == rf.END_MISS) & (spec == 1)
    assert through.mean() > 0.85 and stats.closest_hit_rays == w*h + spec.sum()
    assert np.array_equal(nrm[through], np.broadcast_to(np.array((0.5, 0.5, 0.0), F), (through.sum(), 3)))
    assert np.array_equal(nrm[back], np.broadcast_to(np.array(A, F), (back.sum(), 3)))     # the sky behind the camera
    cos_i = d[:, 2]
    cos_t = np.sqrt(1.0 - (1.0 - cos_i**2)/1.5**2)
    t = 5.0/cos_i + 1.0/cos_t
    assert np.max(np.abs(T[through] - t[through])) <= 2*EPSILON + 1e-4
    dist = walk(s, cam, st, w, h, DISTANCE)[0]
    assert np.max(np.abs(dist[through, 0] - (1.0 - t[through]/15.0))) <= (2*EPSILON + 1e-4)/15.0
    alb = walk(s, cam, st, w, h, ALBEDO)[0]
    assert np.array_equal(alb[through], np.broadcast_to(np.array(WALL, F), (through.sum(), 3)))
    assert np.all(alb[back] == 1.0)


def test_an_emitter_seen_in_a_mirror(rt):
    w, h = 32, 24
    s = rt.Scene()
    mirror = s.add_material(0, (0.9, 0.9, 0.9), 0.0, 0.0, 1.5, 1.0, 0.0)
    lamp = s.add_emissive_material((2.0, 3.0, 4.0))
    s.add_plane(mirror, (0.0, 0.0, -1.0), -2.0)
    s.add_sphere(lamp, 1.5, rt.translate((0.0, 0.0, -4.0)))
    two_sided_sky(s)
    s.create_scene_bvh()
    cam, st = pinhole(rt, w, h)
    alb, end, spec, T, stats, o, d = walk(s, cam, st, w, h, ALBEDO)
    lit = end == rf.END_EMITTER
    assert 20 < lit.sum() < w*h - 20 and np.all(end[~lit] == rf.END_MISS) and np.all(spec == 1)
    assert np.all(alb == 1.0)
    nrm = walk(s, cam, st, w, h, NORMAL)[0]
    k = int(np.argmax(d[:, 2]))                          # the sample nearest the axis: the sphere's point facing +z
    assert lit[k] and np.max(np.abs(nrm[k] - (0.5, 0.5, 1.0))) <= 5e-2 and abs(T[k] - (2.0 + 2.0 + 2.5)) <= 2e-2
    assert np.array_equal(nrm[~lit], np.broadcast_to(np.array(A, F), ((~lit).sum(), 3)))


def test_misses_are_the_sky_of_the_last_direction(rt):
    w, h = 16, 12
    s = rt.Scene()
    mirror = s.add_material(0, (0.9, 0.9, 0.9), 0.0, 0.0, 1.5, 1.0, 0.0)
    s.add_plane(mirror, (0.0, 0.0, -1.0), -2.0)
    two_sided_sky(s)
    s.create_scene_bvh()
    for at, sky, bounces in (((0.0, 0.0, 5.0), A, 1), ((0.0, 0.0, -5.0), A, 0)):
        cam, st = pinhole(rt, w, h, at=at)
        for feature in (NORMAL, DISTANCE, ALBEDO):
            out, end, spec, T, stats, o, d = walk(s, cam, st, w, h, feature)
            assert np.all(end == rf.END_MISS) and np.all(spec == bounces)
            want = (1.0, 1.0, 1.0) if feature == ALBEDO else sky
            assert np.array_equal(out, np.broadcast_to(np.array(want, F), out.shape)), (at, feature)
            assert stats.closest_hit_rays == (1 + bounces)*w*h
    # towards the mirror with no bounce to follow: the mirror itself, not the sky (B is what a ray along +z would see)
    cam, st = pinhole(rt, w, h, bounces=1)
    out, end, spec, T, stats, o, d = walk(s, cam, st, w, h, NORMAL)
    assert np.all(end == rf.END_BOUND) and np.all(spec == 0) and np.all(out == np.array((0.5, 0.5, 0.0), F))


@pytest.mark.parametrize("metallic", [1.0, 0.9])
def test_facing_mirrors_reach_the_bound(rt, metallic):
    """tests/recursive_cases.py's two facing mirrors at max_bounce_count 63.  As perfect mirrors every walk takes
    63 hits and ends at the bound: ALBEDO 1, DISTANCE 0, 62 bounces followed.  As the case has them (metallic
    0.9) a walk may take the diffuse branch on the way: then ALBEDO is that mirror's albedo."""
    w, h = 9, 7
    s, cam, st, fc = mirrors_scene(rt, w, h)
    albedos = [np.array((0.99, 0.98, 0.97), F), np.array((0.97, 0.99, 0.98), F)]
    if metallic == 1.0:
        s = rt.Scene()
        for k, (n, alb) in enumerate(zip(((0.0, 0.0, -1.0), (0.0, 0.0, 1.0)), albedos)):
            s.add_plane(s.add_material(0, tuple(float(x) for x in alb), 0.0, 0.0, 1.5, 1.0, 0.0), n, -5.0)
        s.set_sky((0.5, 0.6, 0.7), (0.2, 0.2, 0.2))
        s.create_scene_bvh()
    assert st.max_bounce_count == 63
    st = with_settings(st, samples_per_pixel=8)
    xy, so = all_samples(w, h, 8)
    alb, end, spec, T, stats = rf.trace_samples(s.desc(), cam, st, w, h, xy, so, ALBEDO)
    dist = rf.trace_samples(s.desc(), cam, st, w, h, xy, so, DISTANCE)[0]
    bound = end == rf.END_BOUND
    assert np.all(spec[bound] == 62) and np.all(alb[bound, :3] == 1.0) and np.all(dist[bound, :3] == 0.0)
    assert stats.closest_hit_rays == len(xy) + spec.sum()
    if metallic == 1.0:
        assert bound.all() and np.all(T > 62*10.0)
    else:
        diffuse = end == rf.END_DIFFUSE
        assert np.all(bound | diffuse) and diffuse.sum() > 0.9*len(xy)
        # hit k + 1 is on the mirror at z = 5 for even k
        want = np.where((spec[diffuse] % 2 == 0)[:, None], albedos[0], albedos[1])
        assert np.array_equal(alb[diffuse, :3], want)
    # the frame driver counts the same bounces
    frame, fstats, fspec = rf.render(s.desc(), cam, st, fc, w, h, ALBEDO)
    assert fspec == spec.sum() and fstats.closest_hit_rays - fstats.samples == fspec


# ---- 3. the anchor

@pytest.mark.parametrize("name", ["c1", "c3", "c4"])
def test_anchor_to_the_first_hit_integrators(rt, name):
    w, h = 48, 32
    scene, cam, st, fc, post = rt.load_preset(name, w, h)
    for bounces in (1, 0):
        st = with_settings(st, samples_per_pixel=2, max_bounce_count=bounces)
        for feature, integ in ((NORMAL, NORMALS), (DISTANCE, DISTANCES)):
            a, sa, spec = rf.render(scene.desc(), cam, st, fc, w, h, feature, total_frame_index=2)
            b, sb = rb.render(scene.desc(), cam, with_settings(st, integrator=integ), fc, w, h, total_frame_index=2)
            assert np.array_equal(bits(a), bits(b)), (name, bounces, feature)
            assert sa.closest_hit_rays == sb.closest_hit_rays == sa.samples == 2*w*h and spec == 0
    # with more bounces every preset follows some: the rays past the camera's are the specular bounces
    st = with_settings(st, max_bounce_count=8)
    a, sa, spec = rf.render(scene.desc(), cam, st, fc, w, h, DISTANCE, total_frame_index=2)
    assert spec > 0 and sa.closest_hit_rays - sa.samples == spec


# ---- 4. the prefix identity

def test_the_walk_is_the_advanced_integrators_prefix(rt):
    """Black diffuse surfaces, a black sky, emitters, mirrors (albedo > 0) and glass, NEE off: an Advanced sample
    carries radiance exactly when its specular prefix ends on an emitter, which is when the walk with the same
    key ends there."""
    w, h, spp = 40, 30, 4
    s = rt.Scene()
    black = s.add_diffuse_material((0.0, 0.0, 0.0), 1.5)
    rough = s.add_material(0, (0.8, 0.7, 0.9), 0.0, 0.0, 1.5, 1.0, 0.3)      # fully metallic: no diffuse branch
    mirror = s.add_material(0, (0.9, 0.9, 0.9), 0.0, 0.0, 1.5, 1.0, 0.0)
    glass = s.add_translucent_material((0.1, 0.2, 0.3), 1.5)
    lamp = s.add_emissive_material((6.0, 5.0, 4.0))
    s.add_plane(black, (0.0, 1.0, 0.0), 0.0)
    s.add_sphere(rough, 1.5, rt.translate((-2.5, 1.5, 0.5)))
    s.add_sphere(glass, 1.2, rt.translate((1.0, 1.2, -1.5)))
    s.add_box(mirror, (0.2, 2.0, 2.0), rt.translate((4.0, 2.0, 1.0)) * rt.rotate_y(0.5))
    s.add_sphere(lamp, 1.0, rt.translate((0.5, 4.5, 0.0)))
    s.add_sphere(lamp, 0.5, rt.translate((1.0, 1.0, 3.0)))
    s.set_sky((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 3.0, -9.0), (0.0, 1.5, 0.0), 45.0)
    st = an.settings(rt, spp=spp, bounces=8)
    st = with_settings(st, next_event_estimation=0, russian_roulette=0)
    xy, so = all_samples(w, h, spp)
    adv, _ = ob.trace_samples(s.desc(), cam, st, w, h, xy, so, total_frame_index=4)
    out, end, spec, T, stats = rf.trace_samples(s.desc(), cam, st, w, h, xy, so, ALBEDO, total_frame_index=4)
    lit = np.any(adv[:, :3] != 0.0, axis=1)
    on_emitter = end == rf.END_EMITTER
    assert np.array_equal(lit, on_emitter)
    after_bounce_0 = on_emitter & (spec > 0)             # seen in the mirror, the metal or through the glass
    assert after_bounce_0.sum() > 10 and (on_emitter & (spec == 0)).sum() > 50
    assert np.array_equal(adv[:, 3:], out[:, 3:])        # the same camera sample


# ---- 5. the filter

def _frames(w, h, seed, invalid_fraction=0.02):
    beauty, g0, g1 = rd.random_frames(w, h, seed, invalid_fraction)
    return beauty, g0, g1, rf.random_albedo(w, h, seed, invalid_fraction)


def test_nothing_new_switched_on_is_ref_denoise(rt):
    for w, h, seed in ((1, 1, 1), (5, 3, 2), (37, 21, 3)):
        beauty, g0, g1, albedo = _frames(w, h, seed)
        for iterations in (1, 3, 5):
            p = rf.params(iterations, 1.0, (0.1, 0.05), 10.0)
            want = rd.denoise(beauty, g0, g1, p.base)
            assert np.array_equal(bits(rf.denoise(beauty, g0, g1, None, p)), bits(want))
        # the albedo present, its term and the demodulation off: it only decides validity
        got = rf.denoise(beauty, g0, g1, albedo, p)
        if w*h > 100:
            assert not np.array_equal(bits(got), bits(want))
            with np.errstate(all="ignore"):
                bad = ~(np.isfinite(albedo).all(axis=2) & (albedo[..., 3] > 0.001) &
                        np.isfinite(albedo[..., :3]/albedo[..., 3:]).all(axis=2))
            assert bad.sum() > 3 and np.array_equal(bits(got[bad]), bits(beauty[bad]))


def test_a_constant_image_stays_constant(rt):
    """Every term on.  Without demodulation a constant image; with it, a constant irradiance under the albedo
    (floored as the filter floors it), which is constant once demodulated."""
    w, h = 23, 17
    _, g0, g1, albedo = _frames(w, h, 5, invalid_fraction=0.0)
    for demodulate in (0, 1):
        beauty = np.zeros((h, w, 4), F)
        beauty[..., 3] = 2.0
        a = np.maximum(albedo[..., :3]/albedo[..., 3:], F(0.05)) if demodulate else F(1.0)
        beauty[..., :3] = F(0.7)*a*F(2.0)
        p = rf.params(4, 1.0, (0.1, 0.05), 10.0, 0.1, demodulate, 0.05)
        out = rf.denoise(beauty, g0, g1, albedo, p)
        want = beauty[..., :3]/beauty[..., 3:]
        assert np.all(out[..., 3] == 1.0)
        assert np.max(np.abs(out[..., :3] - want)/want) <= 1e-6


def test_invalid_pixels_pass_through_and_reach_no_neighbour(rt):
    w, h = 21, 15
    beauty, g0, g1, albedo = _frames(w, h, 7, invalid_fraction=0.0)
    p = rf.params(3, 1.0, (0.1, 0.05), 10.0, 0.1, 1, 0.05)
    a = albedo.copy()
    spots = {"w0": (4, 5), "nan": (9, 12), "neg": (2, 17), "overflow": (12, 3)}
    a[spots["w0"]] = (0.5, 0.5, 0.5, 0.0005)
    a[spots["nan"]] = (np.nan, 0.5, 0.5, 1.0)
    a[spots["neg"]] = (0.5, 0.5, 0.5, -1.0)
    a[spots["overflow"]] = (3e38, 1.0, 1.0, 0.5)
    out = rf.denoise(beauty, g0, g1, a, p)
    for yx in spots.values():
        assert np.array_equal(bits(out[yx]), bits(beauty[yx])), yx
    # other invalid values in the same spots: every other pixel keeps its bits
    a2, b2 = a.copy(), beauty.copy()
    a2[spots["w0"]] = (0.0, 0.0, 0.0, -np.inf)
    a2[spots["nan"]] = (np.inf, np.nan, 1.0, 2.0)
    b2[spots["neg"]] = (123.0, 4.0, 5.0, 1.0)
    out2 = rf.denoise(b2, g0, g1, a2, p)
    mask = np.ones((h, w), bool)
    for yx in spots.values():
        mask[yx] = False
        assert np.array_equal(bits(out2[yx]), bits(b2[yx])), yx
    assert np.array_equal(bits(out[mask]), bits(out2[mask]))
    assert np.all(out[mask][:, 3] == 1.0) and np.all(np.isfinite(out[mask]))


def test_demodulation_keeps_a_texture_edge(rt):
    """beauty = a two-valued checker albedo times a constant irradiance, every edge term off, 3 iterations.
    Demodulated, the image is constant to an ulp and the B3 kernel leaves it alone: the output is the input
    within 1e-6 relative.  Without demodulation the blur crosses the checker edges: relative L2 above 1e-2."""
    w, h = 40, 28
    yy, xx = np.mgrid[0:h, 0:w]
    ch = (((xx // 5) ^ (yy // 4)) & 1).astype(bool)
    alb = np.where(ch[..., None], np.array((0.8, 0.6, 0.3), F), np.array((0.15, 0.25, 0.5), F)).astype(F)
    irradiance = np.array((1.5, 1.25, 0.75), F)
    wt = F(4.0)
    beauty = np.concatenate([alb*irradiance*wt, np.full((h, w, 1), wt, F)], axis=2).astype(F)
    albedo = np.concatenate([alb*wt, np.full((h, w, 1), wt, F)], axis=2).astype(F)
    want = (beauty[..., :3]/beauty[..., 3:]).astype(np.float64)
    on = rf.denoise(beauty, None, None, albedo, rf.params(3, 0.0, (0.0, 0.0), 10.0, 0.0, 1, 0.05))
    off = rf.denoise(beauty, None, None, albedo, rf.params(3, 0.0, (0.0, 0.0), 10.0, 0.0, 0, 0.0))
    assert np.all(on[..., 3] == 1.0) and np.all(off[..., 3] == 1.0)
    rel = np.abs(on[..., :3] - want)/want
    l2 = np.linalg.norm(off[..., :3] - want)/np.linalg.norm(want)
    print(f"demodulated: max rel {rel.max():.3e}; not demodulated: rel L2 {l2:.3e}")
    assert rel.max() <= 1e-6
    assert l2 > 1e-2


def test_an_albedo_below_the_floor_is_divided_by_the_floor(rt):
    w, h = 9, 7
    beauty = np.ones((h, w, 4), F)
    beauty[..., :3] = F(0.02)
    albedo = np.ones((h, w, 4), F)
    albedo[..., :3] = (0.0, 0.01, 0.5)
    out = rf.denoise(beauty, None, None, albedo, rf.params(2, 0.0, (0.0, 0.0), 0.0, 0.0, 1, 0.1))
    assert np.all(np.isfinite(out)) and np.max(np.abs(out[..., :3] - F(0.02))) <= 1e-8


# ---- 6. the entries that need no device

def test_defaults_and_workspace_need_no_device(rt):
    p = rt.abi.DenoiseFeaturesParams()
    assert C.sizeof(p) == 32 + 32
    assert rt.lib().rt_denoise_features_default_params(C.byref(p)) == 0
    base = rt.default_denoise_params()
    assert bytes(p.base) == bytes(base)                  # the existing four base values are kept
    assert p.sigma_albedo >= 0 and p.demodulate in (0, 1) and (not p.demodulate or 0 < p.albedo_floor < 1)
    assert list(p.reserved) == [0]*5
    assert bytes(rt.default_denoise_features_params()) == bytes(p)
    assert rt.lib().rt_denoise_features_default_params(None) == rt.abi.RT_ERROR_INVALID
    assert rt.lib().rt_denoise_features_workspace_bytes(1920, 1080) == 80*1920*1080
    assert rt.denoise_features_workspace_bytes(65535, 65535) == 80*65535*65535
    assert rt.lib().rt_abi_version() == 8
    a = rt.abi
    assert (a.RT_FEATURE_NORMAL, a.RT_FEATURE_DISTANCE, a.RT_FEATURE_ALBEDO, a.RT_FEATURE_COUNT) == (0, 1, 2, 3)
    assert a.RT_INTEGRATOR_COUNT == 6 and rt.integrator_name(6) is None


def test_host_entry_needs_a_device_after_its_checks(rt):
    px = np.ones((4, 4, 4), F)
    if rt.device_count() > 0:
        assert rt.denoise_features(px, px, px, px).shape == (4, 4, 4)
    else:
        with pytest.raises(rt.RenderError) as e:
            rt.denoise_features(px, px, px, px)
        assert e.value.code == rt.abi.RT_ERROR_NO_DEVICE
    # a bad argument is refused first, with or without one
    p = rt.default_denoise_features_params()
    p.demodulate, p.albedo_floor = 1, 0.0
    with pytest.raises(rt.RenderError) as e:
        rt.denoise_features(px, px, px, px, params=p)
    assert e.value.code == rt.abi.RT_ERROR_INVALID and "albedo_floor" in str(e.value)


def _call_device(rt, p, beauty=1, normal=1, distance=1, albedo=1, w=4, h=4, out=1):
    v = lambda x: C.c_void_p(x or None)
    return rt.lib().rt_denoise_features_device(0, v(beauty), v(normal), v(distance), v(albedo), w, h,
                                               C.byref(p) if p is not None else None, None, v(out), None)


def _call_host(rt, p, beauty=1, normal=1, distance=1, albedo=1, w=4, h=4, out=1):
    fp = C.POINTER(C.c_float)
    px = np.ones((4, 4, 4), F)
    res = np.zeros((4, 4, 4), F)
    buf = rt.abi.AccumulationBuffer(w, h, 0, px.ctypes.data_as(fp))
    f = lambda on: px.ctypes.data_as(fp) if on else None
    return rt.lib().rt_denoise_features(0, C.byref(buf) if beauty else None, f(normal), f(distance), f(albedo),
                                        C.byref(p) if p is not None else None, res.ctypes.data_as(fp) if out else None)


BAD = [("d_beauty|beauty", dict(beauty=0), None), ("d_out|out_pixels", dict(out=0), None),
       ("rt_denoise_features_params", dict(), "null"), ("w", dict(w=0), None), ("h", dict(h=0), None),
       ("iterations", dict(), ("base.iterations", 0)), ("iterations", dict(), ("base.iterations", 9)),
       ("sigma_color", dict(), ("base.sigma_color", math.nan)),
       ("sigma_guide[0]", dict(), ("sigma_guide0", -0.5)), ("sigma_guide[1]", dict(), ("sigma_guide1", math.inf)),
       ("firefly_clamp", dict(), ("base.firefly_clamp", -1.0)),
       ("sigma_guide[0]", dict(normal=0), None), ("sigma_guide[1]", dict(distance=0), None),
       ("sigma_albedo", dict(), ("sigma_albedo", -1.0)), ("sigma_albedo", dict(), ("sigma_albedo", math.nan)),
       ("sigma_albedo", dict(), ("sigma_albedo", math.inf)),
       ("demodulate", dict(), ("demodulate", 2)), ("demodulate", dict(), ("demodulate", -1)),
       ("albedo_floor", dict(), ("albedo_floor", 0.0)), ("albedo_floor", dict(), ("albedo_floor", -0.1)),
       ("albedo_floor", dict(), ("albedo_floor", math.nan)), ("albedo_floor", dict(), ("albedo_floor", math.inf)),
       ("sigma_albedo", dict(albedo=0), ("demodulate", 0)), ("demodulate", dict(albedo=0), ("sigma_albedo", 0.0))]


@pytest.mark.parametrize("case", range(len(BAD)))
@pytest.mark.parametrize("entry", ["device", "host"])
def test_bad_arguments_are_refused_by_name(rt, entry, case):
    """Every bad argument is RT_ERROR_INVALID with the field named, before any device is touched (the device
    pointers here are never dereferenced)."""
    names, kw, field = BAD[case]
    p = rf.params(3, 1.0, (0.1, 0.05), 10.0, 0.1, 1, 0.05)
    if field == "null":
        p = None
    elif field is not None:
        k, v = field
        if k.startswith("sigma_guide"):
            p.base.sigma_guide[int(k[-1])] = v
        elif k.startswith("base."):
            setattr(p.base, k[5:], v)
        else:
            setattr(p, k, v)
    err = (_call_device if entry == "device" else _call_host)(rt, p, **kw)
    assert err == rt.abi.RT_ERROR_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert re.search(r"(?<![\w\[])(" + "|".join(re.escape(n) for n in names.split("|")) + r")(?![\w\[])", msg), msg
    # the checker refuses the same parameters
    if p is not None and not set(kw) & {"beauty", "out", "w", "h"}:
        px = np.ones((4, 4, 4), F)
        frames = [None if kw.get(k, 1) == 0 else px for k in ("normal", "distance", "albedo")]
        rf.denoise(px, *frames, p, expect=rt.abi.RT_ERROR_INVALID)


def test_render_entries_check_their_arguments(rt):
    st = rt.abi.Settings()
    post = rt.abi.PostSettings()
    out = np.zeros((4, 4), np.uint32)
    u32 = C.POINTER(C.c_uint32)
    lib = rt.lib()
    for feature in (-1, 3, 100):
        assert lib.rt_render_feature_device(None, None, C.byref(st), None, None, 0, 4, 4, 0, feature, None, None,
                                            None) == rt.abi.RT_ERROR_INVALID
        assert "feature" in lib.rt_last_error().decode() and str(feature) in lib.rt_last_error().decode()
        assert lib.rt_render_feature(None, None, C.byref(st), None, None, 0, feature, None, None) == rt.abi.RT_ERROR_INVALID
        assert "feature" in lib.rt_last_error().decode()
    assert lib.rt_render_feature_device(None, None, C.byref(st), None, None, 0, 4, 4, 0, 0, None, None,
                                        None) == rt.abi.RT_ERROR_INVALID
    p = rt.default_denoise_features_params()
    p.demodulate = 3
    err = lib.rt_render_picture_features_denoised(None, None, C.byref(st), None, None, 0, 4, 4, C.byref(post), C.byref(p),
                                                  0, out.ctypes.data_as(u32), None)
    assert err == rt.abi.RT_ERROR_INVALID and "scene" in lib.rt_last_error().decode()
    for kw, word in ((dict(st=None), "settings"), (dict(post=None), "post"), (dict(out=None), "out_bgra"),
                     (dict(w=0), "w is 0"), (dict(h=0), "h is 0"), (dict(), "demodulate")):
        a = dict(st=C.byref(st), post=C.byref(post), out=out.ctypes.data_as(u32), w=4, h=4)
        a.update(kw)
        err = lib.rt_render_picture_features_denoised(C.c_void_p(1), None, a["st"], None, None, 0, a["w"], a["h"], a["post"],
                                                      C.byref(p), 0, a["out"], None)
        assert err == rt.abi.RT_ERROR_INVALID and word in lib.rt_last_error().decode(), word


# ---- 7. usefulness: the new defaults on the oracle's own noisy frames

def _tonemapped_rel_l2(a, ref):
    def tm(x):
        c = np.maximum(x[:, :, :3].astype(np.float64) / x[:, :, 3:].astype(np.float64), 0.0)
        return 1.0 - np.exp(-c)
    return float(np.linalg.norm(tm(a) - tm(ref)) / np.linalg.norm(tm(ref)))


GUIDE_SPP = 16           # the feature frames' samples per pixel in the usefulness test (the sweep)


@pytest.mark.parametrize("name,w,h,strict", [("c1", 128, 128, True), ("c3", 160, 90, True), ("c4", 160, 90, False)])
def test_feature_defaults_reduce_the_error(rt, name, w, h, strict):
    """The recipe of test_default_parameters_reduce_the_error (4 spp beauty, a 512 spp oracle frame of another
    total_frame_index as the reference), three figures in one run: the noisy frame's tonemapped rel L2, the
    error with first-hit guides and the existing defaults, the error with feature frames and the new defaults.
    Gates: below the noisy error on C1 and C3, not above it on C4.  Measured (DESIGN.md has the table):
    C1 0.283 / 0.132 / 0.131, C3 0.369 / 0.189 / 0.181, C4 0.310 / 0.288 / 0.278: C4's ratio goes from 0.93 to
    0.90, which is no real improvement (not a gate)."""
    scene, cam, st, fc, post = rt.load_preset(name, w, h)
    st.samples_per_pixel = 4
    noisy, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=16, total_frame_index=0)
    first = [rb.render(scene.desc(), cam, with_settings(st, integrator=i), fc, w, h, total_frame_index=0)[0]
             for i in (NORMALS, DISTANCES)]
    gst = with_settings(st, samples_per_pixel=GUIDE_SPP)
    feats = [rf.render(scene.desc(), cam, gst, fc, w, h, f, total_frame_index=0)[0] for f in (NORMAL, DISTANCE, ALBEDO)]
    st.samples_per_pixel = 512
    ref, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=16, total_frame_index=7)
    e_noisy = _tonemapped_rel_l2(noisy, ref)
    e_first = _tonemapped_rel_l2(rd.denoise(noisy, first[0], first[1], rt.default_denoise_params()), ref)
    e_feat = _tonemapped_rel_l2(rf.denoise(noisy, *feats, rt.default_denoise_features_params()), ref)
    print(f"{name}: noisy {e_noisy:.4f} first-hit {e_first:.4f} ({e_first/e_noisy:.3f}) "
          f"features {e_feat:.4f} ({e_feat/e_noisy:.3f})")
    if strict:
        assert e_feat < e_noisy
    else:
        assert e_feat <= e_noisy
