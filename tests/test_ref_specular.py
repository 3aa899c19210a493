"""The specular G-buffer on the CPU ("A specular G-buffer"): the plain-C checker tests/ref_specular held to
what the definition promises on scenes with known chains, the ghost test's conditions on the checker and
tests/ref_temporal's accumulate stage, and the product library's refusals.  No device is needed.
"""
import ctypes as C

import numpy as np
import pytest

import random_scenes
import ref_specular_binding as sb
import ref_temporal_binding as tb

W, H = sb.W, sb.H
CY, CX = H//2 - 3, W//2                  # a pixel a little above the frame's centre
EYE = np.eye(3, dtype=np.float32)


def last_error(rt):
    return rt.lib().rt_last_error().decode()


def cam_p(cam):
    return np.array([cam.p.x, cam.p.y, cam.p.z], np.float64)


# ---- max_events = 0 is the primary-hit G-buffer

@pytest.mark.parametrize("name", ["c1", "random"])
def test_no_events_is_the_primary_hit_gbuffer(rt, name):
    if name == "c1":
        scene, cam, st, fc, post = rt.load_preset("c1", 48, 27)
    else:
        scene, cam, st, fc = random_scenes.random_scene(rt, 5, 48, 27, mesh_instances=6)
    for amount in (0.0, 2.0):
        g, c, wk = sb.gbuffer_specular(scene.desc(), cam, amount, 48, 27, sb.params(max_events=0))
        want = tb.gbuffer(scene.desc(), cam, amount, 48, 27)
        assert sb.mismatches(g, want) == 0
        assert (c["chain"] == 0).all()
        assert np.array_equal(c["first_primitive"], want["primitive"])
        assert np.array_equal(tb.bits(c["first_t"]), tb.bits(want["t"]))
        assert np.isin(c["end"], (sb.END_MISS, sb.END_EMITTER, sb.END_DIFFUSE, sb.END_ROUGH, sb.END_STACK, sb.END_CAP)).all()
        assert ((c["end"] == sb.END_MISS) == (want["primitive"] == sb.MISS)).all()


# ---- a planar mirror: the unfolded point is the mirror image of the surface seen

@pytest.mark.parametrize("normal", [sb.MIRROR_N, sb.TILTED_N], ids=["floor", "tilted"])
def test_planar_mirror_texel_is_the_householder_image(rt, normal):
    """Every texel of one reflection and a final hit, against the float64 image, under the ideal mirror (the plane's
    normal normalised in float64), of the final hit point F and normal the checker's walk ended on.

    The bound on p, in units of u = 2^-23 (|camera.p|_inf + T), from the operations between the two (r = 2^-24 = u/2
    relative per rounding; t1, t2 the two rays' lengths, t1 + t2 <= T):
      * the first vertex I1 = cp + t1 D: two roundings, and t1 itself three (the plane's quotient): I1 lies off the
        mirror by at most 5r (|cp| + t1).  The image flips that offset and the unfolding does not: 2 x 5r = 5 u;
      * the reflected direction: the f32 normal is 2r off the ideal one per component, which the reflection doubles
        (4r), and reflect() rounds three times a component (3r): 7r along t2 = 3.5 u;
      * the second origin I1 + EPSILON rd and F = O2 + t2 rd: two roundings each, 4r = 2 u;
      * T = (t1 + EPSILON) + t2, T D and cp + T D: four roundings, 2 u.
    t2's own error moves F and T alike and cancels.  12.5 u; the bound is 16 u.  Measured: 1.67 u (tilted), 0.88 u (floor).

    The bound on n, in units of 2^-23: H's entries carry the normal's 2r twice and two roundings (6r), the row sums
    of M N three terms of them and three roundings: (3 x 6 + 3) r = 10.5 u; the bound is 12.  Measured: 0.75 (tilted), 0
    (floor: every product is with 0 or 1)."""
    scene, cam = sb.mirror_scene(rt, normal=normal)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H)
    m = (c["chain"] == sb.ONE_REFLECTION) & (g["primitive"] != sb.MISS)
    assert m.sum() > 1000
    assert (c["end"][m] == sb.END_DIFFUSE).all() and (c["first_primitive"][m] == (sb.PLANE_BIT | 0)).all()
    n64 = np.array(normal, np.float64)
    n64 /= np.linalg.norm(n64)
    house = np.eye(3) - 2.0*np.outer(n64, n64)
    image = wk["final_p"][m].astype(np.float64) @ house.T
    unit = 2.0**-23*(np.abs(cam_p(cam)).max() + g["t"][m].astype(np.float64))
    err = (np.abs(g["p"][m].astype(np.float64) - image).max(axis=1)/unit).max()
    nerr = np.abs(g["n"][m].astype(np.float64) - wk["final_n"][m].astype(np.float64) @ house.T).max()/2.0**-23
    print(f"mirror {normal}: {int(m.sum())} texels, p within {err:.2f} u (bound 16), n within {nerr:.2f} x 2^-23 (bound 12)")
    assert err <= 16.0
    assert nerr <= 12.0
    # t is the path length, and the unfolded point lies that far along the camera ray
    assert np.array_equal(tb.bits(g["t"][m]), tb.bits(wk["T"][m]))
    assert (g["t"][m] > c["first_t"][m]).all()
    d = tb.gbuffer_rays(cam, 0.0, W, H)[m].astype(np.float64)
    assert np.abs(g["p"][m] - (cam_p(cam) + g["t"][m][:, None].astype(np.float64)*d)).max() <= 2.0**-22*12.0


# ---- two mirrors: the cap

@pytest.mark.parametrize("cap", [0, 1, 2, 5, 16])
def test_two_mirrors_end_at_the_cap(rt, cap):
    scene, cam = sb.two_mirrors(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(max_events=cap))
    assert (sb.events(c) == cap).all()
    assert (sb.reflect_bits(c) == (1 << cap) - 1).all()
    assert (c["end"] == sb.END_CAP).all()
    assert (wk["level"] == 0).all()
    # the planes alternate, starting with the one the camera looks at
    first = c["first_primitive"]
    other = np.where(first == (sb.PLANE_BIT | 0), sb.PLANE_BIT | 1, sb.PLANE_BIT | 0).astype(np.uint32)
    assert np.array_equal(g["primitive"], first if cap % 2 == 0 else other)
    # two reflections in parallel mirrors are a translation: M is the identity again, the normal the first one's
    if cap % 2 == 0:
        assert np.array_equal(wk["M"], np.broadcast_to(EYE, wk["M"].shape))
    if cap == 0:
        assert sb.mismatches(g, tb.gbuffer(scene.desc(), cam, 0.0, W, H)) == 0


# ---- refraction: the stack

def test_glass_slab_is_two_refractions(rt):
    scene, cam = sb.glass_slab(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H)
    through = c["chain"] == 2                                   # two events, no reflection
    assert through[CY, CX] and through.sum() > 500
    assert (c["first_primitive"][through] == 1).all()           # the box, added after the wall
    assert (g["primitive"][through] == (sb.PLANE_BIT | 0)).all() and (c["end"][through] == sb.END_DIFFUSE).all()
    assert (wk["level"][through] == 0).all() and (wk["max_level"][through] == 1).all()
    assert np.array_equal(wk["M"][through], np.broadcast_to(EYE, wk["M"][through].shape))
    # no reflection: the normal is the wall's own, and the path is longer than the straight line to the wall by little
    assert np.array_equal(g["n"][through], wk["final_n"][through])
    straight = tb.gbuffer(scene.desc(), cam, 0.0, W, H)["t"]
    assert (g["t"][through] > straight[through]).all() and (g["t"][through] < 8.0/np.cos(np.radians(40.0)) + 0.5).all()


def test_nested_glass_reaches_level_three_and_returns(rt):
    scene, cam = sb.nested_glass(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H)
    assert c["chain"][CY, CX] == 6                              # in, in, in, out, out, out
    core = c["chain"] == 6
    assert core.sum() > 200
    assert (wk["max_level"][core] == 3).all() and (wk["level"][core] == 0).all()
    assert (c["end"][core] == sb.END_DIFFUSE).all() and (g["primitive"][core] == (sb.PLANE_BIT | 0)).all()
    assert np.array_equal(wk["M"][core], np.broadcast_to(EYE, wk["M"][core].shape))


def test_nine_nested_spheres_end_at_the_stack(rt):
    scene, cam = sb.nine_spheres(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(max_events=16))
    assert c["end"][CY, CX] == sb.END_STACK
    full = c["end"] == sb.END_STACK
    assert full.sum() > 200
    assert (c["chain"][full] == 7).all()                        # seven refractions; the eighth entry is refused
    assert (wk["level"][full] == 7).all()
    assert (g["primitive"][full] == 8).all() and (c["first_primitive"][full] == 1).all()    # primitive 0 is reserved
    # rays that pass outside the eighth sphere without a reflection come out again
    out = (c["end"] == sb.END_MISS) & (sb.events(c) > 0) & (sb.reflect_bits(c) == 0)
    assert out.any() and (wk["level"][out] == 0).all() and (sb.events(c)[out] % 2 == 0).all()


def test_total_internal_reflection_reflects(rt):
    """From inside a block of glass (ior 1.5, critical angle 41.8 degrees) at 50.3 degrees to the face x = 1."""
    scene = sb.glass_block(rt)
    o = np.array([0.1, 0.05, 0.2])
    d = np.array([1.0, 1.2, 0.1])
    g, c, wk = sb.walk_ray(scene.desc(), o, d/np.linalg.norm(d), sb.params(max_events=1))
    assert int(c["chain"]) == sb.ONE_REFLECTION and int(c["end"]) == sb.END_CAP
    assert int(wk["level"]) == 0
    assert np.array_equal(wk["M"], np.diag([-1.0, 1.0, 1.0]).astype(np.float32))
    assert abs(float(c["first_t"]) - 0.9*np.linalg.norm(d)) < 1e-5
    # the second vertex is on the top face y = 3, reached by the mirrored direction from (1, 1.13, 0.29)
    s = (3.0 - 1.13)/1.2
    assert np.allclose(wk["final_p"], (1.0 - s, 3.0, 0.29 + 0.1*s), atol=2e-3)
    # below the critical angle the same face refracts, and the ray leaves the scene
    d = np.array([1.0, 0.5, 0.1])
    g, c, wk = sb.walk_ray(scene.desc(), o, d/np.linalg.norm(d), sb.params(max_events=1))
    assert int(c["chain"]) == 1 and int(c["end"]) == sb.END_MISS


def test_camera_inside_glass_sees_both_sides_of_the_critical_angle(rt):
    scene, cam = sb.inside_glass(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(max_events=1))
    assert (c["first_primitive"] == 1).all() and (c["end"] == sb.END_CAP).sum() > 300
    # the camera ray meets the block from inside: its normal faces along the ray
    d = tb.gbuffer_rays(cam, 0.0, W, H)
    first, _, _ = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(max_events=0))
    assert ((first["n"]*d).sum(axis=2) > 0).all()
    reflected = c["chain"] == sb.ONE_REFLECTION
    refracted = c["chain"] == 1
    assert reflected.sum() > 300 and refracted.sum() > 300 and (reflected | refracted).all()
    assert (c["end"][refracted] == sb.END_MISS).all() and (c["end"][reflected] == sb.END_CAP).all()
    # on the face x = 1 the two sides are split by the angle of incidence alone
    face = np.abs(first["n"][..., 0] - 1.0) < 1e-6
    cos_i = d[..., 0]/np.linalg.norm(d, axis=2)
    critical = np.sqrt(1.0 - (1.0/1.5)**2)
    assert (reflected[face] == (cos_i[face] < critical)).mean() > 0.97       # Fresnel passes 0.5 just inside the angle
    assert reflected[face & (cos_i < critical)].all()


# ---- the other ends

def test_rough_metal_ends_as_a_surface(rt):
    scene, cam = sb.rough_metal(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H)
    floor = c["first_primitive"] == (sb.PLANE_BIT | 0)
    assert floor.sum() > 1000
    assert (c["end"][floor] == sb.END_ROUGH).all() and (c["chain"][floor] == 0).all()
    assert sb.mismatches(g, tb.gbuffer(scene.desc(), cam, 0.0, W, H)) == 0
    # with the bar above its roughness the same floor is a mirror
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(roughness_max=0.5))
    assert (c["chain"][floor] == sb.ONE_REFLECTION).all()
    # and a threshold above 1 makes it no mirror at all: a metal that does not transmit is the diffuse branch
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H, sb.params(reflect_threshold=1.5))
    assert (c["end"][floor] == sb.END_DIFFUSE).all() and (c["chain"] == 0).all()


def test_miss_after_a_reflection(rt):
    scene, cam = sb.mirror_and_sky(rt)
    g, c, wk = sb.gbuffer_specular(scene.desc(), cam, 0.0, W, H)
    floor = c["first_primitive"] == (sb.PLANE_BIT | 0)
    assert floor.sum() > 1000 and (~floor).sum() > 500
    assert (c["chain"][floor] == sb.ONE_REFLECTION).all() and (c["chain"][~floor] == 0).all()
    assert (c["end"] == sb.END_MISS).all()
    assert (c["first_t"][floor] > 0).all() and (c["first_t"][~floor] == 0).all()
    d = tb.gbuffer_rays(cam, 0.0, W, H)
    assert np.array_equal(tb.bits(g["p"]), tb.bits(d))          # the primary direction, reflected or not
    assert (g["t"] == 0).all() and (g["n"] == 0).all() and (g["primitive"] == sb.MISS).all()


# ---- the ghost test's conditions, on the checker and tests/ref_temporal's accumulate stage

def test_ghost_conditions_hold_on_the_cpu(rt):
    inp = sb.ghost_inputs()
    scene, cams = inp["scene"], inp["cameras"]
    assert inp["mirror"].sum() > 1000 and inp["direct"].sum() > 1000
    accumulate = lambda cur, g, prev, pc: tb.accumulate(cur, g, prev, pc, 0.0, tb.params())
    plain = [tb.gbuffer(scene.desc(), cam, 0.0, sb.GW, sb.GH) for cam in cams]
    with_specular = sb.ghost_run(accumulate, inp["current"], inp["specular"], cams)
    with_plain = sb.ghost_run(accumulate, inp["current"], plain, cams)
    sb.ghost_assert(with_specular, with_plain, inp)


# ---- the product library's refusals, by name (no device: every one of them comes before the scene is looked at)

def test_defaults_and_workspace(rt):
    p = rt.default_gbuffer_specular_params()
    assert (p.max_events, p.reflect_threshold, p.roughness_max, p.reserved) == (8, 0.5, 0.25, 0)
    assert rt.lib().rt_gbuffer_specular_default_params(None) == rt.abi.RT_ERROR_INVALID and "null out" in last_error(rt)
    assert C.sizeof(rt.abi.SpecularTexel2) == 16 and C.sizeof(rt.abi.GBufferSpecularParams) == 16
    for w, h in ((1, 1), (7, 130), (1920, 1080)):
        base = rt.temporal_workspace_bytes(w, h)
        assert rt.temporal_specular_workspace_bytes(w, h) == ((base + 15) & ~15) + 32*w*h


def test_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    gp, cp_ = C.POINTER(rt.abi.GBufferTexel), C.POINTER(rt.abi.SpecularTexel2)
    g = np.zeros((h, w), tb.dtype())
    fake_scene = C.c_void_p(0)                        # the scene is checked last: nothing before it needs one
    nan, inf = float("nan"), float("inf")
    bad_params = [("max_events must be in 0..16", dict(max_events=17)),
                  ("reflect_threshold must be finite", dict(reflect_threshold=-0.1)),
                  ("reflect_threshold must be finite", dict(reflect_threshold=nan)),
                  ("reflect_threshold must be finite", dict(reflect_threshold=inf)),
                  ("roughness_max must be finite", dict(roughness_max=-1.0)),
                  ("roughness_max must be finite", dict(roughness_max=nan)),
                  ("roughness_max must be finite", dict(roughness_max=inf))]

    def gb(text, camera=C.byref(cam), w_=w, h_=h, o=g.ctypes.data_as(gp), p=sb.params()):
        code = lib.rt_gbuffer_specular(fake_scene, camera, 0.0, w_, h_, None if p is None else C.byref(p), o, None)
        assert code == rt.abi.RT_ERROR_INVALID, (text, code)
        assert last_error(rt).startswith("rt_gbuffer_specular:") and text in last_error(rt), (text, last_error(rt))
    gb("null camera", camera=None)
    gb("null out", o=None)
    gb("w is 0", w_=0)
    gb("h is 0", h_=0)
    gb("below 2^32", w_=70000, h_=70000)
    gb("null rt_gbuffer_specular_params", p=None)
    for text, change in bad_params:
        gb(text, p=sb.params(**change))
    gb("null scene")
    assert lib.rt_gbuffer_specular_device(fake_scene, C.byref(cam), 0.0, w, h, C.byref(sb.params()), None, None,
                                          None) == rt.abi.RT_ERROR_INVALID
    assert "rt_gbuffer_specular_device: null d_out" in last_error(rt)

    state = rt.abi.TemporalState()
    state.d_workspace = 1                             # never dereferenced: every call below is refused first
    out = np.zeros((h, w, 4), np.float32)
    fp = C.POINTER(C.c_float)
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    base = dict(camera=C.byref(cam), settings=C.byref(st), filter=C.byref(fc), tiles=C.byref(tiles), w=w, h=h,
                p=rt.default_temporal_params(), state=state, sp=sb.params(), cp=None, out=out.ctypes.data_as(fp))

    def drv(text, **change):
        a = dict(base, **change)
        ref = lambda x: None if x is None else C.byref(x)
        code = lib.rt_render_temporal_specular(fake_scene, a["camera"], a["settings"], a["filter"], a["tiles"], 0, a["w"],
                                               a["h"], 0, ref(a["p"]), ref(a["state"]), ref(a["sp"]), ref(a["cp"]), a["out"],
                                               None, None)
        assert code == rt.abi.RT_ERROR_INVALID, (text, code)
        assert last_error(rt).startswith("rt_render_temporal_specular:") and text in last_error(rt), (text, last_error(rt))
    drv("null rt_gbuffer_specular_params", sp=None)
    for text, change in bad_params:
        drv(text, sp=sb.params(**change))
    clip = rt.default_temporal_clip_params
    for text, field, value in (("radius must be in 1..3", "radius", 0), ("radius must be in 1..3", "radius", 4),
                               ("gamma must be finite", "gamma", -1.0), ("gamma must be finite", "gamma", nan),
                               ("min_count must be finite", "min_count", inf)):
        cp = clip()
        setattr(cp, field, value)
        drv(text, cp=cp)
    drv("null rt_temporal_params", p=None)
    drv("null rt_temporal_state", state=None)
    drv("null settings", settings=None)
    drv("w is 0", w=0)
    drv("null camera", camera=None)
    drv("null out_pixels", out=None)
    drv("null scene")
    drv("null scene", cp=clip())
    assert (state.frames, state.parity, state.w, state.h) == (0, 0, 0, 0) and not out.any()
