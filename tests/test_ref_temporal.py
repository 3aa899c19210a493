"""Temporal accumulation on the CPU ("Temporal accumulation"): the plain-C checker tests/ref_temporal held
to what the definition promises, and the product library's refusals.  No device is needed.

* the projection into the previous camera inverts the G-buffer's own ray, lens distortion included;
* a camera translated parallel to a plane shifts the picture by the closed form;
* the blend rules, on hand-made inputs;
* every refusal of the public entries, by name.
"""
import ctypes as C

import numpy as np
import pytest

import ref_temporal_binding as tb

F = np.float32
AMOUNTS = (-3.0, -0.5, 0.0, 1.0, 2.0, 6.0)        # the reference's slider runs from -3 to 6


def aimed_camera(rt, w, h):
    """C1's camera moved off its axis and aimed at a point beside the scene's centre."""
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    cam.p = rt.v3(cam.p.x + 0.7, cam.p.y + 0.4, cam.p.z - 0.3)
    rt.aim_camera_at(cam, (0.5, 0.8, -0.2))
    return cam


# ---- 1. the projection inverts the G-buffer's ray

@pytest.mark.parametrize("w,h,stride", [(65, 33, 1), (130, 70, 1), (5, 3, 1), (1920, 1080, 7)])
def test_projection_inverts_the_gbuffer_ray(rt, w, h, stride):
    cam = aimed_camera(rt, w, h)
    o = np.array([cam.p.x, cam.p.y, cam.p.z], np.float32)
    yy, xx = np.divmod(np.arange(w*h)[::stride], w)
    worst = 0.0
    for amount in AMOUNTS:
        d = tb.gbuffer_rays(cam, amount, w, h).reshape(-1, 3)[::stride]
        for dist in (0.5, 10.0, 1e4):
            P = (o + F(dist)*d).astype(np.float32)
            ok, fx, fy = tb.project_many(cam, amount, P, w, h)
            assert ok.all(), (amount, dist, int((~ok).sum()))
            err = float(np.maximum(np.abs(fx - xx), np.abs(fy - yy)).max())
            worst = max(worst, err)
            assert err <= 1.0/64.0, (amount, dist, err)
    print(f"round trip {w}x{h}: worst {worst:.3e} pixel")


def test_folded_distortion_is_finite_or_flagged(rt):
    """On a tall frame the forward distortion folds and has no inverse: whatever comes back is finite or no-history."""
    w, h, amount = 7, 130, 2.0
    cam = aimed_camera(rt, w, h)
    o = np.array([cam.p.x, cam.p.y, cam.p.z], np.float32)
    d = tb.gbuffer_rays(cam, amount, w, h).reshape(-1, 3)
    ok, fx, fy = tb.project_many(cam, amount, (o + F(10.0)*d).astype(np.float32), w, h)
    assert (np.isfinite(fx) & np.isfinite(fy))[ok].all()
    assert ((fx >= -1) & (fx < w) & (fy >= -1) & (fy < h))[ok].all()


# ---- hand-made G-buffers: one plane facing the camera

def plane_gbuffer(cam, w, h, depth, primitive=tb.PLANE_BIT | 0):
    """The G-buffer a camera without distortion sees of the plane `depth` in front of it, facing it."""
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    P = tb.point_at(cam, 0.0, w, h, x, y, np.full((h, w), depth))
    g = np.zeros((h, w), tb.dtype())
    g["p"] = P
    g["t"] = np.linalg.norm(P - np.array([cam.p.x, cam.p.y, cam.p.z]), axis=2)
    g["n"] = (cam.z.x, cam.z.y, cam.z.z)
    g["primitive"] = primitive
    return g


def pixel_shift(cam, w, d, depth):
    """The closed form: a translation by d parallel to a plane at `depth` moves the picture by this many pixels."""
    return d*cam.film_distance*w/(2.0*depth*cam.half_film_w)


def ramp_history(w, h):
    """A history whose red channel is the column and whose green channel the row."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return np.stack([x, y, np.full_like(x, 0.25), np.ones_like(x)], axis=2)


@pytest.mark.parametrize("shift", [3.0, 2.5])
def test_parallel_translation_shifts_by_the_closed_form(shift):
    w, h, depth = 24, 9, 4.0
    cam0 = tb.make_camera(p=(0.2, 0.1, 1.0), aspect=w/h)
    d = shift*2.0*depth*cam0.half_film_w/(cam0.film_distance*w)
    assert pixel_shift(cam0, w, d, depth) == pytest.approx(shift)
    cam1 = tb.moved(cam0, (d, 0.0, 0.0))
    g0, g1 = plane_gbuffer(cam0, w, h, depth), plane_gbuffer(cam1, w, h, depth)
    # where the checker puts every pixel of the new frame in the old one
    ok, fx, fy = tb.project_many(cam0, 0.0, g1["p"].reshape(-1, 3), w, h)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    want_fx = x.reshape(-1) - shift
    assert np.abs(fx - want_fx)[ok].max() < 1e-3 and np.abs(fy - y.reshape(-1))[ok].max() < 1e-3
    assert ok[want_fx >= 0].all() and not ok[want_fx < -1.01].any()        # between: a tap or two, or beyond the corner
    # and what the stage makes of it: a black current frame halves the shifted ramp
    cur = np.zeros((h, w, 4), np.float32)
    cur[..., 3] = 1.0
    hist, length = tb.accumulate(cur, g1, (ramp_history(w, h), np.ones((h, w), np.float32), g0), cam0, 0.0, tb.params())
    covered = x >= np.ceil(shift)                    # every tap inside the old frame
    assert (length[covered] == 2.0).all()
    assert np.abs(hist[..., 0][covered] - (x[covered] - shift)/2.0).max() < 1e-3
    assert np.abs(hist[..., 1][covered] - y[covered]/2.0).max() < 1e-3
    strip = x < np.floor(shift)                      # the uncovered strip: as wide as the shift
    assert (length[strip] == 1.0).all() and (hist[..., :3][strip] == 0.0).all()
    assert int(strip[0].sum()) == int(np.floor(shift))


# ---- 2. the blend rules

def current_frame(w, h, seed=5):
    rng = np.random.default_rng(seed)
    wt = rng.uniform(0.5, 3.0, (h, w, 1))
    return np.concatenate([rng.uniform(0.0, 2.0, (h, w, 3))*wt, wt], axis=2).astype(np.float32)


def resolved(cur, clamp=10.0):
    c = cur[..., :3]/cur[..., 3:]
    return np.minimum(np.maximum(c, F(0)), F(clamp)).astype(np.float32)


def test_first_frame_and_no_history_parameter():
    w, h = 6, 4
    cam = tb.make_camera(aspect=w/h)
    g = plane_gbuffer(cam, w, h, 5.0)
    cur = current_frame(w, h)
    cur[0, 0, :3] = 100.0*cur[0, 0, 3]               # a firefly: clamped to 10
    cur[0, 1, :3] = -1.0                             # negative radiance: clamped to 0
    want = np.concatenate([resolved(cur), np.ones((h, w, 1), np.float32)], axis=2)
    hist, length = tb.accumulate(cur, g, None, None, 0.0, tb.params())
    assert np.array_equal(tb.bits(hist), tb.bits(want)) and (length == 1.0).all()
    assert hist[0, 0, 0] == 10.0 and hist[0, 1, 0] == 0.0
    # max_history = 1 with a full history behind it: the clamped current frame, bit for bit
    prev = (ramp_history(w, h), np.full((h, w), 9.0, np.float32), g)
    hist1, length1 = tb.accumulate(cur, g, prev, cam, 0.0, tb.params(max_history=1.0))
    assert np.array_equal(tb.bits(hist1), tb.bits(want)) and (length1 == 1.0).all()
    # no clamp when 0
    hist0, _ = tb.accumulate(cur, g, None, None, 0.0, tb.params(firefly_clamp=0.0))
    assert hist0[0, 0, 0] == pytest.approx(100.0)


def test_standing_camera_takes_one_tap():
    """Snap: a standing camera reads its own pixel and nothing of the neighbours; the blend is the stated expression."""
    w, h = 7, 5
    cam = tb.make_camera(p=(0.3, 0.2, 2.0), aspect=w/h)
    g = plane_gbuffer(cam, w, h, 5.0)
    cur = current_frame(w, h)
    ph = ramp_history(w, h)
    ph[2, 3, :3] = 1e6                               # a neighbour's history that would show in any other pixel
    pl = np.full((h, w), 3.0, np.float32)
    hist, length = tb.accumulate(cur, g, (ph, pl, g), cam, 0.0, tb.params())
    c = resolved(cur)
    want = (ph[..., :3] + (c - ph[..., :3])*(F(1.0)/F(4.0))).astype(np.float32)
    assert np.array_equal(tb.bits(hist[..., :3]), tb.bits(want)) and (hist[..., 3] == 1.0).all()
    assert (length == 4.0).all()
    # the cap
    _, capped = tb.accumulate(cur, g, (ph, np.full((h, w), 32.0, np.float32), g), cam, 0.0, tb.params())
    assert (capped == 32.0).all()
    # without snap the same position takes four taps, three of weight 0 or nearly: still the own pixel's history
    hist4, length4 = tb.accumulate(cur, g, (ph, pl, g), cam, 0.0, tb.params(snap=0.0))
    far = np.ones((h, w), bool)
    far[1:4, 2:5] = False
    assert np.abs(hist4[..., :3][far] - want[far]).max() < 1e-3 and (np.abs(length4 - 4.0) < 1e-3).all()


def half_pixel_case(w=8, h=6, depth=5.0):
    """A camera moved by half a pixel in x and y: every inner pixel takes four taps of weight 1/4."""
    cam0 = tb.make_camera(p=(0.0, 0.0, 1.0), aspect=w/h)
    dx = 0.5*2.0*depth*cam0.half_film_w/(cam0.film_distance*w)
    dy = 0.5*2.0*depth*cam0.half_film_h/(cam0.film_distance*h)
    cam1 = tb.moved(cam0, (dx, dy, 0.0))
    return cam0, plane_gbuffer(cam0, w, h, depth), plane_gbuffer(cam1, w, h, depth)


def expect_mean(ph, pl, taps):
    hs = np.array([ph[y, x, :3] for x, y in taps], np.float64)
    return hs.mean(axis=0), float(np.mean([pl[y, x] for x, y in taps]))


@pytest.mark.parametrize("fault", ["none", "primitive", "normal", "plane", "length", "nan"])
def test_a_dropped_tap_renormalises_the_rest(fault):
    w, h = 8, 6
    cam0, g0, g1 = half_pixel_case(w, h)
    rng = np.random.default_rng(3)
    ph = np.concatenate([rng.uniform(0.0, 4.0, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(np.float32)
    pl = rng.integers(1, 9, (h, w)).astype(np.float32)
    cur = np.zeros((h, w, 4), np.float32)
    cur[..., 3] = 1.0
    px, py = 4, 3                                    # the pixel under test: taps (3..4, 2..3) of the old frame
    ok, fx, fy = tb.project(cam0, 0.0, g1["p"][py, px], w, h)
    assert ok and fx == pytest.approx(px - 0.5, abs=1e-3) and fy == pytest.approx(py - 0.5, abs=1e-3)
    taps = [(3, 2), (4, 2), (3, 3), (4, 3)]
    g0 = g0.copy()
    bx, by = taps[1]
    if fault == "primitive":
        g0["primitive"][by, bx] = 5
    elif fault == "normal":
        g0["n"][by, bx] = (0.8, 0.0, 0.6)            # cos 0.6 < 0.9
    elif fault == "plane":
        g0["p"][by, bx, 2] += 0.5                    # 0.5 off the plane; the limit is 0.02 * t of about 5
    elif fault == "length":
        pl[by, bx] = 0.0
    elif fault == "nan":
        ph[by, bx, 1] = np.nan
    kept = taps if fault == "none" else [t for t in taps if t != (bx, by)]
    hist, length = tb.accumulate(cur, g1, (ph, pl, g0), cam0, 0.0, tb.params(max_history=64.0))
    mean, L = expect_mean(ph, pl, kept)
    N = L + 1.0
    assert length[py, px] == pytest.approx(N, rel=1e-4)
    assert hist[py, px, :3] == pytest.approx(mean*(1.0 - 1.0/N), rel=1e-3)
    # a pixel that shares no tap with the faulty one is the four-tap mean
    mean2, L2 = expect_mean(ph, pl, [(0, 4), (1, 4), (0, 5), (1, 5)])
    assert length[5, 1] == pytest.approx(L2 + 1.0, rel=1e-4) and hist[5, 1, :3] == pytest.approx(mean2*(1.0 - 1.0/(L2 + 1.0)), rel=1e-3)


def test_taps_outside_the_image_and_all_taps_dropped():
    w, h = 8, 6
    cam0, g0, g1 = half_pixel_case(w, h)
    ph = ramp_history(w, h)
    pl = np.full((h, w), 2.0, np.float32)
    cur = current_frame(w, h)
    hist, length = tb.accumulate(cur, g1, (ph, pl, g0), cam0, 0.0, tb.params())
    # pixel (0, 3) sits at (-0.5, 2.5) of the old frame: the taps of column -1 are outside, the two of column 0 count
    c = resolved(cur)
    want = 2.5 + (c[3, 0, 1] - 2.5)/3.0
    assert length[3, 0] == 3.0 and hist[3, 0, 1] == pytest.approx(want, rel=1e-4)
    assert hist[3, 0, 0] == pytest.approx(c[3, 0, 0]/3.0, rel=1e-4)          # column 0 alone: red is 0
    # every tap of another primitive: no history at all
    other = g0.copy()
    other["primitive"] = 9
    hist2, length2 = tb.accumulate(cur, g1, (ph, pl, other), cam0, 0.0, tb.params())
    assert (length2 == 1.0).all() and np.array_equal(tb.bits(hist2[..., :3]), tb.bits(c))


def test_an_invalid_current_pixel_passes_through_and_is_no_tap():
    w, h = 6, 4
    cam = tb.make_camera(aspect=w/h)
    g = plane_gbuffer(cam, w, h, 5.0)
    cur = current_frame(w, h)
    cur[1, 1] = (np.nan, 1.0, 2.0, 1.0)
    cur[1, 2] = (1.0, 1.0, 1.0, 0.0)
    cur[1, 3] = (3.0, 2.0, 1.0, -2.0)
    cur[1, 4] = (1.0, 1.0, 1.0, 0.001)
    prev = (ramp_history(w, h), np.full((h, w), 2.0, np.float32), g)
    hist, length = tb.accumulate(cur, g, prev, cam, 0.0, tb.params())
    for x in (1, 2, 3, 4):
        assert np.array_equal(tb.bits(hist[1, x]), tb.bits(cur[1, x])) and length[1, x] == 0.0
    assert (np.delete(length.reshape(-1), [7, 8, 9, 10]) == 3.0).all()
    # the next frame: those pixels have length 0 and start again
    hist2, length2 = tb.accumulate(current_frame(w, h, 6), g, (hist, length, g), cam, 0.0, tb.params())
    assert (length2[1, 1:5] == 1.0).all() and np.isfinite(hist2).all()
    assert (np.delete(length2.reshape(-1), [7, 8, 9, 10]) == 4.0).all()


@pytest.mark.parametrize("delta", [(0.5, 0.0, 0.0), (100.0, -30.0, 7.0)])
def test_the_sky_keeps_its_history_under_a_translation(delta):
    """A miss is reprojected by its direction: a pure translation leaves every sky pixel where it was."""
    w, h, amount = 12, 7, 1.0
    cam0 = tb.make_camera(p=(1.0, 2.0, 3.0), aspect=w/h)
    cam1 = tb.moved(cam0, delta)

    def sky(cam):
        g = np.zeros((h, w), tb.dtype())
        g["p"] = tb.gbuffer_rays(cam, amount, w, h)
        g["primitive"] = tb.MISS
        return g
    cur = current_frame(w, h)
    ph = ramp_history(w, h)
    hist, length = tb.accumulate(cur, sky(cam1), (ph, np.full((h, w), 5.0, np.float32), sky(cam0)), cam0, amount, tb.params())
    c = resolved(cur)
    want = (ph[..., :3] + (c - ph[..., :3])*(F(1.0)/F(6.0))).astype(np.float32)
    assert (length == 6.0).all() and np.array_equal(tb.bits(hist[..., :3]), tb.bits(want))
    # a hit does not take the sky's history, nor the sky a hit's
    hit = plane_gbuffer(cam1, w, h, 5.0)
    _, l2 = tb.accumulate(cur, hit, (ph, np.full((h, w), 5.0, np.float32), sky(cam0)), cam0, amount, tb.params())
    assert (l2 == 1.0).all()


def test_synthetic_cases_exercise_every_rule():
    """The seeded inputs the GPU test replays: all kinds of outcome occur in them."""
    for w, h, amount in tb.SIZES:
        cur, g, prev, cam = tb.synthetic_case(w, h, amount)
        hist, length = tb.checked(w, h, amount)
        n = w*h
        assert (length == 0.0).sum() > 0.05*n > 0                       # invalid current pixels
        assert (length == 1.0).sum() > 0.1*n                            # no history
        assert ((length > 1.0) & (length < 32.0)).sum() > 0.1*n         # a blend
        assert (length == 32.0).sum() > 0                               # the cap
        assert (length != np.rint(length)).sum() > 0.05*n               # four taps of unlike lengths
        assert np.isfinite(hist[length > 0]).all()


# ---- 3. refusals, through the product library, before any device is touched

def last_error(rt):
    return (rt.lib().rt_last_error() or b"").decode()


def test_default_params_and_workspace(rt):
    assert rt.lib().rt_abi_version() == 8
    p = rt.default_temporal_params()
    assert (p.max_history, p.normal_cos, p.plane_tolerance, p.snap, p.firefly_clamp) == (32.0, F(0.9), F(0.02), 1.0/32.0, 10.0)
    assert list(p.reserved) == [0, 0, 0]
    assert rt.temporal_workspace_bytes(1920, 1080) == 1920*1080*120
    assert C.sizeof(rt.abi.GBufferTexel) == 32 and np.dtype(rt.abi.GBUFFER_DTYPE).itemsize == 32
    assert rt.lib().rt_temporal_default_params(None) == rt.abi.RT_ERROR_INVALID and "null out" in last_error(rt)


def test_accumulate_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    fp, gp = C.POINTER(C.c_float), C.POINTER(rt.abi.GBufferTexel)
    cur, hist, ph = (np.zeros((h, w, 4), np.float32) for _ in range(3))
    length, pl = (np.zeros((h, w), np.float32) for _ in range(2))
    g, pg = (np.zeros((h, w), tb.dtype()) for _ in range(2))
    cam = tb.make_camera()
    f = lambda a: a.ctypes.data_as(fp)
    G = lambda a: a.ctypes.data_as(gp)
    base = dict(current=f(cur), gbuffer=G(g), prev_history=f(ph), prev_length=f(pl), prev_gbuffer=G(pg), prev_camera=C.byref(cam),
                w=w, h=h, p=rt.default_temporal_params(), history=f(hist), length=f(length))

    def refused(entry, prefix, text, **change):
        a = dict(base, **change)
        p = a["p"]
        fn = getattr(lib, entry)
        code = fn(0, a["current"], a["gbuffer"], a["prev_history"], a["prev_length"], a["prev_gbuffer"], a["prev_camera"], 0.0,
                  a["w"], a["h"], None if p is None else C.byref(p), a["history"], a["length"],
                  *(() if entry == "rt_temporal_accumulate" else (None,)))
        assert code == rt.abi.RT_ERROR_INVALID, (entry, text, code)
        msg = last_error(rt)
        assert msg.startswith(entry + ":") and text.replace("@", prefix) in msg, (entry, text, msg)

    def P(**kw):
        p = rt.default_temporal_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for entry, prefix in (("rt_temporal_accumulate", ""), ("rt_temporal_accumulate_device", "d_")):
        for name in ("current", "gbuffer", "history", "length"):
            refused(entry, prefix, f"null @{name}", **{name: None})
        refused(entry, prefix, "null rt_temporal_params", p=None)
        refused(entry, prefix, "w is 0", w=0)
        refused(entry, prefix, "h is 0", h=0)
        for name in ("prev_history", "prev_length", "prev_gbuffer"):          # some but not all of the three
            refused(entry, prefix, f"null @{name}", **{name: None})
        refused(entry, prefix, "null prev_camera", prev_camera=None)
        refused(entry, prefix, "@history aliases @prev_history", history=f(ph))
        refused(entry, prefix, "@length aliases @prev_length", length=f(pl))
        for bad in (0.5, -1.0, float("nan"), float("inf")):
            refused(entry, prefix, "max_history", p=P(max_history=bad))
        for bad in (-1.5, 1.5, float("nan")):
            refused(entry, prefix, "normal_cos", p=P(normal_cos=bad))
        for field in ("plane_tolerance", "snap", "firefly_clamp"):
            for bad in (-0.1, float("nan"), float("inf")):
                refused(entry, prefix, field, p=P(**{field: bad}))


def test_gbuffer_and_driver_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    out = np.zeros((h, w, 4), np.float32)
    g = np.zeros((h, w), tb.dtype())
    fp, gp = C.POINTER(C.c_float), C.POINTER(rt.abi.GBufferTexel)
    fake_scene = C.c_void_p(0)                       # the scene is checked last: nothing before it needs one

    def gb(text, camera=C.byref(cam), w_=w, h_=h, o=g.ctypes.data_as(gp)):
        assert lib.rt_gbuffer(fake_scene, camera, 0.0, w_, h_, o) == rt.abi.RT_ERROR_INVALID
        assert last_error(rt).startswith("rt_gbuffer:") and text in last_error(rt), last_error(rt)
    gb("null camera", camera=None)
    gb("null out", o=None)
    gb("w is 0", w_=0)
    gb("h is 0", h_=0)
    gb("below 2^32", w_=70000, h_=70000)
    gb("null scene")
    assert lib.rt_gbuffer_device(fake_scene, C.byref(cam), 0.0, w, h, None, None) == rt.abi.RT_ERROR_INVALID
    assert "rt_gbuffer_device: null d_out" in last_error(rt)

    state = rt.abi.TemporalState()
    state.d_workspace = 64                           # never followed: every call below is refused first
    base = dict(camera=C.byref(cam), settings=C.byref(st), filter=C.byref(fc), tiles=C.byref(tiles), w=w, h=h,
                p=rt.default_temporal_params(), state=state, out=out.ctypes.data_as(fp))

    def drv(text, **change):
        a = dict(base, **change)
        p, s = a["p"], a["state"]
        code = lib.rt_render_temporal(fake_scene, a["camera"], a["settings"], a["filter"], a["tiles"], 0, a["w"], a["h"], 0,
                                      None if p is None else C.byref(p), None if s is None else C.byref(s), a["out"], None, None)
        assert code == rt.abi.RT_ERROR_INVALID, (text, code)
        assert last_error(rt).startswith("rt_render_temporal:") and text in last_error(rt), (text, last_error(rt))
    drv("null rt_temporal_params", p=None)
    bad = rt.default_temporal_params()
    bad.max_history = 0.0
    drv("max_history", p=bad)
    drv("null rt_temporal_state", state=None)
    drv("null d_workspace", state=rt.abi.TemporalState())
    drv("null settings", settings=None)
    drv("w is 0", w=0)
    drv("h is 0", h=0)
    drv("null camera", camera=None)
    drv("null filter", filter=None)
    drv("null tiles", tiles=None)
    drv("null out_pixels", out=None)
    drv("null scene")
    assert (state.frames, state.parity, state.w, state.h) == (0, 0, 0, 0)
