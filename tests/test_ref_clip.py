"""Neighbourhood clipping of the temporal history, on the CPU: the checker of the window statistics (tests/ref_clip)
against a numpy float32 restatement that adds in the stated order, against float64, on a constant image, around invalid
pixels and without a firefly clamp; the checker of the accumulate stage with a clip against the deform checker it extends
and against the texel it clips to; the layouts, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import ref_clip_binding as cb
import ref_deform_binding as db
import ref_temporal_binding as tb

F = np.float32


def same(a, b):
    return np.array_equal(tb.bits(a), tb.bits(b))


# ---- 1. the statistics

def np_values(cur, clamp):
    """Steps 1 and 2 in numpy float32 -> (h, w, 4): {r, g, b, 1} of a valid pixel, +0 four times of an invalid one."""
    cur = np.asarray(cur, F)
    with np.errstate(all="ignore"):
        c = cur[..., :3]/cur[..., 3:4]
    valid = (cur[..., 3] > F(0.001)) & np.isfinite(c).all(axis=2)
    c = np.where(c > 0, c, F(0))
    if clamp > 0:
        c = np.where(c < F(clamp), c, F(clamp))
    out = np.zeros(cur.shape, F)
    out[valid, :3] = c[valid]
    out[valid, 3] = 1.0
    return out


def np_stats(cur, r, clamp):
    """The statistics in numpy float32, every sum in the stated order: rows first, then columns."""
    v = np_values(cur, clamp)
    h, w, _ = v.shape
    with np.errstate(all="ignore"):
        seven = np.concatenate([v[..., :3], v[..., :3]*v[..., :3], v[..., 3:]], axis=2)
        pad = np.zeros((h + 2*r, w + 2*r, 7), F)
        pad[r:r + h, r:r + w] = seven
        H = pad[:, 0:w].copy()
        for d in range(1, 2*r + 1):
            H = H + pad[:, d:d + w]
        S = H[0:h].copy()
        for d in range(1, 2*r + 1):
            S = S + H[d:d + h]
        n = S[..., 6:7]
        some = n[..., 0] > 0
        mean = S[..., :3]/n
        var = S[..., 3:6]/n - mean*mean
        var = np.where(var > 0, var, F(0))
        out = np.zeros((h, w), cb.ndtype())
        out["mean"][some], out["count"][some], out["sigma"][some] = mean[some], n[..., 0][some], np.sqrt(var)[some]
    return out


@pytest.mark.parametrize("radius", cb.RADII)
@pytest.mark.parametrize("w,h", cb.STAT_SIZES)
def test_statistics_equal_numpy_in_the_stated_order(rt, w, h, radius):
    cur = cb.stats_image(w, h)
    got = cb.stats_checked(w, h, radius)
    want = np_stats(cur, radius, 10.0)
    assert same(got, want)
    assert not got["reserved"].any() and not np.isnan(got.view(F)).any()
    if w*h > 100:
        assert (got["count"] < (2*radius + 1)**2).any() and (got["sigma"] > 0).any()


def window64(x, r):
    """A window's mean and standard deviation in float64 over the in-image pixels of x (h, w, 3)."""
    h, w, _ = x.shape
    pad, ones = np.zeros((h + 2*r, w + 2*r, 3)), np.zeros((h + 2*r, w + 2*r, 1))
    pad[r:r + h, r:r + w], ones[r:r + h, r:r + w] = x, 1.0
    offsets = [(dy, dx) for dy in range(2*r + 1) for dx in range(2*r + 1)]
    s1 = sum(pad[dy:dy + h, dx:dx + w] for dy, dx in offsets)
    s2 = sum(pad[dy:dy + h, dx:dx + w]**2 for dy, dx in offsets)
    n = sum(ones[dy:dy + h, dx:dx + w] for dy, dx in offsets)
    mean = s1/n
    return mean, np.sqrt(np.maximum(s2/n - mean*mean, 0.0))


def errors64(v, wt):
    """(observed, inputs) over radii 1 to 3 for colours v and weights wt in float64: the buffer holds (v*wt, wt) rounded to
    float32; observed is the checker's mean and sigma against float64 from the unrounded v, inputs the same statistics
    in float64 arithmetic from the float32 buffer against it."""
    cur = np.concatenate([v*wt, wt], axis=2).astype(F)
    r64 = cur[..., :3].astype(np.float64)/cur[..., 3:4].astype(np.float64)
    observed = inputs = 0.0
    for r in cb.RADII:
        got = cb.neighbourhood(cur, r, 0.0)
        want_m, want_s = window64(v, r)
        in_m, in_s = window64(r64, r)
        inputs = max(inputs, float(np.abs(in_m - want_m).max()), float(np.abs(in_s - want_s).max()))
        observed = max(observed, float(np.abs(got["mean"] - want_m).max()), float(np.abs(got["sigma"] - want_s).max()))
    return observed, inputs


def test_statistics_against_float64(rt):
    """The checker's mean and sigma (the kernel's, bit for bit) against the window's mean and standard deviation in
    float64 from unrounded colours.  The bound is 4 x the largest error the float64 model shows for rounding the inputs
    alone (errors64).  The image is what the stage is given, a frame of one sample per pixel: heavy-tailed colours,
    exp(N(0, 1.5)), the radiance of every synthetic case of this suite, under weights of 0.5 to 4.  There a window's
    mean^2 and variance are of one size.  Measured (65 x 33, radii 1 to 3): observed 6.90e-6, the inputs' own 2.58e-6, so
    the bound is 1.03e-5 ("Neighbourhood clipping").
    The bound in this form cannot hold on a low-contrast image, and the test says so instead of hiding it: var = S2/n -
    mean*mean in float32 loses mean^2/var of its digits, which float64 arithmetic from rounded inputs does not.  Uniform
    colours of 0.5 to 1.5 (mean^2/var = 12) are printed, not asserted: observed 1.33e-6 against the inputs' 4.95e-8, 27
    times.  That is 5e-6 of the sigma of 0.29 the clip would multiply by gamma."""
    w, h = tb.SIZES[0][:2]
    rng = np.random.default_rng(31)
    flat, flat_in = errors64(rng.uniform(0.5, 1.5, (h, w, 3)), rng.uniform(0.5, 4.0, (h, w, 1)))
    print(f"statistics, uniform colours of 0.5 to 1.5 (not asserted): observed {flat:.3e}, the inputs' own rounding {flat_in:.3e}")
    observed, inputs = errors64(np.exp(rng.normal(0.0, 1.5, (h, w, 3))), rng.uniform(0.5, 4.0, (h, w, 1)))
    bound = 4.0*inputs
    print(f"statistics: observed max |checker - float64| {observed:.3e}, the inputs' own rounding {inputs:.3e}, bound {bound:.3e}")
    assert inputs > 0.0 and observed <= bound


@pytest.mark.parametrize("radius", cb.RADII)
def test_constant_image_and_the_count_at_the_borders(rt, radius):
    for w, h in cb.STAT_SIZES:
        cur = np.empty((h, w, 4), F)
        cur[..., :3], cur[..., 3] = 1.0, 2.0                        # 0.5 under a weight of 2
        got = cb.neighbourhood(cur, radius, 10.0)
        assert (tb.bits(got["mean"]) == tb.bits(F(0.5))).all() and not tb.bits(got["sigma"]).any()
        xs, ys = np.arange(w), np.arange(h)
        nx = np.minimum(xs + radius, w - 1) - np.maximum(xs - radius, 0) + 1
        ny = np.minimum(ys + radius, h - 1) - np.maximum(ys - radius, 0) + 1
        assert same(got["count"], (ny[:, None]*nx[None, :]).astype(F))


def test_invalid_pixels_leave_their_neighbours_sums_alone(rt):
    w, h, r = 23, 19, 2
    rng = np.random.default_rng(5)
    wt = rng.uniform(0.5, 4.0, (h, w, 1))
    base = np.concatenate([rng.uniform(0.0, 3.0, (h, w, 3))*wt, wt], axis=2).astype(F)
    full = cb.neighbourhood(base, r, 10.0)
    qy, qx = 9, 11
    results = []
    for kind in ("zero weight", "the threshold", "nan", "inf"):
        cur = base.copy()
        if kind == "zero weight":
            cur[qy, qx, 3] = 0.0
        elif kind == "the threshold":
            cur[qy, qx, 3] = F(0.001)
        elif kind == "nan":
            cur[qy, qx, 1] = np.nan
        else:
            cur[qy, qx, 0] = np.inf
        got = cb.neighbourhood(cur, r, 10.0)
        assert same(got, np_stats(cur, r, 10.0)), kind
        inside = np.zeros((h, w), bool)
        inside[qy - r:qy + r + 1, qx - r:qx + r + 1] = True
        assert same(got[~inside], full[~inside]), kind
        assert (got["count"][inside] == full["count"][inside] - 1).all(), kind
        assert not np.isnan(got.view(F)).any(), kind
        results.append(got)
    # whichever way a pixel is invalid, it adds the same +0
    assert all(same(results[0], other) for other in results[1:])
    # the centre's own texel is written, from its neighbours
    assert results[0]["count"][qy, qx] == (2*r + 1)**2 - 1


def test_without_a_firefly_clamp_no_field_is_nan(rt):
    """firefly_clamp 0.  A colour of 1e20: its square overflows, so S2 is infinite while mean*mean is not, and sigma is
    +inf.  A colour of 1e30: mean*mean overflows too, var = inf - inf is NaN and goes to 0; the mean stays finite.  Two
    colours of 3e38 in one window: S1 overflows and the mean is +inf.  DESIGN.md says that no field is ever NaN."""
    w, h, r = 12, 9, 3
    near = np.zeros((h, w), bool)
    near[1:8, 2:9] = True                              # the windows that hold pixel (5, 4)
    cur = np.ones((h, w, 4), F)
    cur[4, 5, :3] = 1e20
    got = cb.neighbourhood(cur, r, 0.0)
    assert np.isposinf(got["sigma"][near]).all() and np.isfinite(got["mean"]).all() and not np.isnan(got.view(F)).any()
    assert not tb.bits(got["sigma"][~near]).any() and same(got, np_stats(cur, r, 0.0))
    cur[4, 5, :3] = 1e30
    got = cb.neighbourhood(cur, r, 0.0)
    assert not tb.bits(got["sigma"]).any() and np.isfinite(got["mean"]).all() and float(got["mean"].max()) > 1e28
    assert same(got, np_stats(cur, r, 0.0))
    cur[4, 6, :3] = 3e38
    cur[4, 5, :3] = 3e38
    got = cb.neighbourhood(cur, r, 0.0)
    both = np.zeros((h, w), bool)
    both[1:8, 3:9] = True
    assert np.isposinf(got["mean"][both]).all() and not tb.bits(got["sigma"][both]).any() and not np.isnan(got.view(F)).any()
    # and with the default clamp nothing overflows
    got = cb.neighbourhood(cur, r, 10.0)
    assert np.isfinite(got.view(F)).all() and float(got["mean"].max()) <= 10.0


# ---- 2. the stage

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_without_a_clip_it_is_the_deform_checker(rt, w, h, amount):
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p = tb.params()
    nb = cb.clip_texels(w, h, amount)
    table = db.host_table(tp, arrays)
    for moments in (False, True):
        for velocity in (False, True):
            for t, s in ((table, surf), (None, None)):
                want = db.accumulate_deform(cur, g, prev, cam, amount, p, moving, s, t, want_moments=moments, want_velocity=velocity)
                for texels, gamma, min_count in ((None, 1.0, 2.0), (nb, 1.0, 50.0), (nb, 0.0, 49.5)):
                    got = cb.accumulate_clip(cur, g, prev, cam, amount, p, moving, s, t, texels, gamma, min_count,
                                             want_moments=moments, want_velocity=velocity)
                    for a, b in zip(got[:4], want):
                        assert (a is None) == (b is None) and (a is None or same(a, b))
                    assert not tb.bits(got[4]).any()
    assert 40.0 <= float(nb["count"].max()) <= 49.0        # so a min_count of 49.5 or 50 switches every texel off


@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_gamma_0_blends_the_texels_mean_with_the_current_colour(rt, w, h, amount):
    cur = db.deform_case(w, h, amount)[0]
    nb = cb.clip_texels(w, h, amount)
    hist, length, _, _, amt = cb.checked(w, h, amount, False, False, 0.0)
    c = np_values(cur, tb.params().firefly_clamp)
    clipped = (c[..., 3] > 0) & (length > 1) & (nb["count"] >= 2)
    a = F(1.0)/length[clipped]
    m = nb["mean"][clipped]
    want = m + (c[..., :3][clipped] - m)*a[:, None]
    print(f"{w}x{h}: {int(clipped.sum())} pixels with a history and a texel, {int((amt > 0).sum())} of them moved")
    assert clipped.sum() > 100 and same(hist[clipped][:, :3], want)
    # the rest is the deform checker's
    plain = db.checked(w, h, amount, False, False)
    assert same(hist[~clipped], plain[0][~clipped]) and same(length, plain[1]) and not tb.bits(amt[~clipped]).any()


@pytest.mark.parametrize("gamma", [1.0, 4.0])
@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_history_inside_the_box_is_left_alone(rt, w, h, amount, gamma):
    plain = db.checked(w, h, amount, True, True)
    got = cb.checked(w, h, amount, True, True, gamma)
    inside = tb.bits(got[4]) == 0
    moved = got[4] > 0
    print(f"{w}x{h}, gamma {gamma}: {int(moved.sum())} pixels clipped, the largest by {float(got[4].max()):.3f}")
    assert (inside | moved).all() and moved.sum() >= 4 and inside.sum() > 200
    assert same(got[0][inside], plain[0][inside]) and (tb.bits(got[0][moved]) != tb.bits(plain[0][moved])).any()
    # length, moments and velocity are the deform stage's everywhere
    assert same(got[1], plain[1]) and same(got[2], plain[2]) and same(got[3], plain[3])
    # a wider box clips no more pixels, and none by more
    if gamma == 4.0:
        narrow = cb.checked(w, h, amount, True, True, 1.0)[4]
        assert (got[4] <= narrow).all() and moved.sum() < (narrow > 0).sum()


def test_without_history_and_on_invalid_pixels_nothing_is_clipped(rt):
    w, h, amount = tb.SIZES[0]
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p, nb, table = tb.params(), cb.clip_texels(w, h, amount), db.host_table(tp, arrays)
    got = cb.accumulate_clip(cur, g, None, None, 0.0, p, moving, surf, table, nb, 0.0, 0.0, want_moments=True, want_velocity=True)
    want = db.accumulate_deform(cur, g, None, None, 0.0, p, moving, surf, table, want_moments=True, want_velocity=True)
    assert all(same(a, b) for a, b in zip(got[:4], want)) and not tb.bits(got[4]).any()
    # invalid pixels of a call with history: the texel is never read
    got = cb.checked(w, h, amount, True, True, 0.0)
    plain = db.checked(w, h, amount, True, True)
    invalid = plain[1] == 0
    assert invalid.sum() > 20 and not tb.bits(got[4][invalid]).any()
    assert all(same(a[invalid], b[invalid]) for a, b in zip(got[:4], plain))


def test_a_nan_or_an_infinite_bound_leaves_the_history_alone(rt):
    w, h, amount = tb.SIZES[0]
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p, table = tb.params(), db.host_table(tp, arrays)
    nb = cb.clip_texels(w, h, amount).copy()
    nb["mean"][:, 0:20] = np.nan                    # both bounds NaN
    nb["sigma"][:, 20:40] = np.inf                  # lo = -inf, hi = +inf
    nb["sigma"][:, 40:50] = np.nan
    odd = np.zeros((h, w), bool)
    odd[:, :50] = True
    got = cb.accumulate_clip(cur, g, prev, cam, amount, p, moving, surf, table, nb, 1.0, 2.0)
    plain = db.checked(w, h, amount, False, False)
    assert same(got[0][odd], plain[0][odd]) and not tb.bits(got[4][odd]).any()
    assert (got[4][~odd] > 0).any() and same(got[1], plain[1])
    # gamma 0 against an infinite sigma: 0 * inf is a NaN bound
    got = cb.accumulate_clip(cur, g, prev, cam, amount, p, moving, surf, table, nb, 0.0, 2.0)
    inf = np.zeros((h, w), bool)
    inf[:, 20:40] = True
    assert same(got[0][inf], plain[0][inf]) and not tb.bits(got[4][inf]).any()


# ---- 3. layouts and refusals that need no device

def test_layouts(rt):
    abi = rt.abi
    assert C.sizeof(abi.NeighbourhoodTexel) == 32 == np.dtype(abi.NEIGHBOURHOOD_DTYPE).itemsize
    assert C.sizeof(abi.TemporalClipParams) == 16
    for name, _ in abi.NeighbourhoodTexel._fields_:
        assert getattr(abi.NeighbourhoodTexel, name).offset == np.dtype(abi.NEIGHBOURHOOD_DTYPE).fields[name][1]
    deform = rt.temporal_deform_workspace_bytes(130, 70, 5)
    assert rt.temporal_clipped_workspace_bytes(130, 70, 5) == (deform + 15)//16*16 + 36*130*70
    assert rt.temporal_clipped_workspace_bytes(3, 3, 0) >= rt.temporal_deform_workspace_bytes(3, 3, 0) + 36*9
    cp = rt.default_temporal_clip_params()
    assert (cp.radius, cp.min_count, cp.reserved) == (3, 2.0, 0) and cp.gamma > 0
    assert rt.lib().rt_temporal_clip_default_params(None) == abi.RT_ERROR_INVALID


def refused(rt, code, text):
    assert code == rt.abi.RT_ERROR_INVALID
    message = rt.lib().rt_last_error().decode()
    assert text in message, message


def test_refusals_by_name(rt):
    lib, abi = rt.lib(), rt.abi
    w, h = 4, 3
    p = tb.params()
    buf, other, third = ((C.c_float*(w*h*8))() for _ in range(3))
    cam = tb.make_camera()
    ptr = lambda a: C.cast(a, C.c_void_p)
    fp, gp, npt = C.POINTER(C.c_float), C.POINTER(abi.GBufferTexel), C.POINTER(abi.NeighbourhoodTexel)
    nan, inf = float("nan"), float("inf")

    def stats(**kw):
        a = dict(current=ptr(buf), out=ptr(other), w=w, h=h, radius=3, clamp=10.0)
        a.update(kw)
        return lib.rt_temporal_neighbourhood_device(0, a["current"], a["w"], a["h"], a["radius"], a["clamp"], a["out"], None)
    e = "rt_temporal_neighbourhood_device: "
    refused(rt, stats(current=None), e + "null d_current")
    refused(rt, stats(out=None), e + "null d_out")
    refused(rt, stats(w=0), e + "w is 0")
    refused(rt, stats(h=0), e + "h is 0")
    refused(rt, stats(w=65536, h=65536), e + "w*h must be below 2^32")
    refused(rt, stats(w=0xFFFFFFFF, h=2), e + "w*h must be below 2^32")
    refused(rt, stats(radius=0), e + "radius must be in 1..3")
    refused(rt, stats(radius=4), e + "radius must be in 1..3")
    for bad in (-1.0, nan, inf):
        refused(rt, stats(clamp=bad), e + "firefly_clamp must be finite and >= 0")
    refused(rt, stats(out=ptr(buf)), e + "d_out aliases d_current")
    code = lib.rt_temporal_neighbourhood(0, C.cast(buf, fp), w, h, 3, 10.0, C.cast(buf, npt))
    refused(rt, code, "rt_temporal_neighbourhood: out aliases current")
    refused(rt, lib.rt_temporal_neighbourhood(0, C.cast(buf, fp), w, h, 7, 10.0, C.cast(other, npt)),
            "rt_temporal_neighbourhood: radius must be in 1..3")
    refused(rt, lib.rt_temporal_neighbourhood(0, None, w, h, 3, 10.0, C.cast(other, npt)), "rt_temporal_neighbourhood: null current")

    def stage(**kw):
        a = dict(current=ptr(buf), gbuffer=ptr(buf), hist=ptr(other), length=ptr(other), p=C.byref(p), w=w, h=h, surf=None,
                 deform=None, dcount=0, nb=ptr(third), gamma=1.0, min_count=2.0, amount=ptr(other))
        a.update(kw)
        return lib.rt_temporal_accumulate_clip_device(0, a["current"], a["gbuffer"], None, None, None, C.byref(cam), 0.0, a["w"],
                                                      a["h"], a["p"], a["hist"], a["length"], None, None, 0, None, None, None,
                                                      a["surf"], a["deform"], a["dcount"], a["nb"], a["gamma"], a["min_count"],
                                                      a["amount"])
    e = "rt_temporal_accumulate_clip_device: "
    # the deform stage's
    refused(rt, stage(current=None), e + "null d_current")
    refused(rt, stage(hist=None), e + "null d_history")
    refused(rt, stage(w=0), e + "w is 0")
    refused(rt, stage(p=None), e + "null rt_temporal_params")
    refused(rt, stage(dcount=2), e + "null d_deform with a deform_count")
    refused(rt, stage(deform=ptr(buf), dcount=2), e + "null d_surface with a deform table")
    # its own
    for bad in (-0.5, nan, inf):
        refused(rt, stage(gamma=bad), e + "gamma must be finite and >= 0")
        refused(rt, stage(min_count=bad), e + "min_count must be finite and >= 0")
    code = lib.rt_temporal_accumulate_clip(0, C.cast(buf, fp), C.cast(buf, gp), None, None, None, C.byref(cam), 0.0, w, h,
                                           C.byref(p), C.cast(other, fp), C.cast(other, fp), None, 0, None, None, None, None,
                                           None, 0, C.cast(third, npt), -1.0, 2.0, None)
    refused(rt, code, "rt_temporal_accumulate_clip: gamma must be finite and >= 0")
    # the driver: the clip parameters first, then rt_render_temporal_deform_device's order
    state = abi.TemporalMotionState()
    st, _ = rt.default_settings()
    fc = rt.load_reconstruction_kernel("Box")
    tiles = abi.TileSet(64, 64, 0, 1)
    cp = rt.default_temporal_clip_params()
    one = (abi.M4x4Inv*1)()

    def driver(**kw):
        a = dict(p=C.byref(p), state=C.byref(state), st=C.byref(st), cam=C.byref(cam), fc=C.byref(fc), tiles=C.byref(tiles),
                 out=ptr(buf), w=w, h=h, cp=C.byref(cp))
        a.update(kw)
        return lib.rt_render_temporal_clipped_device(None, a["cam"], a["st"], a["fc"], a["tiles"], 0, a["w"], a["h"], 0, a["p"],
                                                     a["state"], 0, None, a["cp"], a["out"], None, None, None, None)
    e = "rt_render_temporal_clipped_device: "
    refused(rt, driver(cp=None), e + "null rt_temporal_clip_params")
    for field, bad, text in (("radius", 0, "radius must be in 1..3"), ("radius", 4, "radius must be in 1..3"),
                             ("gamma", -1.0, "gamma must be finite and >= 0"), ("gamma", nan, "gamma must be finite and >= 0"),
                             ("min_count", inf, "min_count must be finite and >= 0")):
        broken = rt.default_temporal_clip_params()
        setattr(broken, field, bad)
        refused(rt, driver(cp=C.byref(broken)), e + "rt_temporal_clip_params: " + text)
    refused(rt, driver(p=None), e + "null rt_temporal_params")
    refused(rt, driver(state=None), e + "null rt_temporal_motion_state")
    refused(rt, driver(), e + "rt_temporal_motion_state: null d_workspace")
    state.d_workspace = C.addressof(buf)
    refused(rt, driver(), e + "rt_temporal_motion_state: null transforms")
    state.transforms = C.cast(one, C.POINTER(abi.M4x4Inv))
    refused(rt, driver(st=None), e + "null settings")
    refused(rt, driver(w=0), e + "w is 0")
    refused(rt, driver(out=None), e + "null d_out")
    refused(rt, driver(), e + "null scene")
    code = lib.rt_render_temporal_clipped(None, C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), 0, w, h, 0, C.byref(p),
                                          C.byref(state), 0, None, C.byref(cp), None, None, None, None)
    refused(rt, code, "rt_render_temporal_clipped: null out_pixels")
    # nothing was written anywhere
    assert not any(bytes(b).strip(b"\0") for b in (buf, other, third)) and state.frames == 0
