"""Variance-guided filtering of the temporal history on the CPU ("Variance-guided filtering"): the plain-C
checker tests/ref_svgf held to the accumulate stage's own checker, to float64 means, to hand-made G-buffers and to the
filter's closed forms; the default parameters on the oracle's own frames; and the argument checks of the product
library, which refuse by name before any device is touched.  No GPU is needed (tests/test_gpu_svgf.py has the device).
"""
import ctypes as C

import numpy as np
import pytest

import ref_denoise_binding as rd
import ref_svgf_binding as sb
import ref_temporal_binding as tb

F = np.float32


def tm64(c):
    """tm of a float64 colour (..., 3)."""
    return 1.0 - np.exp(-(0.2126*c[..., 0] + 0.7152*c[..., 1] + 0.0722*c[..., 2]))


# ---- 1. accumulate with moments

@pytest.mark.parametrize("w,h", sb.KERNEL_SIZES)
def test_moments_stage_keeps_the_accumulate_stage_bit_for_bit(w, h):
    cur, g, prev, cam = sb.moments_case(w, h)
    for p in (tb.params(), tb.params(snap=0.0, firefly_clamp=0.0), tb.params(max_history=2.5, normal_cos=-1.0, plane_tolerance=10.0),
              tb.params(max_history=1.0)):
        want_hist, want_len = tb.accumulate(cur, g, prev[:3], cam, 2.0, p)
        hist, length, mom = sb.accumulate_moments(cur, g, prev, cam, 2.0, p)
        assert np.array_equal(tb.bits(hist), tb.bits(want_hist)) and np.array_equal(tb.bits(length), tb.bits(want_len))
        assert not (mom == -7.0).any()                       # no pixel left out
    want_hist, want_len = tb.accumulate(cur, g, None, None, 0.0, tb.params())
    hist, length, mom = sb.accumulate_moments(cur, g, None, None, 0.0, tb.params())
    assert np.array_equal(tb.bits(hist), tb.bits(want_hist)) and np.array_equal(tb.bits(length), tb.bits(want_len))


def test_moments_rules_by_hand():
    """Invalid pixels write {0, 0}; no history and N == 1 give {t, t*t} exactly; a tap blends by the stated expression;
    garbage moments stay in the moments."""
    w, h = 7, 5
    cam = tb.make_camera(p=(0.3, 0.2, 2.0), aspect=w/h)
    g = sb.plane_gbuffer(cam, w, h, 5.0)
    rng = np.random.default_rng(3)
    wt = rng.uniform(0.5, 3.0, (h, w, 1))
    cur = np.concatenate([rng.uniform(0.0, 2.0, (h, w, 3))*wt, wt], axis=2).astype(F)
    cur[0, 0] = (1.0, np.nan, 1.0, 1.0)
    cur[0, 1, 3] = 0.0
    cur[1, 1, :3] = 100.0*cur[1, 1, 3]                   # a firefly: t is of the clamped colour
    hist, length, mom = sb.accumulate_moments(cur, g, None, None, 0.0, tb.params())
    c = hist[..., :3].astype(np.float64)
    t = tm64(c)
    ok = length == 1.0
    assert not ok[0, 0] and not ok[0, 1] and ok.sum() == w*h - 2
    assert (mom[~ok] == 0.0).all()
    assert np.abs(mom[..., 0][ok] - t[ok]).max() < 1e-6
    assert np.array_equal(tb.bits(mom[..., 1][ok]), tb.bits((mom[..., 0]*mom[..., 0])[ok]))      # t2 = t*t in f32
    assert mom[1, 1, 0] == pytest.approx(1.0 - np.exp(-10.0), abs=1e-6)
    # a standing camera: the own pixel's moments, blended with a = 1/4
    ph = np.concatenate([rng.uniform(0.0, 2.0, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(F)
    pl = np.full((h, w), 3.0, F)
    pm = rng.uniform(0.0, 1.0, (h, w, 2)).astype(F)
    pm[2, 3] = (np.nan, np.inf)                          # garbage in: garbage out, in the moments of that pixel only
    hist2, length2, mom2 = sb.accumulate_moments(cur, g, (ph, pl, g, pm), cam, 0.0, tb.params())
    a = F(1.0)/F(4.0)
    tt = np.stack([mom[..., 0], mom[..., 1]], axis=2)
    with np.errstate(invalid="ignore"):                # the garbage pixel
        want = (pm + (tt - pm)*a).astype(F)
    sel = ok.copy()
    sel[2, 3] = False
    assert (length2[ok] == 4.0).all()
    assert np.array_equal(tb.bits(mom2[sel]), tb.bits(want[sel]))
    assert np.isnan(mom2[2, 3]).all() and np.isfinite(hist2[2, 3]).all() and np.isfinite(mom2[sel]).all()
    # max_history 1: {t, t*t} exactly
    _, length1, mom1 = sb.accumulate_moments(cur, g, (ph, pl, g, pm), cam, 0.0, tb.params(max_history=1.0))
    assert (length1[ok] == 1.0).all() and np.array_equal(tb.bits(mom1), tb.bits(mom))


def test_standing_camera_moments_are_the_float64_means():
    """Eight frames from one camera: the moments are the means of t and t*t within rel 1e-5 (the bar of the history's
    own standing-camera test), and the variance is their (m2 - m1*m1)/N."""
    w, h, n = 24, 10, 8
    cam = tb.make_camera(p=(0.3, 0.2, 2.0), aspect=w/h)
    g = sb.plane_gbuffer(cam, w, h, 5.0)
    rng = np.random.default_rng(11)
    frames = np.concatenate([np.exp(rng.normal(-0.5, 1.0, (n, h, w, 3))), np.ones((n, h, w, 1))], axis=3).astype(F)
    prev = None
    for k in range(n):
        hist, length, mom = sb.accumulate_moments(frames[k], g, prev, cam, 0.0, tb.params())
        prev = (hist, length, g, mom)
    assert (length == float(n)).all()
    t = tm64(np.minimum(frames[..., :3].astype(np.float64), 10.0))
    m1, m2 = t.mean(axis=0), (t*t).mean(axis=0)
    rel = lambda a, b: float(np.linalg.norm(a - b)/np.linalg.norm(b))
    print("standing camera: rel L2 of m1, m2", rel(mom[..., 0], m1), rel(mom[..., 1], m2))
    assert rel(mom[..., 0], m1) <= 1e-5 and rel(mom[..., 1], m2) <= 1e-5
    var = sb.variance(mom, length, g, tb.params(), 4.0)
    want = np.maximum(mom[..., 1] - mom[..., 0]*mom[..., 0], F(0))/F(n)
    assert np.array_equal(tb.bits(var), tb.bits(want.astype(F)))
    assert np.abs(var - (m2 - m1*m1)/n).max() < 1e-6


# ---- 2. the variance window's tap rule

def window_case(w=9, h=9):
    cam = tb.make_camera(p=(0.0, 0.0, 1.0), aspect=w/h)
    g = sb.plane_gbuffer(cam, w, h, 5.0, primitive=1)
    rng = np.random.default_rng(5)
    m1 = rng.uniform(0.2, 0.8, (h, w))
    m = np.stack([m1, m1*m1 + 0.01], axis=2).astype(F)
    return cam, g, m, np.ones((h, w), F)


def window_mean(m, length, mask, y, x):
    """The definition in numpy, with the sums in window order in f32."""
    h, w = length.shape
    cnt = A1 = A2 = F(0)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            qy, qx = y + dy, x + dx
            if 0 <= qy < h and 0 <= qx < w and ((dy == 0 and dx == 0) or mask[qy, qx]):
                cnt, A1, A2 = cnt + F(1), A1 + m[qy, qx, 0], A2 + m[qy, qx, 1]
    M1, M2 = A1/cnt, A2/cnt
    s2 = M2 - M1*M1
    return (s2 if s2 > 0 else F(0))/length[y, x], int(cnt)


@pytest.mark.parametrize("fault", ["none", "primitive", "normal", "plane", "length", "miss"])
def test_variance_window_tap_rule(fault):
    cam, g, m, length = window_case()
    h, w = length.shape
    mask = np.ones((h, w), bool)
    right = np.zeros((h, w), bool)
    right[:, 5:] = True
    if fault == "primitive":                                 # an edge between two primitives
        g["primitive"][right] = 2
        mask = ~right
    elif fault == "normal":                                  # a turned normal: cos 0.8 < 0.9
        g["n"][right] = (0.6, 0.0, 0.8)
        mask = ~right
    elif fault == "plane":                                   # a step in the plane: 0.3 against 0.02 * t of about 5
        g["p"][right] += np.array([0.0, 0.0, -0.3], F)
        mask = ~right
    elif fault == "length":                                  # neighbours without a history of their own
        length[right] = 0.5
        length[2, 2] = np.nan
        mask = ~right
        mask[2, 2] = False
    elif fault == "miss":                                    # the sky: the primitive alone decides
        g = sb.miss_gbuffer(cam, w, h)
    var, counted = sb.variance(m, length, g, tb.params(), 4.0, want_counted=True)
    for (y, x) in [(4, 4), (0, 0), (8, 3), (4, 1), (1, 4)]:     # the interior, two corners' sides, the borders
        want, cnt = window_mean(m, length, mask, y, x)
        assert counted[y, x] == cnt, (fault, y, x)
        assert var[y, x] == want, (fault, y, x)
    # the centre's window is columns 1..7: all 49 taps, or the four columns left of the edge (less the NaN length)
    assert counted[4, 4] == {"none": 49, "miss": 49, "length": 27}.get(fault, 28)
    if fault == "length":
        assert (var[right] == 0.0).all() and var[2, 2] == 0.0 and (counted[right] == 0).all()


def test_variance_centre_always_counts_and_long_histories_skip_the_window():
    cam, g, m, length = window_case()
    g["n"][4, 4] = 0.0                                       # a zero normal fails dot >= normal_cos against itself
    var, counted = sb.variance(m, length, g, tb.params(), 4.0, want_counted=True)
    assert counted[4, 4] == 1
    s2 = m[4, 4, 1] - m[4, 4, 0]*m[4, 4, 0]
    assert var[4, 4] == s2
    # length >= spatial_below: the pixel's own moments over its length, no window; the threshold itself included
    length[:] = 4.0
    length[0, 0] = np.nextafter(F(4.0), F(0.0))
    m[1, 1] = (0.5, 0.2)                                     # m2 < m1*m1: clamped at 0
    var, counted = sb.variance(m, length, g, tb.params(), 4.0, want_counted=True)
    own = np.maximum(m[..., 1] - m[..., 0]*m[..., 0], F(0))/length
    sel = np.ones(length.shape, bool)
    sel[0, 0] = False
    assert np.array_equal(tb.bits(var[sel]), tb.bits(own[sel].astype(F))) and (counted[sel] == 0).all()
    assert counted[0, 0] == 16 and var[1, 1] == 0.0
    # spatial_below 0: never a window
    _, counted = sb.variance(m, np.ones_like(length), g, tb.params(), 0.0, want_counted=True)
    assert (counted == 0).all()


# ---- 3. the filter

def sky(w, h):
    cam = tb.make_camera(aspect=w/h)
    return sb.miss_gbuffer(cam, w, h)


def test_filter_closed_forms_without_edge_stopping():
    """All sigmas 0 on an all-miss G-buffer: every weight is the B3 kernel's.  Variance 1 everywhere gives an interior
    pixel var_1 = sum(k^2) = (70/256)^2; a constant colour stays constant."""
    w, h = 16, 12
    g = sky(w, h)
    col = np.tile(np.array([0.7, 0.3, 0.2, 1.0], F), (h, w, 1))
    p = sb.filter_params(iterations=1, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0)
    out, var = sb.denoise_variance(col, np.ones((h, w), F), g, p)
    assert np.abs(var[2:-2, 2:-2] - (70.0/256.0)**2).max() <= 1e-6
    assert np.abs(out - col).max() <= 1e-6
    out5, _ = sb.denoise_variance(col, np.ones((h, w), F), g, sb.filter_params(iterations=5, sigma_color=0.0,
                                                                                sigma_normal=0.0, sigma_plane=0.0))
    assert np.abs(out5 - col).max() <= 1e-6
    # and with the default sigmas on a plane: still constant
    cam = tb.make_camera(aspect=w/h)
    outp, _ = sb.denoise_variance(col, np.full((h, w), 0.01, F), sb.plane_gbuffer(cam, w, h, 5.0), sb.filter_params())
    assert np.abs(outp - col).max() <= 1e-6


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_filter_without_edge_stopping_is_the_denoise_stage(iterations):
    w, h = 33, 21
    beauty, _, _ = rd.random_frames(w, h, seed=4)
    want = rd.denoise(beauty, None, None, rd.params(iterations, 0.0, (0.0, 0.0), 10.0))
    p = sb.filter_params(iterations=iterations, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0)
    out, _ = sb.denoise_variance(beauty, np.full((h, w), 0.5, F), sky(w, h), p)
    assert np.array_equal(tb.bits(out), tb.bits(want))


def test_zero_variance_keeps_a_pixel_among_different_neighbours():
    """Variance 0: the colour term's scale is variance_epsilon alone.  At 1e-3, neighbours whose l differs by 0.12 or
    more have e >= 120 and weigh expf(-e) = 0, so the pixel keeps its colour within 2 ulp."""
    w, h = 12, 10
    rng = np.random.default_rng(8)
    grey = np.array([0.1, 0.5, 1.0, 2.0, 4.0])[(np.arange(w)[None, :] + 2*np.arange(h)[:, None]) % 5]
    col = np.stack([grey, grey, grey, np.ones((h, w))], axis=2).astype(F)
    g = sb.plane_gbuffer(tb.make_camera(aspect=w/h), w, h, 5.0)
    out, var = sb.denoise_variance(col, np.zeros((h, w), F), g, sb.filter_params(iterations=5, variance_epsilon=1e-3))
    ulp = np.abs(tb.bits(out[..., :3]).astype(np.int64) - tb.bits(col[..., :3]).astype(np.int64))
    assert ulp.max() <= 2 and (var == 0.0).all() and (out[..., 3] == 1.0).all()
    del rng


def test_invalid_pixels_pass_through_and_feed_no_neighbour():
    w, h = 14, 11
    col, var, g = (a.copy() for a in sb.filter_case(w, h))
    col[...] = np.abs(np.nan_to_num(col, nan=1.0, posinf=1.0)) + F(0.01)
    col[..., 3] = 1.0
    var[...] = 0.01
    spots = {(2, 3): ("col", (np.nan, 1.0, 1.0, 1.0)), (5, 5): ("col", (1.0, 1.0, 1.0, 0.0)), (7, 2): ("col", (1.0, 1.0, 1.0, -3.0)),
             (3, 9): ("var", np.nan), (8, 8): ("var", -0.5), (6, 11): ("var", np.inf)}
    for yx, (what, v) in spots.items():
        (col if what == "col" else var)[yx] = v
    out, vout = sb.denoise_variance(col, var, g, sb.filter_params())
    for yx in spots:
        assert np.array_equal(tb.bits(out[yx]), tb.bits(col[yx])) and np.array_equal(tb.bits(vout[yx]), tb.bits(var[yx])), yx
    # other values in the invalid spots: every other pixel keeps its bits
    col2, var2 = col.copy(), var.copy()
    for yx, (what, v) in spots.items():
        if what == "col":
            col2[yx] = (9e9, np.inf, 0.0, 0.0005)
        else:
            var2[yx] = -np.inf
            col2[yx] = (55.0, 55.0, 55.0, 1.0)
    out2, vout2 = sb.denoise_variance(col2, var2, g, sb.filter_params())
    mask = np.ones((h, w), bool)
    for yx in spots:
        mask[yx] = False
    assert np.array_equal(tb.bits(out[mask]), tb.bits(out2[mask])) and np.array_equal(tb.bits(vout[mask]), tb.bits(vout2[mask]))
    assert np.isfinite(out[mask]).all() and (out[mask][:, 3] == 1.0).all() and (vout[mask] >= 0).all()


def test_hits_and_misses_do_not_mix():
    """A sky above a wall, both constant but different: with every sigma 0 the border still stays sharp."""
    w, h = 10, 12
    cam = tb.make_camera(aspect=w/h)
    g = sb.plane_gbuffer(cam, w, h, 5.0)
    top = sb.miss_gbuffer(cam, w, h)
    g[:6] = top[:6]
    col = np.ones((h, w, 4), F)
    col[:6, :, :3] = 3.0
    p = sb.filter_params(iterations=4, sigma_color=0.0, sigma_normal=0.0, sigma_plane=0.0)
    out, _ = sb.denoise_variance(col, np.full((h, w), 0.1, F), g, p)
    assert np.abs(out - col).max() <= 1e-6


def test_synthetic_cases_exercise_every_branch():
    for (w, h) in sb.KERNEL_SIZES[2:]:
        m, length, g = sb.variance_case(w, h)
        _, counted = sb.variance(m, length, g, tb.params(), sb.SPATIAL_BELOW, want_counted=True)
        win = (length >= 1) & (length < 4)
        assert win.any() and (length >= 4).any() and (~(length >= 1)).any() and (length == 4.0).any()
        assert (counted[win] >= 1).all() and counted[win].min() == 1 and counted[win].max() > 8 and (counted[~win] == 0).all()
        col, var, g = sb.filter_case(w, h)
        miss = g["primitive"] == sb.MISS
        assert miss.any() and (~miss).any() and (miss[:, 1:] != miss[:, :-1]).any()
        assert ((g["n"] == 0).all(axis=2) & ~miss).any() and (g["t"][~miss] > 0).all()
        assert np.isnan(var).any() and (var < 0).any() and np.isinf(var).any() and (var == 0).any()
        out, vout = sb.checked_filter(w, h, 0)
        assert not (out == -7.0).any() and not (vout == -7.0).any()
    cur, g, prev, cam = sb.moments_case(65, 33)
    _, length, _ = sb.accumulate_moments(cur, g, prev, cam, 2.0, tb.params())
    assert (length == 0).any() and (length == 1).any() and (length > 1).any()


# ---- 4. the default parameters on the oracle's own frames

def test_default_parameters_reduce_the_error(rt):
    """DESIGN.md's 16-frame camera path on C3 (here at 160x90), 1 spp a frame by the oracle, the last frame against a
    256-spp frame at the last camera: with the recorded defaults the filtered history's tonemapped RMSE is below the
    unfiltered history's.  Measured here: history 0.0914, filtered 0.0808 (DESIGN.md has the table at 480x270)."""
    case = sb.path_case("c3", 160, 90)
    hist, length, mom, g = sb.run_path(case, rt.default_temporal_params())
    var = sb.variance(mom, length, g, rt.default_temporal_params(), rt.abi.RT_TEMPORAL_SPATIAL_BELOW_DEFAULT)
    out, _ = sb.denoise_variance(hist, var, g, rt.default_denoise_variance_params())
    ref = case[3]
    e_raw, e_hist, e_out = sb.tm_rmse(case[1][-1], ref), sb.tm_rmse(hist, ref), sb.tm_rmse(out, ref)
    print(f"c3 160x90: raw {e_raw:.4f} history {e_hist:.4f} filtered {e_out:.4f} ratio {e_out/e_hist:.3f}")
    assert e_out < e_hist


# ---- 5. the entries that need no device, and the refusals by name

def last_error(rt):
    return (rt.lib().rt_last_error() or b"").decode()


def test_default_params_sizes_and_workspaces(rt):
    assert rt.lib().rt_abi_version() == 8
    p = rt.default_denoise_variance_params()
    assert C.sizeof(p) == 32 and C.sizeof(rt.abi.TemporalFilteredState) == C.sizeof(rt.abi.TemporalState)
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_plane, p.variance_epsilon, p.firefly_clamp) == \
        (4, F(4.0), F(0.2), F(0.02), F(0.03), 10.0)
    assert list(p.reserved) == [0, 0]
    assert rt.denoise_variance_workspace_bytes(1920, 1080) == 1920*1080*40
    assert rt.temporal_filtered_workspace_bytes(1920, 1080) == 1920*1080*180
    assert rt.lib().rt_denoise_variance_default_params(None) == rt.abi.RT_ERROR_INVALID and "null out" in last_error(rt)


def test_struct_layouts_match_the_header(tmp_path, rt):
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_denoise_variance_params), '
                   'offsetof(rt_denoise_variance_params, variance_epsilon), sizeof(rt_temporal_filtered_state), '
                   'offsetof(rt_temporal_filtered_state, lens_distortion), offsetof(rt_temporal_filtered_state, d_workspace)); '
                   'return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(sb.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    a = rt.abi
    assert got == [C.sizeof(a.DenoiseVarianceParams), a.DenoiseVarianceParams.variance_epsilon.offset,
                   C.sizeof(a.TemporalFilteredState), a.TemporalFilteredState.lens_distortion.offset,
                   a.TemporalFilteredState.d_workspace.offset]


def _refusal(rt, entry, call, text):
    code = call()
    assert code == rt.abi.RT_ERROR_INVALID, (entry, text, code)
    msg = last_error(rt)
    assert msg.startswith(entry + ":") and text in msg, (entry, text, msg)


def TP(rt, **kw):
    p = rt.default_temporal_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def FP(rt, **kw):
    p = rt.default_denoise_variance_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_accumulate_moments_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    fp, gp = C.POINTER(C.c_float), C.POINTER(rt.abi.GBufferTexel)
    cur, hist, ph = (np.zeros((h, w, 4), F) for _ in range(3))
    length, pl = (np.zeros((h, w), F) for _ in range(2))
    mom, pm = (np.zeros((h, w, 2), F) for _ in range(2))
    g, pg = (np.zeros((h, w), tb.dtype()) for _ in range(2))
    cam = tb.make_camera()
    f = lambda a: a.ctypes.data_as(fp)
    G = lambda a: a.ctypes.data_as(gp)
    base = dict(current=f(cur), gbuffer=G(g), prev_history=f(ph), prev_length=f(pl), prev_gbuffer=G(pg), prev_moments=f(pm),
                prev_camera=C.byref(cam), w=w, h=h, p=rt.default_temporal_params(), history=f(hist), length=f(length),
                moments=f(mom))

    def refused(entry, prefix, text, **change):
        a = dict(base, **change)
        p = a["p"]
        call = lambda: getattr(lib, entry)(0, a["current"], a["gbuffer"], a["prev_history"], a["prev_length"], a["prev_gbuffer"],
                                           a["prev_moments"], a["prev_camera"], 0.0, a["w"], a["h"],
                                           None if p is None else C.byref(p), a["history"], a["length"], a["moments"],
                                           *(() if entry == "rt_temporal_accumulate_moments" else (None,)))
        _refusal(rt, entry, call, text.replace("@", prefix))

    for entry, prefix in (("rt_temporal_accumulate_moments", ""), ("rt_temporal_accumulate_moments_device", "d_")):
        for name in ("current", "gbuffer", "history", "length", "moments"):
            refused(entry, prefix, f"null @{name}", **{name: None})
        refused(entry, prefix, "null rt_temporal_params", p=None)
        refused(entry, prefix, "w is 0", w=0)
        refused(entry, prefix, "h is 0", h=0)
        for name in ("prev_history", "prev_length", "prev_gbuffer", "prev_moments"):      # some but not all of the four
            refused(entry, prefix, f"null @{name} beside other previous buffers", **{name: None})
        refused(entry, prefix, "null @prev_history beside other previous buffers", prev_history=None, prev_length=None,
                prev_gbuffer=None)                                                         # the moments alone
        refused(entry, prefix, "null prev_camera", prev_camera=None)
        refused(entry, prefix, "@history aliases @prev_history", history=f(ph))
        refused(entry, prefix, "@length aliases @prev_length", length=f(pl))
        refused(entry, prefix, "@moments aliases @prev_moments", moments=f(pm))
        for bad in (0.5, float("nan"), float("inf")):
            refused(entry, prefix, "max_history", p=TP(rt, max_history=bad))
        refused(entry, prefix, "normal_cos", p=TP(rt, normal_cos=1.5))
        for field in ("plane_tolerance", "snap", "firefly_clamp"):
            for bad in (-0.1, float("nan"), float("inf")):
                refused(entry, prefix, field, p=TP(rt, **{field: bad}))


def test_variance_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    fp, gp = C.POINTER(C.c_float), C.POINTER(rt.abi.GBufferTexel)
    mom = np.zeros((h, w, 2), F)
    length, var = (np.zeros((h, w), F) for _ in range(2))
    g = np.zeros((h, w), tb.dtype())
    f = lambda a: a.ctypes.data_as(fp)
    base = dict(moments=f(mom), length=f(length), gbuffer=g.ctypes.data_as(gp), w=w, h=h, p=rt.default_temporal_params(),
                below=4.0, variance=f(var))

    def refused(entry, prefix, text, **change):
        a = dict(base, **change)
        p = a["p"]
        call = lambda: getattr(lib, entry)(0, a["moments"], a["length"], a["gbuffer"], a["w"], a["h"],
                                           None if p is None else C.byref(p), a["below"], a["variance"],
                                           *(() if entry == "rt_temporal_variance" else (None,)))
        _refusal(rt, entry, call, text.replace("@", prefix))

    for entry, prefix in (("rt_temporal_variance", ""), ("rt_temporal_variance_device", "d_")):
        for name in ("moments", "length", "gbuffer", "variance"):
            refused(entry, prefix, f"null @{name}", **{name: None})
        refused(entry, prefix, "null rt_temporal_params", p=None)
        refused(entry, prefix, "w is 0", w=0)
        refused(entry, prefix, "h is 0", h=0)
        refused(entry, prefix, "normal_cos", p=TP(rt, normal_cos=float("nan")))
        refused(entry, prefix, "plane_tolerance", p=TP(rt, plane_tolerance=-1.0))
        for bad in (-1.0, float("nan"), float("inf")):
            refused(entry, prefix, "spatial_below", below=bad)
        refused(entry, prefix, "@variance aliases @moments", variance=f(mom))
        refused(entry, prefix, "@variance aliases @length", variance=f(length))
        refused(entry, prefix, "@variance aliases @gbuffer", variance=C.cast(g.ctypes.data_as(gp), fp))


def test_filter_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    fp, gp = C.POINTER(C.c_float), C.POINTER(rt.abi.GBufferTexel)
    col, out = (np.zeros((h, w, 4), F) for _ in range(2))
    var, vout = (np.zeros((h, w), F) for _ in range(2))
    g = np.zeros((h, w), tb.dtype())
    f = lambda a: a.ctypes.data_as(fp)
    gf = C.cast(g.ctypes.data_as(gp), fp)
    base = dict(color=f(col), variance=f(var), gbuffer=g.ctypes.data_as(gp), w=w, h=h, p=rt.default_denoise_variance_params(),
                out=f(out), variance_out=f(vout))

    def refused(entry, prefix, text, **change):
        a = dict(base, **change)
        p = a["p"]
        dev = entry.endswith("_device")
        call = lambda: getattr(lib, entry)(0, a["color"], a["variance"], a["gbuffer"], a["w"], a["h"],
                                           None if p is None else C.byref(p), *((None,) if dev else ()), a["out"],
                                           a["variance_out"], *((None,) if dev else ()))
        _refusal(rt, entry, call, text.replace("@", prefix))

    for entry, prefix in (("rt_denoise_variance", ""), ("rt_denoise_variance_device", "d_")):
        for name in ("color", "variance", "gbuffer", "out"):
            refused(entry, prefix, f"null @{name}", **{name: None})
        refused(entry, prefix, "null rt_denoise_variance_params", p=None)
        refused(entry, prefix, "w is 0", w=0)
        refused(entry, prefix, "h is 0", h=0)
        for bad in (0, 9, -1):
            refused(entry, prefix, "iterations must be in 1..8", p=FP(rt, iterations=bad))
        for field in ("sigma_color", "sigma_normal", "sigma_plane", "firefly_clamp"):
            for bad in (-0.1, float("nan"), float("inf")):
                refused(entry, prefix, field + " must be finite and >= 0", p=FP(rt, **{field: bad}))
        for bad in (0.0, -1e-3, float("nan"), float("inf")):
            refused(entry, prefix, "variance_epsilon must be finite and > 0", p=FP(rt, variance_epsilon=bad))
        refused(entry, prefix, "@out aliases @variance", out=f(var))
        refused(entry, prefix, "@out aliases @gbuffer", out=gf)
        refused(entry, prefix, "@variance_out aliases @color", variance_out=f(col))
        refused(entry, prefix, "@variance_out aliases @gbuffer", variance_out=gf)
        refused(entry, prefix, "@variance_out aliases @out", variance_out=f(out))
    dev = lambda **kw: lib.rt_denoise_variance_device(0, kw.get("c", f(col)), f(var), kw.get("g", g.ctypes.data_as(gp)),
                                                      kw.get("w", w), h, C.byref(base["p"]), kw.get("ws"), f(out), None, None)
    _refusal(rt, "rt_denoise_variance_device", lambda: dev(w=70000), "larger than 65535")
    _refusal(rt, "rt_denoise_variance_device", lambda: dev(g=C.c_void_p(g.ctypes.data + 4)), "d_gbuffer is not 16-byte aligned")
    _refusal(rt, "rt_denoise_variance_device", lambda: dev(ws=C.c_void_p(72)), "d_workspace is not 16-byte aligned")


def test_driver_refusals_by_name(rt):
    w, h = 4, 3
    lib = rt.lib()
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    out = np.zeros((h, w, 4), F)
    fp = C.POINTER(C.c_float)
    fake_scene = C.c_void_p(0)                       # the scene is checked last: nothing before it needs one
    state = rt.abi.TemporalFilteredState()
    state.d_workspace = 64                           # never followed: every call below is refused first
    base = dict(camera=C.byref(cam), settings=C.byref(st), filter=C.byref(fc), tiles=C.byref(tiles), w=w, h=h,
                p=rt.default_temporal_params(), below=4.0, fp=rt.default_denoise_variance_params(), state=state,
                out=out.ctypes.data_as(fp))

    def drv(entry, text, **change):
        a = dict(base, **change)
        p, q, s = a["p"], a["fp"], a["state"]
        dev = entry.endswith("_device")
        call = lambda: getattr(lib, entry)(fake_scene, a["camera"], a["settings"], a["filter"], a["tiles"], 0, a["w"], a["h"], 0,
                                           None if p is None else C.byref(p), a["below"], None if q is None else C.byref(q),
                                           None if s is None else C.byref(s), a["out"], None, None, None,
                                           *((None,) if dev else ()), None)
        _refusal(rt, entry, call, text)

    for entry, out_name in (("rt_render_temporal_filtered", "out_pixels"), ("rt_render_temporal_filtered_device", "d_out")):
        drv(entry, "null rt_temporal_params", p=None)
        drv(entry, "max_history", p=TP(rt, max_history=0.0))
        drv(entry, "spatial_below", below=float("nan"))
        drv(entry, "null rt_denoise_variance_params", fp=None)
        drv(entry, "variance_epsilon", fp=FP(rt, variance_epsilon=0.0))
        drv(entry, "iterations", fp=FP(rt, iterations=0))
        drv(entry, "null rt_temporal_filtered_state", state=None)
        drv(entry, "null d_workspace", state=rt.abi.TemporalFilteredState())
        bad = rt.abi.TemporalFilteredState()
        bad.d_workspace, bad.parity = 64, 2
        drv(entry, "parity must be 0 or 1", state=bad)
        drv(entry, "null settings", settings=None)
        drv(entry, "w is 0", w=0)
        drv(entry, "h is 0", h=0)
        drv(entry, "null camera", camera=None)
        drv(entry, "null filter", filter=None)
        drv(entry, "null tiles", tiles=None)
        drv(entry, "null " + out_name, out=None)
        drv(entry, "null scene")
    assert (state.frames, state.parity, state.w, state.h) == (0, 0, 0, 0)


def test_host_entries_need_a_device_after_their_checks(rt):
    w, h = 5, 3
    cur, g, prev, cam = sb.moments_case(w, h)
    m, length, gv = sb.variance_case(w, h)
    col, var, gf = sb.filter_case(w, h)
    calls = [lambda: rt.temporal_accumulate_moments(cur, g, prev, cam, 2.0), lambda: rt.temporal_variance(m, length, gv),
             lambda: rt.denoise_variance(col, var, gf)]
    for call in calls:
        if rt.device_count() > 0:
            call()
        else:
            with pytest.raises(rt.RenderError) as e:
                call()
            assert e.value.code == rt.abi.RT_ERROR_NO_DEVICE
    # a bad argument is refused first, with or without one
    with pytest.raises(rt.RenderError) as e:
        rt.denoise_variance(col, var, gf, FP(rt, variance_epsilon=0.0))
    assert e.value.code == rt.abi.RT_ERROR_INVALID
