"""The robust estimator without a device ("The robust estimator"): the plain-C checker tests/ref_robust
against an independent numpy float32 restatement, bit for bit; hand-worked known answers; properties against
float64; and every refusal of the new entries, which are raised by name before the device is touched.

The bounds of the float64 comparisons, with u = 2^-24 (f32 unit roundoff), first order in u:

* The pooled mean (gini_scale = 0) of n valid buffers with radiance sums >= 0.  A sum of n non-negative terms added
  in a chain carries a relative error <= (n-1)u; numerator and denominator each do, and the division adds u:
  <= (2n-1)u = (n - 1/2) 2^-23 < n 2^-23 relative, per channel.  (With sums of both signs a channel can cancel and
  no relative bound holds, so the pixels compared are those whose valid buffers are all >= 0.)
* The Gini coefficient G = 2T/(nS) - (n+1)/n of the same f32 keys g_i >= 0.  S: n-1 additions, relative (n-1)u.
  T: each product (i+1) g_i rounds once and the chain adds n-1 times, relative n u.  2T is exact, (float)n S and
  the division round once each: A = 2T/(nS) is off by (2n+1)u relative, and A <= 2 because T <= nS.  (n+1)/n <= 4/3
  rounds once, the subtraction once with a result < 1.  |G32 - G64| <= (2(2n+1) + 4/3 + 1)u < (4n + 5)u.  The
  clamp to >= 0 is a contraction.  The test doubles the bound for the terms of second order.
"""
import ctypes as C

import numpy as np
import pytest

import ref_robust_binding as rr

F = np.float32
U = 2.0**-24


# ---- 1. the checker against numpy float32, bit for bit

@pytest.mark.parametrize("K", rr.COUNTS)
@pytest.mark.parametrize("w,h", rr.SIZES)
def test_checker_against_numpy(w, h, K):
    stack = rr.synthetic_stack(w, h, K)
    for gs, mt in ((1.0, 15), (2.0, 15), (1.0, 1), (0.0, 15)):
        out, info = (rr.checked(w, h, K) if (gs, mt) == (1.0, 15) else rr.combine(stack, rr.params(gs, mt)))
        want_out, want_info, _ = rr.numpy_combine(stack, gs, mt)
        assert np.array_equal(rr.bits(out), rr.bits(want_out)), (gs, mt)
        assert np.array_equal(rr.bits(info), rr.bits(want_info)), (gs, mt)
    # the info buffer is optional, and the output does not depend on it
    alone, none = rr.combine(stack, rr.params(), want_info=False)
    assert none is None and np.array_equal(rr.bits(alone), rr.bits(rr.checked(w, h, K)[0]))


def test_the_synthetic_stacks_hold_every_kind_of_pixel():
    """What the stacks promise, on the largest: trimmed and untrimmed pixels, pixels without a valid buffer that pass
    buffer 0's NaN or negative weight through, buffer 0 invalid beside valid others, every special slot."""
    K = 16
    stack = rr.synthetic_stack(65, 33, K)
    out, info = rr.checked(65, 33, K)
    n, c = info[..., 2], info[..., 1]
    assert (c > 0).any() and (c == 0).any() and (n == K).any() and (n == 0).any() and ((n > 0) & (n < K)).any()
    dead = n == 0
    assert np.array_equal(rr.bits(out[dead]), rr.bits(stack[0][dead]))
    assert np.isnan(out[dead]).any() and (out[dead][:, 3] < 0).any()
    assert ((stack[0, ..., 3] == 0) & (n > 0)).any()
    assert (out[~dead][:, 3] == 1.0).all() and np.isfinite(out[~dead]).all()
    w = stack[..., 3]
    assert (w == F(0.001)).any() and (w == np.nextafter(F(0.001), F(1))).any() and np.isinf(stack).any()
    assert (np.signbit(stack[..., 0]) & (stack[..., 0] == 0)).any()
    assert (stack[..., :3].astype(np.float64).sum(axis=3) < 0).any()
    assert ((info[..., 0] == 0) & (n >= 3)).any()                     # all-zero keys: S = 0, G = 0


# ---- 2. known answers, worked by hand

def _stack_of_keys(keys, weight=1.0):
    """One pixel; buffer k holds a grey-free radiance (key, 0, 0) with the given weight."""
    s = np.zeros((len(keys), 1, 1, 4), np.float32)
    s[:, 0, 0, 0] = np.asarray(keys, np.float32)*F(weight)
    s[:, 0, 0, 3] = weight
    return s


def test_five_buffers_one_outlier():
    # keys 1 1 100 1 1 (the outlier in buffer 2): ranked 1 1 1 1 100, S = 104, T = 1 + 2 + 3 + 4 + 5*100 = 510,
    # G = 2*510/(5*104) - 6/5 = 1020/520 - 6/5 = 0.7615..., x = 1 * G * 5/2 = 1.90 -> c = 1 (cmax = (5-1)/2 = 2);
    # kept ranks 1..3 are three buffers of key 1: the output is exactly 1, the kept weight 3.
    out, info = rr.combine(_stack_of_keys([1, 1, 100, 1, 1]))
    G = F(F(1020)/F(520) - F(6)/F(5))
    assert rr.bits(info[0, 0, 0]) == rr.bits(G) and 0.76 < G < 0.77
    assert info[0, 0].tolist()[1:] == [1.0, 5.0, 3.0]
    assert out[0, 0].tolist() == [1.0, 0.0, 0.0, 1.0]
    # gini_scale 2: x = 3.8 >= cmax = 2 -> c = 2, the median alone
    out, info = rr.combine(_stack_of_keys([1, 1, 100, 1, 1]), rr.params(2.0))
    assert info[0, 0].tolist()[1:] == [2.0, 5.0, 1.0] and out[0, 0, 0] == 1.0
    # max_trim = 0 and gini_scale = 0 each give the pooled mean, 104/5
    for p in (rr.params(1.0, 0), rr.params(0.0, 15)):
        out, info = rr.combine(_stack_of_keys([1, 1, 100, 1, 1]), p)
        assert rr.bits(out[0, 0, 0]) == rr.bits(F(104)/F(5)) and info[0, 0].tolist()[1:] == [0.0, 5.0, 5.0]
    assert rr.bits(info[0, 0, 0]) == rr.bits(G)                       # G is reported whatever the scale


def test_eight_equal_buffers():
    # keys 0.75 each: S = 6, T = 0.75*36 = 27 (every partial sum exact), 2T/(nS) = 54/48 = 1.125 = 9/8: G = 0 exactly
    s = np.zeros((8, 1, 1, 4), np.float32)
    s[:, 0, 0] = (0.25, 0.25, 0.25, 1.0)
    out, info = rr.combine(s, rr.params(1000.0))
    assert info[0, 0].tolist() == [0.0, 0.0, 8.0, 8.0]
    assert out[0, 0].tolist() == [0.25, 0.25, 0.25, 1.0]


def test_two_valid_buffers_never_trim():
    # n = 2: G = 0 by definition and cmax = (2-1)/2 = 0, whatever the scale
    for keys, K in (([1, 1e6], 2), ([np.nan, 1, np.inf, 1e6, np.nan], 5)):
        s = _stack_of_keys(keys)
        out, info = rr.combine(s, rr.params(1e6))
        assert info[0, 0].tolist() == [0.0, 0.0, 2.0, 2.0]
        assert rr.bits(out[0, 0, 0]) == rr.bits((F(1) + F(1e6))/F(2))


def test_weights_pool_and_ties_rank_by_index():
    # keys 2 2 2 with weights 1 2 4 and one key 50 (weight 1) in buffer 1: ranked b0 b2 b3 b1.
    # S = 56, T = 2 + 4 + 6 + 200 = 212, G = 424/224 - 5/4 = 0.642..., x = G*2 = 1.28 -> c = 1 = cmax;
    # kept ranks 1..2 = buffers 2 and 3 (the tie broke by index: buffer 0 went first): (4 + 8)/(2 + 4) = 2, weight 6.
    s = np.zeros((4, 1, 1, 4), np.float32)
    for k, (key, wt) in enumerate(((2, 1), (50, 1), (2, 2), (2, 4))):
        s[k, 0, 0] = (key*wt, 0, 0, wt)
    out, info = rr.combine(s)
    assert rr.bits(info[0, 0, 0]) == rr.bits(F(F(424)/F(224) - F(5)/F(4)))
    assert info[0, 0].tolist()[1:] == [1.0, 4.0, 6.0] and out[0, 0].tolist() == [2.0, 0.0, 0.0, 1.0]


def test_a_sum_that_overflows():
    # keys 0 0 1e38: S = 1e38 and nS = 3e38 are finite, T = 3e38, 2T = +inf: G = +inf.  gini_scale 1: x = +inf >= cmax,
    # c = 1, the median 0.  gini_scale 0: x = 0*inf = NaN, which trims nothing: the pooled mean.
    s = _stack_of_keys([0, 0, 1e38])
    out, info = rr.combine(s)
    assert np.isposinf(info[0, 0, 0]) and info[0, 0].tolist()[1:] == [1.0, 3.0, 1.0] and out[0, 0, 0] == 0.0
    out, info = rr.combine(s, rr.params(0.0))
    assert np.isposinf(info[0, 0, 0]) and info[0, 0].tolist()[1:] == [0.0, 3.0, 3.0]
    assert rr.bits(out[0, 0, 0]) == rr.bits(F(1e38)/F(3))
    # keys 2e38 2e38 2e38: S = +inf, not finite: G = 0
    out, info = rr.combine(_stack_of_keys([2e38, 2e38, 2e38]))
    assert info[0, 0].tolist()[:3] == [0.0, 0.0, 3.0]


def test_negative_keys_rank_first_and_count_as_zero():
    # keys -5 1 1 1 100: g = 0 1 1 1 100, S = 103, T = 2 + 3 + 4 + 500 = 509, G = 1018/515 - 6/5 = 0.776..., c = 1:
    # the negative buffer and the outlier are dropped
    out, info = rr.combine(_stack_of_keys([1, 100, 1, -5, 1]))
    assert rr.bits(info[0, 0, 0]) == rr.bits(F(F(1018)/F(515) - F(6)/F(5)))
    assert info[0, 0].tolist()[1:] == [1.0, 5.0, 3.0] and out[0, 0, 0] == 1.0


# ---- 3. properties against float64

def _valid64(stack):
    s64 = stack.astype(np.float64)
    with np.errstate(all="ignore"):
        m = stack[..., :3]/stack[..., 3:]
        key = (m[..., 0] + m[..., 1]) + m[..., 2]
        valid = (stack[..., 3] > F(0.001)) & np.isfinite(stack).all(axis=-1) & np.isfinite(m).all(axis=-1) & np.isfinite(key)
    return s64, key, valid


@pytest.mark.parametrize("K", [3, 8, 17, 32])
def test_scale_zero_is_the_pooled_mean(K):
    stack = rr.synthetic_stack(65, 33, K)
    out, info = rr.combine(stack, rr.params(0.0))
    s64, _, valid = _valid64(stack)
    n = valid.sum(axis=0)
    assert np.array_equal(info[..., 2], n.astype(np.float32)) and (info[..., 1] == 0).all()
    pooled = np.where(valid[..., None], s64, 0.0).sum(axis=0)
    positive = (n > 0) & np.where(valid[..., None], stack[..., :3] >= 0, True).all(axis=(0, 3))
    assert positive.sum() > 0.6*positive.size
    want = pooled[..., :3]/np.where(n > 0, pooled[..., 3], 1.0)[..., None]
    err = np.abs(out[..., :3].astype(np.float64) - want)
    bound = (n*2.0**-23)[..., None]*np.abs(want)
    assert (err[positive] <= bound[positive]).all(), float((err[positive]/np.maximum(bound[positive], 1e-300)).max())
    assert (np.abs(info[..., 3].astype(np.float64) - pooled[..., 3])[positive] <= (n*U*pooled[..., 3])[positive]).all()


@pytest.mark.parametrize("K", [3, 8, 17, 32])
def test_gini_against_float64(K):
    stack = rr.synthetic_stack(65, 33, K)
    _, info = rr.checked(65, 33, K)
    _, key, valid = _valid64(stack)
    g = np.where(valid & (key > 0), key, 0).astype(np.float64)          # the same f32 keys, in float64 from here
    g = np.sort(np.where(valid, g, np.inf), axis=0)                      # negative keys are 0: they tie with the zeros
    n = valid.sum(axis=0)
    ranks = np.arange(1, K + 1, dtype=np.float64)[:, None, None]
    live = ranks <= n
    g = np.where(live, g, 0.0)
    S, T = g.sum(axis=0), (ranks*g).sum(axis=0)
    use = (n >= 3) & (S > 0) & (g.max(axis=0) < 1e30)
    assert use.sum() > 0.6*use.size
    with np.errstate(all="ignore"):
        G64 = np.maximum(2*T/(n*S) - (n + 1)/n, 0.0)
    err = np.abs(info[..., 0].astype(np.float64) - G64)[use]
    bound = (2*(4*n + 5)*U)[use]
    print("G: max error", err.max(), "of a bound of", bound.max())
    assert (err <= bound).all()
    assert (info[..., 0][use] < 1.0).all() and (G64[use] > 0.3).any()


@pytest.mark.parametrize("K", [8, 16])
def test_a_permutation_keeps_the_trim_and_the_kept_set(K):
    """Weights of 1 and integer radiance make every sum exact whatever its order.  Buffer k of a pixel is named by a
    label: r = 65536 v with the v pairwise distinct in 0..15, b = 2^label.  The keys r + b are pairwise distinct, and
    out.b * weight is the bit set of the kept labels, exactly."""
    rng = np.random.default_rng(K)
    npx = 200
    v = np.stack([rng.permutation(16)[:K] for _ in range(npx)], axis=1)            # (K, npx)
    v[K - 1, ::3] = 15*8                                                             # an outlier in a third of the pixels
    labels = np.arange(K)[:, None]
    s = np.zeros((K, 1, npx, 4), np.float32)
    s[:, 0, :, 0] = 65536.0*v
    s[:, 0, :, 2] = 2.0**labels
    s[:, 0, :, 3] = 1.0
    out, info = rr.combine(s)
    assert (info[..., 1] > 0).any() and len(np.unique(info[..., 1])) > 1
    kept = np.rint(out[..., 2].astype(np.float64)*info[..., 3]).astype(np.int64)
    assert (np.array([bin(x).count("1") for x in kept.ravel()]) == (K - 2*info[..., 1]).ravel()).all()
    for _ in range(3):
        perm = rng.permutation(K)
        out_p, info_p = rr.combine(s[perm])
        assert np.array_equal(info_p[..., 1], info[..., 1])                          # c
        assert np.array_equal(np.rint(out_p[..., 2].astype(np.float64)*info_p[..., 3]).astype(np.int64), kept)
        assert np.array_equal(rr.bits(out_p), rr.bits(out)) and np.array_equal(rr.bits(info_p), rr.bits(info))


# ---- 4. refusals, by name, before the device is touched (no scene exists without a device: the scene is NULL)

def _last(rt):
    return (rt.lib().rt_last_error() or b"").decode()


def _robust_params(rt, **kw):
    p = rt.default_robust_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _combine(rt, entry, stack=True, count=8, w=4, h=4, p="ok", out=True):
    pp = rt.default_robust_params() if p == "ok" else p
    pref = C.byref(pp) if pp is not None else None
    if entry == "device":
        return rt.lib().rt_robust_combine_device(0, C.c_void_p(0x1000) if stack else None, count, w, h, pref,
                                                 C.c_void_p(0x2000) if out else None, None, None)
    fp = C.POINTER(C.c_float)
    buf = np.ones((32, 4, 4, 4), np.float32)
    o = np.zeros((4, 4, 4), np.float32)
    return rt.lib().rt_robust_combine(0, buf.ctypes.data_as(fp) if stack else None, count, w, h, pref,
                                      o.ctypes.data_as(fp) if out else None, None)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_combine_refusals(rt, entry):
    name = "rt_robust_combine_device" if entry == "device" else "rt_robust_combine:"
    cases = [(dict(stack=False), "null stack"), (dict(p=None), "null rt_robust_params"), (dict(out=False), "null out"),
             (dict(w=0), "w is 0"), (dict(h=0), "h is 0"), (dict(count=0), "count"), (dict(count=1), "count"),
             (dict(count=33), "count")]
    cases += [(dict(p=_robust_params(rt, gini_scale=v)), "gini_scale") for v in (-0.5, float("nan"), float("inf"))]
    for kw, word in cases:
        assert _combine(rt, entry, **kw) == rt.abi.RT_ERROR_INVALID, kw
        assert word in _last(rt) and _last(rt).startswith(name), (kw, _last(rt))
    if rt.device_count() == 0:                              # every argument good: only the device is missing
        assert _combine(rt, "host") == rt.abi.RT_ERROR_NO_DEVICE


def _driver(rt, entry, p="ok", spp=8, w=130, h=70, camera=True, settings=True, filt=True, out=True, post=True, shard=(0, 1)):
    cam, st, fc, ps = rt.abi.Camera(), rt.abi.Settings(), rt.abi.FilterCache(), rt.abi.PostSettings()
    tiles = rt.abi.TileSet(64, 64, *shard) if shard is not None else None
    tiles_r = C.byref(tiles) if tiles is not None else None
    st.samples_per_pixel = spp
    pp = rt.default_robust_params() if p == "ok" else p
    pref = C.byref(pp) if pp is not None else None
    cam_r, st_r, fc_r = (C.byref(cam) if camera else None, C.byref(st) if settings else None, C.byref(fc) if filt else None)
    if entry == "device":
        return rt.lib().rt_render_robust_device(None, cam_r, st_r, fc_r, tiles_r, 0, w, h, 0, pref, None,
                                                C.c_void_p(0x1000) if out else None, None, None, None)
    if entry == "host":
        px = np.zeros((max(h, 1), max(w, 1), 4), np.float32)
        return rt.lib().rt_render_robust(None, cam_r, st_r, fc_r, tiles_r, 0, w, h, 0, pref,
                                         px.ctypes.data_as(C.POINTER(C.c_float)) if out else None, None, None)
    pic = np.zeros((max(h, 1), max(w, 1)), np.uint32)
    return rt.lib().rt_render_picture_robust(None, cam_r, st_r, fc_r, tiles_r, 0, w, h, C.byref(ps) if post else None,
                                             pref, None, 0, pic.ctypes.data_as(C.POINTER(C.c_uint32)) if out else None, None)


@pytest.mark.parametrize("entry", ["device", "host", "picture"])
def test_driver_refusals(rt, entry):
    name = {"device": "rt_render_robust_device", "host": "rt_render_robust:", "picture": "rt_render_picture_robust"}[entry]
    out_word = {"device": "null d_out", "host": "null out", "picture": "null out_bgra"}[entry]
    cases = [(dict(p=None), "null rt_robust_params"), (dict(camera=False), "null camera"), (dict(settings=False), "null settings"),
             (dict(filt=False), "null filter"), (dict(out=False), out_word), (dict(w=0), "w is 0"), (dict(h=0), "h is 0"),
             (dict(spp=0), "samples_per_pixel"), (dict(spp=12), "samples_per_pixel"),             # 12 is no multiple of 8
             (dict(p=_robust_params(rt, buffers=5), spp=8), "samples_per_pixel"),
             (dict(shard=None), "null tiles"), (dict(shard=(1, 2)), "shard_count"), (dict(shard=(0, 0)), "shard_count"),
             (dict(), "null scene")]                                                            # all else good: the scene
    cases += [(dict(p=_robust_params(rt, buffers=v), spp=66), "buffers") for v in (0, 1, 33)]
    cases += [(dict(p=_robust_params(rt, gini_scale=v)), "gini_scale") for v in (-1.0, float("nan"), float("inf"))]
    if entry == "picture":
        cases.append((dict(post=False), "null post"))
    for kw, word in cases:
        assert _driver(rt, entry, **kw) == rt.abi.RT_ERROR_INVALID, kw
        assert word in _last(rt) and _last(rt).startswith(name), (kw, _last(rt))


def test_the_checker_makes_the_same_refusals(rt):
    fp = C.POINTER(C.c_float)
    buf, o = np.ones((32, 4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32)
    good = dict(stack=buf.ctypes.data_as(fp), count=8, w=4, h=4, p=rr.params(), out=o.ctypes.data_as(fp))

    def call(**kw):
        a = dict(good, **kw)
        return rr.load().ref_robust_combine(0, a["stack"], a["count"], a["w"], a["h"], C.byref(a["p"]) if a["p"] is not None else None,
                                            a["out"], None)
    assert call() == 0
    bad = [dict(stack=None), dict(p=None), dict(out=None), dict(w=0), dict(h=0), dict(count=0), dict(count=1), dict(count=33)]
    bad += [dict(p=rr.params(v)) for v in (-0.5, float("nan"), float("inf"))]
    for kw in bad:
        assert call(**kw) == rt.abi.RT_ERROR_INVALID, kw


def test_defaults_and_layouts(rt):
    """No device needed: the defaults, the workspace size and the ctypes mirror's size."""
    p = rt.default_robust_params()
    assert (p.buffers, p.gini_scale, p.max_trim) == (8, 1.0, 15) and list(p.reserved) == [0]*5
    assert C.sizeof(rt.abi.RobustParams) == 32
    assert rt.robust_workspace_bytes(130, 70) == 8*130*70*16 and rt.robust_workspace_bytes(1920, 1080, 32) == 32*1920*1080*16
    assert rt.lib().rt_abi_version() == 8
