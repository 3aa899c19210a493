"""The denoise stage on the CPU: the plain-C checker tests/ref_denoise (which the device must match bit for
bit, tests/test_gpu_denoise.py) against an independent numpy restatement and against the properties the
definition promises ("The denoise stage"), and the library's entries that need no device."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import ref_denoise_binding as rd

F = np.float32
HK = [F(1.0)/F(16.0), F(1.0)/F(4.0), F(3.0)/F(8.0), F(1.0)/F(4.0), F(1.0)/F(16.0)]


def restate(beauty, guide0, guide1, p, expf):
    """The definition in numpy float32 scalars, tap by tap in its order; expf is the oracle's."""
    h, w, _ = beauty.shape
    guides = [guide0, guide1]
    finite = lambda v: bool(np.isfinite(v))
    valid = np.zeros((h, w), bool)
    col = np.zeros((h, w, 3), F)
    lum = np.zeros((h, w), F)
    gres = [np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)]

    def l_of(c):
        y = F(F(F(0.2126)*c[0]) + F(F(0.7152)*c[1])) + F(F(0.0722)*c[2])
        return F(F(1.0) - F(expf(F(-y))))

    with np.errstate(all="ignore"):
        for y, x in itertools.product(range(h), range(w)):
            s = beauty[y, x]
            ok = bool(s[3] > F(0.001))
            c = [F(0), F(0), F(0)]
            if ok:
                c = [F(s[k] / s[3]) for k in range(3)]
                ok = all(finite(v) for v in c)
            for k in range(2):
                if guides[k] is None:
                    continue
                q = guides[k][y, x]
                if q[3] > F(0.001):
                    r = [F(q[j] / q[3]) for j in range(3)]
                    gres[k][y, x] = r
                    ok = ok and all(finite(v) for v in r)
                else:
                    ok = False
            valid[y, x] = ok
            if ok:
                for k in range(3):
                    v = c[k] if c[k] > F(0) else F(0)
                    if p.firefly_clamp > 0:
                        v = v if v < F(p.firefly_clamp) else F(p.firefly_clamp)
                    c[k] = v
                col[y, x] = c
                lum[y, x] = l_of(c)
        inv_g = [F(0), F(0)]
        for k in range(2):
            if p.sigma_guide[k] > 0:
                sg = F(p.sigma_guide[k])
                inv_g[k] = F(F(1.0) / F(sg*sg))
        for it in range(p.iterations):
            s = 1 << it
            inv_c = F(0)
            if p.sigma_color > 0:
                sc = F(F(p.sigma_color)*F(2.0**-it))
                inv_c = F(F(1.0) / F(sc*sc))
            ncol, nlum = np.zeros_like(col), np.zeros_like(lum)
            for y, x in itertools.product(range(h), range(w)):
                if not valid[y, x]:
                    continue
                num = [F(0), F(0), F(0)]
                den = F(0)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + s*dx, y + s*dy
                        if qx < 0 or qx >= w or qy < 0 or qy >= h or not valid[qy, qx]:
                            continue
                        e = F(0)
                        if p.sigma_color > 0:
                            d = F(lum[y, x] - lum[qy, qx])
                            e = F(e + F(F(d*d)*inv_c))
                        for k in range(2):
                            if guides[k] is None or not p.sigma_guide[k] > 0:
                                continue
                            a, b, c = (F(gres[k][y, x, j] - gres[k][qy, qx, j]) for j in range(3))
                            e = F(e + F(F(F(F(a*a) + F(b*b)) + F(c*c))*inv_g[k]))
                        wt = F(F(HK[dy + 2]*HK[dx + 2])*F(expf(F(-e))))
                        for j in range(3):
                            num[j] = F(num[j] + F(wt*col[qy, qx, j]))
                        den = F(den + wt)
                c = [F(num[j] / den) for j in range(3)]
                ncol[y, x] = c
                nlum[y, x] = l_of(c)
            col, lum = ncol, nlum
    out = np.array(beauty, F, copy=True)
    out[valid, :3] = col[valid]
    out[valid, 3] = F(1.0)
    return out


def test_checker_matches_numpy_restatement(oracle):
    """33 x 17 random HDR, 3 iterations, every term on: bit-identical to the restatement above."""
    oracle.oracle_set_math_mode(0)
    beauty, g0, g1 = rd.random_frames(33, 17, seed=11)
    p = rd.params(3, 1.0, (0.1, 0.05), 10.0)
    got = rd.denoise(beauty, g0, g1, p)
    want = restate(beauty, g0, g1, p, lambda v: oracle.oracle_expf(float(v)))
    assert int(np.count_nonzero(rd.bits(got) != rd.bits(want))) == 0
    valid = got[:, :, 3] == 1.0
    assert 0.9 < valid.mean() < 1.0                     # the input has invalid pixels, and not only those


PARAM_SETS = [rd.params(1, 0.0, (0.0, 0.0), 0.0), rd.params(3, 1.0, (0.1, 0.05), 10.0), rd.params(5, 0.5, (0.0, 0.2), 0.0),
              rd.params(8, 2.0, (0.3, 0.0), 1.5), rd.params(2, 0.0, (0.1, 0.05), 10.0)]


@pytest.mark.parametrize("pi", range(len(PARAM_SETS)))
def test_constant_image_stays_constant(pi):
    """A constant valid image stays constant to 1e-6 relative (a quotient of two rounded sums need not be
    exact), whatever the guides hold."""
    p = PARAM_SETS[pi]
    w, h = 37, 21
    _, g0, g1 = rd.random_frames(w, h, seed=5, invalid_fraction=0.0)
    value = np.array([0.7, 0.05, 1.3], F)
    beauty = np.empty((h, w, 4), F)
    beauty[:, :, :3] = value*F(2.0)               # weight 2: the resolve is exact
    beauty[:, :, 3] = 2.0
    if p.firefly_clamp > 0:
        value = np.minimum(value, F(p.firefly_clamp))
    out = rd.denoise(beauty, g0, g1, p)
    assert np.all(out[:, :, 3] == 1.0)
    rel = np.abs(out[:, :, :3].astype(np.float64) - value) / value
    print("constant image: max relative deviation", rel.max())
    assert rel.max() <= 1e-6


def test_all_terms_off_is_the_b3_blur():
    """One iteration with every term off: the border-renormalised separable B3 blur, in float64, to 1e-6."""
    w, h = 29, 23
    beauty, _, _ = rd.random_frames(w, h, seed=2, invalid_fraction=0.0)
    out = rd.denoise(beauty, None, None, rd.params(1, 0.0, (0.0, 0.0), 0.0))
    c = (beauty[:, :, :3] / beauty[:, :, 3:]).astype(F).astype(np.float64)
    k = np.array([1/16, 1/4, 3/8, 1/4, 1/16])

    def blur(a, axis):
        n = a.shape[axis]
        num, den = np.zeros_like(a), np.zeros(n)
        for d in range(-2, 3):
            src = np.arange(n) + d
            ok = (src >= 0) & (src < n)
            idx = np.clip(src, 0, n - 1)
            shape = [1, 1, 1]
            shape[axis] = n
            num += np.take(a, idx, axis=axis)*(k[d + 2]*ok).reshape(shape)
            den += k[d + 2]*ok
        return num, den
    nx, dx = blur(c, 1)
    ny, dy = blur(nx, 0)
    want = ny / (dy[:, None, None]*dx[None, :, None])
    assert np.max(np.abs(out[:, :, :3] - want) / np.maximum(np.abs(want), 1e-30)) < 1e-6
    assert np.all(out[:, :, 3] == 1.0)


def test_no_leak_across_a_guide_edge():
    """Guide values 1.0 apart with sigma_guide 0.05: e = 400 and expf(-400) is exactly 0, so the right half's
    colours cannot reach the left half's output, for 5 iterations."""
    w, h = 40, 18
    beauty, _, _ = rd.random_frames(w, h, seed=7, invalid_fraction=0.0)
    guide = np.zeros((h, w, 4), F)
    guide[:, :, 3] = 2.0
    guide[:, w//2:, 0] = 2.0                      # resolved x: 0 on the left, 1 on the right
    p = rd.params(5, 1.0, (0.05, 0.0), 10.0)
    a = rd.denoise(beauty, guide, None, p)
    other, _, _ = rd.random_frames(w, h, seed=8, invalid_fraction=0.0)
    changed = beauty.copy()
    changed[:, w//2:] = other[:, w//2:]
    b = rd.denoise(changed, guide, None, p)
    assert np.array_equal(rd.bits(a[:, :w//2]), rd.bits(b[:, :w//2]))
    assert not np.array_equal(rd.bits(a[:, w//2:]), rd.bits(b[:, w//2:]))
    # the same through guide 1
    p1 = rd.params(5, 1.0, (0.0, 0.05), 10.0)
    a1, b1 = rd.denoise(beauty, None, guide, p1), rd.denoise(changed, None, guide, p1)
    assert np.array_equal(rd.bits(a1[:, :w//2]), rd.bits(b1[:, :w//2]))


def test_invalid_pixels_pass_through_and_reach_no_neighbour():
    w, h = 31, 19
    beauty, g0, g1 = rd.random_frames(w, h, seed=4, invalid_fraction=0.0)
    spots = {"nan": (3, 4), "inf": (9, 10), "w0": (15, 2), "wneg": (7, 25), "guide": (12, 17)}
    b, a0, a1 = beauty.copy(), g0.copy(), g1.copy()
    b[spots["nan"]] = (np.nan, 1.0, 2.0, 1.0)
    b[spots["inf"]] = (1.0, np.inf, 2.0, 2.0)
    b[spots["w0"]] = (1.0, 2.0, 3.0, 0.0)
    b[spots["wneg"]] = (1.0, 2.0, 3.0, -1.5)
    a1[spots["guide"]] = (0.1, np.nan, 0.2, 1.0)
    p = rd.params(3, 1.0, (0.1, 0.05), 10.0)
    out = rd.denoise(b, a0, a1, p)
    for yx in spots.values():
        assert np.array_equal(rd.bits(out[yx]), rd.bits(b[yx])), yx        # all four floats, bit for bit
    # another invalid value in each spot: every other pixel keeps its bits
    b2, a02 = b.copy(), a0.copy()
    b2[spots["nan"]] = (5.0, 5.0, 5.0, -np.inf)
    b2[spots["inf"]] = (np.nan, np.nan, np.nan, np.nan)
    b2[spots["w0"]] = (9e9, 0.0, 0.0, 0.0005)
    b2[spots["wneg"]] = (3e38, 1.0, 1.0, 0.5)                             # the resolved value overflows
    b2[spots["guide"]] = (123.0, 4.0, 5.0, 1.0)                           # valid beauty, the guide stays invalid
    a02[spots["w0"]] = (0.0, 0.0, 0.0, -1.0)
    out2 = rd.denoise(b2, a02, a1, p)
    mask = np.ones((h, w), bool)
    for yx in spots.values():
        mask[yx] = False
        assert np.array_equal(rd.bits(out2[yx]), rd.bits(b2[yx])), yx
    assert np.array_equal(rd.bits(out[mask]), rd.bits(out2[mask]))
    assert np.all(out[mask][:, 3] == 1.0) and np.all(np.isfinite(out[mask]))


def test_firefly_clamp_comes_before_the_filter():
    w, h = 17, 13
    beauty, g0, g1 = rd.random_frames(w, h, seed=9, invalid_fraction=0.0)
    p = rd.params(3, 1.0, (0.1, 0.05), 10.0)
    hot, ten = beauty.copy(), beauty.copy()
    hot[6, 8] = (1e30, 1e30, 1e30, 1.0)
    ten[6, 8] = (10.0, 10.0, 10.0, 1.0)
    assert np.array_equal(rd.bits(rd.denoise(hot, g0, g1, p)), rd.bits(rd.denoise(ten, g0, g1, p)))
    p0 = rd.params(3, 1.0, (0.1, 0.05), 0.0)                               # and without a clamp it is not
    assert not np.array_equal(rd.bits(rd.denoise(hot, g0, g1, p0)), rd.bits(rd.denoise(ten, g0, g1, p0)))


# ---- usefulness: the default parameters on the oracle's own noisy frames
def _tonemapped_rel_l2(a, ref):
    def tm(x):
        c = np.maximum(x[:, :, :3].astype(np.float64) / x[:, :, 3:].astype(np.float64), 0.0)
        return 1.0 - np.exp(-c)
    return float(np.linalg.norm(tm(a) - tm(ref)) / np.linalg.norm(tm(ref)))


@pytest.mark.parametrize("name,w,h,strict", [("c1", 128, 128, True), ("c3", 160, 90, True), ("c4", 160, 90, False)])
def test_default_parameters_reduce_the_error(rt, name, w, h, strict):
    """4 spp beauty (oracle) + 4 spp normals and distances (tests/ref_integrators), denoised with the default
    parameters, against a 512 spp oracle frame of another total_frame_index: tonemapped rel L2 below the
    noisy frame's on C1 and C3, not above it on C4 (its noise sits behind glass, which first-hit guides do
    not describe).  Measured ratios: C1 0.55, C3 0.50, C4 0.92 in the prototype."""
    import oracle_binding as ob
    import ref_binding as rb
    scene, cam, st, fc, post = rt.load_preset(name, w, h)
    st.samples_per_pixel = 4
    noisy, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=16, total_frame_index=0)
    gst = rt.abi.Settings.from_buffer_copy(st)
    gst.integrator = rt.abi.RT_INTEGRATOR_NORMALS
    normals, _ = rb.render(scene.desc(), cam, gst, fc, w, h, total_frame_index=0)
    gst.integrator = rt.abi.RT_INTEGRATOR_DISTANCES
    distances, _ = rb.render(scene.desc(), cam, gst, fc, w, h, total_frame_index=0)
    st.samples_per_pixel = 512
    ref, _ = ob.render(scene.desc(), cam, st, fc, w, h, rng_mode=0, threads=16, total_frame_index=7)
    den = rd.denoise(noisy, normals, distances, rt.default_denoise_params())
    e_noisy, e_den = _tonemapped_rel_l2(noisy, ref), _tonemapped_rel_l2(den, ref)
    print(f"{name}: noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den/e_noisy:.3f}")
    if strict:
        assert e_den < e_noisy
    else:
        assert e_den <= e_noisy


# ---- the entries that need no device
def test_default_params_and_workspace_need_no_device(rt):
    p = rt.abi.DenoiseParams()
    assert C.sizeof(p) == 32
    assert rt.lib().rt_denoise_default_params(C.byref(p)) == 0
    assert 1 <= p.iterations <= 8 and p.sigma_color >= 0 and p.firefly_clamp >= 0
    assert list(p.reserved) == [0, 0, 0]
    d = rt.default_denoise_params()
    assert bytes(d) == bytes(p)
    assert rt.lib().rt_denoise_default_params(None) == rt.abi.RT_ERROR_INVALID
    assert rt.lib().rt_denoise_workspace_bytes(1920, 1080) == 64*1920*1080
    assert rt.denoise_workspace_bytes(65535, 65535) == 64*65535*65535
    assert rt.lib().rt_abi_version() == 8


def test_host_entry_refuses_to_run_without_a_device(rt):
    if rt.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(rt.RenderError) as e:
        rt.denoise(np.ones((4, 4, 4), F))
    assert e.value.code == rt.abi.RT_ERROR_NO_DEVICE


def _call_device(rt, p, beauty=1, g0=1, g1=1, w=4, h=4, out=1):
    return rt.lib().rt_denoise_device(0, C.c_void_p(beauty or None), C.c_void_p(g0 or None), C.c_void_p(g1 or None), w, h,
                                      C.byref(p) if p is not None else None, None, C.c_void_p(out or None), None)


def _call_host(rt, p, beauty=True, g0=True, g1=True, w=4, h=4, out=True):
    fp = C.POINTER(C.c_float)
    px = np.ones((4, 4, 4), F)
    res = np.zeros((4, 4, 4), F)
    buf = rt.abi.AccumulationBuffer(w, h, 0, px.ctypes.data_as(fp))
    return rt.lib().rt_denoise(0, C.byref(buf) if beauty else None, px.ctypes.data_as(fp) if g0 else None,
                               px.ctypes.data_as(fp) if g1 else None, C.byref(p) if p is not None else None,
                               res.ctypes.data_as(fp) if out else None)


BAD = [("d_beauty|beauty", dict(beauty=0), None), ("d_out|out_pixels", dict(out=0), None),
       ("rt_denoise_params", dict(), "null"), ("w", dict(w=0), None), ("h", dict(h=0), None),
       ("iterations", dict(), ("iterations", 0)), ("iterations", dict(), ("iterations", 9)),
       ("iterations", dict(), ("iterations", -1)),
       ("sigma_color", dict(), ("sigma_color", -1.0)), ("sigma_color", dict(), ("sigma_color", math.nan)),
       ("sigma_color", dict(), ("sigma_color", math.inf)),
       ("sigma_guide[0]", dict(), ("sigma_guide0", -0.5)), ("sigma_guide[0]", dict(), ("sigma_guide0", math.inf)),
       ("sigma_guide[1]", dict(), ("sigma_guide1", math.nan)), ("sigma_guide[1]", dict(), ("sigma_guide1", -2.0)),
       ("firefly_clamp", dict(), ("firefly_clamp", -1.0)), ("firefly_clamp", dict(), ("firefly_clamp", math.nan)),
       ("firefly_clamp", dict(), ("firefly_clamp", math.inf)),
       ("sigma_guide[0]", dict(g0=0), None), ("sigma_guide[1]", dict(g1=0), None)]


@pytest.mark.parametrize("case", range(len(BAD)))
@pytest.mark.parametrize("entry", ["device", "host"])
def test_bad_arguments_are_refused_by_name(rt, entry, case):
    """Every bad argument is RT_ERROR_INVALID with the field named, before any device is touched (the device
    pointers here are never dereferenced)."""
    import re
    names, kw, field = BAD[case]
    p = rd.params(3, 1.0, (0.1, 0.05), 10.0)
    if field == "null":
        p = None
    elif field is not None:
        k, v = field
        if k.startswith("sigma_guide"):
            p.sigma_guide[int(k[-1])] = v
        else:
            setattr(p, k, v)
    if entry == "device":
        err = _call_device(rt, p, **{k: v for k, v in kw.items()})
    else:
        err = _call_host(rt, p, **{k: bool(v) if k in ("beauty", "g0", "g1", "out") else v for k, v in kw.items()})
    assert err == rt.abi.RT_ERROR_INVALID
    msg = rt.lib().rt_last_error().decode()
    assert re.search(r"(?<![\w\[])(" + "|".join(re.escape(n) for n in names.split("|")) + r")(?![\w\[])", msg), msg


def test_picture_entry_checks_its_arguments(rt):
    p = rd.params()
    p.iterations = 0
    post = rt.abi.PostSettings()
    out = np.zeros((4, 4), np.uint32)
    st = rt.abi.Settings()
    err = rt.lib().rt_render_picture_denoised(None, None, C.byref(st), None, None, 0, 4, 4, C.byref(post), C.byref(p), 0,
                                              out.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    assert err == rt.abi.RT_ERROR_INVALID and "scene" in rt.lib().rt_last_error().decode()
