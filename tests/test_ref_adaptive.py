"""Adaptive sampling by tiles without a device: the plain-C checker of the tile error estimate
(tests/ref_adaptive) against a numpy float64 restatement of the metric, and every refusal of the three entry
pairs (rt_render_tiles*, rt_tile_error*, rt_render_adaptive*), which are raised by name before the device is
touched ("Adaptive sampling by tiles").

The bound of the float64 comparison.  With u = 2^-24 (f32 unit roundoff), a resolved channel a = A/w carries a
relative error u, so a difference |a - b| an absolute error <= u(|a| + |b|) + u|a - b|; the three-term sum, the
mean m (two additions, a division, two additions), the root and the division add a few u relative to e: 8u
covers them.  Per pixel |e32 - e64| <= u * (sum_c(|a_c| + |b_c|)) / sqrt(max(m, floor)) * (1 + 8u) + 8u e.  A
tile's sum adds at most ceil(n/256) - 1 + 8 terms in a chain (the per-thread loop, then the tree), each
rounding relative to a partial sum <= the whole (e >= 0): <= (n/256 + 8) u times the mean.  The test computes
that bound per tile in float64 and doubles it.
"""
import ctypes as C

import numpy as np
import pytest

import ref_adaptive_binding as ra

U = 2.0**-24


def _bound(a, b, tw, th, ids, floor=1e-4):
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    h, w, _ = a64.shape
    tcx, _ = ra.tile_grid(w, h, tw, th)
    valid = (a[..., 3] > np.float32(0.001)) & (b[..., 3] > np.float32(0.001))
    valid &= np.isfinite(a64).all(axis=2) & np.isfinite(b64).all(axis=2)
    with np.errstate(all="ignore"):
        ra_, rb_ = a64[..., :3]/a64[..., 3:], b64[..., :3]/b64[..., 3:]
        m = ((a64[..., :3] + b64[..., :3])/(a64[..., 3:] + b64[..., 3:])).sum(axis=2)
        den = np.sqrt(np.maximum(m, float(np.float32(floor))))
        e = np.abs(ra_ - rb_).sum(axis=2)/den
        px = U*(np.abs(ra_) + np.abs(rb_)).sum(axis=2)/den*(1 + 8*U) + 8*U*e
    out = []
    for t in ids:
        x0, y0 = tw*(t % tcx), th*(t // tcx)
        v = valid[y0:y0 + th, x0:x0 + tw]
        n = int(v.sum())
        if not n:
            out.append(0.0)
            continue
        mean_e = e[y0:y0 + th, x0:x0 + tw][v].sum()/n
        out.append(2.0*(px[y0:y0 + th, x0:x0 + tw][v].sum()/n + (v.size/256 + 8 + 1)*U*mean_e))
    return np.array(out)


@pytest.mark.parametrize("w,h,tw,th", ra.SHAPES)
def test_checker_against_float64(w, h, tw, th):
    a, b, sub = ra.synthetic_case(w, h, tw, th)
    tcx, tcy = ra.tile_grid(w, h, tw, th)
    for ids in (None, sub):
        err, valid = ra.tile_error(a, b, tw, th, ids)
        want, want_valid = ra.numpy_tile_error(a, b, tw, th, ids)
        listed = list(range(tcx*tcy)) if ids is None else ids
        assert np.array_equal(valid, want_valid)
        bound = _bound(a, b, tw, th, listed)
        finite = np.isfinite(want)
        assert np.array_equal(np.isposinf(err), ~finite)
        diff = np.abs(err[finite].astype(np.float64) - want[finite])
        print(f"{w}x{h} tiles {tw}x{th} list={'all' if ids is None else 'sub'}: max |f32 - f64| {diff.max():.3e}, "
              f"bound {bound[finite].min():.3e}..{bound[finite].max():.3e}, errors {want[finite].min():.3e}..{want[finite].max():.3e}")
        assert (diff <= bound[finite]).all()
    # the tile with no valid pixel: +INFINITY and a count of 0
    err, valid = ra.tile_error(a, b, tw, th)
    assert np.isposinf(err[-1]) and valid[-1] == 0
    # the inputs hold what the definition names: invalid pixels of every kind, pixels under the floor, valid ones
    if w*h > 1000:
        assert np.isnan(a).any() and np.isinf(b).any() and (a[..., 3] < 0).any() and (b[..., 3] == 0).any()
        assert ((a[..., :3].sum(axis=2) == 0) & (a[..., 3] > 0.001)).any()
        assert 0 < valid.sum() < w*h


def test_edge_tiles_of_the_ragged_frame():
    """130x70 with 64x64 tiles: the edge tiles are 2 wide and 6 tall, and the counts say so."""
    w, h = 130, 70
    a = np.ones((h, w, 4), np.float32)
    b = np.full((h, w, 4), 2.0, np.float32)
    err, valid = ra.tile_error(a, b, 64, 64)
    assert valid.tolist() == [64*64, 64*64, 2*64, 64*6, 64*6, 2*6]
    assert np.array_equal(ra.bits(err), ra.bits(np.zeros(6, np.float32)))       # a = b = (1, 1, 1) after the resolve


@pytest.mark.parametrize("w,h,tw,th", ra.SHAPES)
def test_equal_halves_give_exactly_zero(w, h, tw, th):
    a, _, _ = ra.synthetic_case(w, h, tw, th)
    err, valid = ra.tile_error(a, a.copy(), tw, th)
    assert valid[-1] == 0 and np.isposinf(err[-1])
    assert (err[valid > 0] == 0.0).all() and (valid > 0).any()


def test_m_under_the_floor():
    """A dark pixel divides by sqrt(floor), not by sqrt(m): the floor is what bounds its error."""
    a = np.zeros((1, 1, 4), np.float32)
    b = np.zeros((1, 1, 4), np.float32)
    a[0, 0] = (2e-6, 0, 0, 1)
    b[0, 0] = (0, 0, 0, 1)
    for floor in (1e-4, 1e-2):
        err, valid = ra.tile_error(a, b, 1, 1, p=ra.params(floor))
        want = np.float32(2e-6)/np.sqrt(np.float32(floor))
        assert valid[0] == 1 and err[0] == want, (err[0], want)


def test_the_sum_order_is_the_documented_one():
    """17x16 tile: partial i of 256 adds pixels i and i + 256, then the tree i += i + s, s = 128 .. 1."""
    w, h = 17, 16
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(0.1, 5.0, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(np.float32)
    b = np.concatenate([rng.uniform(0.1, 5.0, (h, w, 3)), np.ones((h, w, 1))], axis=2).astype(np.float32)
    f = np.float32
    pa, pb = a.reshape(-1, 4), b.reshape(-1, 4)
    e = np.zeros(w*h, np.float32)
    for i in range(w*h):
        ar, br = pa[i, :3]/pa[i, 3], pb[i, :3]/pb[i, 3]
        mw = pa[i, 3] + pb[i, 3]
        m3 = (pa[i, :3] + pb[i, :3])/mw
        d = f(f(abs(f(ar[0] - br[0])) + abs(f(ar[1] - br[1]))) + abs(f(ar[2] - br[2])))
        m = f(f(m3[0] + m3[1]) + m3[2])
        e[i] = d/np.sqrt(max(m, f(1e-4)))
    part = np.zeros(256, np.float32)
    for i in range(256):
        for j in range(i, w*h, 256):
            part[i] = part[i] + e[j]
    s = 128
    while s:
        part[:s] = part[:s] + part[s:2*s]
        s //= 2
    err, valid = ra.tile_error(a, b, 17, 16)
    assert valid[0] == w*h
    assert ra.bits(err)[0] == ra.bits(f(part[0]/f(w*h)))[()]


# ---- refusals, by name, before the device is touched (no scene exists without a device: the scene is NULL)

def _last(rt):
    return (rt.lib().rt_last_error() or b"").decode()


def _ids(*v):
    return (C.c_uint32*len(v))(*v)


def _render_tiles_device(rt, ids, count, w=130, h=70, tile=64, scene=None, pixels=0x1000):
    cam, st, fc = rt.abi.Camera(), rt.abi.Settings(), rt.abi.FilterCache()
    return rt.lib().rt_render_tiles_device(scene, C.byref(cam), C.byref(st), C.byref(fc), tile, tile, ids, count, 0, w, h,
                                           0, C.c_void_p(pixels), None, None)


def _render_tiles_host(rt, ids, count, w=130, h=70, tile=64):
    cam, st, fc = rt.abi.Camera(), rt.abi.Settings(), rt.abi.FilterCache()
    px = np.zeros((h, w, 4), np.float32)
    buf = rt.abi.AccumulationBuffer(w, h, 0, px.ctypes.data_as(C.POINTER(C.c_float)))
    return rt.lib().rt_render_tiles(None, C.byref(cam), C.byref(st), C.byref(fc), tile, tile, ids, count, 0, C.byref(buf), None)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("ids,word", [((3, 1, 2), "not strictly ascending"),          # unsorted
                                      ((0, 2, 2), "not strictly ascending"),          # a duplicate id
                                      ((0, 6), "out of range"),                       # 130x70: six tiles
                                      (None, "null tile_ids")])
def test_render_tiles_refuses_a_bad_list(rt, entry, ids, word):
    call = _render_tiles_device if entry == "device" else _render_tiles_host
    arr = None if ids is None else _ids(*ids)
    assert call(rt, arr, 3 if ids is None else len(ids)) == rt.abi.RT_ERROR_INVALID
    assert word in _last(rt) and "tile_ids" in _last(rt), _last(rt)
    assert _last(rt).startswith("rt_render_tiles_device" if entry == "device" else "rt_render_tiles:")


def test_render_tiles_refuses_null_pointers_and_zero_sizes(rt):
    ok = _ids(0, 1, 5)
    assert _render_tiles_device(rt, ok, 3) == rt.abi.RT_ERROR_INVALID and "null scene" in _last(rt)
    assert _render_tiles_host(rt, ok, 3) == rt.abi.RT_ERROR_INVALID and "null scene" in _last(rt)
    assert _render_tiles_device(rt, ok, 0) == rt.abi.RT_ERROR_INVALID and "null scene" in _last(rt)
    for kw, word in ((dict(w=0), "w is 0"), (dict(h=0), "h is 0"), (dict(tile=0), "tile_w is 0")):
        assert _render_tiles_device(rt, ok, 3, **kw) == rt.abi.RT_ERROR_INVALID and word in _last(rt), _last(rt)
    cam, st, fc = rt.abi.Camera(), rt.abi.Settings(), rt.abi.FilterCache()
    assert rt.lib().rt_render_tiles(None, C.byref(cam), C.byref(st), C.byref(fc), 64, 64, ok, 3, 0, None, None) == rt.abi.RT_ERROR_INVALID
    assert "null accum" in _last(rt)


def _tile_error_host(rt, a="ok", b="ok", w=130, h=70, tile=64, ids=None, count=6, p="ok", err="ok", valid="ok"):
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    buf = np.ones((max(h, 1), max(w, 1), 4), np.float32)
    e, v = np.zeros(64, np.float32), np.zeros(64, np.uint32)
    pp = rt.default_tile_error_params() if p == "ok" else p
    return rt.lib().rt_tile_error(0, buf.ctypes.data_as(fp) if a == "ok" else None, buf.ctypes.data_as(fp) if b == "ok" else None,
                                  w, h, tile, tile, ids, count, C.byref(pp) if pp is not None else None,
                                  e.ctypes.data_as(fp) if err == "ok" else None, v.ctypes.data_as(up) if valid == "ok" else None)


def _tile_error_device(rt, a=0x1000, b=0x2000, w=130, h=70, tile=64, ids=None, count=6, p="ok", err=0x3000, valid=0x4000):
    pp = rt.default_tile_error_params() if p == "ok" else p
    vp = lambda x: C.c_void_p(x) if x else None
    return rt.lib().rt_tile_error_device(0, vp(a), vp(b), w, h, tile, tile, vp(ids), count,
                                         C.byref(pp) if pp is not None else None, vp(err), vp(valid), None)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_tile_error_refusals(rt, entry):
    call = _tile_error_device if entry == "device" else _tile_error_host
    name = "rt_tile_error_device" if entry == "device" else "rt_tile_error:"
    bad_floor = [rt.default_tile_error_params() for _ in range(4)]
    for p, v in zip(bad_floor, (0.0, -1.0, float("nan"), float("inf"))):
        p.floor = v
    cases = [(dict(a=None), "null half_a"), (dict(b=None), "null half_b"), (dict(err=None), "null tile_error"),
             (dict(valid=None), "null tile_valid"), (dict(p=None), "null rt_tile_error_params"),
             (dict(w=0), "w is 0"), (dict(h=0), "h is 0"), (dict(tile=0), "tile_w is 0"),
             (dict(count=0), "tile_count is 0"), (dict(count=7), "tile_count is above"),
             (dict(count=5), "null tile_ids means every tile")] + [(dict(p=p), "floor") for p in bad_floor]
    for kw, word in cases:
        assert call(rt, **kw) == rt.abi.RT_ERROR_INVALID, kw
        assert word in _last(rt) and _last(rt).startswith(name), (kw, _last(rt))
    if entry == "host":                                     # a host list is checked on the host
        assert call(rt, ids=_ids(0, 9), count=2) == rt.abi.RT_ERROR_INVALID
        assert "tile_ids[1] = 9 is out of range" in _last(rt)


def _adaptive(rt, entry, p, w=130, h=70, tile=64, pixels=True):
    cam, st, fc = rt.abi.Camera(), rt.abi.Settings(), rt.abi.FilterCache()
    pp = C.byref(p) if p is not None else None
    if entry == "device":
        return rt.lib().rt_render_adaptive_device(None, C.byref(cam), C.byref(st), C.byref(fc), tile, tile, 0, w, h, 0, pp,
                                                  None, C.c_void_p(0x1000) if pixels else None, None, None, None)
    px = np.zeros((max(h, 1), max(w, 1), 4), np.float32)
    buf = rt.abi.AccumulationBuffer(w, h, 0, px.ctypes.data_as(C.POINTER(C.c_float)) if pixels else None)
    return rt.lib().rt_render_adaptive(None, C.byref(cam), C.byref(st), C.byref(fc), tile, tile, 0, pp, C.byref(buf), None, None)


def _params(rt, **kw):
    p = rt.default_adaptive_params()
    for k, v in kw.items():
        if k == "floor":
            p.error.floor = v
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("entry", ["device", "host"])
def test_adaptive_refusals(rt, entry):
    name = "rt_render_adaptive_device" if entry == "device" else "rt_render_adaptive:"
    cases = [(dict(step_spp=3, min_spp=3, max_spp=9), "step_spp"),                # odd
             (dict(step_spp=0), "step_spp"),
             (dict(min_spp=64, max_spp=32), "min_spp is above max_spp"),
             (dict(min_spp=24), "min_spp must be a multiple"), (dict(min_spp=0), "min_spp"),
             (dict(max_spp=250), "max_spp must be a multiple"),
             (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"),
             (dict(threshold=float("inf")), "threshold"), (dict(floor=0.0), "floor"), (dict(floor=float("nan")), "floor")]
    for kw, word in cases:
        assert _adaptive(rt, entry, _params(rt, **kw)) == rt.abi.RT_ERROR_INVALID, kw
        assert word in _last(rt) and _last(rt).startswith(name), (kw, _last(rt))
    assert _adaptive(rt, entry, None) == rt.abi.RT_ERROR_INVALID and "null rt_adaptive_params" in _last(rt)
    assert _adaptive(rt, entry, _params(rt)) == rt.abi.RT_ERROR_INVALID and "null scene" in _last(rt)
    assert _adaptive(rt, entry, _params(rt), w=0) == rt.abi.RT_ERROR_INVALID and "w is 0" in _last(rt)
    assert _adaptive(rt, entry, _params(rt), tile=0) == rt.abi.RT_ERROR_INVALID and "tile_w is 0" in _last(rt)
    if entry == "host":
        assert _adaptive(rt, entry, _params(rt), pixels=False) == rt.abi.RT_ERROR_INVALID and "null accum" in _last(rt)


def test_defaults_and_layouts(rt):
    """No device needed: the defaults, the workspace size and the ctypes mirrors' sizes."""
    p = rt.default_adaptive_params()
    assert (p.min_spp, p.max_spp, p.step_spp) == (16, 256, 16)
    assert p.error.floor == np.float32(1e-4) and rt.default_tile_error_params().floor == np.float32(1e-4)
    assert p.threshold >= 0 and np.isfinite(p.threshold)
    assert C.sizeof(rt.abi.TileErrorParams) == 16 and C.sizeof(rt.abi.AdaptiveParams) == 48
    assert rt.adaptive_workspace_bytes(130, 70) == 32*130*70 + 12*6
    assert rt.lib().rt_abi_version() == 8
