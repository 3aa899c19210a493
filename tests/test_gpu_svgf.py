"""Variance-guided filtering of the temporal history on the device ("Variance-guided filtering"): the three
kernels (rt_temporal_accumulate_moments_device, rt_temporal_variance_device, rt_denoise_variance_device) against the
plain-C checker tests/ref_svgf, bit for bit, on seeded buffers and on real frames of a moving camera; the moments
stage's history against rt_temporal_accumulate_device's; the driver (rt_render_temporal_filtered_device) against the
same loop written here on the public entries below it, bit for bit; a changed frame size; rt_cancel; the host entries.

Scenes are the suite's small presets (C1 at 130x70, C3 and C4 at 192x108) with the exact splat configured and one or
two samples per pixel: what can go wrong is the filter and the bookkeeping, not the paths.
"""
import threading

import numpy as np
import pytest

import ref_svgf_binding as sb
import ref_temporal_binding as tb
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 3          # total_frame_index of every frame here
BELOW = sb.SPATIAL_BELOW


def rays(s):
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def mismatches(a, b):
    a, b = tb.bits(host(a)), tb.bits(host(b))
    assert a.shape == b.shape
    return int(np.count_nonzero(a != b))


def texels(d):
    """A device G-buffer (h, w, 8) float32 -> the structured host array (h, w)."""
    a = d.cpu().numpy()
    return a.view(tb.dtype()).reshape(a.shape[0], a.shape[1])


def to_device(torch, a):
    """A host array (structured G-buffers as their 8 words) -> a device tensor."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.float32).reshape(a.shape + (8,))
    d = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize(0)
    return d


def garbage(torch, *shape, fill=-5.0):
    d = torch.full(shape, fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    return d


def ptr(t):
    return t.data_ptr() if t is not None else None


def device_moments(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h):
    """rt_temporal_accumulate_moments_device into outputs that start as garbage -> (d_history, d_length, d_moments)."""
    d_hist, d_len, d_mom = garbage(torch, h, w, 4), garbage(torch, h, w), garbage(torch, h, w, 2)
    ph, pl, pg, pm = d_prev if d_prev is not None else (None, None, None, None)
    rt.temporal_accumulate_moments_device(ptr(d_cur), ptr(d_g), ptr(ph), ptr(pl), ptr(pg), ptr(pm), cam, amount, w, h, p,
                                          ptr(d_hist), ptr(d_len), ptr(d_mom))
    return d_hist, d_len, d_mom


def device_accumulate(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h):
    d_hist, d_len = garbage(torch, h, w, 4), garbage(torch, h, w)
    ph, pl, pg = d_prev[:3] if d_prev is not None else (None, None, None)
    rt.temporal_accumulate_device(ptr(d_cur), ptr(d_g), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p, ptr(d_hist), ptr(d_len))
    return d_hist, d_len


def device_variance(rt, torch, d_mom, d_len, d_g, p, below, w, h):
    d_var = garbage(torch, h, w)
    rt.temporal_variance_device(ptr(d_mom), ptr(d_len), ptr(d_g), w, h, p, below, ptr(d_var))
    return d_var


def device_filter(rt, torch, d_col, d_var, d_g, p, w, h, want_variance=True, workspace=False):
    d_out = garbage(torch, h, w, 4)
    d_vout = garbage(torch, h, w) if want_variance else None
    ws = garbage(torch, rt.denoise_variance_workspace_bytes(w, h)//4, fill=float("nan")) if workspace else None
    rt.denoise_variance_device(ptr(d_col), ptr(d_var), ptr(d_g), w, h, p, ptr(d_out), d_variance_out=ptr(d_vout),
                               d_workspace=ptr(ws))
    return d_out, d_vout


# ---- 1. the three kernels against the checker on seeded buffers

@pytest.mark.parametrize("w,h", sb.KERNEL_SIZES)
def test_moments_kernel_matches_the_checker(rt, w, h):
    import torch
    amount = 2.0
    cur, g, prev, cam = sb.moments_case(w, h, amount)
    d_cur, d_g = to_device(torch, cur), to_device(torch, g)
    d_prev = tuple(to_device(torch, a) for a in prev)
    bad = same = 0
    # the defaults; no snap and no clamp; a short history with loose surface tests; no history to speak of; strict tests
    for q in (tb.params(), tb.params(snap=0.0, firefly_clamp=0.0), tb.params(max_history=2.5, normal_cos=-1.0, plane_tolerance=10.0),
              tb.params(max_history=1.0), tb.params(normal_cos=1.0, plane_tolerance=0.0, snap=0.5)):
        want = sb.accumulate_moments(cur, g, prev, cam, amount, q)
        got = device_moments(rt, torch, d_cur, d_g, d_prev, cam, amount, q, w, h)
        bad += sum(mismatches(a, b) for a, b in zip(got, want))
        # the history and the length are rt_temporal_accumulate_device's
        ref = device_accumulate(rt, torch, d_cur, d_g, d_prev, cam, amount, q, w, h)
        same += mismatches(got[0], ref[0]) + mismatches(got[1], ref[1])
    want = sb.accumulate_moments(cur, g, None, None, 0.0, tb.params())
    got = device_moments(rt, torch, d_cur, d_g, None, None, 0.0, tb.params(), w, h)
    bad += sum(mismatches(a, b) for a, b in zip(got, want))
    # the inputs are only read
    assert mismatches(d_cur, cur) == 0 and mismatches(texels(d_g), g) == 0 and mismatches(d_prev[3], prev[3]) == 0
    # the host entry
    want = sb.accumulate_moments(cur, g, prev, cam, amount, tb.params())
    bad += sum(mismatches(a, b) for a, b in zip(rt.temporal_accumulate_moments(cur, g, prev, cam, amount, tb.params()), want))
    REPORT[f"svgf_moments_{w}x{h}"] = {"mismatches": bad, "against_accumulate": same}
    print(w, h, "moments: mismatches", bad, "history and length against rt_temporal_accumulate_device", same)
    assert bad == 0 and same == 0


@pytest.mark.parametrize("w,h", sb.KERNEL_SIZES)
def test_variance_kernel_matches_the_checker(rt, w, h):
    import torch
    m, length, g = sb.variance_case(w, h)
    d_m, d_l, d_g = to_device(torch, m), to_device(torch, length), to_device(torch, g)
    bad = 0
    # the default threshold; never a window; always a window; loose and strict surface tests
    for below, q in ((BELOW, tb.params()), (0.0, tb.params()), (100.0, tb.params()),
                     (BELOW, tb.params(normal_cos=-1.0, plane_tolerance=10.0)), (BELOW, tb.params(normal_cos=1.0, plane_tolerance=0.0))):
        want = sb.variance(m, length, g, q, below)
        assert not (want == -7.0).any()
        bad += mismatches(device_variance(rt, torch, d_m, d_l, d_g, q, below, w, h), want)
    assert mismatches(d_m, m) == 0 and mismatches(d_l, length) == 0 and mismatches(texels(d_g), g) == 0
    bad += mismatches(rt.temporal_variance(m, length, g, tb.params(), BELOW), sb.variance(m, length, g, tb.params(), BELOW))
    REPORT[f"svgf_variance_{w}x{h}"] = {"mismatches": bad}
    print(w, h, "variance: mismatches", bad)
    assert bad == 0


@pytest.mark.parametrize("w,h", sb.KERNEL_SIZES)
def test_filter_kernel_matches_the_checker(rt, w, h):
    import torch
    col, var, g = sb.filter_case(w, h)
    d_col, d_var, d_g = to_device(torch, col), to_device(torch, var), to_device(torch, g)
    bad = 0
    for k, kw in enumerate(sb.FILTER_PARAMS):               # iterations 1 and 5 among them: at step 16 the taps leave 5x3
        want_out, want_var = sb.checked_filter(w, h, k)
        got_out, got_var = device_filter(rt, torch, d_col, d_var, d_g, sb.filter_params(**kw), w, h, workspace=(k % 2 == 0))
        bad += mismatches(got_out, want_out) + mismatches(got_var, want_var)
    assert mismatches(d_col, col) == 0 and mismatches(d_var, var) == 0 and mismatches(texels(d_g), g) == 0
    # no variance output; then in place: d_out the colour and d_variance_out the variance
    p = sb.filter_params()
    want_out, want_var = sb.checked_filter(w, h, 0)
    got_out, none = device_filter(rt, torch, d_col, d_var, d_g, p, w, h, want_variance=False)
    bad += mismatches(got_out, want_out)
    assert none is None
    rt.denoise_variance_device(ptr(d_col), ptr(d_var), ptr(d_g), w, h, p, ptr(d_col), d_variance_out=ptr(d_var))
    bad += mismatches(d_col, want_out) + mismatches(d_var, want_var)
    # the host entry
    h_out, h_var = rt.denoise_variance(col, var, g, p)
    bad += mismatches(h_out, want_out) + mismatches(h_var, want_var)
    REPORT[f"svgf_filter_{w}x{h}"] = {"mismatches": bad}
    print(w, h, "filter: mismatches", bad)
    assert bad == 0


# ---- 2. real frames

class Case:
    """A scene on the device in the exact splat mode."""

    def __init__(self, rt, preset, w, h):
        import torch
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        self.scene, self.cam, self.st, self.fc, self.post = rt.load_preset(preset, w, h)
        self.dev = rt.DeviceScene(self.scene, 0)
        self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)

    def settings(self, spp):
        s = self.rt.abi.Settings.from_buffer_copy(self.st)
        s.samples_per_pixel = spp
        return s

    def frame(self, cam, spp, frame_count):
        """One frame into a zeroed device buffer -> (d_frame, stats)."""
        d = garbage(self.torch, self.h, self.w, 4, fill=0.0)
        s = self.dev.render_device(cam, self.settings(spp), self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI,
                                   frame_count=frame_count)
        return d, s

    def gbuffer(self, cam):
        d = garbage(self.torch, self.h, self.w, 8, fill=float("nan"))
        self.dev.gbuffer_device(cam, self.w, self.h, d.data_ptr(), lens_distortion=self.st.lens_distortion)
        return d

    def state(self):
        """A fresh rt_temporal_filtered_state over a workspace that starts as garbage -> (state, the workspace's tensor)."""
        ws = garbage(self.torch, self.rt.temporal_filtered_workspace_bytes(self.w, self.h)//4, fill=float("nan"))
        st = self.rt.TemporalFilteredState()
        st.d_workspace = ws.data_ptr()
        return st, ws

    def driver(self, cam, spp, frame_count, p, fp, state):
        """rt_render_temporal_filtered_device into buffers that start as garbage -> ((out, history, length, variance), stats)."""
        t = self.torch
        outs = (garbage(t, self.h, self.w, 4, fill=9.0), garbage(t, self.h, self.w, 4, fill=9.0), garbage(t, self.h, self.w, fill=9.0),
                garbage(t, self.h, self.w, fill=9.0))
        s = self.dev.render_temporal_filtered_device(cam, self.settings(spp), self.fc, self.w, self.h, p, fp, state, ptr(outs[0]),
                                                     d_history_out=ptr(outs[1]), d_length_out=ptr(outs[2]),
                                                     d_variance_out=ptr(outs[3]), spatial_below=BELOW, frame_count=frame_count,
                                                     total_frame_index=TFI)
        return outs, s

    def close(self):
        self.dev.close()


def moved_along(rt, cam, dx=0.0, dy=0.0, dz=0.0):
    c = rt.abi.Camera.from_buffer_copy(cam)
    c.p = rt.v3(*[getattr(cam.p, k) + dx*getattr(cam.x, k) + dy*getattr(cam.y, k) + dz*getattr(cam.z, k) for k in "xyz"])
    return c


def camera_path(rt, cam, k):
    return moved_along(rt, cam, dx=0.05*k, dy=0.02*k, dz=-0.1*k)


@pytest.mark.parametrize("preset", ["c3", "c4"])
def test_kernels_match_the_checker_on_a_moving_camera(rt, preset):
    """Five frames of a moving camera at 192x108: the device's own frames and G-buffers through the three stages, each
    stage's output held to the checker on the same inputs."""
    import torch
    case = Case(rt, preset, 192, 108)
    try:
        w, h, amount = case.w, case.h, case.st.lens_distortion
        p, fp = tb.params(), sb.filter_params()
        d_prev, prev, prev_cam = None, None, None
        bad = {"moments": 0, "variance": 0, "filter": 0}
        window = []
        for k in range(5):
            cam = camera_path(rt, case.cam, k)
            f, _ = case.frame(cam, 2, 2*k)
            g = case.gbuffer(cam)
            d_hist, d_len, d_mom = device_moments(rt, torch, f, g, d_prev, prev_cam, amount, p, w, h)
            want = sb.accumulate_moments(host(f), texels(g), prev, prev_cam, amount, p)
            bad["moments"] += sum(mismatches(a, b) for a, b in zip((d_hist, d_len, d_mom), want))
            d_var = device_variance(rt, torch, d_mom, d_len, g, p, BELOW, w, h)
            want_var = sb.variance(host(d_mom), host(d_len), texels(g), p, BELOW)
            bad["variance"] += mismatches(d_var, want_var)
            d_out, d_vout = device_filter(rt, torch, d_hist, d_var, g, fp, w, h)
            want_out, want_vout = sb.denoise_variance(host(d_hist), host(d_var), texels(g), fp)
            bad["filter"] += mismatches(d_out, want_out) + mismatches(d_vout, want_vout)
            window.append(float(((host(d_len) >= 1) & (host(d_len) < BELOW)).mean()))
            d_prev, prev, prev_cam = (d_hist, d_len, g, d_mom), (host(d_hist), host(d_len), texels(g), host(d_mom)), cam
        REPORT[f"svgf_kernels_{preset}_moving"] = dict(bad, window_share=window)
        print(preset, "moving camera: mismatches", bad, "share of pixels that take the window", window)
        assert bad == {"moments": 0, "variance": 0, "filter": 0}
        # three frames in which every valid pixel takes the window, then the pixels with a history of 4 leave it
        assert min(window[:3]) > 0.9 and window[4] < 0.7 and float((host(d_len) > 1).mean()) > 0.3
    finally:
        case.close()


# ---- 3. the driver against the loop

@pytest.fixture(scope="module")
def c1(rt):
    case = Case(rt, "c1", 130, 70)
    yield case
    case.close()


def test_driver_equals_the_hand_written_loop(rt, c1):
    import torch
    case, w, h = c1, c1.w, c1.h
    amount = case.st.lens_distortion
    p, fp = tb.params(), sb.filter_params()
    state, ws = case.state()
    prev, prev_cam = None, None
    bad, shares = 0, []
    for k in range(4):
        cam = camera_path(rt, case.cam, k)
        # rt_render_temporal_filtered_device's definition, on the public entries below it
        f, want_stats = case.frame(cam, 1, k)
        g = case.gbuffer(cam)
        want_hist, want_len, want_mom = device_moments(rt, torch, f, g, prev, prev_cam, amount, p, w, h)
        want_var = device_variance(rt, torch, want_mom, want_len, g, p, BELOW, w, h)
        want_out, _ = device_filter(rt, torch, want_hist, want_var, g, fp, w, h, want_variance=False)
        (got_out, got_hist, got_len, got_var), stats = case.driver(cam, 1, k, p, fp, state)
        bad += (mismatches(got_out, want_out) + mismatches(got_hist, want_hist) + mismatches(got_len, want_len) +
                mismatches(got_var, want_var))
        assert rays(stats) == rays(want_stats) and stats.samples == w*h
        assert (state.frames, state.parity, state.w, state.h) == (k + 1, (k + 1) % 2, w, h)
        assert bytes(state.camera) == bytes(cam) and state.lens_distortion == amount
        prev, prev_cam = (want_hist, want_len, g, want_mom), cam
        shares.append(float((host(got_len) > 1).mean()))
    REPORT["svgf_driver_c1"] = {"mismatches": bad, "share_with_history": shares}
    print("C1 filtered driver: mismatches", bad, "share of pixels with a history per frame", shares)
    assert bad == 0 and shares[0] == 0.0 and min(shares[1:]) > 0.3
    del ws


def test_driver_restarts_on_another_frame_size_and_host_entry_equals_device(rt, c1):
    """A state of 130x70 given a 65x33 frame restarts (its workspace holds the smaller frame's); the host-pointer entry
    then equals the device one fed the same state, frame by frame."""
    state, ws = c1.state()
    p, fp = tb.params(), sb.filter_params()
    c1.driver(c1.cam, 1, 0, p, fp, state)
    c1.driver(c1.cam, 1, 1, p, fp, state)
    assert (state.frames, state.w, state.h) == (2, 130, 70)
    small = Case(rt, "c1", 65, 33)
    try:
        other, ws2 = small.state()
        for k in range(2):
            out, hist, length, var, stats = small.dev.render_temporal_filtered(small.cam, small.settings(1), small.fc, 65, 33,
                                                                               state, p, fp, frame_count=k, total_frame_index=TFI)
            (d_out, d_hist, d_len, d_var), d_stats = small.driver(small.cam, 1, k, p, fp, other)
            assert mismatches(d_out, out) + mismatches(d_hist, hist) + mismatches(d_len, length) + mismatches(d_var, var) == 0
            assert rays(stats) == rays(d_stats)
            ok = np.isfinite(hist).all(axis=2)
            assert ok.mean() > 0.99 and (length[ok] == 1.0).all() if k == 0 else float((length[ok] == 2.0).mean()) > 0.9
            assert (state.frames, state.w, state.h, state.parity) == (3 + k, 65, 33, other.parity)
        out2, none_h, none_l, none_v, _ = small.dev.render_temporal_filtered(small.cam, small.settings(1), small.fc, 65, 33, state,
                                                                             p, fp, frame_count=2, total_frame_index=TFI,
                                                                             want_extras=False)
        assert none_h is None and none_l is None and none_v is None and state.frames == 5 and np.isfinite(out2).mean() > 0.99
        del ws2
    finally:
        small.close()
    del ws


# ---- 4. cancel

def test_cancel_leaves_the_state_alone(rt):
    """rt_cancel from another thread while the frame runs returns RT_ERROR_CANCELLED; the state and the outputs stay."""
    import torch
    case = Case(rt, "c3", 192, 108)
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
        while not returned.is_set():
            case.dev.cancel()
            returned.wait(0.005)

    try:
        p, fp = tb.params(), sb.filter_params()
        state, ws = case.state()
        case.driver(case.cam, 2, 0, p, fp, state)
        before = bytes(state)
        outs = (garbage(torch, case.h, case.w, 4, fill=3.0), garbage(torch, case.h, case.w, 4, fill=3.0),
                garbage(torch, case.h, case.w, fill=3.0), garbage(torch, case.h, case.w, fill=3.0))
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                case.dev.render_temporal_filtered_device(case.cam, case.settings(16384), case.fc, case.w, case.h, p, fp, state,
                                                         ptr(outs[0]), d_history_out=ptr(outs[1]), d_length_out=ptr(outs[2]),
                                                         d_variance_out=ptr(outs[3]), frame_count=1, total_frame_index=TFI)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
        assert bytes(state) == before and all(bool((o == 3.0).all()) for o in outs)
        # the next frame goes on from the state as it was
        (_, _, length, _), _ = case.driver(case.cam, 2, 1, p, fp, state)
        assert state.frames == 2 and float((host(length) == 2.0).mean()) > 0.9
        del ws
    finally:
        case.close()
