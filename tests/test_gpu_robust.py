"""The robust estimator on the device ("The robust estimator"): the kernel (rt_robust_combine_device,
rt_robust_combine) against the plain-C checker tests/ref_robust, bit for bit; the driver (rt_render_robust_device)
against the same loop written here on rt_render_device and the combine, bit for bit; its pooled mean against the
uniform frame of the same samples; the picture entry against its sequence of public entries; rt_cancel.

Scenes are the suite's small presets (C1 at 130x70, C3 at 192x108) with the exact splat configured, a few samples per
pixel: what can go wrong is the slicing and the combine, not the paths.  The driver's buffers are the frame's shards
by sample passes, and a pass shard streams whatever splat is configured, so "bit for bit" between
the driver and the loop here also says that the streaming splat repeats itself.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import ref_robust_binding as rr
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 3          # total_frame_index of every frame here


def rays(s):
    """What two renders of the same samples must agree on: the ray counts and the TraversalStats."""
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def add_rays(total, s):
    t = total or (0, 0, 0, {}, {})
    add = lambda a, b: {k: a.get(k, 0) + v for k, v in b.items()}
    return (t[0] + s.closest_hit_rays, t[1] + s.shadow_rays, t[2] + s.samples, add(t[3], s.traversal[0].as_dict()),
            add(t[4], s.traversal[1].as_dict()))


def same_bits(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    b = b.cpu().numpy() if hasattr(b, "cpu") else b
    return np.array_equal(rr.bits(a), rr.bits(b))


def mismatches(a, b):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return int(np.count_nonzero(rr.bits(a) != rr.bits(b)))


# ---- 1. the kernel against the checker

def device_combine(rt, torch, d_stack, p, out=None, info=True):
    """rt_robust_combine_device on a device stack (K, h, w, 4) -> (d_out, d_info); `out` = a buffer index writes
    the output over that buffer of the stack.  Fresh outputs start as garbage."""
    K, h, w, _ = d_stack.shape
    d_out = d_stack[out] if out is not None else torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    d_info = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0") if info else None
    torch.cuda.synchronize(0)
    code = rt.lib().rt_robust_combine_device(0, C.c_void_p(d_stack.data_ptr()), K, w, h, C.byref(p), C.c_void_p(d_out.data_ptr()),
                                             C.c_void_p(d_info.data_ptr()) if info else None, None)
    assert code == 0, rt.lib().rt_last_error()
    return d_out, d_info


@pytest.mark.parametrize("K", rr.COUNTS)
@pytest.mark.parametrize("w,h", rr.SIZES)
def test_combine_matches_the_checker(rt, w, h, K):
    import torch
    stack = rr.synthetic_stack(w, h, K)
    want_out, want_info = rr.checked(w, h, K)
    d_stack = torch.from_numpy(np.array(stack)).to("cuda:0")
    p = rr.params()
    bad = 0
    got_out, got_info = device_combine(rt, torch, d_stack, p)
    bad += mismatches(got_out, want_out) + mismatches(got_info, want_info)
    assert same_bits(d_stack, stack)                                     # the stack is only read
    # other parameters: a scale of 2 under a cap of 1, and the pooled mean
    for gs, mt in ((2.0, 1), (0.0, 15)):
        w_out, w_info = rr.combine(stack, rr.params(gs, mt))
        g_out, g_info = device_combine(rt, torch, d_stack, rr.params(gs, mt))
        bad += mismatches(g_out, w_out) + mismatches(g_info, w_info)
    # a NULL info buffer
    alone, _ = device_combine(rt, torch, d_stack, p, info=False)
    bad += mismatches(alone, want_out)
    # the host entry
    host_out, host_info = rt.robust_combine(stack, p)
    bad += mismatches(host_out, want_out) + mismatches(host_info, want_info)
    host_alone, none = rt.robust_combine(stack, p, want_info=False)
    bad += mismatches(host_alone, want_out)
    # the output over buffer 0 and over buffer K-1 of the stack: the other buffers stay as they were
    for k in (0, K - 1):
        d_alias = torch.from_numpy(np.array(stack)).to("cuda:0")
        a_out, a_info = device_combine(rt, torch, d_alias, p, out=k)
        bad += mismatches(a_out, want_out) + mismatches(a_info, want_info)
        others = [j for j in range(K) if j != k]
        assert same_bits(d_alias[others], stack[others])
    REPORT[f"robust_combine_{w}x{h}_K{K}"] = {"mismatches": bad}
    assert none is None and bad == 0


def test_combine_1080p_grid_stride_and_timing(rt):
    """1920x1080 with K = 8: 8100 blocks of pixels on a grid of 2048, so every thread takes several pixels.  The
    stack is the 65x33 synthetic one repeated.  Times 20 calls with events (a figure for DESIGN.md, no assertion)."""
    import torch
    K, w, h = 8, 1920, 1080
    small = rr.synthetic_stack(65, 33, K).reshape(K, -1, 4)
    reps = -(-w*h // small.shape[1])
    stack = np.ascontiguousarray(np.tile(small, (1, reps, 1))[:, :w*h].reshape(K, h, w, 4))
    want_out, want_info = rr.combine(stack, rr.params())
    d_stack = torch.from_numpy(stack).to("cuda:0")
    got_out, got_info = device_combine(rt, torch, d_stack, rr.params())
    bad = mismatches(got_out, want_out) + mismatches(got_info, want_info)
    times = []
    p = rr.params()
    for _ in range(25):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rt.lib().rt_robust_combine_device(0, C.c_void_p(d_stack.data_ptr()), K, w, h, C.byref(p), C.c_void_p(got_out.data_ptr()),
                                          C.c_void_p(got_info.data_ptr()), None)
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times = sorted(times[5:])
    REPORT["robust_combine_1080p_K8"] = {"mismatches": bad, "ms_median": times[len(times)//2], "ms_min": times[0]}
    print("combine 1080p K=8:", REPORT["robust_combine_1080p_K8"])
    assert bad == 0


# ---- 2. the driver

class Case:
    """A preset on the device in the exact splat mode, with frames rendered into device buffers."""

    def __init__(self, rt, preset, w, h, spp=8, exact=True):
        import torch
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        self.scene, self.cam, self.st, self.fc, self.post = rt.load_preset(preset, w, h)
        self.st.samples_per_pixel = spp
        self.dev = rt.DeviceScene(self.scene, 0)
        if exact:
            self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)

    def full(self, fill=0.0, lead=()):
        d = self.torch.full(tuple(lead) + (self.h, self.w, 4), fill, dtype=self.torch.float32, device="cuda:0")
        self.torch.cuda.synchronize(0)
        return d

    def settings(self, spp):
        s = self.rt.abi.Settings.from_buffer_copy(self.st)
        s.samples_per_pixel = spp
        return s

    def frame(self, d, spp, frame_count=0, shard_index=0, shard_count=1):
        return self.dev.render_device(self.cam, self.settings(spp), self.fc, self.w, self.h, d.data_ptr(),
                                      total_frame_index=TFI, frame_count=frame_count, shard_index=shard_index,
                                      shard_count=shard_count)

    def robust(self, spp, p, frame_count=0, workspace=False, fill=9.0):
        """rt_render_robust_device into buffers that start as garbage -> (d_out, d_info, stats)."""
        d_out, d_info = self.full(fill), self.full(fill)
        ws = self.full(float("nan"), lead=(p.buffers,)) if workspace else None
        stats = self.dev.render_robust_device(self.cam, self.settings(spp), self.fc, self.w, self.h, p, d_out.data_ptr(),
                                              d_info=d_info.data_ptr(), d_workspace=ws.data_ptr() if workspace else None,
                                              frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_info, stats

    def close(self):
        self.dev.close()


def hand_loop(rt, case, spp, p, frame_count=0):
    """rt_render_robust_device's definition, on the public entries below it: buffer k is shard k of K of the frame by
    sample passes."""
    K = p.buffers
    stack = case.full(0.0, lead=(K,))
    total = None
    with case.dev.configured(shard_mode=rt.abi.RT_SHARD_PASSES):
        for k in range(K):
            total = add_rays(total, case.frame(stack[k], spp, frame_count, shard_index=k, shard_count=K))
    out, info = device_combine(rt, case.torch, stack, p)
    return out, info, total


@pytest.fixture(scope="module")
def c3(rt):
    case = Case(rt, "c3", 192, 108)
    yield case
    case.close()


@pytest.fixture(scope="module")
def c1(rt):
    case = Case(rt, "c1", 130, 70)
    yield case
    case.close()


@pytest.mark.parametrize("spp,K", [(8, 4), (6, 3)])
@pytest.mark.parametrize("preset", ["c1", "c3"])
def test_driver_equals_the_hand_written_loop(rt, c1, c3, preset, spp, K):
    case = c1 if preset == "c1" else c3
    p = rr.params(buffers=K)
    want_out, want_info, want_rays = hand_loop(rt, case, spp, p)
    got_out, got_info, stats = case.robust(spp, p, workspace=(K == 4))
    n = got_info[..., 2].cpu().numpy()
    c = got_info[..., 1].cpu().numpy()
    REPORT[f"robust_driver_{preset}_{spp}spp_K{K}"] = {"mismatches": mismatches(got_out, want_out.cpu().numpy()),
                                                       "trimmed_share": float((c > 0).mean())}
    print(preset, spp, K, "share of pixels with c > 0:", float((c > 0).mean()), "seconds", stats.seconds)
    assert same_bits(got_out, want_out) and same_bits(got_info, want_info)
    assert rays(stats) == want_rays and stats.samples == spp*case.w*case.h
    assert stats.seconds > 0 and stats.splat_mode == rt.abi.RT_SPLAT_STREAM      # a pass shard streams
    assert case.dev.config().shard_mode == rt.abi.RT_CONFIG_INHERIT            # the scene's shard mode was put back
    assert (n == K).mean() > 0.99 and bool((got_out[..., 3][got_info[..., 2] > 0] == 1.0).all())
    # the host entry gives the same output
    host_out, host_info, host_stats = case.dev.render_robust(case.cam, case.settings(spp), case.fc, case.w, case.h, p,
                                                            total_frame_index=TFI)
    assert same_bits(got_out, host_out) and same_bits(got_info, host_info) and rays(host_stats) == want_rays


# ---- 3. the pooled mean is the uniform frame

@pytest.mark.parametrize("frame_count", [0, 5])
@pytest.mark.parametrize("preset", ["c1", "c3"])
def test_scale_zero_is_the_uniform_frame(rt, c1, c3, preset, frame_count):
    """gini_scale = 0 pools every buffer: the samples of one uniform frame of samples_per_pixel at frame_count, added
    in another order (per buffer, streamed, then pooled; the uniform frame here is the exact splat's).  The bar is the
    project's for a changed float sum order.  It holds because buffer k is a pass shard of that frame; K frames of
    spp/K samples at frame_count + k*spp/K, which take other random streams, miss it by sampling noise (rel L2 0.10 to
    0.12 on these cases)."""
    case = c1 if preset == "c1" else c3
    spp, K = 8, 4
    got, info, stats = case.robust(spp, rr.params(0.0, buffers=K), frame_count=frame_count)
    uniform = case.full(0.0)
    us = case.frame(uniform, spp, frame_count)
    u = uniform.cpu().numpy().astype(np.float64)
    inf = info.cpu().numpy().astype(np.float64)
    full = (inf[..., 2] == K) & (u[..., 3] > 0.001)                       # every buffer valid there: nothing was left out
    assert full.mean() > 0.99
    want = (u[..., :3]/u[..., 3:])[full]
    g = got.cpu().numpy()[..., :3].astype(np.float64)[full]
    err = float(np.linalg.norm(g - want)/np.linalg.norm(want))
    werr = float(np.abs(inf[..., 3] - u[..., 3])[full].max()/u[..., 3][full].max())
    REPORT[f"robust_pooled_vs_uniform_{preset}_fc{frame_count}"] = {"rel_l2": err, "weight_rel_max": werr}
    print("pooled mean against the uniform frame", preset, frame_count, err, werr)
    assert rays(stats) == rays(us)                                        # the same samples: the same rays
    assert err <= 1e-5 and werr <= 1e-5


# ---- 4. the picture entry

@pytest.mark.parametrize("denoised", [False, True])
def test_picture_entry_is_its_sequence(rt, c3, denoised):
    import torch
    case, spp, guide_spp = c3, 8, 2
    p = rr.params(buffers=4)
    dp = rt.default_denoise_features_params() if denoised else None
    pic, stats = case.dev.render_picture_robust(case.cam, case.settings(spp), case.fc, case.w, case.h, case.post, p, dp,
                                                guide_spp=guide_spp, total_frame_index=TFI)
    beauty, _, want_stats = case.robust(spp, p)
    if denoised:
        feats = [case.full(0.0) for _ in range(3)]
        case.dev.render_features_device(case.cam, case.settings(guide_spp), case.fc, case.w, case.h, *[f.data_ptr() for f in feats],
                                        total_frame_index=TFI)
        code = rt.lib().rt_denoise_features_device(0, C.c_void_p(beauty.data_ptr()), *[C.c_void_p(f.data_ptr()) for f in feats],
                                                   case.w, case.h, C.byref(dp), None, C.c_void_p(beauty.data_ptr()), None)
        assert code == 0, rt.lib().rt_last_error()
    d_pic = torch.zeros((case.h, case.w), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize(0)
    code = rt.lib().rt_postprocess_device(0, C.c_void_p(beauty.data_ptr()), case.w, case.h, C.byref(case.post), TFI + 1,
                                          C.c_void_p(d_pic.data_ptr()), None)
    assert code == 0, rt.lib().rt_last_error()
    want = d_pic.cpu().numpy().view(np.uint32)
    REPORT[f"robust_picture_denoised_{int(denoised)}"] = {"differing_pixels": int(np.count_nonzero(pic != want))}
    assert np.array_equal(pic, want)
    assert rays(stats) == rays(want_stats)
    assert len(np.unique(pic)) > 100                                     # a picture, not a constant


# ---- 5. cancel

def test_cancel_mid_loop(rt):
    """rt_cancel from another thread while the frames run returns RT_ERROR_CANCELLED; the next call is bit-exact."""
    case = Case(rt, "c3", 640, 360)
    small = rr.params(buffers=4)
    long = rr.params(buffers=32)                          # 32 frames of 512 spp: far longer than the cancel takes to land
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
        while not returned.is_set():
            case.dev.cancel()
            returned.wait(0.005)

    try:
        before, before_info, _ = case.robust(8, small)
        d = case.full(3.0)
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                case.dev.render_robust_device(case.cam, case.settings(32*512), case.fc, case.w, case.h, long, d.data_ptr(),
                                              total_frame_index=TFI)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
        assert bool((d == 3.0).all())                      # a cancelled call leaves the caller's buffer alone
        after, after_info, _ = case.robust(8, small)
    finally:
        case.close()
    assert same_bits(after, before) and same_bits(after_info, before_info)


def test_nothing_existing_moved(rt):
    """A default rt_render_device frame of C3-small (the default, streaming splat) is byte-identical before and after a
    robust render on the same scene."""
    case = Case(rt, "c3", 192, 108, exact=False)
    try:
        before, after = case.full(0.0), case.full(0.0)
        sb = case.frame(before, 16)
        case.robust(8, rr.params(buffers=4))
        sa = case.frame(after, 16)
    finally:
        case.close()
    assert same_bits(after, before)
    assert rays(sa) == rays(sb) and sa.splat_mode == sb.splat_mode == rt.abi.RT_SPLAT_STREAM
