"""Temporal accumulation on the device ("Temporal accumulation"): the G-buffer kernel (rt_gbuffer,
rt_gbuffer_device) and the accumulate kernel (rt_temporal_accumulate, rt_temporal_accumulate_device) against the
plain-C checker tests/ref_temporal, bit for bit; the driver (rt_render_temporal_device) against the same loop written
here on the public entries below it, bit for bit; a standing camera's history against the mean of its frames; a
camera moving along a wall against the closed form; rt_cancel.

Scenes are the suite's small presets (C1 at 130x70, C3 and C4 at 192x108) with the exact splat configured and one or
two samples per pixel: what can go wrong is the reprojection and the bookkeeping, not the paths.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import ref_temporal_binding as tb
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 3          # total_frame_index of every frame here


def rays(s):
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def mismatches(a, b):
    return int(np.count_nonzero(tb.bits(host(a)) != tb.bits(host(b))))


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


class Case:
    """A scene on the device in the exact splat mode."""

    def __init__(self, rt, preset, w, h, scene=None, cam=None):
        import torch
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        if scene is None:
            self.scene, self.cam, self.st, self.fc, self.post = rt.load_preset(preset, w, h)
        else:
            self.scene, self.cam = scene, cam
            self.st, self.post = rt.default_settings()
            self.st.lens_distortion = 0.0
            self.fc = rt.load_reconstruction_kernel("Box")       # every pixel's weight is its sample count
        self.dev = rt.DeviceScene(self.scene, 0)
        self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)

    def full(self, fill, *shape):
        d = self.torch.full(shape, fill, dtype=self.torch.float32, device="cuda:0")
        self.torch.cuda.synchronize(0)
        return d

    def settings(self, spp):
        s = self.rt.abi.Settings.from_buffer_copy(self.st)
        s.samples_per_pixel = spp
        return s

    def frame(self, cam, spp, frame_count):
        """One frame into a zeroed device buffer -> (d_frame, stats)."""
        d = self.full(0.0, self.h, self.w, 4)
        s = self.dev.render_device(cam, self.settings(spp), self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI,
                                   frame_count=frame_count)
        return d, s

    def gbuffer(self, cam):
        d = self.full(float("nan"), self.h, self.w, 8)
        self.dev.gbuffer_device(cam, self.w, self.h, d.data_ptr(), lens_distortion=self.st.lens_distortion)
        return d

    def state(self):
        """A fresh rt_temporal_state over a workspace that starts as garbage -> (state, the workspace's tensor)."""
        ws = self.torch.full((self.rt.temporal_workspace_bytes(self.w, self.h)//4,), float("nan"), dtype=self.torch.float32,
                             device="cuda:0")
        self.torch.cuda.synchronize(0)
        st = self.rt.TemporalState()
        st.d_workspace = ws.data_ptr()
        return st, ws

    def driver(self, cam, spp, frame_count, p, state):
        """rt_render_temporal_device into buffers that start as garbage -> (d_out, d_length, stats)."""
        d_out, d_len = self.full(9.0, self.h, self.w, 4), self.full(9.0, self.h, self.w)
        s = self.dev.render_temporal_device(cam, self.settings(spp), self.fc, self.w, self.h, p, state, d_out.data_ptr(),
                                            d_length_out=d_len.data_ptr(), frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_len, s

    def close(self):
        self.dev.close()


def device_accumulate(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h):
    """rt_temporal_accumulate_device into outputs that start as garbage -> (d_history, d_length)."""
    d_hist = torch.full((h, w, 4), -5.0, dtype=torch.float32, device="cuda:0")
    d_len = torch.full((h, w), -5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    ph, pl, pg = d_prev if d_prev is not None else (None, None, None)
    rt.temporal_accumulate_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                  d_hist.data_ptr(), d_len.data_ptr())
    return d_hist, d_len


def moved_along(rt, cam, dx=0.0, dy=0.0, dz=0.0):
    """A copy of `cam` translated along its own axes."""
    c = rt.abi.Camera.from_buffer_copy(cam)
    c.p = rt.v3(*[getattr(cam.p, k) + dx*getattr(cam.x, k) + dy*getattr(cam.y, k) + dz*getattr(cam.z, k) for k in "xyz"])
    return c


@pytest.fixture(scope="module")
def c1(rt):
    case = Case(rt, "c1", 130, 70)
    yield case
    case.close()


@pytest.fixture(scope="module")
def c3(rt):
    case = Case(rt, "c3", 192, 108)
    yield case
    case.close()


# ---- 1. the G-buffer against the checker

def gbuffer_mismatches(got, want):
    return {f: int(np.count_nonzero(tb.bits(np.ascontiguousarray(got[f])) != tb.bits(np.ascontiguousarray(want[f]))))
            for f in ("p", "t", "n", "primitive")}


@pytest.mark.parametrize("preset,w,h", [("c1", 130, 70), ("c3", 192, 108), ("c4", 192, 108), ("c1", 1, 1), ("c1", 5, 3),
                                        ("c1", 7, 130)])
def test_gbuffer_matches_the_checker(rt, preset, w, h):
    case = Case(rt, preset, w, h)
    try:
        amount = case.st.lens_distortion                 # the preset's own
        want = tb.gbuffer(case.scene.desc(), case.cam, amount, w, h)
        got = case.dev.gbuffer(case.cam, w, h, amount)
        bad = gbuffer_mismatches(got, want)
        hit = want["primitive"] != tb.MISS
        REPORT[f"gbuffer_{preset}_{w}x{h}"] = dict(bad, hits=int(hit.sum()), lens_distortion=float(amount))
        print(preset, w, h, "lens distortion", amount, "hits", int(hit.sum()), "of", w*h, "mismatches", bad)
        assert bad == {"p": 0, "t": 0, "n": 0, "primitive": 0}
        # a second call on the same scene, and the device entry into a buffer that starts as garbage
        again = case.dev.gbuffer(case.cam, w, h, amount)
        assert np.array_equal(tb.bits(again), tb.bits(got))
        assert np.array_equal(tb.bits(texels(case.gbuffer(case.cam))), tb.bits(got))
        # a miss is the ray's direction, no distance and no normal
        if (~hit).any():
            d = tb.gbuffer_rays(case.cam, amount, w, h)
            assert np.array_equal(tb.bits(got["p"][~hit]), tb.bits(d[~hit]))
            assert (got["t"][~hit] == 0).all() and (got["n"][~hit] == 0).all()
    finally:
        case.close()


def test_gbuffer_grid_stride_at_1080p(rt, c3):
    """1920x1080 is 16200 blocks of pixels on a grid of 1024: every thread takes 15 or 16 pixels.  Five rows of the
    frame, every third column, held to rt_debug_intersect on the checker's rays of those pixels."""
    w, h = 1920, 1080
    scene, cam, st, fc, post = rt.load_preset("c3", w, h)
    got = c3.dev.gbuffer(cam, w, h, st.lens_distortion)
    rows = [0, 1, 539, 1078, 1079]
    d = tb.gbuffer_rays(cam, st.lens_distortion, w, h)
    o = (cam.p.x, cam.p.y, cam.p.z)
    q = [rt.abi.RayQuery(rt.v3(*o), rt.v3(*[float(c) for c in d[y, x]]), 3.402823466e38, 0) for y in rows for x in range(0, w, 3)]
    want = c3.dev.intersect(q)
    bad = 0
    for k, (y, x) in enumerate((y, x) for y in rows for x in range(0, w, 3)):
        g, r = got[y, x], want[k]
        if r.primitive == tb.MISS:
            bad += not (g["primitive"] == tb.MISS and g["t"] == 0 and np.array_equal(tb.bits(g["p"]), tb.bits(d[y, x])))
        else:
            bad += not (g["primitive"] == r.primitive and g["t"] == r.t and tuple(g["p"]) == (r.hit_p.x, r.hit_p.y, r.hit_p.z)
                        and tuple(g["n"]) == (r.n.x, r.n.y, r.n.z))
    assert bad == 0


# ---- 2. the accumulate kernel against the checker

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_accumulate_matches_the_checker_on_synthetic_inputs(rt, w, h, amount):
    import torch
    cur, g, prev, cam = tb.synthetic_case(w, h, amount)
    want_hist, want_len = tb.checked(w, h, amount)
    d_cur, d_g = to_device(torch, cur), to_device(torch, g)
    d_prev = tuple(to_device(torch, a) for a in prev)
    p = tb.params()
    got_hist, got_len = device_accumulate(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h)
    bad = mismatches(got_hist, want_hist) + mismatches(got_len, want_len)
    # the inputs are only read
    assert mismatches(d_cur, cur) == 0 and mismatches(texels(d_g), g) == 0
    assert mismatches(d_prev[0], prev[0]) == 0 and mismatches(d_prev[1], prev[1]) == 0 and mismatches(texels(d_prev[2]), prev[2]) == 0
    # other parameters: no snap, no clamp, a short history, loose and strict surface tests
    for q in (tb.params(snap=0.0, firefly_clamp=0.0), tb.params(max_history=2.5, normal_cos=-1.0, plane_tolerance=10.0),
              tb.params(max_history=1.0), tb.params(normal_cos=1.0, plane_tolerance=0.0, snap=0.5)):
        w_hist, w_len = tb.accumulate(cur, g, prev, cam, amount, q)
        g_hist, g_len = device_accumulate(rt, torch, d_cur, d_g, d_prev, cam, amount, q, w, h)
        bad += mismatches(g_hist, w_hist) + mismatches(g_len, w_len)
    # no history
    w_hist, w_len = tb.accumulate(cur, g, None, None, 0.0, p)
    g_hist, g_len = device_accumulate(rt, torch, d_cur, d_g, None, None, 0.0, p, w, h)
    bad += mismatches(g_hist, w_hist) + mismatches(g_len, w_len)
    # the host entry
    h_hist, h_len = rt.temporal_accumulate(cur, g, prev, cam, amount, p)
    bad += mismatches(h_hist, want_hist) + mismatches(h_len, want_len)
    REPORT[f"temporal_accumulate_{w}x{h}"] = {"mismatches": bad}
    assert bad == 0


def test_accumulate_refuses_an_aliased_history(rt):
    import torch
    w, h, amount = tb.SIZES[0]
    cur, g, prev, cam = tb.synthetic_case(w, h, amount)
    d_cur, d_g = to_device(torch, cur), to_device(torch, g)
    d_prev = tuple(to_device(torch, a) for a in prev)
    d_len = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    d_hist = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    for hist, length, text in ((d_prev[0], d_len, "d_history aliases d_prev_history"), (d_hist, d_prev[1], "d_length aliases d_prev_length")):
        with pytest.raises(rt.RenderError) as ei:
            rt.temporal_accumulate_device(d_cur.data_ptr(), d_g.data_ptr(), d_prev[0].data_ptr(), d_prev[1].data_ptr(),
                                          d_prev[2].data_ptr(), cam, amount, w, h, tb.params(), hist.data_ptr(), length.data_ptr())
        assert ei.value.code == rt.abi.RT_ERROR_INVALID and text in str(ei.value)
    assert mismatches(d_prev[0], prev[0]) == 0 and mismatches(d_prev[1], prev[1]) == 0


def test_accumulate_matches_the_checker_on_two_real_cameras(rt, c3):
    """C3 at 192x108 from two cameras a short flight apart: the kernels' own G-buffers and frames, the checker's blend."""
    import torch
    case, w, h = c3, c3.w, c3.h
    amount = case.st.lens_distortion
    cam_a = case.cam
    cam_b = moved_along(rt, cam_a, dx=1.0, dy=-0.3, dz=-1.0)
    p = tb.params()
    fa, _ = case.frame(cam_a, 2, 0)
    fb, _ = case.frame(cam_b, 2, 2)
    ga, gb = case.gbuffer(cam_a), case.gbuffer(cam_b)
    ha, la = device_accumulate(rt, torch, fa, ga, None, None, 0.0, p, w, h)
    hb, lb = device_accumulate(rt, torch, fb, gb, (ha, la, ga), cam_a, amount, p, w, h)
    want_a = tb.accumulate(host(fa), texels(ga), None, None, 0.0, p)
    want_b = tb.accumulate(host(fb), texels(gb), (host(ha), host(la), texels(ga)), cam_a, amount, p)
    bad = mismatches(ha, want_a[0]) + mismatches(la, want_a[1]) + mismatches(hb, want_b[0]) + mismatches(lb, want_b[1])
    share = float((host(lb) > 1).mean())
    REPORT["temporal_accumulate_c3_two_cameras"] = {"mismatches": bad, "share_with_history": share}
    print("C3, two cameras: share of pixels with a history", share)
    assert bad == 0 and share > 0.3                      # most of the picture is kept


# ---- 3. the driver against the loop

def camera_path(rt, cam, k):
    return moved_along(rt, cam, dx=0.05*k, dy=0.02*k, dz=-0.1*k)


def test_driver_equals_the_hand_written_loop(rt, c1):
    import torch
    case, w, h = c1, c1.w, c1.h
    amount = case.st.lens_distortion
    p = tb.params()
    state, ws = case.state()
    prev, prev_cam = None, None
    bad, shares = 0, []
    for k in range(4):
        cam = camera_path(rt, case.cam, k)
        # rt_render_temporal_device's definition, on the public entries below it
        f, want_stats = case.frame(cam, 1, k)
        g = case.gbuffer(cam)
        want_hist, want_len = device_accumulate(rt, torch, f, g, prev, prev_cam, amount, p, w, h)
        got_hist, got_len, stats = case.driver(cam, 1, k, p, state)
        bad += mismatches(got_hist, want_hist) + mismatches(got_len, want_len)
        assert rays(stats) == rays(want_stats) and stats.samples == w*h
        assert (state.frames, state.parity, state.w, state.h) == (k + 1, (k + 1) % 2, w, h)
        assert bytes(state.camera) == bytes(cam) and state.lens_distortion == amount
        prev, prev_cam = (want_hist, want_len, g), cam
        shares.append(float((host(got_len) > 1).mean()))
    REPORT["temporal_driver_c1"] = {"mismatches": bad, "share_with_history": shares}
    print("C1 driver: share of pixels with a history per frame", shares)
    assert bad == 0 and shares[0] == 0.0 and min(shares[1:]) > 0.3
    # another frame size restarts the state; the host entry and a NULL length output
    small = Case(rt, "c1", 65, 33)
    try:
        # (the 130x70 workspace holds a 65x33 frame's)
        out, length, _ = small.dev.render_temporal(small.cam, small.settings(1), small.fc, 65, 33, state, p, frame_count=0,
                                                   total_frame_index=TFI)
        assert (length[np.isfinite(out).all(axis=2)] == 1.0).all() and (state.frames, state.w, state.h) == (5, 65, 33)
        out2, none, _ = small.dev.render_temporal(small.cam, small.settings(1), small.fc, 65, 33, state, p, frame_count=1,
                                                  total_frame_index=TFI, want_length=False)
        assert none is None and state.frames == 6 and np.isfinite(out2).mean() > 0.99
    finally:
        small.close()
    del ws


def test_standing_camera_is_the_mean_of_its_frames(rt, c1):
    """Eight 1-spp frames of C1 with frame_count 0..7; the preset's Box filter gives every pixel weight 1.  The
    history is a running mean of eight f32 steps: the robust driver's pooled-mean bar, rel L2 1e-5."""
    case, w, h = c1, c1.w, c1.h
    p = tb.params()
    frames = np.stack([host(case.frame(case.cam, 1, k)[0]) for k in range(8)]).astype(np.float64)
    with np.errstate(all="ignore"):
        colour = frames[..., :3]/frames[..., 3:]
    good = (np.isfinite(colour).all(axis=3) & (frames[..., 3] > 0.001)).all(axis=0)
    print("standing camera: pixels finite in all eight frames", float(good.mean()))
    assert good.mean() >= 0.99                            # else the input is to blame
    state, ws = case.state()
    for k in range(8):
        hist, length, _ = case.driver(case.cam, 1, k, p, state)
    hist, length = host(hist).astype(np.float64), host(length)
    want = np.clip(colour, 0.0, 10.0).mean(axis=0)
    err = float(np.linalg.norm(hist[..., :3][good] - want[good])/np.linalg.norm(want[good]))
    REPORT["temporal_standing_camera_c1"] = {"rel_l2": err, "good_share": float(good.mean())}
    print("standing camera: history against the float64 mean, rel L2", err)
    assert (length[good] == 8.0).all() and (hist[..., 3][good] == 1.0).all()
    assert err <= 1e-5
    del ws


def wall_scene(rt):
    """Planes only: one wall facing the camera, under a sky."""
    s = rt.Scene()
    m = s.add_diffuse_material((0.6, 0.5, 0.4), 1.5)
    s.add_plane(m, (0.0, 0.0, -1.0), -3.0)           # z = 3, facing -z
    s.set_sky((0.6, 0.7, 0.9), (0.1, 0.1, 0.1))
    s.create_scene_bvh()
    return s


def test_moving_camera_along_a_wall(rt):
    """A camera 8 units in front of a wall, translated parallel to it: the picture moves by the closed form
    d * film_distance * w / (2 * z * half_film_w) pixels, and the strip that comes into view has no history."""
    w, h, depth, shift = 130, 70, 8.0, 4.5
    cam0 = rt.abi.Camera()
    cam0.vfov = rt.DEG_TO_RAD*50.0
    cam0.aspect_ratio = w/h
    cam0.lens_radius = 0.0
    cam0.focus_distance = 10.0
    cam0.p = rt.v3(0.0, 1.0, -5.0)
    rt.aim_camera_at(cam0, (0.0, 1.0, 0.0))
    rt.recompute_camera(cam0)
    d = shift*2.0*depth*cam0.half_film_w/(cam0.film_distance*w)
    cam1 = moved_along(rt, cam0, dx=d)
    case = Case(rt, None, w, h, scene=wall_scene(rt), cam=cam0)
    try:
        p = tb.params()
        state, ws = case.state()
        h0, l0, _ = case.driver(cam0, 1, 0, p, state)
        h1, l1, _ = case.driver(cam1, 1, 1, p, state)
        g0, g1 = texels(case.gbuffer(cam0)), texels(case.gbuffer(cam1))
        assert (g0["primitive"] == tb.PLANE_BIT).all() and np.abs(g0["t"][h//2, w//2] - depth) < 0.05
        # the checker on the same G-buffers and frames: the same lengths, pixel by pixel
        f1 = host(case.frame(cam1, 1, 1)[0])
        want_hist, want_len = tb.accumulate(f1, g1, (host(h0), host(l0), g0), cam0, case.st.lens_distortion, p)
        l1 = host(l1)
        assert np.array_equal(l1, want_len) and mismatches(h1, want_hist) == 0
        assert (host(l0) == 1.0).all() and ((l1 == 1.0) | (l1 == 2.0)).all()
        # the uncovered strip: floor(shift) columns at one edge, in every row that is clear of the corners
        rows = slice(h//4, 3*h//4)
        fresh = l1[rows] == 1.0
        cols = np.nonzero(fresh.any(axis=0))[0]
        assert fresh[:, cols].all() and len(cols) == int(np.floor(shift))
        assert list(cols) in (list(range(len(cols))), list(range(w - len(cols), w)))
        del ws
    finally:
        case.close()


# ---- 4. cancel

def test_cancel_leaves_the_state_alone(rt):
    """rt_cancel from another thread while the frame runs returns RT_ERROR_CANCELLED; the state and the outputs stay."""
    case = Case(rt, "c3", 640, 360)
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
        while not returned.is_set():
            case.dev.cancel()
            returned.wait(0.005)

    try:
        p = tb.params()
        state, ws = case.state()
        case.driver(case.cam, 2, 0, p, state)
        before = bytes(state)
        d_out, d_len = case.full(3.0, case.h, case.w, 4), case.full(3.0, case.h, case.w)
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                case.dev.render_temporal_device(case.cam, case.settings(16384), case.fc, case.w, case.h, p, state,
                                                d_out.data_ptr(), d_length_out=d_len.data_ptr(), frame_count=1,
                                                total_frame_index=TFI)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
        assert bytes(state) == before and bool((d_out == 3.0).all()) and bool((d_len == 3.0).all())
        # the next frame goes on from the state as it was (C3's mesh with zero normals, 3 % of the frame, keeps no
        # history under the default normal_cos: DESIGN.md)
        _, length, _ = case.driver(case.cam, 2, 1, p, state)
        assert state.frames == 2 and float((host(length) == 2.0).mean()) > 0.9
        del ws
    finally:
        case.close()
