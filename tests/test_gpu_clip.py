"""Neighbourhood clipping of the temporal history, on the GPU: k_neighbourhood and k_temporal_accumulate_clip against their
plain-C checker (tests/ref_clip) bit for bit, the driver against the loop it is defined as, rt_cancel and a refused call,
the ghost of a moved box's shadow with and without the clip, and the refusals of the device entries."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch        # before the product library's first HIP call: a process has room for one HIP runtime, torch's own

import ref_clip_binding as cb
import ref_deform_binding as db
import ref_temporal_binding as tb
from parity_report import REPORT

pytestmark = pytest.mark.gpu

F = np.float32
TFI = 3          # total_frame_index of every frame here


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def mismatches(a, b):
    a, b = tb.bits(host(a)).reshape(-1), tb.bits(host(b)).reshape(-1)       # texels as their eight words
    assert a.shape == b.shape
    return int(np.count_nonzero(a != b))


def to_device(a):
    """A host array (structured arrays as their 32-bit words) -> a device tensor."""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.float32).reshape(a.shape + (a.dtype.itemsize//4,))
    d = torch.from_numpy(np.array(a)).to("cuda:0")
    torch.cuda.synchronize(0)
    return d


def full(fill, *shape):
    d = torch.full(shape, fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize(0)
    return d


def ptr(t):
    return t.data_ptr() if t is not None else None


def untouched(*ts):
    return all(bool((t == t.flatten()[0]).all()) for t in ts)


def device_stats(rt, d_cur, w, h, radius, clamp):
    d_out = full(-5.0, h, w, 8)
    rt.temporal_neighbourhood_device(d_cur.data_ptr(), w, h, radius, clamp, d_out.data_ptr())
    return d_out


def device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_motion, count, d_surf, d_deform, dcount, moments, velocity,
                 d_nb, gamma, min_count, want_amount, deform_entry=False):
    """rt_temporal_accumulate_clip_device (or the deform stage) into outputs that start as garbage
    -> (history, length, moments, velocity, clip amount)."""
    d_hist, d_len = full(-5.0, h, w, 4), full(-5.0, h, w)
    d_mom = full(-5.0, h, w, 2) if moments else None
    d_vel = full(-5.0, h, w, 2) if velocity else None
    d_amt = full(-5.0, h, w) if want_amount else None
    ph, pl, pg, pm = d_prev if d_prev is not None else (None, None, None, None)
    common = dict(d_motion=ptr(d_motion), motion_count=count, d_prev_moments=ptr(pm) if moments else None, d_moments=ptr(d_mom),
                  d_velocity=ptr(d_vel), d_surface=ptr(d_surf), d_deform=ptr(d_deform), deform_count=dcount)
    if deform_entry:
        rt.temporal_accumulate_deform_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                             d_hist.data_ptr(), d_len.data_ptr(), **common)
    else:
        rt.temporal_accumulate_clip_device(d_cur.data_ptr(), d_g.data_ptr(), ptr(ph), ptr(pl), ptr(pg), cam, amount, w, h, p,
                                           d_hist.data_ptr(), d_len.data_ptr(), d_neighbourhood=ptr(d_nb), gamma=gamma,
                                           min_count=min_count, d_clip_amount=ptr(d_amt), **common)
    return d_hist, d_len, d_mom, d_vel, d_amt


# ---- 1. the statistics against the checker

@pytest.mark.parametrize("w,h", cb.STAT_SIZES)
def test_statistics_match_the_checker(rt, w, h):
    cur = cb.stats_image(w, h)
    d_cur = to_device(cur)
    bad = {}
    for radius in cb.RADII:
        got = device_stats(rt, d_cur, w, h, radius, 10.0)
        bad[radius] = mismatches(got, cb.stats_checked(w, h, radius))
    print(f"{w}x{h}: words that differ from the checker per radius", bad)
    REPORT[f"clip_statistics_{w}x{h}"] = {str(k): v for k, v in bad.items()}
    assert not any(bad.values())
    # no clamp; the host twin
    got = device_stats(rt, d_cur, w, h, 2, 0.0)
    assert mismatches(got, cb.neighbourhood(cur, 2, 0.0)) == 0
    assert mismatches(rt.temporal_neighbourhood(cur, 3, 10.0), cb.stats_checked(w, h, 3)) == 0


# ---- 2. the stage against the checker

@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_stage_matches_the_checker(rt, w, h, amount):
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p = tb.params()
    nb = cb.clip_texels(w, h, amount)
    d_cur, d_g, d_surf, d_moving = to_device(cur), to_device(g), to_device(surf), to_device(moving)
    d_prev = tuple(to_device(a) for a in prev)
    d_arrays = {k: (to_device(t), None if n is None else to_device(n)) for k, (t, n) in arrays.items()}
    table = db.table(tp, {k: (t.data_ptr(), 0 if n is None else n.data_ptr(), w*h) for k, (t, n) in d_arrays.items()})
    d_table = to_device(table)
    # the texels are the device's own, which are the checker's
    d_nb = device_stats(rt, d_cur, w, h, 3, p.firefly_clamp)
    assert mismatches(d_nb, nb) == 0
    bad, clipped = {}, {}
    for gamma in cb.GAMMAS:
        for moments in (False, True):
            for extras in (False, True):            # velocity and clip amount
                got = device_stage(rt, d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), d_surf, d_table, len(table),
                                   moments, extras, d_nb, gamma, 2.0, extras)
                want = cb.checked(w, h, amount, moments, extras, gamma, extras)
                assert all((a is None) == (b is None) for a, b in zip(got, want))
                bad[(gamma, moments, extras)] = sum(mismatches(a, b) for a, b in zip(got, want) if b is not None)
        clipped[gamma] = int((cb.checked(w, h, amount, True, True, gamma, True)[4] > 0).sum())
    print(f"{w}x{h}: words that differ from the checker", bad, "pixels clipped per gamma", clipped)
    REPORT[f"clip_stage_{w}x{h}"] = {str(k): v for k, v in bad.items()}
    assert not any(bad.values()) and clipped[0.0] > clipped[1.0] > clipped[4.0] > 0
    # without history
    got = device_stage(rt, d_cur, d_g, None, None, 0.0, p, w, h, d_moving, len(moving), d_surf, d_table, len(table), True, True,
                       d_nb, 1.0, 2.0, True)
    want = cb.accumulate_clip(cur, g, None, None, 0.0, p, moving, surf, db.host_table(tp, arrays), nb, 1.0, 2.0, want_moments=True,
                              want_velocity=True)
    assert sum(mismatches(a, b) for a, b in zip(got, want)) == 0
    # the host twin: host buffers, a table on the host whose vertex pointers are the device's
    got = rt.temporal_accumulate_clip(cur, g, prev, cam, amount, p, moving, surf, table, nb, 1.0, 2.0, want_moments=True,
                                      want_velocity=True)
    assert sum(mismatches(a, b) for a, b in zip(got, cb.checked(w, h, amount, True, True, 1.0, True))) == 0
    del d_arrays


# ---- 3. the driver against the loop it is defined as

W, H = 96, 64


class Loop:
    """A scene on the device in the exact splat mode, with what a clipped temporal loop needs."""

    def __init__(self, rt, scene, cam, st, fc, w, h):
        self.rt, self.scene, self.cam, self.st, self.fc, self.w, self.h = rt, scene, cam, st, fc, w, h
        self.dev = rt.DeviceScene(scene, 0)
        self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        self.count = len(self.dev.primitive_transforms())

    def frame(self, frame_count):
        d = full(0.0, self.h, self.w, 4)
        s = self.dev.render_device(self.cam, self.st, self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI,
                                   frame_count=frame_count)
        return d, s

    def gbuffer_surface(self):
        d, s = full(float("nan"), self.h, self.w, 8), full(float("nan"), self.h, self.w, 4)
        self.dev.gbuffer_surface_device(self.cam, self.w, self.h, d.data_ptr(), s.data_ptr(), lens_distortion=self.st.lens_distortion)
        return d, s

    def state(self, clipped=True):
        """A fresh rt_temporal_motion_state over a workspace that starts as garbage -> (state, what it points at)."""
        size = self.rt.temporal_clipped_workspace_bytes if clipped else self.rt.temporal_motion_workspace_bytes
        ws = full(float("nan"), (size(self.w, self.h, self.count) + 3)//4)
        store = (self.rt.abi.M4x4Inv*self.count)()
        st = self.rt.TemporalMotionState()
        st.d_workspace, st.transforms, st.transform_cap = ws.data_ptr(), C.cast(store, C.POINTER(self.rt.abi.M4x4Inv)), self.count
        return st, (ws, store)

    def clipped_driver(self, frame_count, p, state, cp, st=None, outputs=None):
        d_out, d_len, d_amt = outputs or (full(9.0, self.h, self.w, 4), full(9.0, self.h, self.w), full(9.0, self.h, self.w))
        s = self.dev.render_temporal_clipped_device(self.cam, st or self.st, self.fc, self.w, self.h, p, state, [], cp,
                                                    d_out.data_ptr(), d_length_out=d_len.data_ptr(),
                                                    d_clip_amount_out=d_amt.data_ptr(), frame_count=frame_count,
                                                    total_frame_index=TFI)
        return d_out, d_len, d_amt, s

    def motion_driver(self, frame_count, p, state):
        d_out, d_len = full(9.0, self.h, self.w, 4), full(9.0, self.h, self.w)
        self.dev.render_temporal_motion_device(self.cam, self.st, self.fc, self.w, self.h, p, state, d_out.data_ptr(),
                                               d_length_out=d_len.data_ptr(), frame_count=frame_count, total_frame_index=TFI)
        return d_out, d_len

    def move(self, step):
        for pid, t in step.items():
            self.scene.set_primitive_transform(pid, t)
        self.scene.create_scene_bvh()
        self.dev.update_instances()

    def close(self):
        self.dev.close()


def rays(s):
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def test_driver_equals_the_loop_on_the_public_entries(rt):
    scene, cam, st, fc, _ = rt.load_preset("c1", W, H)
    st.samples_per_pixel = 1
    loop = Loop(rt, scene, cam, st, fc, W, H)
    try:
        p, cp = tb.params(), rt.default_temporal_clip_params()
        amount = st.lens_distortion
        state, keep = loop.state()
        prev, prev_tr, bad, shares, clipped = None, None, 0, [], []
        for k in range(3):
            if k:
                loop.move({3: rt.translate((3.0 - 0.3*k, 2.0 + 0.1*k, -4.0 - 0.2*k))})
            # rt_render_temporal_clipped_device's definition, on the public entries below it
            f, want_stats = loop.frame(k)
            g, s = loop.gbuffer_surface()
            nb = device_stats(rt, f, W, H, cp.radius, p.firefly_clamp)
            tr = loop.dev.primitive_transforms()
            if prev is None:
                want = device_stage(rt, f, g, None, None, amount, p, W, H, None, 0, s, None, 0, False, False, nb, cp.gamma,
                                    cp.min_count, True)
            else:
                motion, table = rt.motion_table(tr, prev_tr), loop.dev.deform_table([], prev_tr)
                assert int(motion["moved"].sum()) == 1 and not table["deformed"].any()
                want = device_stage(rt, f, g, prev + (None,), cam, amount, p, W, H, to_device(motion), len(motion), s,
                                    to_device(table), len(table), False, False, nb, cp.gamma, cp.min_count, True)
            got_hist, got_len, got_amt, stats = loop.clipped_driver(k, p, state, cp)
            bad += mismatches(got_hist, want[0]) + mismatches(got_len, want[1]) + mismatches(got_amt, want[4])
            assert rays(stats) == rays(want_stats) and stats.samples == W*H
            assert (state.frames, state.parity, state.w, state.h, state.primitive_count) == (k + 1, (k + 1) % 2, W, H, loop.count)
            assert bytes(state.camera) == bytes(cam) and bytes(keep[1]) == tr.tobytes()
            prev, prev_tr = (want[0], want[1], g), tr
            shares.append(float((host(got_len) > 1).mean()))
            clipped.append(int((host(got_amt) > 0).sum()))
        print("C1 clipped driver: share of pixels with a history per frame", shares, "pixels clipped", clipped)
        REPORT["clip_driver_c1"] = {"mismatches": bad, "share_with_history": shares, "clipped": clipped}
        assert bad == 0 and shares[0] == 0.0 and min(shares[1:]) > 0.5 and clipped[0] == 0 and min(clipped[1:]) > 0
        # a refused call leaves the state and the outputs as they were
        before = bytes(state)
        outputs = (full(3.0, H, W, 4), full(3.0, H, W), full(3.0, H, W))
        broken = rt.default_temporal_clip_params()
        broken.gamma = -1.0
        with pytest.raises(rt.RenderError, match="rt_temporal_clip_params: gamma must be finite and >= 0") as ei:
            loop.clipped_driver(3, p, state, broken, outputs=outputs)
        assert ei.value.code == rt.abi.RT_ERROR_INVALID and bytes(state) == before and untouched(*outputs)
        # and so does rt_cancel from another thread while the frame runs
        returned = threading.Event()

        def cancel_until_returned():
            # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
            while not returned.is_set():
                loop.dev.cancel()
                returned.wait(0.005)

        long_frame, _ = rt.default_settings()
        C.memmove(C.byref(long_frame), C.byref(st), C.sizeof(st))
        long_frame.samples_per_pixel = 16384
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                loop.clipped_driver(3, p, state, cp, st=long_frame, outputs=outputs)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED and bytes(state) == before and untouched(*outputs)
        # the next frame goes on from the state as it was; the host twin
        out, length, amt, _ = loop.dev.render_temporal_clipped(cam, st, fc, W, H, state, [], p, cp, frame_count=3,
                                                               total_frame_index=TFI)
        assert state.frames == 4 and float((length > 2).mean()) > 0.5 and (amt >= 0).all() and np.isfinite(out).all()
        del keep
    finally:
        loop.close()


# ---- 4. the ghost the feature exists for

def test_clip_removes_the_ghost_of_a_moved_shadow(rt):
    """A standing camera, a floor, a sphere light and a box whose shadow lies on the floor for frames 0..7; then the box
    moves out of the picture, shadow and all (with both shadows in the mask the history is too dark in one and too bright
    in the other, and the mask's mean hides both), and frames 8..11 follow.  Over the floor pixels whose
    1024-spp luminance differs between the two configurations by more than half of the larger, the mean history of
    frame 11 is nearer the new configuration's 1024-spp mean under the clipped driver than under
    rt_render_temporal_motion_device with the same rt_temporal_params.  Only the direction is asserted.  Measured (the
    default clip parameters): see profiles/clip_quality.txt."""
    scene, box, cam, st, fc = cb.ghost_scene(rt, W, H)
    loop = Loop(rt, scene, cam, st, fc, W, H)
    try:
        p, cp = tb.params(), rt.default_temporal_clip_params()

        def reference():
            many, _ = rt.default_settings()
            C.memmove(C.byref(many), C.byref(st), C.sizeof(st))
            many.samples_per_pixel = 1024
            acc, _ = loop.dev.render(cam, many, fc, W, H, total_frame_index=TFI)
            g = loop.dev.gbuffer(cam, W, H, st.lens_distortion)
            return acc[..., :3]/acc[..., 3:4], g["primitive"] == tb.PLANE_BIT

        ref_old, floor_old = reference()
        cstate, ckeep = loop.state()
        mstate, mkeep = loop.state(clipped=False)
        for k in range(12):
            if k == 8:
                loop.move({box: rt.translate(cb.GHOST_BOX_AT[1])})
            ch, _, amt, _ = loop.clipped_driver(k, p, cstate, cp)
            mh, _ = loop.motion_driver(k, p, mstate)
        ref_new, floor_new = reference()
        mask = cb.ghost_mask(ref_old, ref_new, floor_old & floor_new)
        want = float(cb.luminance(ref_new)[mask].mean())
        clipped_bias = abs(float(cb.luminance(host(ch)[..., :3])[mask].mean()) - want)
        plain_bias = abs(float(cb.luminance(host(mh)[..., :3])[mask].mean()) - want)
        print(f"ghost: mask {int(mask.sum())} pixels, {100.0*mask.mean():.1f} % of the frame; 1024-spp mean luminance there "
              f"{want:.4f}; bias at frame 11: clipped {clipped_bias:.4f}, unclipped {plain_bias:.4f}, "
              f"ratio {clipped_bias/max(plain_bias, 1e-12):.3f}; pixels clipped in frame 11: {int((host(amt) > 0).sum())}")
        REPORT["clip_ghost"] = {"mask": int(mask.sum()), "clipped_bias": clipped_bias, "unclipped_bias": plain_bias}
        assert mask.sum() >= 100
        assert clipped_bias < plain_bias
        del ckeep, mkeep
    finally:
        loop.close()


# ---- 5. refusals, each by name and leaving the outputs untouched

def test_refusals_leave_the_outputs_untouched(rt):
    w, h = 16, 8
    p = tb.params()
    nan, inf = float("nan"), float("inf")
    d_cur, d_out = full(1.0, h, w, 4), full(7.0, h, w, 8)

    def refused(call, text):
        with pytest.raises(rt.RenderError, match=text) as info:
            call()
        assert info.value.code == rt.abi.RT_ERROR_INVALID

    stats = lambda **kw: rt.temporal_neighbourhood_device(**{**dict(d_current=d_cur.data_ptr(), w=w, h=h, radius=3, firefly_clamp=10.0,
                                                                    d_out=d_out.data_ptr()), **kw})
    e = "rt_temporal_neighbourhood_device: "
    refused(lambda: stats(d_current=None), e + "null d_current")
    refused(lambda: stats(d_out=None), e + "null d_out")
    refused(lambda: stats(w=0), e + "w is 0")
    refused(lambda: stats(h=0), e + "h is 0")
    refused(lambda: stats(w=65536, h=65536), e + r"w\*h must be below 2\^32")
    refused(lambda: stats(radius=0), e + r"radius must be in 1\.\.3")
    refused(lambda: stats(radius=4), e + r"radius must be in 1\.\.3")
    for bad in (-1.0, nan, inf):
        refused(lambda: stats(firefly_clamp=bad), e + "firefly_clamp must be finite and >= 0")
    refused(lambda: stats(d_out=d_cur.data_ptr()), e + "d_out aliases d_current")
    assert untouched(d_out, d_cur)
    # the stage
    d_g, d_hist, d_len, d_amt, d_nb = full(0.0, h, w, 8), full(7.0, h, w, 4), full(7.0, h, w), full(7.0, h, w), full(0.5, h, w, 8)
    stage = lambda **kw: rt.temporal_accumulate_clip_device(d_cur.data_ptr(), d_g.data_ptr(), None, None, None, None, 0.0, w, h, p,
                                                            d_hist.data_ptr(), d_len.data_ptr(),
                                                            **{**dict(d_neighbourhood=d_nb.data_ptr(), gamma=1.0, min_count=2.0,
                                                                      d_clip_amount=d_amt.data_ptr()), **kw})
    e = "rt_temporal_accumulate_clip_device: "
    for bad in (-0.5, nan, inf):
        refused(lambda: stage(gamma=bad), e + "gamma must be finite and >= 0")
        refused(lambda: stage(min_count=bad), e + "min_count must be finite and >= 0")
    refused(lambda: stage(deform_count=2), e + "null d_deform with a deform_count")
    refused(lambda: stage(d_deform=d_nb.data_ptr(), deform_count=2), e + "null d_surface with a deform table")
    refused(lambda: stage(motion_count=2), e + "null d_motion with a motion_count")
    refused(lambda: stage(d_prev_moments=d_nb.data_ptr()), e + "d_prev_moments without d_moments")
    assert untouched(d_hist, d_len, d_amt)
    # the driver
    scene, cam, st, fc, _ = rt.load_preset("c1", w, h)
    loop = Loop(rt, scene, cam, st, fc, w, h)
    try:
        state, keep = loop.state()
        outputs = (full(9.0, h, w, 4), full(9.0, h, w), full(9.0, h, w))
        e = "rt_render_temporal_clipped_device: "
        refused(lambda: loop.clipped_driver(0, p, state, None, outputs=outputs), e + "null rt_temporal_clip_params")
        for field, bad, text in (("radius", 0, r"radius must be in 1\.\.3"), ("radius", 4, r"radius must be in 1\.\.3"),
                                 ("gamma", nan, "gamma must be finite and >= 0"), ("min_count", -1.0, "min_count must be finite and >= 0")):
            broken = rt.default_temporal_clip_params()
            setattr(broken, field, bad)
            refused(lambda: loop.clipped_driver(0, p, state, broken, outputs=outputs), e + "rt_temporal_clip_params: " + text)
        refused(lambda: loop.clipped_driver(0, tb.params(snap=-1.0), state, rt.default_temporal_clip_params(), outputs=outputs),
                e + "rt_temporal_params: snap must be finite and >= 0")
        assert untouched(*outputs) and state.frames == 0
        del keep
    finally:
        loop.close()
