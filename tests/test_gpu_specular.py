"""The specular G-buffer on the device ("A specular G-buffer"): k_gbuffer_specular against the plain-C checker
tests/ref_specular bit for bit, every texel and side record; the equivalences and refusals of its entries; the ghost
test, the point of the feature; the driver against the loop written on the public entries; rt_cancel.
"""
import ctypes as C
import threading

import numpy as np
import pytest
import torch        # before the product library's first HIP call: a process has room for one HIP runtime, torch's own

import layout_matrix as lm
import ref_specular_binding as sb
import ref_temporal_binding as tb
from test_gpu_temporal import Case, TFI, device_accumulate, host, mismatches, rays, texels, to_device

pytestmark = pytest.mark.gpu


def device_specular(rt, dev, cam, w, h, p, amount=0.0, want_chain=True, fill=float("nan")):
    """rt_gbuffer_specular_device into buffers that start as garbage -> (texels (h, w), side records (h, w) or None, the
    texels' device tensor)."""
    import torch
    d_g = torch.full((h, w, 8), fill, dtype=torch.float32, device="cuda:0")
    d_c = torch.full((h, w, 4), fill, dtype=torch.float32, device="cuda:0") if want_chain else None
    torch.cuda.synchronize(0)
    dev.gbuffer_specular_device(cam, w, h, p, d_g.data_ptr(), d_c.data_ptr() if want_chain else None, lens_distortion=amount)
    chain = d_c.cpu().numpy().view(rt.abi.SPECULAR_CHAIN_DTYPE).reshape(h, w) if want_chain else None
    return texels(d_g), chain, d_g


def against_the_checker(rt, scene, cam, w, h, p, amount=0.0, dev=None):
    """-> (texel words that differ, side-record words that differ, the checker's side records)."""
    own = dev is None
    if own:
        dev = rt.DeviceScene(scene, 0)
    try:
        g, c, _ = device_specular(rt, dev, cam, w, h, p, amount)
    finally:
        if own:
            dev.close()
    want_g, want_c, _ = sb.gbuffer_specular(scene.desc(), cam, amount, w, h, p)
    return sb.mismatches(g, want_g), sb.mismatches(c, want_c), want_c


# ---- the kernel against the checker, bit for bit

@pytest.mark.parametrize("name", sorted(sb.SCENES))
def test_scenes_match_the_checker(rt, name):
    scene, cam = sb.SCENES[name](rt)
    for p in (sb.params(), sb.params(max_events=16, reflect_threshold=0.3, roughness_max=0.6), sb.params(max_events=1)):
        bad_g, bad_c, want_c = against_the_checker(rt, scene, cam, sb.W, sb.H, p)
        print(f"{name} max_events {p.max_events}: events per pixel {sb.events(want_c).mean():.2f}, ends "
              f"{np.bincount(want_c['end'].ravel(), minlength=6).tolist()}, mismatching words {bad_g} + {bad_c}")
        assert (bad_g, bad_c) == (0, 0)


def test_reflection_from_inside_matches_the_checker(rt):
    """The kernel's `inside` branch with a reflection (total internal reflection, the stack naming the far side): a
    camera inside the glass block, every first hit from inside, some texels reflecting at event 0 and some refracting."""
    scene, cam = sb.inside_glass(rt)
    dev = rt.DeviceScene(scene, 0)
    try:
        for p in (sb.params(max_events=1), sb.params()):
            g, c, _ = device_specular(rt, dev, cam, sb.W, sb.H, p)
            want_g, want_c, _ = sb.gbuffer_specular(scene.desc(), cam, 0.0, sb.W, sb.H, p)
            assert sb.mismatches(g, want_g) == 0 and sb.mismatches(c, want_c) == 0
            assert (c["first_primitive"] == 1).all()
            assert ((c["chain"] & sb.REFLECT0) != 0).sum() > 300 and ((c["chain"] & sb.REFLECT0) == 0).sum() > 300
        plain = dev.gbuffer(cam, sb.W, sb.H)
        assert ((plain["n"]*tb.gbuffer_rays(cam, 0.0, sb.W, sb.H)).sum(axis=2) > 0).all()      # hit from inside
    finally:
        dev.close()


@pytest.mark.parametrize("preset", ["c3", "c4"])
def test_presets_match_the_checker(rt, preset):
    w, h = 96, 54
    scene, cam, st, fc, post = rt.load_preset(preset, w, h)
    bad_g, bad_c, want_c = against_the_checker(rt, scene, cam, w, h, sb.params(), st.lens_distortion)
    print(f"{preset}: events per pixel {sb.events(want_c).mean():.2f}, ends "
          f"{np.bincount(want_c['end'].ravel(), minlength=6).tolist()}, mismatching words {bad_g} + {bad_c}")
    assert (bad_g, bad_c) == (0, 0)
    assert sb.events(want_c).max() >= 2                   # the presets' glass is walked through


@pytest.mark.parametrize("w,h", [(1, 1), (7, 130)])
def test_odd_frames_match_the_checker(rt, w, h):
    scene, cam = sb.mirror_scene(rt, w, h)
    assert against_the_checker(rt, scene, cam, w, h, sb.params(), amount=2.0)[:2] == (0, 0)


def test_a_frame_larger_than_the_grid_matches_the_checker(rt):
    """512 x 257 = 131 584 pixels over the grid's 1024 x 128 = 131 072 threads: 512 lanes walk a second pixel."""
    w, h = 512, 257
    scene, cam = sb.mirror_scene(rt, w, h)
    bad_g, bad_c, want_c = against_the_checker(rt, scene, cam, w, h, sb.params())
    assert (bad_g, bad_c) == (0, 0)
    assert (want_c["chain"].ravel()[131072:] == sb.ONE_REFLECTION).all()      # the last row looks into the mirror


def test_scene_tables_in_hbm_match_the_checker(rt, monkeypatch):
    """tests/test_gpu_layout_matrix.py's scene under its layout L1: the scene tables stay in HBM."""
    scene, cam, st, fc = lm.matrix_scene(rt)
    for k in lm.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in lm.LAYOUTS["L1"].items():
        monkeypatch.setenv(k, v)
    try:
        dev = rt.DeviceScene(scene, 0)
    finally:
        for k in lm.SWITCHES:
            monkeypatch.delenv(k, raising=False)
    try:
        bad_g, bad_c, want_c = against_the_checker(rt, scene, cam, lm.W, lm.H, sb.params(), st.lens_distortion, dev=dev)
    finally:
        dev.close()
    assert (bad_g, bad_c) == (0, 0)
    assert (sb.events(want_c) > 0).any()


# ---- equivalences and refusals

def test_no_events_is_rt_gbuffer_device(rt):
    w, h = 96, 54
    scene, cam, st, fc, post = rt.load_preset("c4", w, h)
    dev = rt.DeviceScene(scene, 0)
    try:
        g, c, _ = device_specular(rt, dev, cam, w, h, sb.params(max_events=0), st.lens_distortion)
        plain = dev.gbuffer(cam, w, h, lens_distortion=st.lens_distortion)
        assert sb.mismatches(g, plain) == 0
        assert (c["chain"] == 0).all() and np.array_equal(c["first_primitive"], plain["primitive"])
        assert np.array_equal(tb.bits(c["first_t"]), tb.bits(plain["t"]))
    finally:
        dev.close()


def test_host_entry_equals_the_device_entry(rt):
    scene, cam = sb.nested_glass(rt)
    dev = rt.DeviceScene(scene, 0)
    try:
        g, c, _ = device_specular(rt, dev, cam, sb.W, sb.H, sb.params())
        hg, hc = dev.gbuffer_specular(cam, sb.W, sb.H, sb.params())
        assert sb.mismatches(hg, g) == 0 and sb.mismatches(hc, c) == 0
        # without a side record the texels are the same
        only, none, _ = device_specular(rt, dev, cam, sb.W, sb.H, sb.params(), want_chain=False)
        assert none is None and sb.mismatches(only, g) == 0
        hg2, none = dev.gbuffer_specular(cam, sb.W, sb.H, sb.params(), want_chain=False)
        assert none is None and sb.mismatches(hg2, g) == 0
    finally:
        dev.close()


def test_refusals_leave_the_outputs_alone(rt):
    import torch
    w, h = sb.W, sb.H
    scene, cam = sb.mirror_scene(rt)
    dev = rt.DeviceScene(scene, 0)
    try:
        d_g = torch.full((h, w, 8), 7.0, dtype=torch.float32, device="cuda:0")
        d_c = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        nan, inf = float("nan"), float("inf")

        def refused(text, p=sb.params(), camera=cam, w_=w, h_=h, out=d_g.data_ptr()):
            ref = lambda x: None if x is None else C.byref(x)
            code = rt.lib().rt_gbuffer_specular_device(dev._h, ref(camera), 0.0, w_, h_, ref(p), C.c_void_p(out),
                                                       C.c_void_p(d_c.data_ptr()), None)
            why = rt.lib().rt_last_error().decode()
            assert code == rt.abi.RT_ERROR_INVALID, (text, code)
            assert why.startswith("rt_gbuffer_specular_device:") and text in why, (text, why)
        refused("null camera", camera=None)
        refused("null d_out", out=None)
        refused("w is 0", w_=0)
        refused("h is 0", h_=0)
        refused("below 2^32", w_=70000, h_=70000)
        refused("null rt_gbuffer_specular_params", p=None)
        refused("max_events must be in 0..16", p=sb.params(max_events=17))
        for v in (-0.5, nan, inf):
            refused("reflect_threshold must be finite", p=sb.params(reflect_threshold=v))
            refused("roughness_max must be finite", p=sb.params(roughness_max=v))
        torch.cuda.synchronize(0)
        assert bool((d_g == 7.0).all()) and bool((d_c == 7.0).all())
    finally:
        dev.close()


def test_a_stale_scene_is_refused(rt):
    """After rt_scene_update_mesh moved a mesh's bounds and before rt_scene_update_instances, as rt_gbuffer_device."""
    import torch
    import ref_refit_binding as rfit
    scene, cam, st, fc = lm.matrix_scene(rt)
    dev = rt.DeviceScene(scene, 0)
    try:
        tris, idx, _, _ = rfit.mesh_arrays(scene.desc(), 0)
        dev.update_mesh(0, rfit.displaced(rfit.original_order(tris, idx), 0.15, 0.4))
        d_g = torch.full((lm.H, lm.W, 8), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        with pytest.raises(rt.RenderError) as ei:
            dev.gbuffer_specular_device(cam, lm.W, lm.H, sb.params(), d_g.data_ptr())
        assert ei.value.code == rt.abi.RT_ERROR_INVALID
        assert "rt_gbuffer_specular_device:" in str(ei.value) and "rt_scene_update_instances" in str(ei.value)
        with pytest.raises(rt.RenderError):
            dev.gbuffer_device(cam, lm.W, lm.H, d_g.data_ptr())
        assert bool((d_g == 7.0).all())
    finally:
        dev.close()


# ---- the ghost test: no ray-traced radiance, a colour that is a function of the world point seen

def test_history_follows_the_reflection(rt):
    """The mirror scene, 6 cameras translating parallel to the mirror.  Each frame's `current` is the world-space checker
    colour of the point the checker's walk ended on, weight 1; rt_temporal_accumulate_device runs over the frames once
    with rt_gbuffer_device's texels and once with rt_gbuffer_specular_device's.  Inside the mirror (one reflection in
    all six frames, eroded by 2 pixels): with specular texels every length is frame + 1, the last history is nearer the
    last current frame than with plain texels, and within twice the error on the directly seen part of the same wall.

    Measured (profiles/specular_quality.txt): 0.05436 with specular texels, 0.17570 with plain ones, 0.04568 on the
    directly seen wall."""
    import torch
    inp = sb.ghost_inputs()
    scene, cams = inp["scene"], inp["cameras"]
    w, h = sb.GW, sb.GH
    dev = rt.DeviceScene(scene, 0)
    try:
        p = tb.params()
        d_cur = [to_device(torch, cur) for cur in inp["current"]]
        d_plain, d_spec = [], []
        for k, cam in enumerate(cams):
            d = torch.full((h, w, 8), float("nan"), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize(0)
            dev.gbuffer_device(cam, w, h, d.data_ptr())
            d_plain.append(d)
            g, c, d = device_specular(rt, dev, cam, w, h, sb.params())
            assert sb.mismatches(g, inp["specular"][k]) == 0 and sb.mismatches(c, inp["chain"][k]) == 0
            d_spec.append(d)

        def accumulate(cur, g, prev, prev_cam):
            return device_accumulate(rt, torch, cur, g, prev, prev_cam, 0.0, p, w, h)
        on_host = lambda run: [(host(a), host(b)) for a, b in run]
        with_specular = on_host(sb.ghost_run(accumulate, d_cur, d_spec, cams))
        with_plain = on_host(sb.ghost_run(accumulate, d_cur, d_plain, cams))
    finally:
        dev.close()
    sb.ghost_assert(with_specular, with_plain, inp)


# ---- the driver

@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_driver_equals_the_loop_on_the_public_entries(rt, clip):
    import torch
    w, h = 96, 54
    case = Case(rt, "c3", w, h)
    try:
        amount = case.st.lens_distortion
        p, sp = tb.params(), sb.params()
        cp = rt.default_temporal_clip_params() if clip else None
        ws = torch.full((rt.temporal_specular_workspace_bytes(w, h)//4,), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        state = rt.TemporalState()
        state.d_workspace = ws.data_ptr()
        prev, prev_cam, bad = None, None, 0
        for k in range(4):
            cam = tb.moved(case.cam, (0.05*k, 0.02*k, -0.1*k))
            # the driver's definition, on the public entries below it
            f, want_stats = case.frame(cam, 1, k)
            _, _, g = device_specular(rt, case.dev, cam, w, h, sp, amount, want_chain=False)
            if clip:
                nb = case.full(float("nan"), h, w, 8)
                rt.temporal_neighbourhood_device(f.data_ptr(), w, h, cp.radius, p.firefly_clamp, nb.data_ptr())
                want_hist, want_len = case.full(-5.0, h, w, 4), case.full(-5.0, h, w)
                ph, pl, pg = (t.data_ptr() for t in prev) if prev is not None else (None, None, None)
                rt.temporal_accumulate_clip_device(f.data_ptr(), g.data_ptr(), ph, pl, pg, prev_cam, amount, w, h, p,
                                                   want_hist.data_ptr(), want_len.data_ptr(), d_neighbourhood=nb.data_ptr(),
                                                   gamma=cp.gamma, min_count=cp.min_count)
            else:
                want_hist, want_len = device_accumulate(rt, torch, f, g, prev, prev_cam, amount, p, w, h)
            d_out, d_len = case.full(9.0, h, w, 4), case.full(9.0, h, w)
            stats = case.dev.render_temporal_specular_device(cam, case.settings(1), case.fc, w, h, p, state, sp, cp,
                                                             d_out.data_ptr(), d_length_out=d_len.data_ptr(), frame_count=k,
                                                             total_frame_index=TFI)
            bad += mismatches(d_out, want_hist) + mismatches(d_len, want_len)
            assert rays(stats) == rays(want_stats) and stats.samples == w*h
            assert (state.frames, state.parity, state.w, state.h) == (k + 1, (k + 1) % 2, w, h)
            assert bytes(state.camera) == bytes(cam) and state.lens_distortion == amount
            prev, prev_cam = (want_hist, want_len, g), cam
        assert bad == 0
        assert float((host(want_len) > 1).mean()) > 0.3
        # the host entry goes on from the same state; another frame size restarts it
        out, length, _ = case.dev.render_temporal_specular(cam, case.settings(1), case.fc, w, h, state, p, sp, cp, frame_count=4,
                                                           total_frame_index=TFI)
        assert state.frames == 5 and float((length > 4).mean()) > 0.3 and np.isfinite(out).mean() > 0.99
        small = Case(rt, "c3", 48, 27)
        try:
            out, length, _ = small.dev.render_temporal_specular(small.cam, small.settings(1), small.fc, 48, 27, state, p, sp, cp,
                                                                total_frame_index=TFI)
            assert (length[np.isfinite(out).all(axis=2)] == 1.0).all() and (state.frames, state.w, state.h) == (6, 48, 27)
        finally:
            small.close()
        del ws
    finally:
        case.close()


def test_cancel_leaves_the_state_alone(rt):
    """rt_cancel from another thread while the frame runs returns RT_ERROR_CANCELLED; the state and the outputs stay."""
    import torch
    w, h = 640, 360
    case = Case(rt, "c3", w, h)
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
        while not returned.is_set():
            case.dev.cancel()
            returned.wait(0.005)

    try:
        p, sp = tb.params(), sb.params()
        ws = torch.full((rt.temporal_specular_workspace_bytes(w, h)//4,), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
        state = rt.TemporalState()
        state.d_workspace = ws.data_ptr()

        def driver(spp, frame_count, d_out, d_len):
            return case.dev.render_temporal_specular_device(case.cam, case.settings(spp), case.fc, w, h, p, state, sp, None,
                                                            d_out.data_ptr(), d_length_out=d_len.data_ptr(),
                                                            frame_count=frame_count, total_frame_index=TFI)
        d_out, d_len = case.full(3.0, h, w, 4), case.full(3.0, h, w)
        driver(2, 0, d_out, d_len)
        before = bytes(state)
        d_out, d_len = case.full(3.0, h, w, 4), case.full(3.0, h, w)
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                driver(16384, 1, d_out, d_len)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
        assert bytes(state) == before and bool((d_out == 3.0).all()) and bool((d_len == 3.0).all())
        # the next frame goes on from the state as it was
        driver(2, 1, d_out, d_len)
        assert state.frames == 2 and float((host(d_len) == 2.0).mean()) > 0.8
        del ws
    finally:
        case.close()
