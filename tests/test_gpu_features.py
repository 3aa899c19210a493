"""Feature frames and the denoise stage that uses them on the device: rt_render_feature(_device),
rt_denoise_features(_device) and rt_render_picture_features_denoised against the plain-C checker
tests/ref_features, bit for bit ("Feature frames")."""
import ctypes as C

import numpy as np
import pytest

import recursive_cases as rc
import ref_denoise_binding as rd
import ref_features_binding as rf
from parity_report import REPORT
from random_scenes import random_scene

pytestmark = pytest.mark.gpu

NORMAL, DISTANCE, ALBEDO = range(3)
FEATURE_NAME = ("normal", "distance", "albedo")
NORMALS, DISTANCES = 4, 5            # rt_integrator
TFI = 5


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def with_settings(st, **fields):
    c = type(st).from_buffer_copy(st)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def build(rt, name):
    """name -> (scene, cam, st, fc, w, h): the issue's shapes."""
    if name.startswith("random"):
        w, h = 67, 35                                    # ragged against the 64-wide tiles and blocks
        scene, cam, st, fc = random_scene(rt, int(name[6:]), w, h, spp=2)
    elif name == "mirrors":
        w, h = 65, 33
        scene, cam, st, fc = rc.mirrors_scene(rt, w, h)             # max_bounce_count 63: the bound
    else:
        w, h = (64, 64) if name == "c1" else (96, 54)
        scene, cam, st, fc, post = rt.load_preset(name, w, h)
        st.samples_per_pixel = 2
    return scene, cam, st, fc, w, h


@pytest.fixture(scope="module", autouse=True)
def _torch_device():
    """The filter and picture tests hand torch's device buffers to the library: torch opens the device before
    the module's scenes do, whichever test runs first."""
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize(0)


@pytest.fixture(scope="module")
def scenes(rt):
    made = {}

    def get(name):
        if name not in made:
            scene, cam, st, fc, w, h = build(rt, name)
            made[name] = (scene, cam, st, fc, w, h, rt.DeviceScene(scene, 0))
        return made[name]
    yield get
    for v in made.values():
        v[-1].close()


def check_frame(rt, dev, scene, cam, st, fc, w, h, feature, key, **kw):
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        frame, stats = dev.render_feature(cam, st, fc, w, h, feature, **kw)
    want, wstats, spec = rf.render(scene.desc(), cam, st, fc, w, h, feature, **kw)
    n = int(np.count_nonzero(np.any(rf.bits(frame) != rf.bits(want), axis=2)))
    REPORT[key] = {"mismatching_pixels": n, "gpu_closest": int(stats.closest_hit_rays),
                   "cpu_closest": int(wstats.closest_hit_rays), "specular_bounces": spec}
    print(key, REPORT[key])
    assert stats.splat_mode == rt.abi.RT_SPLAT_EXACT
    assert n == 0
    assert stats.closest_hit_rays == wstats.closest_hit_rays and stats.samples == wstats.samples
    assert stats.shadow_rays == 0 and stats.traced_rays[1] == 0
    assert stats.closest_hit_rays - stats.samples == spec
    return frame, stats, spec


# ---- exact-splat parity

@pytest.mark.parametrize("feature", [NORMAL, DISTANCE, ALBEDO])
@pytest.mark.parametrize("name", ["c1", "c3", "c4", "random21", "random22", "random23", "mirrors"])
def test_exact_frames_match_the_checker(rt, scenes, name, feature):
    scene, cam, st, fc, w, h, dev = scenes(name)
    frame, stats, spec = check_frame(rt, dev, scene, cam, st, fc, w, h, feature,
                                     f"feature_{FEATURE_NAME[feature]}_{name}", total_frame_index=TFI)
    assert np.isfinite(frame).all()
    if feature != DISTANCE:                    # (C1 lies wholly past the 15 units DISTANCE saturates at)
        assert np.abs(frame[..., :3]).max() > 0.01
    if name == "mirrors":                      # some walks of this frame run to the bound: 63 hits, 62 bounces followed
        xy, so = rc.all_samples(w, h, st.samples_per_pixel)
        _, end, bounces, _, _ = rf.trace_samples(scene.desc(), cam, st, w, h, xy, so, feature, total_frame_index=TFI)
        assert (end == rf.END_BOUND).sum() > 0 and bounces.max() == 62 and bounces.sum() == spec
    if name in ("c3", "c4"):
        assert spec > 0                        # something is seen through a specular vertex


@pytest.mark.parametrize("feature", [NORMAL, DISTANCE, ALBEDO])
def test_one_pixel_and_per_sample_parity(rt, scenes, feature):
    """1 x 1; and the box filter at 1 spp, where a pixel is its one sample (weight 1)."""
    scene, cam, st, fc, w, h, dev = scenes("c3")
    scene1, cam1, st1, fc1, post = rt.load_preset("c3", 1, 1)
    check_frame(rt, dev, scene, cam1, with_settings(st1, samples_per_pixel=2), fc1, 1, 1, feature,
                f"feature_{FEATURE_NAME[feature]}_1x1")
    box = rt.load_reconstruction_kernel("Box")
    frame, _, _ = check_frame(rt, dev, scene, cam, with_settings(st, samples_per_pixel=1), box, w, h, feature,
                              f"feature_{FEATURE_NAME[feature]}_box_1spp")
    assert np.all(frame[..., 3] == 1.0)
    xy, so = rc.all_samples(w, h, 1)
    samples = rf.trace_samples(scene.desc(), cam, with_settings(st, samples_per_pixel=1), w, h, xy, so, feature)[0]
    assert np.array_equal(rf.bits(frame[..., :3].reshape(-1, 3)), rf.bits(samples[:, :3]))


# ---- the device's own first-hit frames

@pytest.mark.parametrize("bounces", [0, 1])
def test_device_anchor(rt, scenes, bounces):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, max_bounce_count=bounces)
    for mode, parts in ((rt.abi.RT_SPLAT_EXACT, 4), (rt.abi.RT_SPLAT_STREAM, 1), (rt.abi.RT_SPLAT_STREAM, 4)):
        with dev.configured(splat_mode=mode, partitions=parts):
            for feature, integ in ((NORMAL, NORMALS), (DISTANCE, DISTANCES)):
                f, fs = dev.render_feature(cam, st, fc, w, h, feature, total_frame_index=TFI)
                g, gs = dev.render(cam, with_settings(st, integrator=integ), fc, w, h, total_frame_index=TFI)
                assert fs.splat_mode == gs.splat_mode == mode
                assert np.array_equal(rf.bits(f), rf.bits(g)), (mode, parts, feature)
                assert fs.closest_hit_rays == gs.closest_hit_rays == fs.samples == w*h*st.samples_per_pixel


# ---- the schedule does not enter a feature frame

def test_schedule_independence(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, samples_per_pixel=4)
    E = rt.abi.RT_SPLAT_EXACT
    figures = {}
    for feature in (NORMAL, DISTANCE, ALBEDO):
        frames = {}
        for parts, fuse, every in ((1, -1, 1), (4, -1, 1), (4, 0, 3), (1, 1000, 3)):
            with dev.configured(splat_mode=E, partitions=parts, fuse_paths=fuse, drain_every=every):
                frames[(parts, fuse, every)] = dev.render_feature(cam, st, fc, w, h, feature)
        base, bstats = frames[(1, -1, 1)]
        for k, (f, s) in frames.items():
            assert np.array_equal(rf.bits(f), rf.bits(base)), (feature, k)
            assert (s.closest_hit_rays, s.shadow_rays, s.samples) == (bstats.closest_hit_rays, 0, bstats.samples), k
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM):
            stream, sstats = dev.render_feature(cam, st, fc, w, h, feature)
            tiles = [dev.render_feature(cam, st, fc, w, h, feature, shard_index=r, shard_count=2) for r in range(2)]
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM, shard_mode=rt.abi.RT_SHARD_PASSES):
            passes = [dev.render_feature(cam, st, fc, w, h, feature, shard_index=r, shard_count=2) for r in range(2)]
        fig = {"stream_vs_exact": rel_l2(stream, base),
               "tile_shards": rel_l2(sum(p[0].astype(np.float64) for p in tiles), base),
               "pass_shards": rel_l2(sum(p[0].astype(np.float64) for p in passes), base)}
        figures[FEATURE_NAME[feature]] = fig
        print(FEATURE_NAME[feature], fig)
        assert sstats.splat_mode == rt.abi.RT_SPLAT_STREAM and sstats.closest_hit_rays == bstats.closest_hit_rays
        assert fig["stream_vs_exact"] <= 2e-6
        for name, shards in (("tile_shards", tiles), ("pass_shards", passes)):
            assert fig[name] <= 2e-6
            assert sum(p[1].closest_hit_rays for p in shards) == bstats.closest_hit_rays
            assert sum(p[1].samples for p in shards) == bstats.samples
            assert all(p[1].shadow_rays == 0 for p in shards)
    REPORT["feature_schedule"] = figures


# ---- feature frames leave the Advanced schedule alone

def test_no_leak_into_advanced(rt, scenes):
    scene, cam, st, fc, w, h, dev = scenes("c3")
    a = rt.abi
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT, shadow_launch=a.RT_SHADOW_LAUNCH_AUTO):
        f0, s0 = dev.render(cam, st, fc, w, h)
        for feature in (NORMAL, DISTANCE, ALBEDO):
            _, sf = dev.render_feature(cam, st, fc, w, h, feature)
            assert sf.shadow_rays == 0 and sf.traced_rays[1] == 0
        f1, s1 = dev.render(cam, st, fc, w, h)
    assert np.array_equal(rf.bits(f0), rf.bits(f1))
    assert s0.shadow_launch == s1.shadow_launch
    assert (s0.closest_hit_rays, s0.shadow_rays) == (s1.closest_hit_rays, s1.shadow_rays) and s0.shadow_rays > 0


def test_a_bad_feature_is_refused_by_name(rt, scenes):
    scene, cam, st, fc, w, h, dev = scenes("c1")
    for feature in (-1, 3):
        with pytest.raises(rt.RenderError) as e:
            dev.render_feature(cam, st, fc, w, h, feature)
        assert e.value.code == rt.abi.RT_ERROR_INVALID and "feature" in str(e.value)
    # rt_settings::integrator is ignored
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        f0, _ = dev.render_feature(cam, st, fc, w, h, ALBEDO)
        f1, _ = dev.render_feature(cam, with_settings(st, integrator=1), fc, w, h, ALBEDO)
    assert np.array_equal(rf.bits(f0), rf.bits(f1))


# ---- the filter

def _device_denoise(rt, torch, beauty, frames, p, workspace, in_place):
    dev = torch.device("cuda:0")
    h, w, _ = beauty.shape
    d_b = torch.from_numpy(beauty).to(dev)
    d_g = [None if g is None else torch.from_numpy(g).to(dev) for g in frames]
    d_out = d_b if in_place else torch.full((h, w, 4), 123.0, dtype=torch.float32, device=dev)
    d_ws = None
    if workspace:
        d_ws = torch.full((rt.denoise_features_workspace_bytes(w, h) // 4,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(0)
    err = rt.lib().rt_denoise_features_device(0, C.c_void_p(d_b.data_ptr()),
                                              *[C.c_void_p(g.data_ptr()) if g is not None else None for g in d_g],
                                              w, h, C.byref(p), C.c_void_p(d_ws.data_ptr()) if d_ws is not None else None,
                                              C.c_void_p(d_out.data_ptr()), None)
    assert err == 0, rt.lib().rt_last_error()
    if not in_place:
        assert np.array_equal(rf.bits(d_b.cpu().numpy()), rf.bits(beauty))
    return d_out.cpu().numpy()


# 1x1; 5x3: step 2 and beyond are outside; 67x35 and 130x70: ragged, more than one block a row and a column;
# step 16 (5 iterations) crosses every border of the small shapes
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 35), (130, 70)])
def test_filter_is_bit_identical_to_the_checker(rt, w, h):
    import torch
    beauty, g0, g1 = rd.random_frames(w, h, seed=200 + w)
    albedo = rf.random_albedo(w, h, seed=200 + w)
    mismatches, runs = 0, 0
    for iterations in (1, 3, 5):
        # albedo present or absent; its term and the demodulation on or off; a floor most albedos are below
        for has_albedo, sigma_albedo, demodulate, floor in ((True, 0.1, 1, 0.05), (True, 0.0, 1, 0.9), (True, 0.2, 0, 0.0),
                                                            (True, 0.0, 0, 0.0), (False, 0.0, 0, 0.0)):
            p = rf.params(iterations, 1.0, (0.1, 0.05), 10.0, sigma_albedo, demodulate, floor)
            frames = (g0, g1, albedo if has_albedo else None)
            want = rf.bits(rf.denoise(beauty, *frames, p))
            got = [_device_denoise(rt, torch, beauty, frames, p, workspace=True, in_place=False),
                   _device_denoise(rt, torch, beauty, frames, p, workspace=False, in_place=True)]
            if iterations == 3:
                got.append(rt.denoise_features(beauty, *frames, params=p))
            for g in got:
                mismatches += int(np.count_nonzero(rf.bits(g) != want))
            runs += len(got)
    # nothing new switched on: rt_denoise_device's output
    p = rf.params(3, 1.0, (0.1, 0.05), 10.0)
    plain = rt.denoise(beauty, g0, g1, p.base)
    got = _device_denoise(rt, torch, beauty, (g0, g1, None), p, workspace=True, in_place=False)
    assert np.array_equal(rf.bits(plain), rf.bits(got))
    REPORT[f"denoise_features_{w}x{h}"] = {"runs": runs, "mismatching_floats": mismatches}
    print(f"denoise_features_{w}x{h}", REPORT[f"denoise_features_{w}x{h}"])
    assert mismatches == 0


# ---- the picture entry

@pytest.mark.parametrize("guide_spp", [0, 1])
def test_the_picture_entry(rt, scenes, guide_spp):
    """rt_render_picture_features_denoised = the composition of the public entries, byte for byte."""
    import torch
    scene, cam, st0, fc, w, h, dev = scenes("c3")
    st = with_settings(st0, samples_per_pixel=4)
    post = rt.default_settings()[1]
    p = rt.default_denoise_features_params()
    cuda = torch.device("cuda:0")
    d = [torch.zeros((h, w, 4), dtype=torch.float32, device=cuda) for _ in range(4)]
    torch.cuda.synchronize(0)
    bstats = dev.render_device(cam, st, fc, w, h, d[0].data_ptr(), total_frame_index=TFI)
    gst = with_settings(st, samples_per_pixel=guide_spp or st.samples_per_pixel)
    for feature in (NORMAL, DISTANCE, ALBEDO):
        dev.render_feature_device(cam, gst, fc, w, h, feature, d[1 + feature].data_ptr(), total_frame_index=TFI)
    err = rt.lib().rt_denoise_features_device(0, *[C.c_void_p(t.data_ptr()) for t in d], w, h, C.byref(p), None,
                                              C.c_void_p(d[0].data_ptr()), None)
    assert err == 0, rt.lib().rt_last_error()
    want = rt.postprocess(d[0].cpu().numpy(), post, total_frame_index=TFI + 1)
    got, stats = dev.render_picture_features_denoised(cam, st, fc, w, h, post, p, guide_spp=guide_spp,
                                                      total_frame_index=TFI)
    n = int(np.count_nonzero(got != want))
    REPORT[f"denoise_features_picture_guide_spp{guide_spp}"] = {"mismatching_pixels": n}
    assert n == 0 and len(np.unique(got)) > 16
    for f in ("closest_hit_rays", "shadow_rays", "samples", "splat_mode"):
        assert getattr(stats, f) == getattr(bstats, f), f
    assert stats.samples == 4*w*h
