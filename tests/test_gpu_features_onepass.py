"""The three feature frames in one walk on the device: rt_render_features(_device) against the plain-C checker
tests/ref_features (per feature) and against the device's own single-feature frames ("Feature
frames").  After the call buffer f holds what rt_render_feature(_device) with feature f would have added to it:
bit for bit in the exact splat mode and, under one configuration, in the streaming mode."""
import ctypes as C
import threading

import numpy as np
import pytest

import recursive_cases as rc
import ref_features_binding as rf
from parity_report import REPORT
from random_scenes import random_scene

pytestmark = pytest.mark.gpu

NORMAL, DISTANCE, ALBEDO = FEATURES = range(3)
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
    """name -> (scene, cam, st, fc, w, h): the shapes of tests/test_gpu_features.py."""
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
    """The picture test hands torch's device buffers to the library: torch opens the device before the module's
    scenes do, whichever test runs first."""
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


def same(a, b):
    return np.array_equal(rf.bits(a), rf.bits(b))


def mismatches(a, b):
    return int(np.count_nonzero(np.any(rf.bits(a) != rf.bits(b), axis=2)))


def singles(dev, cam, st, fc, w, h, **kw):
    """The three single-feature frames -> ([frame], [stats])."""
    out = [dev.render_feature(cam, st, fc, w, h, f, **kw) for f in FEATURES]
    return [o[0] for o in out], [o[1] for o in out]


def onepass(dev, cam, st, fc, w, h, **kw):
    n, d, a, stats = dev.render_features(cam, st, fc, w, h, **kw)
    return [n, d, a], stats


def check_onepass(rt, dev, scene, cam, st, fc, w, h, key, **kw):
    """An exact one-pass frame against the checker and against the device's single-feature frames."""
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        frames, stats = onepass(dev, cam, st, fc, w, h, **kw)
        own, ostats = singles(dev, cam, st, fc, w, h, **kw)
    fig = {}
    spec = None
    for f in FEATURES:
        want, wstats, spec = rf.render(scene.desc(), cam, st, fc, w, h, f, **kw)
        fig[FEATURE_NAME[f]] = {"vs_checker": mismatches(frames[f], want), "vs_single_feature": mismatches(frames[f], own[f])}
        assert (wstats.closest_hit_rays, wstats.samples) == (ostats[f].closest_hit_rays, ostats[f].samples)
    fig.update(gpu_closest=int(stats.closest_hit_rays), samples=int(stats.samples), specular_bounces=int(spec))
    REPORT[key] = fig
    print(key, fig)
    assert stats.splat_mode == rt.abi.RT_SPLAT_EXACT
    for f in FEATURES:
        assert fig[FEATURE_NAME[f]] == {"vs_checker": 0, "vs_single_feature": 0}, FEATURE_NAME[f]
    # the one walk's counts: a single feature frame's, not three times that
    assert (stats.closest_hit_rays, stats.samples) == (ostats[0].closest_hit_rays, ostats[0].samples)
    assert stats.samples == w*h*st.samples_per_pixel
    assert stats.shadow_rays == 0 and stats.traced_rays[1] == 0
    assert stats.closest_hit_rays - stats.samples == spec
    return frames, stats, spec


# ---- 1. exact-splat parity

@pytest.mark.parametrize("name", ["c1", "c3", "c4", "random21", "random23", "mirrors"])
def test_exact_frames_match_the_checker_and_the_single_frames(rt, scenes, name):
    scene, cam, st, fc, w, h, dev = scenes(name)
    frames, stats, spec = check_onepass(rt, dev, scene, cam, st, fc, w, h, f"features_onepass_{name}", total_frame_index=TFI)
    assert all(np.isfinite(f).all() for f in frames)
    assert not same(frames[NORMAL], frames[ALBEDO])
    if name == "mirrors":                      # some walks of this frame run to the bound: 63 hits, 62 bounces followed
        xy, so = rc.all_samples(w, h, st.samples_per_pixel)
        _, end, bounces, _, _ = rf.trace_samples(scene.desc(), cam, st, w, h, xy, so, NORMAL, total_frame_index=TFI)
        assert (end == rf.END_BOUND).sum() > 0 and bounces.max() == 62 and bounces.sum() == spec
    if name in ("c3", "c4"):
        assert spec > 0                        # something is seen through a specular vertex


# ---- 2. the smallest frames

def test_one_pixel_and_per_sample_parity(rt, scenes):
    """1 x 1 at 2 spp; 5 x 3; and the box filter at 1 spp, where a pixel is its one sample (weight 1)."""
    scene, cam, st, fc, w, h, dev = scenes("c3")
    for sw, sh in ((1, 1), (5, 3)):
        _, cam1, st1, fc1, _ = rt.load_preset("c3", sw, sh)
        check_onepass(rt, dev, scene, cam1, with_settings(st1, samples_per_pixel=2), fc1, sw, sh,
                      f"features_onepass_{sw}x{sh}")
    box = rt.load_reconstruction_kernel("Box")
    st1 = with_settings(st, samples_per_pixel=1)
    frames, _, _ = check_onepass(rt, dev, scene, cam, st1, box, w, h, "features_onepass_box_1spp")
    xy, so = rc.all_samples(w, h, 1)
    for f in FEATURES:
        assert np.all(frames[f][..., 3] == 1.0)
        samples = rf.trace_samples(scene.desc(), cam, st1, w, h, xy, so, f)[0]
        assert same(frames[f][..., :3].reshape(-1, 3), samples[:, :3]), FEATURE_NAME[f]


# ---- 3. the streaming splat: the same records, the same resolve, once per ring

@pytest.mark.parametrize("parts", [1, 4])
def test_streaming_frames_equal_the_single_feature_streaming_frames(rt, scenes, parts):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, samples_per_pixel=4)
    # (a 1024-path pool: four partitions of a frame this small, each with passes of its own)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM, partitions=parts, path_pool=1024):
        frames, stats = onepass(dev, cam, st, fc, w, h, total_frame_index=TFI)
        own, ostats = singles(dev, cam, st, fc, w, h, total_frame_index=TFI)
    fig = {FEATURE_NAME[f]: mismatches(frames[f], own[f]) for f in FEATURES}
    REPORT[f"features_onepass_stream_partitions{parts}"] = fig
    print(parts, fig)
    assert stats.splat_mode == rt.abi.RT_SPLAT_STREAM and all(s.splat_mode == rt.abi.RT_SPLAT_STREAM for s in ostats)
    assert all(v == 0 for v in fig.values())
    assert (stats.closest_hit_rays, stats.samples, stats.shadow_rays) == (ostats[0].closest_hit_rays, ostats[0].samples, 0)
    assert not same(frames[NORMAL], frames[DISTANCE])


# ---- 4. the atomic splat

def test_atomic_frames_are_close_to_the_exact_ones(rt, scenes):
    scene, cam, st, fc, w, h, dev = scenes("c3")
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        exact, estats = onepass(dev, cam, st, fc, w, h)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_ATOMIC):
        atomic, astats = onepass(dev, cam, st, fc, w, h)
    fig = {FEATURE_NAME[f]: rel_l2(atomic[f], exact[f]) for f in FEATURES}
    REPORT["features_onepass_atomic_vs_exact"] = fig
    print(fig)
    assert astats.splat_mode == rt.abi.RT_SPLAT_ATOMIC
    assert (astats.closest_hit_rays, astats.samples) == (estats.closest_hit_rays, estats.samples)
    for f in FEATURES:
        assert fig[FEATURE_NAME[f]] <= 1e-5, FEATURE_NAME[f]


# ---- 5. the schedule does not enter a one-pass frame

def test_schedule_independence(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, samples_per_pixel=4)
    E, S = rt.abi.RT_SPLAT_EXACT, rt.abi.RT_SPLAT_STREAM
    runs = {}
    for key, cfg in (("base", dict(partitions=1)), ("partitions4_default_pool", dict(partitions=4)),
                     ("partitions4", dict(partitions=4, path_pool=1024)),
                     ("drain_every3", dict(partitions=4, path_pool=1024, drain_every=3)),
                     ("pool1024", dict(partitions=1, path_pool=1024, drain_every=3))):
        with dev.configured(splat_mode=E, **cfg):
            runs[key] = onepass(dev, cam, st, fc, w, h)
    base, bstats = runs["base"]
    for key, (frames, stats) in runs.items():
        assert stats.splat_mode == E
        for f in FEATURES:
            assert same(frames[f], base[f]), (key, FEATURE_NAME[f])
        assert (stats.closest_hit_rays, stats.shadow_rays, stats.samples) == (bstats.closest_hit_rays, 0, bstats.samples), key
    # the three rings wrap: a ring of one pass resolved pass by pass, and a ring of three in chunks of two,
    # against the rings the frame gets by itself (one partition each, so the sums are those of one order)
    figures = {}
    with dev.configured(splat_mode=S, partitions=1, path_pool=1024):
        stream, sstats = onepass(dev, cam, st, fc, w, h)
    for key, cfg in (("ring1_chunk1", dict(splat_ring=1, splat_chunk=1)), ("ring3_chunk2", dict(splat_ring=3, splat_chunk=2))):
        with dev.configured(splat_mode=S, partitions=1, path_pool=1024, **cfg):
            frames, stats = onepass(dev, cam, st, fc, w, h)
        assert stats.splat_mode == S and stats.closest_hit_rays == bstats.closest_hit_rays
        for f in FEATURES:
            assert same(frames[f], stream[f]), (key, FEATURE_NAME[f])
    for f in FEATURES:
        figures[FEATURE_NAME[f]] = {"stream_vs_exact": rel_l2(stream[f], base[f])}
        assert figures[FEATURE_NAME[f]]["stream_vs_exact"] <= 2e-6
    assert sstats.splat_mode == S and sstats.closest_hit_rays == bstats.closest_hit_rays
    REPORT["features_onepass_schedule"] = figures
    print(figures)


# ---- 6. shards

def test_shards_sum_to_the_frame(rt, scenes):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, samples_per_pixel=4)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        base, bstats = onepass(dev, cam, st, fc, w, h)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM):
        tiles = [onepass(dev, cam, st, fc, w, h, shard_index=r, shard_count=2) for r in range(2)]
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM, shard_mode=rt.abi.RT_SHARD_PASSES):
        passes = [onepass(dev, cam, st, fc, w, h, shard_index=r, shard_count=2) for r in range(2)]
    figures = {}
    for name, shards in (("tile_shards", tiles), ("pass_shards", passes)):
        fig = {FEATURE_NAME[f]: rel_l2(sum(p[0][f].astype(np.float64) for p in shards), base[f]) for f in FEATURES}
        figures[name] = fig
        print(name, fig)
        for f in FEATURES:
            assert fig[FEATURE_NAME[f]] <= 2e-6, (name, FEATURE_NAME[f])
        assert sum(p[1].closest_hit_rays for p in shards) == bstats.closest_hit_rays
        assert sum(p[1].samples for p in shards) == bstats.samples
        assert all(p[1].shadow_rays == 0 for p in shards)
    REPORT["features_onepass_shards"] = figures


# ---- 7. progressive accumulation

def test_progressive_accumulation(rt, scenes):
    """Two calls (frame_count 0, then 2) into the same three buffers: the single-feature entry used the same way."""
    scene, cam, st, fc, w, h, dev = scenes("c3")
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        acc = [np.zeros((h, w, 4), np.float32) for _ in FEATURES]
        dev.render_features(cam, st, fc, w, h, accums=acc, frame_count=0, total_frame_index=0)
        first = [a.copy() for a in acc]
        dev.render_features(cam, st, fc, w, h, accums=acc, frame_count=2, total_frame_index=1)
        for f in FEATURES:
            one = np.zeros((h, w, 4), np.float32)
            dev.render_feature(cam, st, fc, w, h, f, accum=one, frame_count=0, total_frame_index=0)
            assert same(first[f], one), FEATURE_NAME[f]
            dev.render_feature(cam, st, fc, w, h, f, accum=one, frame_count=2, total_frame_index=1)
            assert same(acc[f], one) and not same(acc[f], first[f]), FEATURE_NAME[f]
    REPORT["features_onepass_progressive"] = {"bit_identical": True}


# ---- 8. the device's own first-hit frames

@pytest.mark.parametrize("bounces", [0, 1])
def test_device_anchor(rt, scenes, bounces):
    scene, cam, st0, fc, w, h, dev = scenes("c4")
    st = with_settings(st0, max_bounce_count=bounces)
    for mode, parts in ((rt.abi.RT_SPLAT_EXACT, 4), (rt.abi.RT_SPLAT_STREAM, 1), (rt.abi.RT_SPLAT_STREAM, 4)):
        with dev.configured(splat_mode=mode, partitions=parts):
            frames, fs = onepass(dev, cam, st, fc, w, h, total_frame_index=TFI)
            for feature, integ in ((NORMAL, NORMALS), (DISTANCE, DISTANCES)):
                g, gs = dev.render(cam, with_settings(st, integrator=integ), fc, w, h, total_frame_index=TFI)
                assert fs.splat_mode == gs.splat_mode == mode
                assert same(frames[feature], g), (mode, parts, feature)
                assert fs.closest_hit_rays == gs.closest_hit_rays == fs.samples == w*h*st.samples_per_pixel


# ---- 9. a one-pass frame leaves the other frames alone

def test_no_leak(rt, scenes):
    scene, cam, st, fc, w, h, dev = scenes("c3")
    a = rt.abi
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT, shadow_launch=a.RT_SHADOW_LAUNCH_AUTO):
        f0, s0 = dev.render(cam, st, fc, w, h)
        before, _ = singles(dev, cam, st, fc, w, h)
        _, sf = onepass(dev, cam, st, fc, w, h)
        assert sf.shadow_rays == 0 and sf.traced_rays[1] == 0
        after, _ = singles(dev, cam, st, fc, w, h)
        f1, s1 = dev.render(cam, st, fc, w, h)
    assert same(f0, f1)
    assert s0.shadow_launch == s1.shadow_launch
    assert (s0.closest_hit_rays, s0.shadow_rays) == (s1.closest_hit_rays, s1.shadow_rays) and s0.shadow_rays > 0
    for f in FEATURES:
        assert same(before[f], after[f]), FEATURE_NAME[f]
    # rt_settings::integrator is ignored
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT):
        other, _ = onepass(dev, cam, with_settings(st, integrator=1), fc, w, h)
    for f in FEATURES:
        assert same(other[f], after[f]), FEATURE_NAME[f]


# ---- 10. rt_cancel

def test_frame_after_cancel_is_bit_exact(rt, scenes):
    """rt_cancel from another thread while a many-iteration one-pass frame renders returns RT_ERROR_CANCELLED, and
    the next one-pass frame is bit-exact."""
    scene, cam, st0, fc, w, h, dev = scenes("c1")
    big = with_settings(st0, samples_per_pixel=4096)        # 16.8M samples through a 1024-path pool
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its loop starts: repeated, the cancel lands inside the loop
        while not returned.is_set():
            dev.cancel()
            returned.wait(0.005)

    with dev.configured(path_pool=1024, partitions=1):
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                dev.render_features(cam, big, fc, w, h)
        finally:
            returned.set()
            canceller.join()
    assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
    check_onepass(rt, dev, scene, cam, st0, fc, w, h, "features_onepass_after_cancel")


# ---- 11. the picture entry renders its feature frames in one walk

@pytest.mark.parametrize("guide_spp", [0, 1])
def test_the_picture_entry(rt, scenes, guide_spp):
    """rt_render_picture_features_denoised = the composition written with rt_render_features_device, byte for byte."""
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
    fstats = dev.render_features_device(cam, gst, fc, w, h, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                        total_frame_index=TFI)
    assert fstats.samples == gst.samples_per_pixel*w*h and fstats.shadow_rays == 0
    err = rt.lib().rt_denoise_features_device(0, *[C.c_void_p(t.data_ptr()) for t in d], w, h, C.byref(p), None,
                                              C.c_void_p(d[0].data_ptr()), None)
    assert err == 0, rt.lib().rt_last_error()
    want = rt.postprocess(d[0].cpu().numpy(), post, total_frame_index=TFI + 1)
    got, stats = dev.render_picture_features_denoised(cam, st, fc, w, h, post, p, guide_spp=guide_spp,
                                                      total_frame_index=TFI)
    n = int(np.count_nonzero(got != want))
    REPORT[f"features_onepass_picture_guide_spp{guide_spp}"] = {"mismatching_pixels": n}
    assert n == 0 and len(np.unique(got)) > 16
    for f in ("closest_hit_rays", "shadow_rays", "samples", "splat_mode"):
        assert getattr(stats, f) == getattr(bstats, f), f
