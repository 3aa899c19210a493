"""Whitted (1) and Ground Truth Recursive (2) on the device, a per-scene opt-in
(rt_scene_set_recursive_integrators): k_recurse's explicit frame stack against the CPU checker's plain recursion
(tests/ref_recursive, tests/ref_recursive_binding.py).

Bars: every listed rt_trace_samples sample bit-identical to the checker; every pixel of the RT_SPLAT_EXACT frame
bit-identical to the checker's single-threaded frame; closest and shadow ray counts equal; the streaming frame
within tests/test_gpu_integrators.py's streaming bound (rel L2 <= 2e-6 of the exact frame).  Two samples also
count as equal when both are NaN or both the same infinity (x86 and gfx950 differ in NaN payload);
tests/test_ref_recursive.py asserts the checker is finite on every case, so equality never passes on garbage.

Shapes and cases: tests/recursive_cases.py (a path pool of 1024, four frame shapes, 1 / 5 / 16 spp, every sampler).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_binding as ob
import recursive_cases as rc
import ref_recursive_binding as rr

pytestmark = pytest.mark.gpu

ADVANCED, WHITTED, GT_RECURSIVE, GT_ITERATIVE = 0, 1, 2, 3
STREAM_BOUND = 2e-6           # tests/test_gpu_integrators.py: rel_l2(stream, exact)
SHARD_BOUND = 1e-5            # the same file's bound on shards summed in float64


def rel_l2(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def cache(rt):
    return rc.SceneCache(rt)


@pytest.fixture(scope="module")
def devs(rt, cache):
    """Scene name -> its DeviceScene with the opt-in on and a 1024-path pool, uploaded on first use."""
    made = {}

    def get(name):
        if name not in made:
            scene = cache.get(name, 64, 48)[0]
            dev = rt.DeviceScene(scene, 0)
            dev.set_recursive_integrators(True)
            dev.configure(path_pool=rc.POOL)
            made[name] = dev
        return made[name]
    yield get
    for d in made.values():
        d.close()


# ---- parity with the checker

@pytest.mark.parametrize("case", rc.cases(), ids=[c[0] for c in rc.cases()])
def test_parity(rt, cache, devs, case):
    cid, name, integ, depth, sampler, (w, h), spp = case
    scene, cam, st0, fc = cache.get(name, w, h)
    dev = devs(name)
    st = rc.case_settings(st0, integ, depth, sampler, spp)
    amb = scene.ambient_light()
    xy, so = rc.all_samples(w, h, spp)
    gpu, gstats = dev.trace_samples(cam, st, w, h, xy, so, total_frame_index=2)
    cpu, cstats = rr.trace_samples(scene.desc(), cam, st, w, h, xy, so, ambient=amb, total_frame_index=2)
    same = rc.same_samples(gpu, cpu)
    print(cid, "samples", len(xy), "differing", int((~same.all(axis=1)).sum()), "closest", int(gstats.closest_hit_rays),
          int(cstats.closest_hit_rays), "shadow", int(gstats.shadow_rays), int(cstats.shadow_rays))
    assert same.all(), f"{int((~same.all(axis=1)).sum())} of {len(xy)} samples differ"
    assert (gstats.closest_hit_rays, gstats.shadow_rays) == (cstats.closest_hit_rays, cstats.shadow_rays)
    assert gstats.samples == len(xy)
    if integ == GT_RECURSIVE:
        assert gstats.shadow_rays == 0 and gstats.traced_rays[1] == 0
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        frame, fstats = dev.render(cam, st, fc, w, h, total_frame_index=2)
    cframe, cfstats = rr.render(scene.desc(), cam, st, fc, w, h, ambient=amb, total_frame_index=2)
    fsame = rc.same_samples(frame, cframe)
    print(cid, "pixels differing", int((~fsame.all(axis=2)).sum()))
    assert fstats.splat_mode == rt.abi.RT_SPLAT_EXACT
    assert fsame.all(), f"{int((~fsame.all(axis=2)).sum())} of {w*h} pixels differ"
    assert (fstats.closest_hit_rays, fstats.shadow_rays, fstats.samples) == (
        cfstats.closest_hit_rays, cfstats.shadow_rays, cfstats.samples) and fstats.samples == w*h*spp
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_STREAM):
        stream, sstats = dev.render(cam, st, fc, w, h, total_frame_index=2)
    err = rel_l2(stream, frame)
    print(cid, "stream rel L2", err)
    assert sstats.splat_mode == rt.abi.RT_SPLAT_STREAM and err <= STREAM_BOUND
    assert (sstats.closest_hit_rays, sstats.shadow_rays) == (fstats.closest_hit_rays, fstats.shadow_rays)


# ---- the opt-in

def test_opt_in(rt, cache):
    scene, cam, st0, fc = cache.get("c1", 64, 48)
    w, h = 64, 48
    adv = rc.with_settings(st0, samples_per_pixel=4)
    xy = np.zeros((4, 2), np.uint32)
    so = np.arange(4, dtype=np.uint32)
    dev = rt.DeviceScene(scene, 0)
    try:
        dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
        before, bstats = dev.render(cam, adv, fc, w, h)

        def refused():
            for integ, word in ((WHITTED, "Whitted"), (GT_RECURSIVE, "Ground Truth Recursive")):
                st = rc.with_settings(adv, integrator=integ)
                assert not dev.integrator_supported(integ) and not rt.scene_integrator_supported(dev, integ)
                for call in (lambda: dev.render(cam, st, fc, w, h), lambda: dev.trace_samples(cam, st, w, h, xy, so)):
                    with pytest.raises(rt.RenderError) as e:
                        call()
                    assert e.value.code == rt.abi.RT_ERROR_INVALID
                    assert word in str(e.value) and "recursion stack" in str(e.value)

        refused()                                              # a fresh scene: today's error text
        dev.set_recursive_integrators(True)
        dev.set_recursive_integrators(True)                    # twice is harmless
        assert [int(dev.integrator_supported(i)) for i in range(-1, 7)] == [0, 1, 1, 1, 1, 1, 1, 0]
        assert [int(rt.integrator_supported(i)) for i in range(6)] == [1, 0, 0, 1, 1, 1]      # the process-wide answer stays
        for integ in (WHITTED, GT_RECURSIVE):
            st = rc.with_settings(adv, integrator=integ)
            frame, stats = dev.render(cam, st, fc, w, h)
            cframe, cstats = rr.render(scene.desc(), cam, st, fc, w, h, ambient=scene.ambient_light())
            assert rc.same_samples(frame, cframe).all() and np.abs(frame[..., :3]).max() > 0.01
            assert (stats.closest_hit_rays, stats.shadow_rays, stats.samples) == (
                cstats.closest_hit_rays, cstats.shadow_rays, w*h*4)
        during, dstats = dev.render(cam, adv, fc, w, h)        # Advanced with the opt-in on
        dev.set_recursive_integrators(False)
        refused()                                              # and off again
        dev.set_recursive_integrators(False)
        after, astats = dev.render(cam, adv, fc, w, h)
    finally:
        dev.close()
    for f, s in ((during, dstats), (after, astats)):
        assert np.array_equal(f.view(np.uint32), before.view(np.uint32))
        assert (s.closest_hit_rays, s.shadow_rays) == (bstats.closest_hit_rays, bstats.shadow_rays)


def test_ambient_light_reaches_the_device(rt, cache, devs):
    """DeviceScene passes the host scene's ambient light on at upload; rt_scene_set_ambient_light changes it."""
    scene, cam, st0, fc = cache.get("lights", 64, 48)
    dev = devs("lights")
    w, h = 64, 48
    st = rc.case_settings(st0, WHITTED, 2, rc.UNIFORM, 2)
    xy, so = rc.all_samples(w, h, 2)
    try:
        for amb in ((0.0, 0.0, 0.0), (3.0, 0.5, 0.25)):
            dev.set_ambient_light(amb)
            gpu, _ = dev.trace_samples(cam, st, w, h, xy, so)
            cpu, _ = rr.trace_samples(scene.desc(), cam, st, w, h, xy, so, ambient=amb)
            assert rc.same_samples(gpu, cpu).all(), amb
        base, _ = rr.trace_samples(scene.desc(), cam, st, w, h, xy, so, ambient=scene.ambient_light())
        assert not np.array_equal(base, cpu)
    finally:
        dev.set_ambient_light(scene.ambient_light())


# ---- every entry point

@pytest.mark.parametrize("integ", [WHITTED, GT_RECURSIVE])
def test_picture_entry(rt, cache, devs, integ):
    """rt_render_picture equals rt_postprocess of the rendered frame."""
    scene, cam, st0, fc = cache.get("c4", 64, 48)
    dev = devs("c4")
    w, h = 64, 48
    st = rc.case_settings(st0, integ, 3, rc.UNIFORM, 4)
    post = rt.default_settings()[1]
    out = np.zeros((h, w), np.uint32)
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    stats = rt.abi.Stats()
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        err = rt.lib().rt_render_picture(dev._h, C.byref(cam), C.byref(st), C.byref(fc), C.byref(tiles), 5, w, h,
                                         C.byref(post), out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats))
        assert err == 0, rt.lib().rt_last_error()
        frame, fstats = dev.render(cam, st, fc, w, h, total_frame_index=5)
    assert np.array_equal(out, rt.postprocess(frame, post, total_frame_index=6))
    assert np.array_equal(out, ob.postprocess(frame, post, total_frame_index=6))
    assert (stats.closest_hit_rays, stats.shadow_rays) == (fstats.closest_hit_rays, fstats.shadow_rays)
    assert len(np.unique(out)) > 16


@pytest.mark.parametrize("integ", [WHITTED, GT_RECURSIVE])
def test_shards_sum_to_the_frame(rt, cache, devs, integ):
    """Tile and pass shards of 2 and 4 sum to the whole frame, with equal counts."""
    scene, cam, st0, fc = cache.get("c3", 65, 33)
    dev = devs("c3")
    w, h = 65, 33
    st = rc.case_settings(st0, integ, 3, rc.STRATIFIED, 8)
    a = rt.abi
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT):
        base, bstats = dev.render(cam, st, fc, w, h, tile=16)
    for mode in (a.RT_SHARD_TILES, a.RT_SHARD_PASSES):
        for n in (2, 4):
            with dev.configured(splat_mode=a.RT_SPLAT_STREAM, shard_mode=mode):
                parts = [dev.render(cam, st, fc, w, h, tile=16, shard_index=r, shard_count=n) for r in range(n)]
            err = rel_l2(sum(p[0].astype(np.float64) for p in parts), base)
            print("shards", integ, mode, n, err)
            assert err <= SHARD_BOUND, (mode, n, err)
            assert sum(p[1].closest_hit_rays for p in parts) == bstats.closest_hit_rays, (mode, n)
            assert sum(p[1].shadow_rays for p in parts) == bstats.shadow_rays, (mode, n)
            assert sum(p[1].samples for p in parts) == bstats.samples == w*h*8
    # an exact-splat tile shard is the checker's
    with dev.configured(splat_mode=a.RT_SPLAT_EXACT):
        part, pstats = dev.render(cam, st, fc, w, h, tile=16, shard_index=1, shard_count=2)
    cpart, cstats = rr.render(scene.desc(), cam, st, fc, w, h, ambient=scene.ambient_light(), tile=16, shard_index=1,
                              shard_count=2)
    assert rc.same_samples(part, cpart).all()
    assert (pstats.closest_hit_rays, pstats.shadow_rays) == (cstats.closest_hit_rays, cstats.shadow_rays)


@pytest.mark.parametrize("integ", [WHITTED, GT_RECURSIVE])
def test_progressive_frames_accumulate(rt, cache, devs, integ):
    """Two progressive frames (frame_count 0, then 4) accumulate as the checker's two do."""
    scene, cam, st0, fc = cache.get("lights", 65, 33)
    dev = devs("lights")
    w, h = 65, 33
    st = rc.case_settings(st0, integ, 4, rc.BLUE_NOISE, 4)
    amb = scene.ambient_light()
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        acc, s0 = dev.render(cam, st, fc, w, h, total_frame_index=0)
        first = acc.copy()
        acc, s1 = dev.render(cam, st, fc, w, h, accum=acc, frame_count=4, total_frame_index=1)
    cacc, c0 = rr.render(scene.desc(), cam, st, fc, w, h, ambient=amb, total_frame_index=0)
    assert rc.same_samples(first, cacc).all()
    cacc, c1 = rr.render(scene.desc(), cam, st, fc, w, h, ambient=amb, accum=cacc, frame_count=4, total_frame_index=1)
    assert rc.same_samples(acc, cacc).all() and not np.array_equal(acc, first)
    assert (s1.closest_hit_rays, s1.shadow_rays) == (c1.closest_hit_rays, c1.shadow_rays)
    assert (s0.closest_hit_rays, s0.shadow_rays) == (c0.closest_hit_rays, c0.shadow_rays)


def test_frame_after_cancel_is_bit_exact(rt, cache, devs):
    """rt_cancel from another thread while a many-iteration frame renders returns RT_ERROR_CANCELLED, and the
    next frame is bit-exact."""
    scene, cam, st0, fc = cache.get("c1", 64, 48)
    dev = devs("c1")
    big = rc.case_settings(st0, GT_RECURSIVE, 5, rc.UNIFORM, 4096)     # 12.6M samples through a 1024-path pool
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its loop starts: repeated, the cancel lands inside the loop
        while not returned.is_set():
            dev.cancel()
            returned.wait(0.005)

    canceller = threading.Thread(target=cancel_until_returned)
    canceller.start()
    try:
        with pytest.raises(rt.RenderError) as ei:
            dev.render(cam, big, fc, 64, 48)
    finally:
        returned.set()
        canceller.join()
    assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
    for integ in (WHITTED, GT_RECURSIVE):
        st = rc.case_settings(st0, integ, 4, rc.UNIFORM, 4)
        with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
            frame, stats = dev.render(cam, st, fc, 64, 48)
        cframe, cstats = rr.render(scene.desc(), cam, st, fc, 64, 48, ambient=scene.ambient_light())
        assert rc.same_samples(frame, cframe).all()
        assert (stats.closest_hit_rays, stats.shadow_rays) == (cstats.closest_hit_rays, cstats.shadow_rays)


@pytest.mark.parametrize("name", ["c3", "random21"])
@pytest.mark.parametrize("integ", [WHITTED, GT_RECURSIVE])
def test_traversal_ref_changes_nothing(rt, cache, devs, name, integ):
    """rt_scene_config::traversal_ref on (the reference-unit walk): frames and counts are unchanged."""
    scene, cam, st0, fc = cache.get(name, 65, 33)
    dev = devs(name)
    w, h = 65, 33
    st = rc.case_settings(st0, integ, 3, rc.UNIFORM, 2)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
        base, bstats = dev.render(cam, st, fc, w, h)
    with dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT, traversal_ref=1):
        ref, rstats = dev.render(cam, st, fc, w, h)
    assert np.array_equal(ref.view(np.uint32), base.view(np.uint32))
    assert (rstats.closest_hit_rays, rstats.shadow_rays, rstats.samples) == (
        bstats.closest_hit_rays, bstats.shadow_rays, bstats.samples)
    assert rstats.traversal_ref[0].mesh_bvh_traversals > 0 and bstats.traversal_ref[0].mesh_bvh_traversals == 0


def test_no_leak_into_advanced_auto_schedule(rt, cache, devs):
    """The AUTO shadow launch of a whole frame on a pool of 4M paths or more follows the shadow rays per
    extension ray the scene's previous Advanced frame traced (merged from 0.15; C3 traces ~0.26).  A Ground
    Truth Recursive frame traces none and a Whitted frame several per extension ray: were either recorded,
    the Advanced frame after it could pick another launch."""
    scene, cam, st0, fc = cache.get("c3", 64, 48)
    dev = devs("c3")
    w, h = 64, 48
    spp = 1400                                           # 64 x 48 x 1400 samples fill a 4M-path pool
    a = rt.abi
    adv = rc.with_settings(st0, integrator=ADVANCED, samples_per_pixel=spp)
    with dev.configured(path_pool=4 << 20, partitions=1, shadow_launch=a.RT_SHADOW_LAUNCH_AUTO):
        dev.render(cam, adv, fc, w, h)                   # the scene's share of shadow rays becomes known
        f0, s0 = dev.render(cam, adv, fc, w, h)
        launches = []
        for integ in (WHITTED, GT_RECURSIVE):
            st = rc.case_settings(st0, integ, 2, rc.UNIFORM, 2)
            _, rs = dev.render(cam, st, fc, w, h)
            assert rs.samples == w*h*2 and rs.traced_rays[0] > 0
            f1, s1 = dev.render(cam, adv, fc, w, h)
            launches.append(int(s1.shadow_launch))
            assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32))
    assert s0.traced_rays[1] >= 0.15*s0.traced_rays[0] and s0.shadow_launch == a.RT_SHADOW_LAUNCH_MERGED
    assert launches == [int(s0.shadow_launch)]*2
