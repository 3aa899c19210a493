"""Adaptive sampling by tiles on the device ("Adaptive sampling by tiles"): frames over a tile list
(rt_render_tiles_device) against the shard frames, the oracle and each other; the tile error estimate
(rt_tile_error_device) against the plain-C checker tests/ref_adaptive, bit for bit; the driver
(rt_render_adaptive_device) against the same loop written here on the two entries below it, bit for bit.

Scenes are the suite's small presets (C1 at 130x70 and 65x33, C3 at 192x108) in the exact splat mode unless said
otherwise, a few samples per pixel: what can go wrong is the layout (ragged tiles, halos, the cache), not the paths.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_binding as ob
import ref_adaptive_binding as ra
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 3          # total_frame_index of every frame here


def rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b)/max(np.linalg.norm(b), 1e-30))


def rays(s):
    """What two renders of the same samples must agree on: the ray counts and the TraversalStats."""
    return (s.closest_hit_rays, s.shadow_rays, s.samples, s.traversal[0].as_dict(), s.traversal[1].as_dict())


def add_rays(total, s):
    t = total or (0, 0, 0, {}, {})
    add = lambda a, b: {k: a.get(k, 0) + v for k, v in b.items()}
    return (t[0] + s.closest_hit_rays, t[1] + s.shadow_rays, t[2] + s.samples, add(t[3], s.traversal[0].as_dict()),
            add(t[4], s.traversal[1].as_dict()))


class Case:
    """A preset on the device in the exact splat mode, with frames rendered into fresh device buffers."""

    def __init__(self, rt, preset, w, h, spp, exact=True):
        import torch
        self.rt, self.torch, self.w, self.h = rt, torch, w, h
        self.scene, self.cam, self.st, self.fc, self.post = rt.load_preset(preset, w, h)
        self.st.samples_per_pixel = spp
        self.dev = rt.DeviceScene(self.scene, 0)
        if exact:
            self.dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)

    def zeros(self, fill=0.0):
        d = self.torch.full((self.h, self.w, 4), fill, dtype=self.torch.float32, device="cuda:0")
        self.torch.cuda.synchronize(0)
        return d

    def settings(self, spp):
        s = self.rt.abi.Settings.from_buffer_copy(self.st)
        s.samples_per_pixel = spp
        return s

    def shard(self, tile, index=0, count=1, d=None, spp=None, frame_count=0):
        d = self.zeros() if d is None else d
        st = self.st if spp is None else self.settings(spp)
        stats = self.dev.render_device(self.cam, st, self.fc, self.w, self.h, d.data_ptr(), total_frame_index=TFI, tile=tile,
                                       shard_index=index, shard_count=count, frame_count=frame_count)
        return d, stats

    def tiles(self, tile, ids, d=None, spp=None, frame_count=0):
        d = self.zeros() if d is None else d
        st = self.st if spp is None else self.settings(spp)
        stats = self.dev.render_tiles_device(self.cam, st, self.fc, self.w, self.h, ids, d.data_ptr(),
                                             total_frame_index=TFI, tile=tile, frame_count=frame_count)
        return d, stats

    def ntiles(self, tile):
        tcx, tcy = ra.tile_grid(self.w, self.h, tile, tile)
        return tcx*tcy

    def close(self):
        self.dev.close()


def same_bits(a, b):
    return np.array_equal(ra.bits(a.cpu().numpy()), ra.bits(b.cpu().numpy()))


@pytest.fixture(scope="module")
def c3(rt):
    """C3 (the mesh, glass, an environment map) at 192x108: 3 x 2 tiles of 64x64, the bottom row 44 tall."""
    case = Case(rt, "c3", 192, 108, 4)
    yield case
    case.close()


# ---- 1. frames over a tile list

# 130x70 and 65x33 with 64x64 tiles (ragged edge tiles, 2 wide and 6 tall; 1 wide and 33 tall), 65x33 with 16x16
# tiles (15 tiles, the last column 1 wide, the last row 1 tall)
@pytest.mark.parametrize("w,h,tile", [(130, 70, 64), (65, 33, 64), (65, 33, 16)])
def test_all_tiles_is_the_whole_frame(rt, w, h, tile):
    case = Case(rt, "c1", w, h, 4)
    try:
        want, ws = case.shard(tile)
        got, gs = case.tiles(tile, list(range(case.ntiles(tile))))
        again, _ = case.shard(tile)                         # and back through the old door: the layout is the shard's again
    finally:
        case.close()
    assert same_bits(got, want) and same_bits(again, want)
    assert rays(gs) == rays(ws) and gs.samples == 4*w*h
    assert gs.splat_mode == rt.abi.RT_SPLAT_EXACT


def test_odd_tiles_are_shard_1_of_2(rt, c3):
    with c3.dev.configured(shard_mode=rt.abi.RT_SHARD_TILES):
        want, ws = c3.shard(64, 1, 2)
    got, gs = c3.tiles(64, [1, 3, 5])
    assert same_bits(got, want)
    assert rays(gs) == rays(ws)
    # the host entry gives the same frame
    host, hs = c3.dev.render_tiles(c3.cam, c3.st, c3.fc, c3.w, c3.h, [1, 3, 5], total_frame_index=TFI)
    assert np.array_equal(ra.bits(host), ra.bits(want.cpu().numpy())) and rays(hs) == rays(ws)


def test_one_interior_tile_against_the_oracle(rt):
    """Tile 7 of the 5 x 3 grid of 16x16 tiles on 65x33: its samples, and its halo in the eight tiles around it."""
    w, h, tile, t = 65, 33, 16, 7
    case = Case(rt, "c1", w, h, 4)
    try:
        got, gs = case.tiles(tile, [t])
    finally:
        case.close()
    gpu = got.cpu().numpy()
    cpu = np.zeros((h, w, 4), np.float32)
    buf = rt.abi.AccumulationBuffer(w, h, 0, cpu.ctypes.data_as(C.POINTER(C.c_float)))
    arr = (C.c_uint32*1)(t)
    cs = rt.abi.Stats()
    assert ob.load().oracle_render_tiles(C.byref(case.scene.desc()), C.byref(case.cam), C.byref(case.st), C.byref(case.fc),
                                         tile, tile, TFI, 0, 1, 1, arr, C.byref(buf), C.byref(cs)) == 0
    same = float(np.all(ra.bits(gpu) == ra.bits(cpu), axis=2).mean())
    x0, y0 = tile*(t % 5), tile*(t // 5)
    outside = np.ones((h, w), bool)
    outside[y0:y0 + tile, x0:x0 + tile] = False
    halo = int((cpu[..., 3][outside] != 0).sum())
    REPORT["adaptive_one_tile_vs_oracle"] = {"pixels_bit_identical": same, "halo_pixels": halo}
    print("one interior tile:", REPORT["adaptive_one_tile_vs_oracle"])
    assert halo > 0 and int((cpu[..., 3] != 0).sum()) < (tile + 2*case.fc.kernel_size + 2)**2
    assert gs.samples == cs.samples == 4*tile*tile
    assert (gs.closest_hit_rays, gs.shadow_rays) == (cs.closest_hit_rays, cs.shadow_rays)
    assert same >= 0.999


def test_two_lists_on_one_scene(rt, c3):
    """Two lists of equal length back to back: a cache keyed by the frame alone would reuse the first pixel map."""
    first, second = [0, 4], [1, 4]
    a, _ = c3.tiles(64, first)
    b, _ = c3.tiles(64, second)
    a2, _ = c3.tiles(64, first)
    fresh = Case(rt, "c3", c3.w, c3.h, 4)
    try:
        want_b, _ = fresh.tiles(64, second)
    finally:
        fresh.close()
    fresh = Case(rt, "c3", c3.w, c3.h, 4)
    try:
        want_a, _ = fresh.tiles(64, first)
    finally:
        fresh.close()
    assert same_bits(a, want_a) and same_bits(b, want_b) and same_bits(a2, want_a)
    assert not same_bits(a, b)


@pytest.mark.parametrize("mode", ["exact", "stream"])
def test_disjoint_lists_sum_to_the_frame(rt, c3, mode):
    splat = rt.abi.RT_SPLAT_EXACT if mode == "exact" else rt.abi.RT_SPLAT_STREAM
    with c3.dev.configured(splat_mode=splat):
        want, ws = c3.shard(64)
        got, s1 = c3.tiles(64, [0, 3, 4])
        got, s2 = c3.tiles(64, [1, 2, 5], d=got)
    err = rel_l2(got.cpu().numpy(), want.cpu().numpy())
    REPORT[f"adaptive_disjoint_lists_{mode}"] = {"rel_l2": err}
    print("disjoint lists", mode, err)
    assert s1.splat_mode == s2.splat_mode == splat
    assert add_rays(add_rays(None, s1), s2) == rays(ws)
    assert err <= 1e-5


def test_an_empty_list_is_an_empty_shard(rt, c3):
    d = c3.zeros(7.0)
    _, stats = c3.tiles(64, [], d=d)
    assert (stats.samples, stats.closest_hit_rays, stats.iterations) == (0, 0, 0)
    assert bool((d == 7.0).all())


# ---- 2. the tile error estimate

def device_tile_error(rt, torch, a, b, tile_w, tile_h, ids, p=None):
    """rt_tile_error_device on device copies -> (errors, counts), downloaded; the outputs start as garbage."""
    d_a = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_b = b if torch.is_tensor(b) else torch.from_numpy(np.ascontiguousarray(b)).to("cuda:0")
    h, w, _ = d_a.shape
    tcx, tcy = ra.tile_grid(w, h, tile_w, tile_h)
    count = tcx*tcy if ids is None else len(ids)
    d_ids = None if ids is None else torch.tensor(list(ids), dtype=torch.int32, device="cuda:0")
    d_err = torch.full((count,), -5.0, dtype=torch.float32, device="cuda:0")
    d_val = torch.full((count,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize(0)
    p = p if p is not None else rt.default_tile_error_params()
    code = rt.lib().rt_tile_error_device(0, C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr()), w, h, tile_w, tile_h,
                                         C.c_void_p(d_ids.data_ptr()) if d_ids is not None else None, count, C.byref(p),
                                         C.c_void_p(d_err.data_ptr()), C.c_void_p(d_val.data_ptr()), None)
    assert code == 0, rt.lib().rt_last_error()
    return d_err.cpu().numpy(), d_val.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("w,h,tw,th", ra.SHAPES)
def test_tile_error_matches_the_checker_on_synthetic_buffers(rt, w, h, tw, th):
    import torch
    a, b, sub = ra.synthetic_case(w, h, tw, th)
    mismatches = 0
    for ids in (None, sub):
        want_e, want_v = ra.tile_error(a, b, tw, th, ids)
        got_e, got_v = device_tile_error(rt, torch, a, b, tw, th, ids)
        mismatches += int(np.count_nonzero(ra.bits(got_e) != ra.bits(want_e))) + int(np.count_nonzero(got_v != want_v))
    assert np.isposinf(got_e[0]) and got_v[0] == 0                      # the sub-list starts at the tile with no valid pixel
    same_e, same_v = device_tile_error(rt, torch, a, a.copy(), tw, th, None)
    assert (same_e[same_v > 0] == 0.0).all()                            # A equal to B: exactly 0
    if tw == th:                                                        # the host entry (square tiles in the wrapper)
        host_e, host_v = rt.tile_error(a, b, tile=tw, tile_ids=sub)
        want_e, want_v = ra.tile_error(a, b, tw, th, sub)
        mismatches += int(np.count_nonzero(ra.bits(host_e) != ra.bits(want_e))) + int(np.count_nonzero(host_v != want_v))
    REPORT[f"tile_error_{w}x{h}_{tw}x{th}"] = {"mismatches": mismatches}
    assert mismatches == 0


def test_tile_error_matches_the_checker_on_rendered_halves(rt, c3):
    import torch
    a, _ = c3.tiles(64, list(range(6)), spp=2, frame_count=0)
    b, _ = c3.tiles(64, list(range(6)), spp=2, frame_count=2)
    ha, hb = a.cpu().numpy(), b.cpu().numpy()
    for tile, ids in ((64, None), (64, [5, 0, 3]), (16, None), (16, list(range(1, 84, 5)))):
        want_e, want_v = ra.tile_error(ha, hb, tile, tile, ids)
        got_e, got_v = device_tile_error(rt, torch, a, b, tile, tile, ids)
        assert np.array_equal(ra.bits(got_e), ra.bits(want_e)) and np.array_equal(got_v, want_v), (tile, ids)
        assert np.isfinite(want_e).all() and (want_e > 0).all()
    print("C3 192x108, 2 + 2 spp, 64x64 tiles:", ra.tile_error(ha, hb, 64, 64)[0])


# ---- 3. the driver

def adaptive_params(rt, mn, mx, step, threshold):
    p = rt.default_adaptive_params()
    p.min_spp, p.max_spp, p.step_spp, p.threshold = mn, mx, step, threshold
    return p


def hand_loop(rt, case, tile, p, fill):
    """rt_render_adaptive_device's definition, on the two public entries below it."""
    torch = case.torch
    n = case.ntiles(tile)
    half = [case.zeros(), case.zeros()]
    active, spp, total, r = list(range(n)), [0]*n, None, 0
    while active and r*p.step_spp < p.max_spp:
        for k in range(2):
            _, s = case.tiles(tile, active, d=half[k], spp=p.step_spp//2, frame_count=r*p.step_spp + k*(p.step_spp//2))
            total = add_rays(total, s)
        for t in active:
            spp[t] += p.step_spp
        if (r + 1)*p.step_spp >= p.min_spp:
            err, _ = device_tile_error(rt, torch, half[0], half[1], tile, tile, active, p.error)
            active = [t for t, e in zip(active, err) if not e <= p.threshold]
        r += 1
    out = case.zeros(fill) + (half[0] + half[1])
    torch.cuda.synchronize(0)
    return out, spp, total


# C3 at 192x108, 64x64 tiles, min 4 / max 12 / step 4 at total_frame_index 3.  The in-between threshold was
# chosen on the CPU, with the oracle's frames of the same lists (oracle_render_tiles) fed to the checker: the
# errors after round 0 are 0.86 2.30 0.84 / 2.91 1.93 2.20, so at 1.2 the two top corners (tiles 0 and 2:
# the environment, the least noisy) retire first at 4 spp; after round 1 tiles 4 and 5 (0.92, 0.94) retire at
# 8 spp, and tiles 1 and 3 (1.45, 1.62: the mesh and its shadow) run to 12.  Expected map: 4 12 4 / 12 8 8.  No
# tile of these presets has an error of exactly 0: the sky is an environment map (C1: a gradient), and the
# filter's weights differ between the halves.
@pytest.mark.parametrize("threshold,fill,workspace", [(0.0, 0.0, False), (1e30, 0.0, True), (1.2, 0.5, True)])
def test_driver_equals_the_hand_written_loop(rt, c3, threshold, fill, workspace):
    torch = c3.torch
    p = adaptive_params(rt, 4, 12, 4, threshold)
    want, want_spp, want_rays = hand_loop(rt, c3, 64, p, fill)
    d = c3.zeros(fill)
    ws = None
    if workspace:
        ws = torch.full((rt.adaptive_workspace_bytes(c3.w, c3.h, 64)//4,), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize(0)
    spp, stats = c3.dev.render_adaptive_device(c3.cam, c3.st, c3.fc, c3.w, c3.h, p, d.data_ptr(),
                                               d_workspace=ws.data_ptr() if ws is not None else None, total_frame_index=TFI)
    print("threshold", threshold, "tile spp", spp.tolist(), "seconds", stats.seconds)
    REPORT[f"adaptive_driver_threshold_{threshold:g}"] = {"tile_spp": spp.tolist(), "samples": int(stats.samples)}
    assert same_bits(d, want)
    assert spp.reshape(-1).tolist() == want_spp
    assert rays(stats) == want_rays
    assert stats.seconds > 0 and stats.splat_mode == rt.abi.RT_SPLAT_EXACT
    if threshold == 0.0:
        # every tile runs to max_spp: the sequence of uniform frames, half by half
        assert set(want_spp) == {12}
        half = [c3.zeros(), c3.zeros()]
        for r in range(3):
            for k in range(2):
                c3.shard(64, d=half[k], spp=2, frame_count=4*r + 2*k)
        assert same_bits(d, half[0] + half[1])
        assert stats.samples == 12*c3.w*c3.h
    elif threshold == 1e30:
        assert set(want_spp) == {4}
    else:
        assert min(want_spp) == 4 and max(want_spp) == 12          # a tile retires at min_spp, a tile runs to max_spp
        assert want_spp[0] == 4 and want_spp[2] == 4                # the corners of the environment retire first


def test_minimal_parameters(rt, c3):
    """max_spp = min_spp = step_spp = 2: one round of one sample per half."""
    p = adaptive_params(rt, 2, 2, 2, 0.0)
    d = c3.zeros()
    spp, stats = c3.dev.render_adaptive_device(c3.cam, c3.st, c3.fc, c3.w, c3.h, p, d.data_ptr(), total_frame_index=TFI)
    a, sa = c3.shard(64, spp=1, frame_count=0)
    b, sb = c3.shard(64, spp=1, frame_count=1)
    assert same_bits(d, c3.zeros() + (a + b))
    assert set(spp.reshape(-1).tolist()) == {2} and stats.samples == 2*c3.w*c3.h
    assert rays(stats) == add_rays(add_rays(None, sa), sb)
    # the host entry gives the same frame
    host, host_spp, _ = c3.dev.render_adaptive(c3.cam, c3.st, c3.fc, c3.w, c3.h, p, total_frame_index=TFI)
    assert np.array_equal(ra.bits(host), ra.bits(d.cpu().numpy())) and np.array_equal(host_spp, spp)


def test_cancel_mid_loop(rt):
    """rt_cancel from another thread while the loop runs returns RT_ERROR_CANCELLED; the next call is bit-exact."""
    case = Case(rt, "c3", 640, 360, 4)
    small = adaptive_params(rt, 4, 8, 4, 1.2)
    long = adaptive_params(rt, 32, 32*400, 32, 0.0)       # far longer than the cancel takes to land
    returned = threading.Event()

    def cancel_until_returned():
        # a frame clears the flag when its wavefront loop starts, so one rt_cancel may be lost: repeated, it lands
        while not returned.is_set():
            case.dev.cancel()
            returned.wait(0.005)

    try:
        before = case.zeros()
        spp_before, _ = case.dev.render_adaptive_device(case.cam, case.st, case.fc, case.w, case.h, small, before.data_ptr(),
                                                        total_frame_index=TFI)
        d = case.zeros(3.0)
        canceller = threading.Thread(target=cancel_until_returned)
        canceller.start()
        try:
            with pytest.raises(rt.RenderError) as ei:
                case.dev.render_adaptive_device(case.cam, case.st, case.fc, case.w, case.h, long, d.data_ptr(),
                                                total_frame_index=TFI)
        finally:
            returned.set()
            canceller.join()
        assert ei.value.code == rt.abi.RT_ERROR_CANCELLED
        assert bool((d == 3.0).all())                      # a cancelled call leaves the caller's buffer alone
        after = case.zeros()
        spp_after, _ = case.dev.render_adaptive_device(case.cam, case.st, case.fc, case.w, case.h, small, after.data_ptr(),
                                                       total_frame_index=TFI)
    finally:
        case.close()
    assert same_bits(after, before) and np.array_equal(spp_after, spp_before)


def test_nothing_existing_moved(rt):
    """A default rt_render_device frame of C3-small (the default, streaming splat) is byte-identical before and after
    an adaptive render on the same scene."""
    case = Case(rt, "c3", 192, 108, 16, exact=False)
    try:
        before, sb = case.shard(64)
        d = case.zeros()
        case.dev.render_adaptive_device(case.cam, case.st, case.fc, case.w, case.h, adaptive_params(rt, 4, 12, 4, 1.2),
                                        d.data_ptr(), total_frame_index=TFI)
        after, sa = case.shard(64)
    finally:
        case.close()
    assert same_bits(after, before)
    assert rays(sa) == rays(sb) and sa.splat_mode == sb.splat_mode == rt.abi.RT_SPLAT_STREAM
