"""The claim -> slot mapping of the dense path generation (no GPU).

A k_shade wave leaves its survivors at the front of its 64 slots; the new paths of the next
iteration claim the free slots behind them in slot order.  k_generate makes 64 consecutive claims
per wave and finds each claim's slot from the scan of the free counts (claim_to_slot: a 64-ary search
over the blocks' first claims, then the lanes' own blocks, then the wave inside the block).
rt_debug_claim_slots runs those steps on the host; here it is compared with the plain enumeration of
the free slots in slot order.
"""
import ctypes as C

import numpy as np
import pytest


def _enumerate(free_w):
    """Every free slot in slot order: wave w's last free_w[w] slots."""
    out = []
    for w, f in enumerate(free_w):
        out.extend(range(64 * w + 64 - int(f), 64 * w + 64))
    return np.array(out, np.uint32)


def _claim_slots(rt, free_w, first, count):
    free_w = np.ascontiguousarray(free_w, np.uint32)
    out = np.full(max(count, 1), 0xFFFFFFFF, np.uint32)
    err = rt.lib().rt_debug_claim_slots(free_w.ctypes.data_as(C.POINTER(C.c_uint32)), len(free_w), first, count,
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return err, out[:count]


def _pattern(name, nwaves):
    rng = np.random.default_rng(5)
    f = np.zeros(nwaves, np.uint32)
    if name == "all_free":
        f[:] = 64
    elif name == "one_in_every_65th_block":     # 64 claims span more than 64 blocks
        f[np.arange(0, nwaves // 4, 65) * 4 + 2] = 1
    elif name == "full_and_empty_blocks":       # blocks of 256 free next to blocks of 0
        blocks = rng.integers(0, 2, nwaves // 4).astype(np.uint32)
        f[:] = np.repeat(blocks, 4) * 64
    elif name == "random":
        f[:] = rng.integers(0, 65, nwaves)
    elif name == "sparse_random":               # mostly full waves, a few free slots here and there
        f[:] = np.where(rng.random(nwaves) < 0.05, rng.integers(1, 4, nwaves), 0)
    elif name == "steady_state":                # about 29 % free, as at the flagship's steady state
        f[:] = np.clip(rng.normal(18.0, 4.0, nwaves), 0, 64).astype(np.uint32)
    else:
        raise KeyError(name)
    return f


PATTERNS = ["all_free", "one_in_every_65th_block", "full_and_empty_blocks", "random", "sparse_random", "steady_state"]


@pytest.mark.parametrize("nwaves", [4, 8, 260, 4096, 66 * 4 * 65])
@pytest.mark.parametrize("name", PATTERNS)
def test_every_claim_maps_to_its_free_slot(rt, name, nwaves):
    free_w = _pattern(name, nwaves)
    want = _enumerate(free_w)
    err, got = _claim_slots(rt, free_w, 0, len(want))
    assert err == 0, rt.lib().rt_last_error()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", PATTERNS)
def test_partial_ranges(rt, name):
    """A first claim in the middle of a block and counts that are no multiple of 64 (the last,
    partial claim of a frame)."""
    free_w = _pattern(name, 3000)
    want = _enumerate(free_w)
    rng = np.random.default_rng(9)
    for _ in range(12):
        if len(want) == 0:
            break
        first = int(rng.integers(0, len(want)))
        count = int(rng.integers(1, min(len(want) - first, 1000) + 1))
        err, got = _claim_slots(rt, free_w, first, count)
        assert err == 0
        assert np.array_equal(got, want[first:first + count]), (first, count)
    for first, count in ((0, 1), (0, 63), (0, 65), (len(want) // 2, 129), (max(len(want) - 7, 0), min(len(want), 7))):
        if first + count <= len(want):
            err, got = _claim_slots(rt, free_w, first, count)
            assert err == 0
            assert np.array_equal(got, want[first:first + count]), (first, count)


def test_nothing_free(rt):
    free_w = np.zeros(4096, np.uint32)
    err, got = _claim_slots(rt, free_w, 0, 0)
    assert err == 0 and len(got) == 0
    err, _ = _claim_slots(rt, free_w, 0, 1)           # no free slot to claim
    assert err != 0


def test_rejects_bad_input(rt):
    assert _claim_slots(rt, np.full(6, 64, np.uint32), 0, 1)[0] != 0        # not whole blocks
    assert _claim_slots(rt, np.full(4, 65, np.uint32), 0, 1)[0] != 0        # more than a wave's slots
    assert _claim_slots(rt, np.full(4, 64, np.uint32), 200, 57)[0] != 0     # past the last free slot
    err, got = _claim_slots(rt, np.full(4, 64, np.uint32), 200, 56)
    assert err == 0 and np.array_equal(got, np.arange(200, 256, dtype=np.uint32))
