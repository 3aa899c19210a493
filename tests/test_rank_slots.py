"""The rank -> slot mapping of the dense ramp-down shade (no GPU).

Once every sample is claimed a k_shade wave's survivors still sit at the front of its 64 slots, and
fewer of them every bounce.  The ramp k_shade ranks the alive paths in slot order and has wave j of
the launch shade the ranks [64j, 64j + 64): it finds a rank's slot from the scan of the free counts
(rank_to_slot: block b holds the ranks from 256 b - claim_base[b] on, a 64-ary search over those keys
that takes the last of equal ones, then the wave inside the block).  rt_debug_rank_slots runs those
steps on the host; here it is compared with the plain enumeration of the alive slots in slot order.
"""
import ctypes as C

import numpy as np
import pytest


def _enumerate(free_w):
    """Every alive slot in slot order: wave w's first 64 - free_w[w] slots."""
    out = []
    for w, f in enumerate(free_w):
        out.extend(range(64 * w, 64 * w + 64 - int(f)))
    return np.array(out, np.uint32)


def _rank_slots(rt, free_w, first, count):
    free_w = np.ascontiguousarray(free_w, np.uint32)
    out = np.full(max(count, 1), 0xFFFFFFFF, np.uint32)
    err = rt.lib().rt_debug_rank_slots(free_w.ctypes.data_as(C.POINTER(C.c_uint32)), len(free_w), first, count,
                                       out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return err, out[:count]


def _check_all(rt, free_w):
    want = _enumerate(free_w)
    err, got = _rank_slots(rt, free_w, 0, len(want))
    assert err == 0, rt.lib().rt_last_error()
    assert np.array_equal(got, want)          # every alive slot once, in slot order
    return want


BLOCKS = [1, 3, 64, 65, 4097]


@pytest.mark.parametrize("nblocks", BLOCKS)
@pytest.mark.parametrize("seed", [1, 2])
def test_random_free_counts(rt, nblocks, seed):
    rng = np.random.default_rng(100 * seed + nblocks)
    free_w = rng.integers(0, 65, 4 * nblocks).astype(np.uint32)
    _check_all(rt, free_w)
    free_w[0] = (int(free_w[0]) - int(free_w.sum()) - 17) % 64                # 64 k + 17 paths alive
    assert (256 * nblocks - int(free_w.sum())) % 64 == 17
    _check_all(rt, free_w)


@pytest.mark.parametrize("nblocks", BLOCKS)
def test_all_full_and_all_empty(rt, nblocks):
    want = _check_all(rt, np.zeros(4 * nblocks, np.uint32))      # every slot alive: the identity
    assert np.array_equal(want, np.arange(256 * nblocks, dtype=np.uint32))
    free_w = np.full(4 * nblocks, 64, np.uint32)                   # nothing alive
    err, got = _rank_slots(rt, free_w, 0, 0)
    assert err == 0 and len(got) == 0
    assert _rank_slots(rt, free_w, 0, 1)[0] != 0


def _with_empty_runs(nblocks, where, rng):
    free_w = rng.integers(0, 64, 4 * nblocks).astype(np.uint32)
    run = max(1, nblocks // 3)
    lo = {"front": 0, "middle": (nblocks - run) // 2, "end": nblocks - run}[where]
    free_w[4 * lo:4 * (lo + run)] = 64
    return free_w


@pytest.mark.parametrize("where", ["front", "middle", "end"])
@pytest.mark.parametrize("nblocks", [3, 64, 65, 200, 4097])
def test_runs_of_empty_blocks(rt, nblocks, where):
    """Empty blocks repeat their neighbour's key: the search takes the last block of equal keys.  A run
    of more than 64 empty blocks (200 and 4,097 blocks) makes a wave's ranks step over whole rounds."""
    free_w = _with_empty_runs(nblocks, where, np.random.default_rng(nblocks))
    _check_all(rt, free_w)


def test_empty_runs_everywhere_and_full_blocks_between(rt):
    rng = np.random.default_rng(3)
    blocks = rng.integers(0, 3, 4097)                    # 0: empty, 1: full, 2: ragged
    free_w = np.where(np.repeat(blocks, 4) == 0, 64, np.where(np.repeat(blocks, 4) == 1, 0,
                                                                 rng.integers(0, 65, 4 * 4097))).astype(np.uint32)
    _check_all(rt, free_w)


def test_one_path_in_every_65th_block(rt):
    """64 ranks that span more than 64 blocks."""
    free_w = np.full(4 * 66 * 65, 64, np.uint32)
    free_w[np.arange(0, 66 * 65, 65) * 4 + 2] = 63
    _check_all(rt, free_w)


def test_partial_ranges(rt):
    """A first rank in the middle of a block and counts that are no multiple of 64 (the last, partial
    wave of the ranks)."""
    rng = np.random.default_rng(9)
    free_w = rng.integers(0, 65, 3000).astype(np.uint32)
    want = _enumerate(free_w)
    assert len(want) % 64 != 0
    for _ in range(12):
        first = int(rng.integers(0, len(want)))
        count = int(rng.integers(1, min(len(want) - first, 1000) + 1))
        err, got = _rank_slots(rt, free_w, first, count)
        assert err == 0
        assert np.array_equal(got, want[first:first + count]), (first, count)
    for first, count in ((0, 1), (0, 63), (0, 65), (len(want) // 2, 129), (len(want) - 7, 7)):
        err, got = _rank_slots(rt, free_w, first, count)
        assert err == 0
        assert np.array_equal(got, want[first:first + count]), (first, count)


def test_rejects_bad_input(rt):
    assert _rank_slots(rt, np.zeros(6, np.uint32), 0, 1)[0] != 0            # not whole blocks
    assert _rank_slots(rt, np.full(4, 65, np.uint32), 0, 1)[0] != 0          # more than a wave's slots
    assert _rank_slots(rt, np.full(4, 60, np.uint32), 10, 7)[0] != 0         # past the last alive path
    err, got = _rank_slots(rt, np.full(4, 60, np.uint32), 10, 6)
    assert err == 0 and np.array_equal(got, np.array([130, 131, 192, 193, 194, 195], np.uint32))
