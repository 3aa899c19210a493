"""The motion-aware accumulate stage against the moments stage, on the GPU: with moments and no table (or an unmoved
one) rt_temporal_accumulate_motion_device is rt_temporal_accumulate_moments_device bit for bit.  The missing link of the
chain deform == motion == moments == plain: tests/test_gpu_motion.py has 'motion == plain without a table',
tests/test_gpu_svgf.py 'moments == plain', tests/test_gpu_deform.py 'deform == motion without a table'.  The inputs and
helpers are tests/test_gpu_motion.py's."""
import pytest

import ref_motion_binding as mb
import ref_temporal_binding as tb
import test_gpu_motion as tm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_moments_without_a_table_are_the_moments_stage(rt, w, h, amount):
    import torch
    cur, g, prev, cam, moving, unmoved = mb.motion_case(w, h, amount)
    p = tb.params()
    d_cur, d_g = tm.to_device(torch, cur), tm.to_device(torch, g)
    d_prev = tuple(tm.to_device(torch, a) for a in prev)
    want = tm.garbage(torch, h, w, 4), tm.garbage(torch, h, w), tm.garbage(torch, h, w, 2)
    rt.temporal_accumulate_moments_device(d_cur.data_ptr(), d_g.data_ptr(), d_prev[0].data_ptr(), d_prev[1].data_ptr(),
                                          d_prev[2].data_ptr(), d_prev[3].data_ptr(), cam, amount, w, h, p,
                                          want[0].data_ptr(), want[1].data_ptr(), want[2].data_ptr())
    # the taps do run: some pixel has a history longer than one frame
    assert int((want[1] > 1.0).sum()) > 20
    for table, count in ((None, 0), (tm.to_device(torch, unmoved), len(unmoved))):
        got = tm.device_stage(rt, torch, d_cur, d_g, d_prev, cam, amount, p, w, h, table, count, True, False)
        bad = [tm.mismatches(a, b) for a, b in zip(got[:3], want)]
        print(f"{w}x{h}, table of {count}: words of history, length, moments that differ from the moments stage", bad)
        assert bad == [0, 0, 0]
