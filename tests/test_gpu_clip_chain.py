"""The clip entry without a neighbourhood is the deform entry, on the device and bit for bit: the last link of the chain
clip == deform == motion == moments == plain that tests/test_gpu_motion_moments.py started."""
import numpy as np
import pytest
import torch        # before the product library's first HIP call: a process has room for one HIP runtime, torch's own

import ref_clip_binding as cb
import ref_deform_binding as db
import ref_temporal_binding as tb
from test_gpu_clip import device_stage, device_stats, full, host, mismatches, to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,amount", tb.SIZES)
def test_clip_entry_without_a_neighbourhood_is_the_deform_entry(rt, w, h, amount):
    cur, g, prev, cam, moving, surf, arrays, tp = db.deform_case(w, h, amount)
    p = tb.params()
    d_cur, d_g, d_surf, d_moving = to_device(cur), to_device(g), to_device(surf), to_device(moving)
    d_prev = tuple(to_device(a) for a in prev)
    d_arrays = {k: (to_device(t), None if n is None else to_device(n)) for k, (t, n) in arrays.items()}
    table = db.table(tp, {k: (t.data_ptr(), 0 if n is None else n.data_ptr(), w*h) for k, (t, n) in d_arrays.items()})
    d_table = to_device(table)
    d_nb = device_stats(rt, d_cur, w, h, 3, p.firefly_clamp)
    for moments in (False, True):
        for velocity in (False, True):
            for history in (d_prev, None):
                args = (d_cur, d_g, history, cam if history else None, amount, p, w, h, d_moving, len(moving), d_surf, d_table,
                        len(table), moments, velocity)
                want = device_stage(rt, *args, None, 0.0, 0.0, False, deform_entry=True)
                # no neighbourhood; texels that min_count switches off
                for nb, gamma, min_count in ((None, 1.0, 0.0), (d_nb, 1.0, 50.0)):
                    got = device_stage(rt, *args, nb, gamma, min_count, True)
                    assert sum(mismatches(a, b) for a, b in zip(got[:4], want[:4]) if b is not None) == 0
                    assert not tb.bits(host(got[4])).any()
    # and with the texels on it is another stage
    args = (d_cur, d_g, d_prev, cam, amount, p, w, h, d_moving, len(moving), d_surf, d_table, len(table), False, False)
    want = device_stage(rt, *args, None, 0.0, 0.0, False, deform_entry=True)
    got = device_stage(rt, *args, d_nb, 1.0, 2.0, True)
    assert mismatches(got[0], want[0]) > 0 and int((host(got[4]) > 0).sum()) == int((cb.checked(w, h, amount, False, False, 1.0)[4] > 0).sum())
    del d_arrays
