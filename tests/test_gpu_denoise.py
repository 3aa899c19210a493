"""The denoise stage on the device: rt_denoise_device, rt_denoise and rt_render_picture_denoised against the
plain-C checker tests/ref_denoise, bit for bit ("The denoise stage")."""
import ctypes as C

import numpy as np
import pytest

import ref_denoise_binding as rd
from parity_report import REPORT

pytestmark = pytest.mark.gpu

TFI = 5          # total_frame_index of the rendered cases


def _device_denoise(rt, torch, beauty, g0, g1, p, workspace, in_place):
    """rt_denoise_device on uploaded copies -> the output buffer, downloaded."""
    dev = torch.device("cuda:0")
    h, w, _ = beauty.shape
    d_b = torch.from_numpy(beauty).to(dev)
    d_g = [None if g is None else torch.from_numpy(g).to(dev) for g in (g0, g1)]
    d_out = d_b if in_place else torch.full((h, w, 4), 123.0, dtype=torch.float32, device=dev)
    d_ws = None
    if workspace:
        d_ws = torch.full((rt.denoise_workspace_bytes(w, h) // 4,), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(0)
    err = rt.lib().rt_denoise_device(0, C.c_void_p(d_b.data_ptr()), *[C.c_void_p(g.data_ptr()) if g is not None else None
                                                                    for g in d_g], w, h, C.byref(p),
                                     C.c_void_p(d_ws.data_ptr()) if d_ws is not None else None,
                                     C.c_void_p(d_out.data_ptr()), None)
    assert err == 0, rt.lib().rt_last_error()
    if not in_place:                                   # the inputs are read-only
        assert np.array_equal(rd.bits(d_b.cpu().numpy()), rd.bits(beauty))
    return d_out.cpu().numpy()


def _host_denoise(rt, beauty, g0, g1, p):
    fp = C.POINTER(C.c_float)
    h, w, _ = beauty.shape
    out = np.zeros((h, w, 4), np.float32)
    buf = rt.abi.AccumulationBuffer(w, h, 0, beauty.ctypes.data_as(fp))
    err = rt.lib().rt_denoise(0, C.byref(buf), *[g.ctypes.data_as(fp) if g is not None else None for g in (g0, g1)],
                              C.byref(p), out.ctypes.data_as(fp))
    assert err == 0, rt.lib().rt_last_error()
    return out


# 1x1; 5x3: every tap past step 1 is outside; 65x33 and 130x7: the ragged shapes (a partial block in x and y,
# more than one block a row); 70x70: step 16 reaches past both borders
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (65, 33), (130, 7), (70, 70)])
def test_bit_identical_to_the_checker(rt, w, h):
    import torch
    beauty, g0, g1 = rd.random_frames(w, h, seed=100 + w)
    if w*h > 1000:
        valid = rd.denoise(beauty, g0, g1, rd.params(1))[:, :, 3] == 1.0
        invalid = 1.0 - valid.mean()
        assert 0.005 < invalid < 0.06, invalid            # about 2 % invalid pixels
    mismatches, runs = 0, 0
    for iterations in (1, 3, 5):
        for guides in ("both", "one", "none"):
            for color in (1.0, 0.0):
                for clamp in (10.0, 0.0):
                    a0, a1 = g0, g1
                    sg = [0.1, 0.05]
                    if guides == "one":                     # guide 0 alone, or guide 1 alone
                        if iterations == 3:
                            a0, sg[0] = None, 0.0
                        else:
                            a1, sg[1] = None, 0.0
                    elif guides == "none":
                        a0 = a1 = None
                        sg = [0.0, 0.0]
                    p = rd.params(iterations, color, sg, clamp)
                    want = rd.bits(rd.denoise(beauty, a0, a1, p))
                    got = [_host_denoise(rt, beauty, a0, a1, p),
                           _device_denoise(rt, torch, beauty, a0, a1, p, workspace=True, in_place=False),
                           _device_denoise(rt, torch, beauty, a0, a1, p, workspace=False, in_place=False),
                           _device_denoise(rt, torch, beauty, a0, a1, p, workspace=True, in_place=True)]
                    for g in got:
                        mismatches += int(np.count_nonzero(rd.bits(g) != want))
                    runs += len(got)
    REPORT[f"denoise_{w}x{h}"] = {"runs": runs, "mismatching_floats": mismatches}
    print(f"denoise_{w}x{h}", REPORT[f"denoise_{w}x{h}"])
    assert mismatches == 0


def test_a_guide_with_its_term_off_still_decides_validity(rt):
    """sigma_guide[k] = 0 with the guide present: its invalid pixels are invalid, its values are not compared."""
    import torch
    beauty, g0, g1 = rd.random_frames(65, 33, seed=21)
    p = rd.params(3, 1.0, (0.0, 0.05), 10.0)
    want = rd.bits(rd.denoise(beauty, g0, g1, p))
    got = _device_denoise(rt, torch, beauty, g0, g1, p, workspace=True, in_place=False)
    n = int(np.count_nonzero(rd.bits(got) != want))
    REPORT["denoise_guide_term_off"] = {"mismatching_floats": n}
    assert n == 0
    assert not np.array_equal(want, rd.bits(rd.denoise(beauty, None, g1, p)))


@pytest.fixture(scope="module")
def c1(rt):
    """C1 at 96 x 64, 4 spp: the beauty, normals and distances frames rendered on the device into device
    buffers, the filter run on them there, and everything downloaded."""
    import torch
    w, h = 96, 64
    scene, cam, st, fc, post = rt.load_preset("c1", w, h)
    st.samples_per_pixel = 4
    dev = rt.DeviceScene(scene, 0)
    cuda = torch.device("cuda:0")

    def frame(integrator, spp):
        s = rt.abi.Settings.from_buffer_copy(st)
        s.integrator, s.samples_per_pixel = integrator, spp
        d = torch.zeros((h, w, 4), dtype=torch.float32, device=cuda)
        torch.cuda.synchronize(0)
        stats = dev.render_device(cam, s, fc, w, h, d.data_ptr(), total_frame_index=TFI)
        return d, stats
    d_b, stats = frame(st.integrator, 4)
    d_n, _ = frame(rt.abi.RT_INTEGRATOR_NORMALS, 4)
    d_d, _ = frame(rt.abi.RT_INTEGRATOR_DISTANCES, 4)
    p = rt.default_denoise_params()
    d_out = torch.zeros((h, w, 4), dtype=torch.float32, device=cuda)
    torch.cuda.synchronize(0)
    err = rt.lib().rt_denoise_device(0, C.c_void_p(d_b.data_ptr()), C.c_void_p(d_n.data_ptr()), C.c_void_p(d_d.data_ptr()),
                                     w, h, C.byref(p), None, C.c_void_p(d_out.data_ptr()), None)
    assert err == 0, rt.lib().rt_last_error()
    case = dict(w=w, h=h, scene=scene, cam=cam, st=st, fc=fc, post=post, dev=dev, p=p, stats=stats,
                beauty=d_b.cpu().numpy(), normals=d_n.cpu().numpy(), distances=d_d.cpu().numpy(),
                device_out=d_out.cpu().numpy(), frame=frame)
    case["checker_out"] = rd.denoise(case["beauty"], case["normals"], case["distances"], p)
    yield case
    dev.close()


def test_device_frames_match_the_checker(rt, c1):
    n = int(np.count_nonzero(rd.bits(c1["device_out"]) != rd.bits(c1["checker_out"])))
    REPORT["denoise_c1_96x64_4spp"] = {"mismatching_floats": n}
    assert n == 0
    assert (c1["device_out"][:, :, 3] == 1.0).mean() > 0.9        # valid pixels come out with weight 1
    assert not np.array_equal(c1["device_out"][:, :, :3], c1["beauty"][:, :, :3] / c1["beauty"][:, :, 3:])
    # render_guides and denoise, the package's host-side path, give the same frames
    normals, distances = c1["dev"].render_guides(c1["cam"], c1["st"], c1["fc"], c1["w"], c1["h"], 4, total_frame_index=TFI)
    assert np.array_equal(rd.bits(normals), rd.bits(c1["normals"]))
    assert np.array_equal(rd.bits(distances), rd.bits(c1["distances"]))
    out = rt.denoise(c1["beauty"], normals, distances)
    assert np.array_equal(rd.bits(out), rd.bits(c1["checker_out"]))


STAT_FIELDS = ("closest_hit_rays", "shadow_rays", "samples", "splat_mode")


@pytest.mark.parametrize("guide_spp", [0, 1])
def test_the_picture_entry(rt, c1, guide_spp):
    """rt_render_picture_denoised = oracle_postprocess (dither texture total_frame_index + 1) of the checker's
    output for the device's own frames; stats are the beauty frame's."""
    import oracle_binding as ob
    w, h, dev = c1["w"], c1["h"], c1["dev"]
    if guide_spp == 0:
        want_px = c1["checker_out"]
    else:
        d_n, _ = c1["frame"](rt.abi.RT_INTEGRATOR_NORMALS, guide_spp)
        d_d, _ = c1["frame"](rt.abi.RT_INTEGRATOR_DISTANCES, guide_spp)
        want_px = rd.denoise(c1["beauty"], d_n.cpu().numpy(), d_d.cpu().numpy(), c1["p"])
        assert not np.array_equal(want_px, c1["checker_out"])
    want = ob.postprocess(want_px, c1["post"], total_frame_index=TFI + 1)
    got, stats = dev.render_picture_denoised(c1["cam"], c1["st"], c1["fc"], w, h, c1["post"], c1["p"], guide_spp=guide_spp,
                                             total_frame_index=TFI)
    n = int(np.count_nonzero(got != want))
    REPORT[f"denoise_picture_guide_spp{guide_spp}"] = {"mismatching_pixels": n}
    assert n == 0
    # the plain picture's stats for the same frame
    tiles = rt.abi.TileSet(64, 64, 0, 1)
    plain = np.zeros((h, w), np.uint32)
    pstats = rt.abi.Stats()
    err = rt.lib().rt_render_picture(dev._h, C.byref(c1["cam"]), C.byref(c1["st"]), C.byref(c1["fc"]), C.byref(tiles), TFI,
                                     w, h, C.byref(c1["post"]), plain.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pstats))
    assert err == 0
    for f in STAT_FIELDS:
        assert getattr(stats, f) == getattr(pstats, f) == getattr(c1["stats"], f), f
    assert stats.traversal_total() == pstats.traversal_total()
    assert stats.samples == 4*w*h                                  # the beauty frame's, not a guide frame's
    assert np.count_nonzero(plain != got) > 0


def test_a_denoised_picture_leaves_no_trace(rt, c1):
    """A plain rt_render_picture after a denoised one is byte-identical to one taken before it."""
    w, h, dev = c1["w"], c1["h"], c1["dev"]
    tiles = rt.abi.TileSet(64, 64, 0, 1)

    def plain():
        out = np.zeros((h, w), np.uint32)
        err = rt.lib().rt_render_picture(dev._h, C.byref(c1["cam"]), C.byref(c1["st"]), C.byref(c1["fc"]), C.byref(tiles),
                                         TFI, w, h, C.byref(c1["post"]), out.ctypes.data_as(C.POINTER(C.c_uint32)), None)
        assert err == 0
        return out
    before = plain()
    dev.render_picture_denoised(c1["cam"], c1["st"], c1["fc"], w, h, c1["post"], total_frame_index=TFI)
    after = plain()
    assert np.array_equal(before, after)
