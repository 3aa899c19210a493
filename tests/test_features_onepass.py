"""The one-pass feature entries without a device: rt_render_features_device and rt_render_features check their
arguments by name before the device is touched, the host form answers RT_ERROR_NO_DEVICE after its checks on
a machine without a GPU, and both are mirrored in abi.py ("Feature frames")."""
import ctypes as C

import numpy as np
import pytest

W, H = 4, 3
FAKE = C.c_void_p(1)          # a scene / device pointer the refusals never dereference


def _structs(rt):
    st, post = rt.default_settings()
    return rt.abi.Camera(), st, rt.abi.FilterCache(), rt.abi.TileSet(64, 64, 0, 1)


def _device(rt, scene=FAKE, camera=1, settings=1, filter=1, tiles=1, w=W, h=H, normal=16, distance=32, albedo=48):
    cam, st, fc, ts = _structs(rt)
    ref = lambda on, v: C.byref(v) if on else None
    ptr = lambda v: C.c_void_p(v) if v else None
    return rt.lib().rt_render_features_device(scene, ref(camera, cam), ref(settings, st), ref(filter, fc), ref(tiles, ts),
                                              0, w, h, 0, ptr(normal), ptr(distance), ptr(albedo), None, None)


def _host(rt, scene=FAKE, camera=1, settings=1, filter=1, tiles=1, shapes=((W, H, 0),)*3, null=(), shared=None):
    cam, st, fc, ts = _structs(rt)
    ref = lambda on, v: C.byref(v) if on else None
    keep = [np.zeros((max(h, 1), max(w, 1), 4), np.float32) for w, h, _ in shapes]
    if shared is not None:
        keep[shared[1]] = keep[shared[0]]
    bufs = [rt.abi.AccumulationBuffer(w, h, fcnt, a.ctypes.data_as(C.POINTER(C.c_float)))
            for (w, h, fcnt), a in zip(shapes, keep)]
    args = [None if i in null else C.byref(b) for i, b in enumerate(bufs)]
    return rt.lib().rt_render_features(scene, ref(camera, cam), ref(settings, st), ref(filter, fc), ref(tiles, ts), 0,
                                       *args, None)


def _refused(rt, err, word):
    msg = rt.lib().rt_last_error().decode()
    assert err == rt.abi.RT_ERROR_INVALID, (err, msg)
    assert word in msg, msg


def test_the_entries_are_exported(rt):
    for name in ("rt_render_features_device", "rt_render_features"):
        assert name in rt.abi.ABI_FUNCTIONS
        assert getattr(rt.lib(), name).restype is C.c_int
    assert len(rt.abi.ABI_FUNCTIONS["rt_render_features_device"][1]) == 14
    assert len(rt.abi.ABI_FUNCTIONS["rt_render_features"][1]) == 10
    assert rt.lib().rt_abi_version() == 8
    assert callable(rt.DeviceScene.render_features) and callable(rt.DeviceScene.render_features_device)


@pytest.mark.parametrize("kw,word", [
    (dict(scene=None), "scene"), (dict(camera=0), "camera"), (dict(settings=0), "settings"), (dict(filter=0), "filter"),
    (dict(tiles=0), "tiles"), (dict(normal=0), "d_normal"), (dict(distance=0), "d_distance"), (dict(albedo=0), "d_albedo"),
    (dict(distance=16), "d_normal and d_distance"), (dict(albedo=16), "d_normal and d_albedo"),
    (dict(albedo=32), "d_distance and d_albedo"), (dict(w=0), "w is 0"), (dict(h=0), "h is 0"),
])
def test_the_device_entry_refuses_by_name(rt, kw, word):
    _refused(rt, _device(rt, **kw), "rt_render_features_device")
    _refused(rt, _device(rt, **kw), word)


@pytest.mark.parametrize("kw,word", [
    (dict(scene=None), "scene"), (dict(camera=0), "camera"), (dict(settings=0), "settings"), (dict(filter=0), "filter"),
    (dict(tiles=0), "tiles"), (dict(null=(0,)), "normal"), (dict(null=(1,)), "distance"), (dict(null=(2,)), "albedo"),
    (dict(shapes=((W, H, 0), (W + 1, H, 0), (W, H, 0))), "distance differs from normal in w or h"),
    (dict(shapes=((W, H, 0), (W, H, 0), (W, H + 1, 0))), "albedo differs from normal in w or h"),
    (dict(shapes=((W, H, 0), (W, H, 2), (W, H, 0))), "distance differs from normal in frame_count"),
    (dict(shapes=((W, H, 0), (W, H, 0), (W, H, 1))), "albedo differs from normal in frame_count"),
    (dict(shared=(0, 1)), "normal and distance"), (dict(shared=(0, 2)), "normal and albedo"),
    (dict(shared=(1, 2)), "distance and albedo"),
    (dict(shapes=((0, H, 0),)*3), "w is 0"), (dict(shapes=((W, 0, 0),)*3), "h is 0"),
])
def test_the_host_entry_refuses_by_name(rt, kw, word):
    _refused(rt, _host(rt, **kw), "rt_render_features")
    _refused(rt, _host(rt, **kw), word)


def test_a_buffer_without_pixels_is_refused(rt):
    cam, st, fc, ts = _structs(rt)
    good = np.zeros((H, W, 4), np.float32)
    bufs = [rt.abi.AccumulationBuffer(W, H, 0, good.ctypes.data_as(C.POINTER(C.c_float))) for _ in range(2)]
    empty = rt.abi.AccumulationBuffer(W, H, 0, None)
    err = rt.lib().rt_render_features(FAKE, C.byref(cam), C.byref(st), C.byref(fc), C.byref(ts), 0, C.byref(bufs[0]),
                                      C.byref(empty), C.byref(bufs[1]), None)
    _refused(rt, err, "distance")


def test_the_host_entry_without_a_device(rt):
    """After its checks the host form needs a GPU: RT_ERROR_NO_DEVICE on a machine without one (with one, the
    GPU suite renders through it)."""
    if rt.device_count() == 0:
        err = _host(rt)
        assert err == rt.abi.RT_ERROR_NO_DEVICE, rt.lib().rt_last_error()
        assert "rt_render_features" in rt.lib().rt_last_error().decode()
    # a bad argument is refused first, with or without one
    _refused(rt, _host(rt, null=(2,)), "albedo")
