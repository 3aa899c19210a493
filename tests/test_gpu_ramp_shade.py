"""The dense ramp-down shade on the device (k_shade's RAMP instantiation) against the CPU
oracle and against the same frame with rt_scene_config::ramp_shade off.

Once every sample is claimed the pool only empties; the ramp k_shade shades the alive paths by rank
(wave j the ranks [64j, 64j + 64), found through the rank -> slot map) and writes at its own slots, so
the survivors move to the front of the pool.  The frames are those of tests/test_gpu_dense_generate.py
(67x41 at 5 spp from pools of 1,024 paths), with the fused drain off (fuse_paths 0) or late (16 paths), so
the ramp runs the whole tail; at this pool the auto threshold would fuse at once.  Every schedule must
give what the existing frame rule asks (>= 99.9 % of the exact-splat frame's pixels equal to the oracle's,
rel L2 <= 1e-6, equal ray counts) and the very bits, counts and TraversalStats of the run with the switch
off, and rt_scene_ramp_stats must report ramp iterations (none with max_bounce_count 0), so that no case
passes by never entering the ramp.
"""
import numpy as np
import pytest

import oracle_binding as ob
from test_gpu_dense_generate import H, POOL, SPP, W, Case, check_frame, rays

pytestmark = pytest.mark.gpu

ON, OFF = 1, 2
FUSE = [0, 16]


@pytest.fixture(scope="module")
def cases(rt):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(rt, name)
        return made[name]
    yield get
    for c in made.values():
        c.dev.close()


def counts(s):
    return (rays(s), int(s.samples), tuple(int(t) for t in s.traced_rays),
            tuple(tuple(sorted(s.traversal[k].as_dict().items())) for k in range(2)))


def on_and_off(c, st=None, ramp_iterations=True, **cfg):
    """The exact-splat frame with the ramp shade on, checked against the run with it off."""
    gpu, gs = c.exact(st=st, ramp_shade=ON, **cfg)
    it_on, paths_on = c.dev.ramp_stats()
    off, os_ = c.exact(st=st, ramp_shade=OFF, **cfg)
    it_off, paths_off = c.dev.ramp_stats()
    print("ramp iterations / paths: on", it_on, paths_on, "off", it_off, paths_off, "frame iterations",
          int(gs.iterations), int(os_.iterations))
    assert np.array_equal(gpu.view(np.uint32), off.view(np.uint32))
    assert counts(gs) == counts(os_)
    # the probe counts the same ramp whichever kernel shades it
    assert (it_on, paths_on) == (it_off, paths_off)
    if ramp_iterations:
        assert it_on >= 1 and paths_on >= it_on
    else:
        assert (it_on, paths_on) == (0, 0)
    return gpu, gs


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("parts", [1, 4])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_partitions(cases, name, parts, fuse):
    c = cases(name)
    gpu, gs = on_and_off(c, partitions=parts, fuse_paths=fuse)
    check_frame(gpu, gs, *c.oracle())


@pytest.mark.parametrize("every", [1, 2, 3])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_drain_cadence(cases, name, every):
    """Iterations with and without the drain kernels, the fused drain late: the standard and the ramp
    form of the bounce interleave on the compact layout."""
    c = cases(name)
    gpu, gs = on_and_off(c, drain_every=every, fuse_paths=16)
    check_frame(gpu, gs, *c.oracle())


@pytest.mark.parametrize("fuse", FUSE)
@pytest.mark.parametrize("launch", ["separate", "merged"])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_shadow_launch(cases, name, launch, fuse):
    c = cases(name)
    a = c.rt.abi
    mode = a.RT_SHADOW_LAUNCH_SEPARATE if launch == "separate" else a.RT_SHADOW_LAUNCH_MERGED
    gpu, gs = on_and_off(c, shadow_launch=mode, fuse_paths=fuse)
    assert gs.shadow_launch == mode
    check_frame(gpu, gs, *c.oracle())


@pytest.mark.parametrize("sampler", ["uniform", "blue_noise", "stratified"])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_samplers(cases, name, sampler):
    c = cases(name)
    a = c.rt.abi
    strategy = {"uniform": a.RT_SAMPLING_UNIFORM, "blue_noise": a.RT_SAMPLING_OPTIMIZED_BLUE_NOISE,
                "stratified": a.RT_SAMPLING_STRATIFIED}[sampler]
    st = c.settings(sampling_strategy=strategy)
    gpu, gs = on_and_off(c, st=st, fuse_paths=0)
    check_frame(gpu, gs, *c.oracle(f"sampler_{sampler}", st=st))


@pytest.mark.parametrize("depth", [1, 2, 12])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_bounce_limits(cases, name, depth):
    """A bounce limit of 1 ends every path in the k_shade of its claim's iteration, so nothing is pending
    when the claims end and no iteration is a ramp one; from 2 on the last claims' paths outlive them."""
    c = cases(name)
    st = c.settings(max_bounce_count=depth)
    gpu, gs = on_and_off(c, st=st, fuse_paths=0, ramp_iterations=depth > 1)
    check_frame(gpu, gs, *c.oracle(f"depth{depth}", st=st))


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_no_bounces_never_ramp(cases, name):
    """max_bounce_count 0: k_generate finishes every path, no ray is cast, no iteration is a ramp one."""
    c = cases(name)
    st = c.settings(max_bounce_count=0)
    gpu, gs = on_and_off(c, st=st, fuse_paths=0, ramp_iterations=False)
    check_frame(gpu, gs, *c.oracle("depth0", st=st))


@pytest.mark.parametrize("fuse", FUSE)
def test_dielectrics(cases, fuse):
    """c4's glass: the material stack is read at the rank's slot (its push too) and moves to the thread's."""
    c = cases("c4")
    gpu, gs = on_and_off(c, fuse_paths=fuse)
    check_frame(gpu, gs, *c.oracle())


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_environment_nee(cases, name):
    c = cases(name)
    gpu, gs = on_and_off(c, env_sampling=1, fuse_paths=0)
    with ob.env_sampling(1):
        cpu, cs = c.oracle("env")
    check_frame(gpu, gs, cpu, cs)
    plain, _ = c.exact(fuse_paths=0)
    assert not np.array_equal(gpu, plain)              # the option was really on


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_stream_splat(cases, name):
    """A streaming-splat frame, bit for bit with the switch on and off."""
    c = cases(name)
    frames = []
    for ramp in (ON, OFF):
        with c.dev.configured(ramp_shade=ramp, fuse_paths=0):
            f, s = c.dev.render(c.cam, c.st, c.fc, W, H)
        assert s.splat_mode == c.rt.abi.RT_SPLAT_STREAM
        frames.append((f, s, c.dev.ramp_stats()))
    (f1, s1, r1), (f0, s0, r0) = frames
    assert np.array_equal(f1.view(np.uint32), f0.view(np.uint32))
    assert counts(s1) == counts(s0) and r1 == r0 and r1[0] >= 1
    assert rays(s1) == rays(c.oracle()[1])


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_sample_list(cases, name):
    """rt_trace_samples: 3,001 samples through the pool of 1,024."""
    c = cases(name)
    rng = np.random.default_rng(17)
    n = 3001
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.uint32)
    s = rng.integers(0, SPP, n).astype(np.uint32)
    out = []
    for ramp in (ON, OFF):
        with c.dev.configured(ramp_shade=ramp, fuse_paths=0):
            g, gs = c.dev.trace_samples(c.cam, c.st, W, H, xy, s)
        out.append((g, gs, c.dev.ramp_stats()))
    (g1, s1, r1), (g0, s0, r0) = out
    print("ramp iterations / paths", r1)
    assert np.array_equal(g1.view(np.uint32), g0.view(np.uint32))
    assert counts(s1) == counts(s0) and r1 == r0 and r1[0] >= 1
    cpu, cs = ob.trace_samples(c.scene.desc(), c.cam, c.st, W, H, xy, s)
    exact = np.all((g1 == cpu) | (np.isnan(g1) & np.isnan(cpu)), axis=1)
    assert exact.mean() >= 0.999
    assert rays(s1) == rays(cs) or exact.mean() < 1.0


def test_switch_values(cases):
    c = cases("c1")
    assert c.dev.config().ramp_shade == 0              # auto: on
    with pytest.raises(c.rt.RenderError):
        c.dev.configure(ramp_shade=3)
    assert POOL == 1024
