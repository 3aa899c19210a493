"""The dense path generation on the device (k_generate) against the CPU oracle.

k_generate makes 64 consecutive sample claims per wave and writes each new path to the slot its
claim maps to, and splats the finished paths compacted within their block.  The frames here are
67x41 pixels at 5 spp (13,735 samples: no multiple of 64 or 256) rendered from pools of 1,024 paths,
so a frame is many iterations with ragged free tails per wave, claims that span several blocks, and a
last, partial claim; every schedule below must give what the existing parity tests ask of the default
one (tests/test_gpu_parity.py): >= 99.9 % of listed samples bit-exact, the exact-splat frame equal to
the oracle's single-threaded frame on >= 99.9 % of pixels (rel L2 <= 1e-6), and equal ray counts.
"""
import numpy as np
import pytest

import oracle_binding as ob
import ref_binding as rb

pytestmark = pytest.mark.gpu

W, H, SPP, POOL = 67, 41, 5, 1024
NORMALS = 4


def rel_l2(a, b):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rays(s):
    return int(s.closest_hit_rays), int(s.shadow_rays)


class Case:
    """A scene on the device with the oracle's results, each computed once."""

    def __init__(self, rt, name):
        self.rt = rt
        self.scene, self.cam, self.st, self.fc, _ = rt.load_preset(name, W, H)
        self.st.samples_per_pixel = SPP
        self.dev = rt.DeviceScene(self.scene, 0)
        self.dev.configure(path_pool=POOL)
        self._cpu = {}

    def settings(self, **fields):
        c = type(self.st).from_buffer_copy(self.st)
        for k, v in fields.items():
            setattr(c, k, v)
        return c

    def oracle(self, key="default", st=None, **kw):
        if key not in self._cpu:
            self._cpu[key] = ob.render(self.scene.desc(), self.cam, st or self.st, self.fc, W, H, rng_mode=0,
                                       threads=1, **kw)
        return self._cpu[key]

    def exact(self, st=None, **cfg):
        with self.dev.configured(splat_mode=self.rt.abi.RT_SPLAT_EXACT, **cfg):
            frame, stats = self.dev.render(self.cam, st or self.st, self.fc, W, H)
        assert stats.splat_mode == self.rt.abi.RT_SPLAT_EXACT
        return frame, stats


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


def check_frame(gpu, gs, cpu, cs):
    same = float(np.all(gpu == cpu, axis=2).mean())
    err = rel_l2(gpu, cpu)
    print("pixels identical", same, "rel L2", err, "rays", rays(gs), rays(cs))
    assert gs.samples == cs.samples == W*H*SPP
    assert same >= 0.999 and err <= 1e-6, (same, err)
    assert rays(gs) == rays(cs)


@pytest.mark.parametrize("parts", [1, 4])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_partitions(cases, name, parts):
    c = cases(name)
    gpu, gs = c.exact(partitions=parts)
    check_frame(gpu, gs, *c.oracle())


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_sample_list(cases, name):
    """rt_trace_samples: the claims index the list, 3,001 samples through a pool of 1,024."""
    c = cases(name)
    rng = np.random.default_rng(17)
    n = 3001
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], axis=1).astype(np.uint32)
    s = rng.integers(0, SPP, n).astype(np.uint32)
    gpu, gs = c.dev.trace_samples(c.cam, c.st, W, H, xy, s)
    cpu, cs = ob.trace_samples(c.scene.desc(), c.cam, c.st, W, H, xy, s)
    exact = np.all((gpu == cpu) | (np.isnan(gpu) & np.isnan(cpu)), axis=1)
    print("bit-exact", float(exact.mean()), "rays", rays(gs), rays(cs))
    assert exact.mean() >= 0.999
    assert rays(gs) == rays(cs) or exact.mean() < 1.0
    assert np.abs(gpu[:, :3] - cpu[:, :3]).sum() / max(np.abs(cpu[:, :3]).sum(), 1e-30) <= 1e-3


@pytest.mark.parametrize("mode", ["tiles", "passes"])
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_shards_of_three(cases, name, mode):
    """Tile shards (16-pixel tiles: 15 of them, ragged at both edges) render with the exact splat and
    equal the oracle's shard; pass shards render with the streaming splat.  Either way the three
    shares sum to the oracle's frame with the oracle's counts."""
    c = cases(name)
    rt = c.rt
    tile = 16 if mode == "tiles" else 64
    cpu, cs = c.oracle(f"tile{tile}", tile=tile)
    shares = []
    for r in range(3):
        if mode == "tiles":
            with c.dev.configured(splat_mode=rt.abi.RT_SPLAT_EXACT):
                g, gs = c.dev.render(c.cam, c.st, c.fc, W, H, tile=tile, shard_index=r, shard_count=3)
            o, os_ = c.oracle(f"tile{tile}_shard{r}", tile=tile, shard_index=r, shard_count=3)
            same = float(np.all(g == o, axis=2).mean())
            print("shard", r, "pixels identical", same, "rel L2", rel_l2(g, o))
            assert same >= 0.999 and rel_l2(g, o) <= 1e-6
            assert rays(gs) == rays(os_) and gs.samples == os_.samples
        else:
            with c.dev.configured(shard_mode=rt.abi.RT_SHARD_PASSES):
                g, gs = c.dev.render(c.cam, c.st, c.fc, W, H, tile=tile, shard_index=r, shard_count=3)
            assert gs.samples == W*H*(SPP*(r + 1)//3 - SPP*r//3)
        shares.append((g, gs))
    total = sum(g.astype(np.float64) for g, _ in shares)
    print("sum rel L2", rel_l2(total, cpu))
    assert rel_l2(total, cpu) <= 1e-5
    assert sum(gs.samples for _, gs in shares) == cs.samples
    assert (sum(gs.closest_hit_rays for _, gs in shares), sum(gs.shadow_rays for _, gs in shares)) == rays(cs)


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_no_bounces(cases, name):
    """max_bounce_count 0: k_generate itself finishes every path (S_DONE, its records written at the
    mapped slot), k_shade moves them to the finished array."""
    c = cases(name)
    st = c.settings(max_bounce_count=0)
    gpu, gs = c.exact(st=st)
    check_frame(gpu, gs, *c.oracle("depth0", st=st))


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_normals(cases, name):
    """The Normals integrator: one camera ray per sample, counted from the claims."""
    c = cases(name)
    st = c.settings(integrator=NORMALS)
    gpu, gs = c.exact(st=st)
    cpu, cs = rb.render(c.scene.desc(), c.cam, st, c.fc, W, H)
    check_frame(gpu, gs, cpu, cs)
    assert gs.closest_hit_rays == gs.samples and gs.shadow_rays == 0


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_stream_splat_smallest_ring(cases, name):
    """A record ring of one pass: the claim limit throttles the claims, so most iterations claim fewer
    samples than there are free slots and the rest are marked free.  The frame is the default streaming
    frame bit for bit, and the oracle's up to float summation order."""
    c = cases(name)
    ref, rs = c.dev.render(c.cam, c.st, c.fc, W, H)
    with c.dev.configured(splat_chunk=1, splat_ring=1):
        gpu, gs = c.dev.render(c.cam, c.st, c.fc, W, H)
    assert rs.splat_mode == gs.splat_mode == c.rt.abi.RT_SPLAT_STREAM
    cpu, cs = c.oracle()
    print("rel L2", rel_l2(gpu, cpu), "iterations", int(rs.iterations), int(gs.iterations))
    assert np.array_equal(ref, gpu)
    assert rays(gs) == rays(rs) == rays(cs)
    assert rel_l2(gpu, cpu) <= 1e-5
    assert np.isfinite(gpu).all()


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_drain_cadence_with_immediate_fuse(cases, name):
    """drain_every 3 with the drain fused while every path is alive: k_generate launches follow the
    retired pool and mark it free."""
    c = cases(name)
    gpu, gs = c.exact(drain_every=3, fuse_paths=1000000000)
    check_frame(gpu, gs, *c.oracle())
    base, bs = c.exact()
    assert np.array_equal(gpu, base) and rays(gs) == rays(bs)
