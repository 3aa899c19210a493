"""Every frame kind of the device library with the scene tables in HBM, not in LDS, and under every top-level form.

k_shade copies the small scene tables into LDS when they fit in 32 KB (scene_in_lds, rt_kernels.hip); when they do not,
or under RT_LDS_SCENE=0, a second set of template instantiations reads them from HBM.  Nearly every scene of the suite
fits, so those instantiations ran for one preset's Advanced frame only.  Here one scene is uploaded under five layouts
(tests/layout_matrix.py: none, RT_LDS_SCENE=0, RT_MLIST_MAX=0, RT_TOP_PROLOGUE=0, and the first two together) and every
frame kind is rendered once under each:

* every result under L1..L4 is bit-identical to the same kind under L0: frames as their 32-bit words, G-buffer and
  surface records, hit records, occlusion flags, per-sample rows, sample and ray counts.  No tolerance anywhere;
* rt_stats::traversal is identical between L0 and L1 and between L2 and L4 (residency does not change the walk); across
  the top-level forms it differs by design and is not compared;
* with traversal_ref on, rt_stats::traversal_ref is identical under all five;
* once per kind, the L1 result is held to the CPU side with the suite's existing bars (the oracle, tests/ref_integrators,
  tests/ref_recursive, tests/ref_features, tests/ref_temporal, tests/ref_deform), so the five cannot agree on a shared
  wrong answer.

A 64 x 48 x 4 frame in the default configuration claims every sample in its first iteration and fuses its drain at once
(the auto threshold is 2.5 x the drain kernel's lanes, far above 12,288 paths), so its ramp-capable k_shade never meets
a ramp iteration.  The Advanced kinds therefore render twice: in the default configuration and with
tests/test_gpu_ramp_shade.py's late fuse (a pool of 1,024 paths, the drain fused below 16), where rt_scene_ramp_stats
must report ramp iterations.  Both frames are in the result and both must be bit-identical across the layouts.

Then a scene whose tables overflow 32 KB by themselves (400 mesh instances), and the edge: the two scenes of N and N + 1
spheres whose blobs are the last that fits and the first that does not, each held to the oracle.

Sizes (tests/layout_matrix.blob_bytes, asserted below against the upload's own figure):
    the matrix scene                          5,504 B     in LDS
    the overflow scene (400 mesh instances)  56,704 B     not in LDS (435 transforms)
    the edge, N = 249 spheres                32,656 B     in LDS: k_shade's largest dynamic-LDS launch
    the edge, N + 1 = 250 spheres            32,784 B     not in LDS
"""
import ctypes as C
import re

import numpy as np
import pytest

import layout_matrix as lm
import oracle_binding as ob
import recursive_cases as rc
from parity_report import REPORT

W, H, SPP, TFI = lm.W, lm.H, lm.SPP, lm.TFI
MATRIX_BYTES, OVERFLOW_BYTES, EDGE = 5504, 56704, (249, 32656, 32784)

# stage 0: the scene as uploaded; 1: after the instance update; 2: after the mesh update
KINDS = (["advanced", "advanced_plain", "advanced_env", "trace_samples", "traversal_ref"] + list(lm.INTEGRATORS) +
         [f"feature_{f}" for f in lm.FEATURES] + ["features"] +
         [f"{i}_{s}" for s in lm.RECURSIVE_SCENES for i in lm.RECURSIVE] +
         ["tiles", "gbuffer", "gbuffer_surface", "intersect", "moved", "deformed"])
STAGE = {"moved": 1, "deformed": 2}
CPU_KINDS = [k for k in KINDS if k not in ("advanced_plain", "trace_samples", "traversal_ref")]


# ---------------------------------------------------------------- the CPU side, shared by both halves

class CpuSide:
    """The oracle's and the checkers' answer for every kind, computed once."""

    def __init__(self, rt):
        self.rt, self.made = rt, {}

    def once(self, key, make):
        if key not in self.made:
            self.made[key] = make()
        return self.made[key]

    def scene(self, stage=0):
        return self.once(("scene", stage), lambda: lm.matrix_scene(self.rt, stage))

    def recursive(self, name):
        return self.once(("recursive", name), lambda: lm.recursive_scene(self.rt, name))

    def overflow(self):
        return self.once("overflow", lambda: lm.overflow_scene(self.rt))

    def answer(self, kind):
        return self.once(("answer", kind), lambda: self._answer(kind))

    def _answer(self, kind):
        main = self.scene(STAGE.get(kind, 0))
        scene, cam, st, fc = main
        if kind in ("advanced", "advanced_env"):
            return lm.cpu_advanced(*main, env=kind == "advanced_env")
        if kind in lm.INTEGRATORS:
            return lm.cpu_integrator(*main, lm.INTEGRATORS[kind])
        if kind == "features" or kind.startswith("feature_"):
            return self.once("cpu_features", lambda: lm.cpu_features(*main))
        if kind in ("gbuffer", "gbuffer_surface"):
            return self.once("cpu_gbuffer", lambda: lm.cpu_gbuffer(scene, cam, st))
        if kind == "intersect":
            rays = lm.query_rays()
            return [ob.intersect(scene.desc(), rays, occ) for occ in (False, True)]
        if kind == "tiles":
            return self._tiles(*main)
        if kind in ("moved", "deformed"):
            return {"advanced": lm.cpu_advanced(*main), "gbuffer": lm.cpu_gbuffer(scene, cam, st)}
        integ, name = next((i, s) for s in lm.RECURSIVE_SCENES for i in lm.RECURSIVE if kind == f"{i}_{s}")
        return lm.cpu_recursive(*self.recursive(name), lm.RECURSIVE[integ])

    def _tiles(self, scene, cam, st, fc):
        a = self.rt.abi
        frame = np.zeros((H, W, 4), np.float32)
        buf = a.AccumulationBuffer(W, H, 0, frame.ctypes.data_as(C.POINTER(C.c_float)))
        ids = (C.c_uint32*2)(3, 0)         # the reference takes its tiles from the last down (oracle_render's own list)
        stats = a.Stats()
        assert ob.load().oracle_render_tiles(C.byref(scene.desc()), C.byref(cam), C.byref(st), C.byref(fc), 32, 32, TFI, 0,
                                             1, 2, ids, C.byref(buf), C.byref(stats)) == 0
        return {"frame": frame, "frame_counts": lm.cpu_counts(stats)}


@pytest.fixture(scope="module")
def cpu(rt):
    return CpuSide(rt)


# ---------------------------------------------------------------- the CPU half: runs without a device

def test_blob_sizes_and_scene_builders(rt, cpu):
    """The blob's size restated from the desc, for the three scenes: the matrix scene fits with room to spare and is
    listed_only under L0 (three mesh slots), the overflow scene cannot shrink back into LDS unnoticed, and the edge is
    where the restated rule puts it."""
    d = cpu.scene()[0].desc()
    assert lm.blob_bytes(rt, d) == MATRIX_BYTES < lm.LDS_BYTES
    assert len(lm.mesh_instances(rt, d)) == 3 and d.mesh_count == 3 and d.skydome_w == 64 and d.plane_count == 2
    assert [int(d.meshes[m].has_normals) for m in range(3)] == [1, 0, 1] and d.light_count == 2
    d = cpu.overflow()[0].desc()
    assert lm.blob_bytes(rt, d) == OVERFLOW_BYTES > lm.LDS_BYTES and len(lm.mesh_instances(rt, d)) == 400 > 63
    assert lm.edge_count(rt) == EDGE and EDGE[1] <= lm.LDS_BYTES < EDGE[2]
    for n in EDGE[0], EDGE[0] + 1:
        d = lm.edge_scene(rt, n)[0].desc()
        # (primitive 0 is the scene model's null primitive on the identity transform; then the light and the spheres)
        assert (d.plane_count, d.light_count, d.primitive_count, d.transform_count, d.mesh_count) == (1, 1, n + 2, n + 2, 0)
    # the updates change what they say they change, on the host model
    before, after = cpu.scene(0)[0].desc(), cpu.scene(1)[0].desc()
    moved = lm.moved_primitives(rt, before)
    types = {int(before.primitives[i].type) for i in moved}
    assert types == {rt.abi.RT_PRIMITIVE_MESH, rt.abi.RT_PRIMITIVE_BOX, rt.abi.RT_PRIMITIVE_SPHERE}
    for i in range(before.primitive_count):
        a = bytes(before.transforms[before.primitives[i].transform_index])
        b = bytes(after.transforms[after.primitives[i].transform_index])
        assert (a != b) == (i in moved), i
    import ref_refit_binding as rfit
    assert not np.array_equal(rfit.mesh_arrays(after, 0)[0], rfit.mesh_arrays(cpu.scene(2)[0].desc(), 0)[0])


@pytest.mark.parametrize("kind", CPU_KINDS)
def test_cpu_side_of_the_matrix(rt, cpu, kind):
    """The oracle and the checkers render every kind of the matrix scene: finite where the device will be held to
    them bit for bit, and not black."""
    got = cpu.answer(kind)
    if kind == "intersect":
        closest, occluded = got
        hits = sum(r.primitive != 0xFFFFFFFF for r in closest)
        assert 100 < hits < len(closest) and 0 < sum(r.primitive != 0xFFFFFFFF for r in occluded)
    elif kind in ("gbuffer", "gbuffer_surface"):
        d = cpu.scene()[0].desc()
        ids = got["primitive"]
        # (five pixels: the generated meshes are small and far.  The updates bring one to the camera, below)
        assert sum(int((ids == p).sum()) for p in lm.mesh_instances(rt, d)) > 0 and (ids & 0x80000000).any()
    elif kind == "features" or kind.startswith("feature_"):
        frames, counts, spec = got
        assert all(np.isfinite(f).all() for f in frames) and counts["samples"] == W*H*SPP and spec > 0
    else:
        part = got["advanced"] if kind in ("moved", "deformed") else got
        assert np.abs(part["frame"][..., :3]).max() > 0.01
        assert part["frame_counts"]["samples"] == ((32*32 + 32*16)*SPP if kind == "tiles" else W*H*SPP)
    if kind == "advanced_env":
        assert lm.differences({"f": got["frame"]}, {"f": cpu.answer("advanced")["frame"]})
    if kind in ("moved", "deformed"):
        before = cpu.answer("advanced") if kind == "moved" else cpu.answer("moved")["advanced"]
        assert lm.differences({"f": got["advanced"]["frame"]}, {"f": before["frame"]})
        mesh = lm.moved_primitives(rt, cpu.scene()[0].desc())[0]
        assert int((got["gbuffer"]["primitive"] == mesh).sum()) >= 100


def test_cpu_side_of_the_overflow_scene_and_the_edge(rt, cpu):
    scene, cam, st, fc = cpu.overflow()
    adv = cpu.once("overflow_advanced", lambda: lm.cpu_advanced(scene, cam, st, fc, 80, 60, tfi=0))
    assert adv["frame_counts"]["samples"] == 80*60*8 and np.abs(adv["frame"][..., :3]).max() > 0.01
    for n in EDGE[0], EDGE[0] + 1:
        e = cpu.once(("edge", n), lambda: lm.cpu_advanced(*lm.edge_scene(rt, n)))
        assert np.isfinite(e["frame"]).all() and e["frame_counts"]["shadow_rays"] > 0


# ---------------------------------------------------------------- the GPU half

TIMING = re.compile(r"\[rt timing\] rt_scene_upload: scene tables (\d+) B \((in|not in) LDS")


def upload(rt, scene, layout, monkeypatch, capfd):
    """rt.DeviceScene under the layout's environment and RT_DEBUG_TIMING, in the exact splat mode
    -> (dev, the blob's size as the upload printed it, whether it said `in LDS`)."""
    for k in lm.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in lm.LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RT_DEBUG_TIMING", "1")
    capfd.readouterr()
    try:
        dev = rt.DeviceScene(scene, 0)
    finally:
        for k in lm.SWITCHES + ("RT_DEBUG_TIMING",):
            monkeypatch.delenv(k, raising=False)
    err = capfd.readouterr().err
    found = TIMING.findall(err)
    assert len(found) == 1, err
    dev.configure(splat_mode=rt.abi.RT_SPLAT_EXACT)
    return dev, int(found[0][0]), found[0][1] == "in"


class Layout:
    """The matrix scene (and, on first use, the recursive scenes) on the device under one layout, with every kind's
    result computed once.  The two updates change the scene for good: a kind of a later stage first renders every
    kind of the stages before it, so the results do not depend on the order the tests run in."""

    def __init__(self, rt, name, monkeypatch, capfd):
        self.rt, self.name, self.results, self.stage, self.recursive, self.info = rt, name, {}, 0, {}, {}
        self.main = lm.matrix_scene(rt)
        want = lm.blob_bytes(rt, self.main[0].desc())
        assert want == MATRIX_BYTES < lm.LDS_BYTES
        self.dev, size, in_lds = upload(rt, self.main[0], name, monkeypatch, capfd)
        assert size == want and in_lds == ("RT_LDS_SCENE" not in lm.LAYOUTS[name]), (name, size, in_lds)

    def close(self):
        self.dev.close()
        for dev, _ in self.recursive.values():
            dev.close()

    def recursive_dev(self, scene_name, monkeypatch, capfd):
        if scene_name not in self.recursive:
            parts = lm.recursive_scene(self.rt, scene_name)
            dev, _, in_lds = upload(self.rt, parts[0], self.name, monkeypatch, capfd)
            assert in_lds == ("RT_LDS_SCENE" not in lm.LAYOUTS[self.name])
            dev.set_recursive_integrators(True)
            dev.configure(path_pool=rc.POOL)
            self.recursive[scene_name] = (dev, parts)
        return self.recursive[scene_name]

    def result(self, kind, monkeypatch, capfd):
        if kind not in self.results:
            need = STAGE.get(kind, 0)
            while self.stage < need:
                for k in KINDS:
                    if STAGE.get(k, 0) == self.stage:
                        self.result(k, monkeypatch, capfd)
                lm.UPDATES[self.stage](self.rt, self.main[0], self.dev)
                self.stage += 1
            assert self.stage == need, (kind, self.stage)
            self.results[kind] = self.compute(kind, monkeypatch, capfd)
        return self.results[kind]

    # -- the kinds

    def frame(self, st=None, prefix="", **cfg):
        scene, cam, st0, fc = self.main
        with self.dev.configured(**cfg):
            frame, s = self.dev.render(cam, st0 if st is None else st, fc, W, H, total_frame_index=TFI)
            ramp = self.dev.ramp_stats()
        assert s.splat_mode == self.rt.abi.RT_SPLAT_EXACT
        return {prefix + "frame": frame, prefix + "counts": lm.counts(s), "traversal_" + prefix: lm.walk(s)}, ramp, s

    def ramped(self, **cfg):
        """A late-fuse frame: rt_scene_ramp_stats must report ramp iterations, so that no layout passes by never
        entering the ramp (the same figures whichever kernel shades it, tests/test_gpu_ramp_shade.py)."""
        out, ramp, _ = self.frame(prefix="late_fuse_" + ("plain_" if cfg.get("ramp_shade") == 2 else ""), **lm.LATE_FUSE, **cfg)
        assert ramp[0] >= 1 and ramp[1] >= ramp[0], (self.name, cfg, ramp)
        self.info.setdefault("ramp", {})[str(sorted(cfg.items()))] = ramp
        return out

    def compute(self, kind, monkeypatch, capfd):
        rt, dev = self.rt, self.dev
        scene, cam, st, fc = self.main
        xy, so = lm.sample_list()
        if kind == "advanced":                       # the default configuration, and the RAMP instantiation's ramp
            out, ramp, _ = self.frame()
            self.info["default_ramp"] = ramp
            out.update(self.ramped())
            assert not lm.differences({"f": out["frame"]}, {"f": out["late_fuse_frame"]})     # the schedule is not in the frame
            return out
        if kind == "advanced_plain":                 # the plain instantiation to the end of the frame
            return self.ramped(ramp_shade=2)
        if kind == "advanced_env":                   # the ENV instantiations, with the ramp and without
            out, _, _ = self.frame(env_sampling=1)
            out.update(self.ramped(env_sampling=1))
            out.update(self.ramped(env_sampling=1, ramp_shade=2))
            with dev.configured(env_sampling=1):
                samples, ss = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=TFI)
            out.update(samples=samples, sample_counts=lm.counts(ss), traversal_samples=lm.walk(ss))
            return out
        if kind == "trace_samples":
            samples, ss = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=TFI)
            return {"samples": samples, "sample_counts": lm.counts(ss), "traversal_samples": lm.walk(ss)}
        if kind == "traversal_ref":
            out, _, s = self.frame(traversal_ref=1)
            out["reference_walk"] = lm.walk(s, "traversal_ref")
            assert s.traversal_ref[0].mesh_bvh_traversals > 0
            return out
        if kind in lm.INTEGRATORS:
            sti = lm.with_settings(st, integrator=lm.INTEGRATORS[kind])
            out, _, s = self.frame(st=sti)
            samples, ss = dev.trace_samples(cam, sti, W, H, xy, so, total_frame_index=TFI)
            assert s.shadow_rays == 0 and ss.shadow_rays == 0
            out.update(samples=samples, sample_counts=lm.counts(ss), traversal_samples=lm.walk(ss))
            return out
        if kind.startswith("feature_"):
            frame, s = dev.render_feature(cam, st, fc, W, H, lm.FEATURES.index(kind[8:]), total_frame_index=TFI)
            return {"frame": frame, "counts": lm.counts(s), "traversal_": lm.walk(s)}
        if kind == "features":
            n, d, a, s = dev.render_features(cam, st, fc, W, H, total_frame_index=TFI)
            return {"normal": n, "distance": d, "albedo": a, "counts": lm.counts(s), "traversal_": lm.walk(s)}
        if kind == "tiles":
            frame, s = dev.render_tiles(cam, st, fc, W, H, [0, 3], total_frame_index=TFI, tile=32)
            return {"frame": frame, "counts": lm.counts(s), "traversal_": lm.walk(s)}
        if kind == "gbuffer":
            return {"gbuffer": dev.gbuffer(cam, W, H, st.lens_distortion)}
        if kind == "gbuffer_surface":
            g, s = dev.gbuffer_surface(cam, W, H, st.lens_distortion)
            return {"gbuffer": g, "surface": s}
        if kind == "intersect":
            rays = lm.query_rays()
            self.info["hits"] = [dev.intersect(rays, occ) for occ in (False, True)]
            return {**lm.hit_arrays(self.info["hits"][0], False), **lm.hit_arrays(self.info["hits"][1], True)}
        if kind == "moved":                          # after rt_scene_update_instances
            out, _, _ = self.frame()
            samples, ss = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=TFI)
            out.update(samples=samples, sample_counts=lm.counts(ss), gbuffer=dev.gbuffer(cam, W, H, st.lens_distortion))
            return out
        if kind == "deformed":                       # after rt_scene_update_mesh and rt_scene_update_instances
            out, _, _ = self.frame()
            samples, ss = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=TFI)
            g, s = dev.gbuffer_surface(cam, W, H, st.lens_distortion)
            out.update(samples=samples, sample_counts=lm.counts(ss), gbuffer=g, surface=s)
            return out
        integ, name = next((i, s) for s in lm.RECURSIVE_SCENES for i in lm.RECURSIVE if kind == f"{i}_{s}")
        rdev, (rscene, rcam, rst0, rfc) = self.recursive_dev(name, monkeypatch, capfd)
        rst = lm.recursive_settings(rst0, lm.RECURSIVE[integ])
        axy, aso = rc.all_samples(W, H, SPP)
        samples, ss = rdev.trace_samples(rcam, rst, W, H, axy, aso, total_frame_index=TFI)
        frame, s = rdev.render(rcam, rst, rfc, W, H, total_frame_index=TFI)
        assert s.splat_mode == rt.abi.RT_SPLAT_EXACT
        return {"samples": samples, "sample_counts": lm.counts(ss), "frame": frame, "counts": lm.counts(s),
                "traversal_": lm.walk(s), "traversal_samples": lm.walk(ss)}


@pytest.fixture(scope="module")
def layouts(rt):
    """Layout name -> its Layout, uploaded on first use: one upload of the matrix scene per layout per module."""
    made = {}

    def get(name, monkeypatch, capfd):
        if name not in made:
            made[name] = Layout(rt, name, monkeypatch, capfd)
        return made[name]
    yield get
    for v in made.values():
        v.close()


def is_walk(key):
    return key.startswith("traversal_")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", list(lm.LAYOUTS))
def test_matrix(rt, layouts, monkeypatch, capfd, layout, kind):
    """One kind under one layout.  L0: the kind renders something.  L1..L4: every word and every count is L0's."""
    base = layouts("L0", monkeypatch, capfd).result(kind, monkeypatch, capfd)
    entry = REPORT.setdefault(f"layout_matrix_{layout}", {})
    if layout == "L0":
        for k, v in base.items():
            if isinstance(v, np.ndarray) and v.dtype == np.float32 and k != "record":
                assert np.abs(np.nan_to_num(v[..., :3])).max() > 0.01, k
            if k.endswith("counts"):
                assert v["samples"] > 0 and v["closest_hit_rays"] > 0, k
        if kind in ("advanced", "advanced_plain", "advanced_env", "trace_samples", "moved", "deformed"):
            assert all(v["shadow_rays"] > 0 for k, v in base.items() if k.endswith("counts"))
        if kind == "advanced_env":                   # the option is really on
            plain = layouts("L0", monkeypatch, capfd).result("advanced", monkeypatch, capfd)
            assert lm.differences({"f": base["frame"]}, {"f": plain["frame"]})
        if kind == "tiles":                          # tile 1 stays empty beyond the filter's reach from tiles 0 and 3
            assert not base["frame"][:16, 48:].any() and base["frame"][:32, :32, 3].any() and base["frame"][32:, 32:, 3].any()
            assert base["counts"]["samples"] == (32*32 + 32*16)*SPP
        entry[kind] = 0
        return
    lay = layouts(layout, monkeypatch, capfd)
    got = lay.result(kind, monkeypatch, capfd)
    bad = lm.differences(got, base, skip=[k for k in got if is_walk(k)])
    twin = lm.SAME_WALK.get(layout)
    if twin:                                         # residency does not change the walk
        other = layouts(twin, monkeypatch, capfd).result(kind, monkeypatch, capfd)
        bad.update({f"{k} (against {twin})": 1 for k in got if is_walk(k) and got[k] != other[k]})
    else:                                            # another top-level form: not compared, only shown
        walks = {k: got[k] != base[k] for k in got if is_walk(k)}
        if walks:
            print(layout, kind, "rt_stats::traversal differs from L0's:", walks)
        if kind in ("advanced", "whitted_c4", "gt_recursive_c4"):      # the switch was read: this is another walk
            assert all(walks.values()), (layout, kind, walks)
    entry[kind] = int(sum(bad.values()))
    print(layout, kind, "mismatches", bad, {k: v for k, v in lay.info.items() if k != "hits"})
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CPU_KINDS)
def test_matrix_against_the_cpu_side(rt, layouts, cpu, monkeypatch, capfd, kind):
    """The L1 result of every kind against the oracle or its checker, with the bars of the test that owns the kind."""
    lay = layouts("L1", monkeypatch, capfd)
    got = lay.result(kind, monkeypatch, capfd)
    want = cpu.answer(kind)
    key = f"layout_matrix_cpu_{kind}"
    if kind in ("advanced", "advanced_env"):                 # tests/test_gpu_scenes._compare
        samples = got if kind == "advanced_env" else lay.result("trace_samples", monkeypatch, capfd)
        fig = lm.advanced_figures(samples["samples"], samples["sample_counts"], got["frame"], got["counts"], want)
        REPORT[key] = fig
        print(key, fig)
        lm.advanced_bars(fig)
    elif kind in ("moved", "deformed"):
        fig = lm.advanced_figures(got["samples"], got["sample_counts"], got["frame"], got["counts"], want["advanced"])
        fig["gbuffer_mismatches"] = lm.gbuffer_mismatches(got["gbuffer"], want["gbuffer"])
        if kind == "deformed":
            fig["surface_mismatches"], fig["mesh_pixels"] = lm.surface_mismatches(rt, cpu.scene(2)[0], got["gbuffer"], got["surface"])
            assert fig["surface_mismatches"] == 0 and fig["mesh_pixels"] >= 100, fig
        REPORT[key] = fig
        print(key, fig)
        lm.advanced_bars(fig)
        assert fig["gbuffer_mismatches"] == 0, fig
    elif kind in lm.INTEGRATORS:                             # tests/test_gpu_integrators.test_parity
        exact = float(np.all(lm.same_or_nan(got["samples"], want["samples"]), axis=1).mean())
        same = float(np.all(got["frame"] == want["frame"], axis=2).mean())
        err = lm.rel_l2(got["frame"], want["frame"])
        REPORT[key] = {"samples_bit_exact": exact, "pixels_identical": same, "frame_rel_l2": err}
        print(key, REPORT[key])
        assert exact >= 0.999 and same >= 0.999 and err <= 1e-6
        assert got["sample_counts"]["closest_hit_rays"] == want["sample_counts"]["closest_hit_rays"]
        assert got["counts"]["closest_hit_rays"] == want["frame_counts"]["closest_hit_rays"]
        assert got["counts"]["samples"] == want["frame_counts"]["samples"] == W*H*SPP
        assert got["counts"]["shadow_rays"] == 0 and got["traversal_"][2][1] == 0
    elif kind == "features" or kind.startswith("feature_"):  # tests/test_gpu_features.test_exact_frames_match_the_checker
        frames, counts, spec = want
        pairs = ([(got[f], frames[i]) for i, f in enumerate(lm.FEATURES)] if kind == "features" else
                 [(got["frame"], frames[lm.FEATURES.index(kind[8:])])])
        n = [int(np.count_nonzero(np.any(lm.words(a) != lm.words(b), axis=2))) for a, b in pairs]
        REPORT[key] = {"mismatching_pixels": n, "specular_bounces": spec}
        print(key, REPORT[key])
        assert not any(n)
        assert (got["counts"]["closest_hit_rays"], got["counts"]["samples"]) == (counts["closest_hit_rays"], counts["samples"])
        assert got["counts"]["shadow_rays"] == 0 and got["counts"]["closest_hit_rays"] - got["counts"]["samples"] == spec
    elif kind == "gbuffer":                                  # tests/test_gpu_temporal.test_gbuffer_matches_the_checker
        REPORT[key] = {"mismatches": lm.gbuffer_mismatches(got["gbuffer"], want)}
        assert REPORT[key]["mismatches"] == 0
    elif kind == "gbuffer_surface":                          # tests/test_gpu_deform.check_surface
        bad, on_mesh = lm.surface_mismatches(rt, cpu.scene()[0], got["gbuffer"], got["surface"])
        REPORT[key] = {"gbuffer_mismatches": lm.gbuffer_mismatches(got["gbuffer"], want), "surface_mismatches": bad,
                       "mesh_pixels": on_mesh}
        print(key, REPORT[key])
        assert REPORT[key]["gbuffer_mismatches"] == 0 and bad == 0 and on_mesh > 0
    elif kind == "intersect":                                # tests/test_gpu_parity.test_intersect_bit_exact
        bad = [lm.intersect_mismatches(lay.info["hits"][k], want[k], bool(k)) for k in range(2)]
        REPORT[key] = {"rays": len(want[0]), "mismatches": bad}
        assert bad == [0, 0]
    elif kind == "tiles":
        pixels = float(np.all(got["frame"] == want["frame"], axis=2).mean())
        REPORT[key] = {"pixels_identical": pixels, "frame_rel_l2": lm.rel_l2(got["frame"], want["frame"])}
        print(key, REPORT[key])
        assert pixels >= 0.999 and REPORT[key]["frame_rel_l2"] <= 1e-6
        assert all(got["counts"][k] == want["frame_counts"][k] for k in ("samples", "closest_hit_rays", "shadow_rays"))
    else:                                                    # tests/test_gpu_recursive.test_parity
        same, fsame = rc.same_samples(got["samples"], want["samples"]), rc.same_samples(got["frame"], want["frame"])
        REPORT[key] = {"samples_differing": int((~same.all(axis=1)).sum()), "pixels_differing": int((~fsame.all(axis=2)).sum())}
        print(key, REPORT[key])
        assert same.all() and fsame.all()
        for mine, theirs in (("sample_counts", "sample_counts"), ("counts", "frame_counts")):
            assert all(got[mine][k] == want[theirs][k] for k in ("samples", "closest_hit_rays", "shadow_rays")), mine
        assert got["counts"]["samples"] == W*H*SPP


# ---------------------------------------------------------------- 2. a scene that overflows on its own

OW, OH = 80, 60


@pytest.fixture(scope="module")
def overflow(rt, cpu):
    """The overflow scene on the device with no switch set, uploaded on first use -> (dev, (scene, cam, st, fc))."""
    made = []

    def get(monkeypatch, capfd):
        if not made:
            parts = cpu.overflow()
            d = parts[0].desc()
            assert lm.blob_bytes(rt, d) == OVERFLOW_BYTES > lm.LDS_BYTES and len(lm.mesh_instances(rt, d)) > 63
            dev, size, in_lds = upload(rt, parts[0], "L0", monkeypatch, capfd)
            assert size == OVERFLOW_BYTES and not in_lds
            made.append((dev, parts))
        return made[0]
    yield get
    for dev, _ in made:
        dev.close()


@pytest.mark.gpu
def test_overflow_advanced(rt, cpu):
    """tests/test_gpu_scenes._compare on the scene whose tables pass 32 KB by themselves."""
    from test_gpu_scenes import _compare
    scene, cam, st, fc = cpu.overflow()
    d = scene.desc()
    assert lm.blob_bytes(rt, d) == OVERFLOW_BYTES > lm.LDS_BYTES and len(lm.mesh_instances(rt, d)) > 63
    _compare(rt, "layout_overflow", scene, cam, st, fc, OW, OH)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gt_iterative", "normals"])
def test_overflow_integrators(rt, cpu, overflow, monkeypatch, capfd, name):
    dev, (scene, cam, st0, fc) = overflow(monkeypatch, capfd)
    st = lm.with_settings(st0, integrator=lm.INTEGRATORS[name])
    xy, so = lm.sample_list(OW, OH, st.samples_per_pixel)
    samples, ss = dev.trace_samples(cam, st, OW, OH, xy, so)
    frame, fs = dev.render(cam, st, fc, OW, OH)
    want = lm.cpu_integrator(scene, cam, st0, fc, lm.INTEGRATORS[name], OW, OH, tfi=0)
    exact = float(np.all(lm.same_or_nan(samples, want["samples"]), axis=1).mean())
    same = float(np.all(frame == want["frame"], axis=2).mean())
    err = lm.rel_l2(frame, want["frame"])
    REPORT[f"layout_overflow_{name}"] = {"samples_bit_exact": exact, "pixels_identical": same, "frame_rel_l2": err}
    print(name, REPORT[f"layout_overflow_{name}"])
    assert fs.splat_mode == rt.abi.RT_SPLAT_EXACT
    assert exact >= 0.999 and same >= 0.999 and err <= 1e-6
    assert ss.closest_hit_rays == want["sample_counts"]["closest_hit_rays"] and ss.shadow_rays == 0
    assert (fs.closest_hit_rays, fs.samples, fs.shadow_rays) == (want["frame_counts"]["closest_hit_rays"], OW*OH*8, 0)


@pytest.mark.gpu
def test_overflow_features_in_one_walk(rt, cpu, overflow, monkeypatch, capfd):
    dev, (scene, cam, st, fc) = overflow(monkeypatch, capfd)
    n, d, a, s = dev.render_features(cam, st, fc, OW, OH, total_frame_index=TFI)
    frames, counts, spec = lm.cpu_features(scene, cam, st, fc, OW, OH)
    bad = [int(np.count_nonzero(np.any(lm.words(x) != lm.words(y), axis=2))) for x, y in zip((n, d, a), frames)]
    REPORT["layout_overflow_features"] = {"mismatching_pixels": bad, "specular_bounces": spec}
    print(REPORT["layout_overflow_features"])
    assert s.splat_mode == rt.abi.RT_SPLAT_EXACT and not any(bad)
    assert (s.closest_hit_rays, s.samples, s.shadow_rays) == (counts["closest_hit_rays"], counts["samples"], 0)
    assert s.closest_hit_rays - s.samples == spec


@pytest.mark.gpu
def test_overflow_gbuffer_surface(rt, cpu, overflow, monkeypatch, capfd):
    dev, (scene, cam, st, fc) = overflow(monkeypatch, capfd)
    g, s = dev.gbuffer_surface(cam, OW, OH, st.lens_distortion)
    want = lm.cpu_gbuffer(scene, cam, st, OW, OH)
    bad, on_mesh = lm.surface_mismatches(rt, scene, g, s)
    REPORT["layout_overflow_gbuffer_surface"] = {"gbuffer_mismatches": lm.gbuffer_mismatches(g, want),
                                                 "surface_mismatches": bad, "mesh_pixels": on_mesh}
    print(REPORT["layout_overflow_gbuffer_surface"])
    assert REPORT["layout_overflow_gbuffer_surface"]["gbuffer_mismatches"] == 0 and bad == 0 and on_mesh >= 100


@pytest.mark.gpu
def test_overflow_switch_is_a_noop(rt, cpu, overflow, monkeypatch, capfd):
    """RT_LDS_SCENE=0 on a scene that is in HBM already: the Advanced frame and its counts are bit-identical."""
    dev, (scene, cam, st, fc) = overflow(monkeypatch, capfd)
    frame, s = dev.render(cam, st, fc, OW, OH, total_frame_index=TFI)
    off, size, in_lds = upload(rt, scene, "L1", monkeypatch, capfd)
    try:
        assert size == OVERFLOW_BYTES and not in_lds
        again, t = off.render(cam, st, fc, OW, OH, total_frame_index=TFI)
    finally:
        off.close()
    bad = lm.differences({"frame": again, "counts": lm.counts(t), "walk": lm.walk(t)},
                         {"frame": frame, "counts": lm.counts(s), "walk": lm.walk(s)})
    REPORT["layout_overflow_switch"] = {"mismatches": int(sum(bad.values()))}
    assert not bad and s.shadow_rays > 0


# ---------------------------------------------------------------- 3. the 32 KB edge

@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fits", "overflows"])
def test_the_32k_edge(rt, cpu, monkeypatch, capfd, which):
    """N spheres: the largest blob that is still at most 32,768 bytes, the largest dynamic-LDS launch k_shade ever
    makes.  N + 1: the first that is not.  The upload says which, and both frames are the oracle's."""
    n, fits, over = lm.edge_count(rt)
    assert (n, fits, over) == EDGE and fits <= lm.LDS_BYTES < over
    n, want_size = (n, fits) if which == "fits" else (n + 1, over)
    scene, cam, st, fc = lm.edge_scene(rt, n)
    assert lm.blob_bytes(rt, scene.desc()) == want_size
    dev, size, in_lds = upload(rt, scene, "L0", monkeypatch, capfd)
    try:
        assert size == want_size
        assert in_lds == (which == "fits")
        xy, so = lm.sample_list()
        samples, ss = dev.trace_samples(cam, st, W, H, xy, so, total_frame_index=TFI)
        frame, fs = dev.render(cam, st, fc, W, H, total_frame_index=TFI)
        dev.configure(splat_mode=rt.abi.RT_SPLAT_STREAM)
        stream, _ = dev.render(cam, st, fc, W, H, total_frame_index=TFI)
    finally:
        dev.close()
    want = cpu.once(("edge", n), lambda: lm.cpu_advanced(scene, cam, st, fc))
    fig = lm.advanced_figures(samples, lm.counts(ss), frame, lm.counts(fs), want)
    fig["stream_rel_l2"] = lm.rel_l2(stream, want["frame"])
    REPORT[f"layout_edge_{which}"] = dict(fig, spheres=n, blob_bytes=size, in_lds=in_lds)
    print(which, REPORT[f"layout_edge_{which}"])
    assert fs.splat_mode == rt.abi.RT_SPLAT_EXACT
    lm.advanced_bars(fig)
    assert fig["stream_rel_l2"] <= 1e-5
