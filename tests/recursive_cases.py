"""Scenes and cases shared by tests/test_ref_recursive.py (CPU) and tests/test_gpu_recursive.py (GPU): the
Whitted and Ground Truth Recursive integrators (rt_scene_set_recursive_integrators) against the CPU checker of
tests/ref_recursive.

The CPU file asserts that the checker alone gives finite samples on every case listed here, so the GPU file's
equality with the checker can never pass on garbage.

Shapes are the smallest at which k_recurse can still go wrong: a path pool of 1024 (lanes refill over many
iterations), frames 64x48, 65x33 (ragged tiles), 130x7 and 1x1, 1 / 5 / 16 spp, every sampler.
Depths 0, 1, 2 and 5 everywhere; 63 for Ground Truth Recursive; 63 for Whitted only between two mirrors (one
chain, the frame stack's last level); at most 8 for Whitted where a medium is visible (2^depth calls).
"""
import numpy as np

import analytic_scenes as an
from random_scenes import random_scene

WHITTED, GT_RECURSIVE = 1, 2
UNIFORM, BLUE_NOISE, STRATIFIED = 0, 1, 2
POOL = 1024
AMBIENT = (0.05, 0.1, 0.15)


def all_samples(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.uint32), ss.ravel().astype(np.uint32)


def with_settings(st, **fields):
    c = type(st).from_buffer_copy(st)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def lights_scene(rt, w, h):
    """Two sphere lights and an emissive box (a light the light loop draws for and gets nothing from) over a
    diffuse floor with a rough metal sphere and a box: the light loop, shadowed and not."""
    s = rt.Scene()
    floor = s.add_diffuse_material((0.7, 0.7, 0.6), 1.3, checkers=True, checker_color=(0.2, 0.3, 0.4))
    metal = s.add_material(0, (0.9, 0.8, 0.7), 0.0, 0.0, 1.5, 0.6, 0.2)
    red = s.add_diffuse_material((0.8, 0.2, 0.2), 1.5)
    la = s.add_emissive_material((40.0, 35.0, 30.0))
    lb = s.add_emissive_material((5.0, 10.0, 20.0))
    lc = s.add_emissive_material((3.0, 3.0, 3.0))
    s.add_plane(floor, (0.0, 1.0, 0.0), 0.0)
    s.add_sphere(metal, 1.5, rt.translate((-1.5, 1.5, 1.0)))
    s.add_box(red, (1.0, 1.0, 1.0), rt.translate((2.0, 1.0, 0.0)) * rt.rotate_y(0.4))
    s.add_sphere(la, 0.5, rt.translate((3.0, 6.0, -2.0)))
    s.add_sphere(lb, 0.8, rt.translate((-4.0, 5.0, 2.0)))
    s.add_box(lc, (0.5, 0.1, 0.5), rt.translate((0.0, 7.0, 1.0)))
    s.set_sky((0.3, 0.4, 0.6), (0.1, 0.1, 0.1))
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 3.0, -9.0), (0.0, 1.0, 0.0), 45.0)
    st = an.settings(rt, spp=1, bounces=4)
    st.vignette_strength = 0.5
    return s, cam, st, rt.load_reconstruction_kernel("Mitchell Netravali")


def mirrors_scene(rt, w, h):
    """Two facing mirrors (metallic 0.9, no roughness, so every level also adds its ambient term) with the
    camera between them: every camera ray bounces between them to the depth limit, one chain with no branch,
    so Whitted reaches depth 63 and the sample folds a term of every level."""
    s = rt.Scene()
    a = s.add_material(0, (0.99, 0.98, 0.97), 0.0, 0.0, 1.5, 0.9, 0.0)
    b = s.add_material(0, (0.97, 0.99, 0.98), 0.0, 0.0, 1.5, 0.9, 0.0)
    s.add_plane(a, (0.0, 0.0, -1.0), -5.0)          # z = 5, facing -z
    s.add_plane(b, (0.0, 0.0, 1.0), -5.0)           # z = -5, facing +z
    s.set_sky((0.5, 0.6, 0.7), (0.2, 0.2, 0.2))
    s.create_scene_bvh()
    cam = an.camera(rt, w, h, (0.0, 0.0, 0.0), (0.0, 0.0, 5.0), 20.0)
    st = an.settings(rt, spp=1, bounces=63)
    return s, cam, st, rt.load_reconstruction_kernel("Box")


SCENES = ["c1", "c3", "c4", "random21", "lights", "mirrors"]


def build(rt, name, w, h):
    """(scene, cam, st, fc): the scene with a non-zero ambient light (Whitted reads it)."""
    if name.startswith("random"):
        scene, cam, st, fc = random_scene(rt, int(name[6:]), w, h, spp=1)       # > 63 top-level slots
    elif name == "lights":
        scene, cam, st, fc = lights_scene(rt, w, h)
    elif name == "mirrors":
        scene, cam, st, fc = mirrors_scene(rt, w, h)
    else:
        scene, cam, st, fc, post = rt.load_preset(name, w, h)
    scene.set_ambient_light(AMBIENT)
    return scene, cam, st, fc


class SceneCache:
    """name, frame shape -> (scene, cam, st, fc).  A scene's geometry does not depend on the frame shape, only
    its camera does: every shape of a name shares the scene built first (one upload per name on the GPU)."""

    def __init__(self, rt):
        self.rt = rt
        self.first = {}
        self.made = {}

    def get(self, name, w, h):
        if (name, w, h) not in self.made:
            scene, cam, st, fc = build(self.rt, name, w, h)
            self.first.setdefault(name, scene)
            self.made[(name, w, h)] = (self.first[name], cam, st, fc)
        return self.made[(name, w, h)]


# (depth, sampler, (w, h), spp): every depth, sampler, frame and spp of the issue's lists appears
COMMON = [
    (0, UNIFORM, (1, 1), 1),
    (1, STRATIFIED, (130, 7), 5),
    (2, BLUE_NOISE, (65, 33), 16),
    (5, UNIFORM, (64, 48), 5),
]


def cases():
    """[(id, scene, integrator, depth, sampler, (w, h), spp)]"""
    out = []
    for name in SCENES:
        for integ in (WHITTED, GT_RECURSIVE):
            todo = list(COMMON)
            if integ == GT_RECURSIVE:
                todo.append((63, STRATIFIED, (65, 33), 1))
            elif name == "mirrors":
                todo.append((63, STRATIFIED, (65, 33), 1))
            else:
                todo.append((8, BLUE_NOISE, (130, 7), 1))
            if name == "mirrors":
                todo = [t for t in todo if t[0] in (0, 2, 63)]
            for depth, sampler, (w, h), spp in todo:
                tag = "whitted" if integ == WHITTED else "gtr"
                out.append((f"{name}-{tag}-d{depth}-s{sampler}-{w}x{h}x{spp}", name, integ, depth, sampler, (w, h), spp))
    return out


def case_settings(st, integ, depth, sampler, spp):
    return with_settings(st, integrator=integ, max_bounce_count=depth, sampling_strategy=sampler, samples_per_pixel=spp)


def same_samples(a, b):
    """Bit-identical, where two samples also count as equal when both are NaN or both the same infinity
    (x86 and gfx950 differ in NaN payload)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
