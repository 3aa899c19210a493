#!/usr/bin/env python3
"""The sweep behind rt_denoise_variance_default_params and RT_TEMPORAL_SPATIAL_BELOW_DEFAULT (DESIGN.md,
"Variance-guided filtering"; the record is profiles/svgf_defaults.txt).  CPU only: the oracle renders DESIGN.md's
16-frame camera path (1 spp a frame) on C3 and C4 and a standing camera on C3, tests/ref_svgf runs the stages, and the
last frame is held to a 256-spp oracle frame at the last camera by its tonemapped (1 - e^-c) RMSE.

    python tools/svgf_defaults_sweep.py [width height]        (default 480 270; needs __graft_entry__.build())
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

rt = entry._import_package()
rt.lib()
import ref_binding as rb  # noqa: E402
import ref_denoise_binding as rd  # noqa: E402
import ref_svgf_binding as sb  # noqa: E402

START = dict(iterations=5, sigma_color=4.0, sigma_normal=0.2, sigma_plane=0.02, variance_epsilon=1e-3)
SWEEP = dict(iterations=[2, 3, 4, 5, 6], sigma_color=[0.0, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0], sigma_normal=[0.0, 0.1, 0.2, 0.4],
             sigma_plane=[0.0, 0.005, 0.01, 0.02, 0.05], variance_epsilon=[1e-4, 1e-3, 1e-2, 1e-1])
BELOW = [0.0, 2.0, 4.0, 8.0, 100.0]


def guides(name, cam, w, h):
    """1-spp Normals and Distances frames at `cam` (tests/ref_integrators): rt_denoise_device's guides."""
    scene, _, st, fc, _ = rt.load_preset(name, w, h)
    st.samples_per_pixel = 1
    out = []
    for integ in (rt.abi.RT_INTEGRATOR_NORMALS, rt.abi.RT_INTEGRATOR_DISTANCES):
        st.integrator = integ
        out.append(rb.render(scene.desc(), cam, st, fc, w, h, total_frame_index=0)[0])
    return out


def main():
    w, h = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (480, 270)
    tp = rt.default_temporal_params()
    cases = {"C3 path": sb.path_case("c3", w, h), "C4 path": sb.path_case("c4", w, h),
             "C3 standing": sb.path_case("c3", w, h, standing=True)}
    runs = {k: sb.run_path(c, tp) for k, c in cases.items()}
    names = list(cases)
    print(f"{w}x{h}, 16 frames of 1 spp, tonemapped RMSE of the last frame against 256 spp; columns: " + ", ".join(names))

    def row(label, fn):
        print(f"{label:<58s} " + "  ".join(f"{fn(k):.4f}" for k in names), flush=True)

    def filtered(k, below=4.0, **kw):
        hist, length, mom, g = runs[k]
        var = sb.variance(mom, length, g, tp, below)
        out, _ = sb.denoise_variance(hist, var, g, sb.filter_params(**dict(START, **kw)))
        return sb.tm_rmse(out, cases[k][3])

    def old_filter(k):
        name = "c4" if k.startswith("C4") else "c3"
        n, d = guides(name, cases[k][0][-1], w, h)
        return sb.tm_rmse(rd.denoise(runs[k][0], n, d, rt.default_denoise_params()), cases[k][3])

    row("the raw 1-spp frame", lambda k: sb.tm_rmse(cases[k][1][-1], cases[k][3]))
    row("the history", lambda k: sb.tm_rmse(runs[k][0], cases[k][3]))
    row("the history + rt_denoise (1-spp guides, its defaults)", old_filter)
    row("the history + the new filter at the starting values", lambda k: filtered(k))
    for k in names:
        length = runs[k][1]
        print(f"  {k}: mean length {float(length.mean()):.2f}, share below 4: {float(((length >= 1) & (length < 4)).mean()):.4f}")
    for field, values in SWEEP.items():
        for v in values:
            row(f"  {field} = {v:g}", lambda k: filtered(k, **{field: v}))
    for v in BELOW:
        row(f"  spatial_below = {v:g}", lambda k: filtered(k, below=v))
    if len(sys.argv) > 3:                                    # a candidate: name=value ...
        kw = {a.split("=")[0]: float(a.split("=")[1]) for a in sys.argv[3:]}
        below = kw.pop("spatial_below", 4.0)
        if "iterations" in kw:
            kw["iterations"] = int(kw["iterations"])
        row("candidate " + " ".join(sys.argv[3:]), lambda k: filtered(k, below=below, **kw))


if __name__ == "__main__":
    main()
