"""Regenerates tests/golden/bvh_sah_full.json: full-SAH trees (method 2) of rth_generate_mesh
meshes, built by the HOST builder (rt_host.cpp's restatement of RT/bvh.cpp:63-131) on the CPU.

Per mesh: the generator's arguments (tris, seed), the actual triangle count, the node count,
the sha256 of the node bytes (node_count x 32) followed by the uint32 entry order, and the
host's build time.  The host build is quadratic: about a minute for each of the two large
meshes.  Run once, from the repository root, after building the library:

    python tests/golden/make_bvh_sah_full.py
"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402

MESHES = [(8000, 1), (70000, 1), (62500, 3)]


def digest(nodes, order):
    return hashlib.sha256(np.ascontiguousarray(nodes).tobytes() + np.ascontiguousarray(order, np.uint32).tobytes()).hexdigest()


def main():
    rt = conftest._import_package()
    from test_bvh_builder import _build, _mesh_entries
    out = []
    for tris_n, seed in MESHES:
        n = rt.lib().rth_generate_mesh(tris_n, seed, None, None)
        tris = np.zeros((n, 3, 3), np.float32)
        rt.lib().rth_generate_mesh(tris_n, seed, tris.ctypes.data_as(C.POINTER(rt.abi.V3)), None)
        c, r = _mesh_entries(rt, tris)
        t0 = time.perf_counter()
        nodes, order = _build(rt, c, r, 2, None)
        ms = (time.perf_counter() - t0) * 1e3
        out.append({"tris": tris_n, "seed": seed, "triangles": int(n), "nodes": int(len(nodes)),
                    "sha256": digest(nodes, order), "host_ms": round(ms, 1)})
        print(out[-1], flush=True)
    with open(os.path.join(HERE, "bvh_sah_full.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
