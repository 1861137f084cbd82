"""The body list edited on the headline scene (xrt_scene_set_bodies): the 999,698-triangle heightfield (m = 707) as one body, and what it costs
to make a second body appear, through the mirror's OctreeSpatialManager.Build():
  (a) a new scene of the terrain and a 12-triangle crate, built from scratch -- the only way before this entry point;
  (b) Build() after appending a second body of the terrain's own mesh (xrt_scene_set_bodies, no mesh octree built);
  (c) Build() after appending a body of a new 12-triangle crate mesh (one mesh octree built, the arrays assembled again, everything uploaded).
Each on a host-only scene (device -1, measurable on any machine) and, where a GPU is visible, on device 0 (the upload included).  Medians of
`reps` runs, milliseconds.  Prints one JSON line.
    python tools/bodies_bench.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib

import numpy as np

xrt = importlib.import_module("xna-ray-trace_amd")
api = xrt.api
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3


def sync(device):
    if device >= 0:
        import torch
        torch.cuda.synchronize()


def timed(fn, device):
    a = time.perf_counter()
    fn()
    sync(device)
    return 1e3 * (time.perf_counter() - a)


def crate_mesh(device):
    return api.Mesh(xrt.fixtures.crate(1), api.Material(0.5), device=device)


def measure(device):
    spec = xrt.configs.heightfield_scene(1920, 1080, m=707)
    terrain = api.Mesh(spec.meshes[0][0], api.Material(0.3), device=device)
    ground = api.SceneObject([terrain])
    a, b, c = [], [], []
    for _ in range(reps):   # (a) from scratch, terrain + crate
        sm = api.OctreeSpatialManager(device)
        sm.Bodies[:] = [ground, api.SceneObject([crate_mesh(device)], (0.0, 40.0, 0.0))]
        a.append(timed(sm.Build, device))
        assert sm.last_build_meshes == 2
        del sm
    sm = api.OctreeSpatialManager(device)
    sm.Bodies[:] = [ground]
    base = timed(sm.Build, device)
    handle = sm.handle.value
    for _ in range(reps):
        sm.Bodies[:] = [ground, api.SceneObject([terrain], (0.0, 30.0, 0.0))]
        b.append(timed(sm.Build, device))                     # (b) a second body of the terrain's mesh
        assert sm.last_build_meshes == 0 and sm.handle.value == handle
        sm.Bodies[:] = [ground, api.SceneObject([crate_mesh(device)], (0.0, 40.0, 0.0))]
        c.append(timed(sm.Build, device))                     # (c) a body of a new crate mesh
        assert sm.last_build_meshes == 1 and sm.handle.value == handle
        sm.Bodies[:] = [ground]
        sm.Build()
    med = lambda v: round(float(np.median(v)), 3)
    return {"build_terrain_alone_ms": round(base, 3), "a_build_from_scratch_ms": med(a), "b_set_bodies_known_mesh_ms": med(b), "c_set_bodies_new_mesh_ms": med(c),
            "b_meshes_built": 0, "c_meshes_built": 1}


out = {"reps": reps, "triangles": int(xrt.fixtures.heightfield(707).ntri), "host_only": measure(-1)}
try:
    import torch
    gpu = torch.cuda.is_available()
except Exception:
    gpu = False
if gpu:
    out["gpu"] = measure(0)
    # (c) on the host is the crate's octree (microseconds), the arrays assembled again and the scene octree; on the GPU also the upload of everything
    out["c_reassembly_ms"] = round(out["host_only"]["c_set_bodies_new_mesh_ms"] - out["host_only"]["b_set_bodies_known_mesh_ms"], 3)
    out["c_upload_ms"] = round(out["gpu"]["c_set_bodies_new_mesh_ms"] - out["host_only"]["c_set_bodies_new_mesh_ms"], 3)
print(json.dumps(out))
