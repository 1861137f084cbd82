"""A mesh's triangles replaced on the headline scene (xrt_scene_set_mesh_triangles): the 999,698-triangle heightfield (m = 707, mesh 0) as one
body plus one body of a 12-triangle crate (mesh 1), and what it costs to give a mesh new geometry:
  (a) xrt_scene_build of everything again (the mirror's Build() at another mesh threshold and back) -- the first way before this entry point;
  (b) a body of a NEW crate mesh through Build() (xrt_scene_add_mesh + xrt_scene_set_bodies: one mesh octree built, the arrays assembled again,
      everything uploaded; the old crate stays in the scene) -- the second way, row (c) of profiles/bodies/README.md;
  (c) xrt_scene_set_mesh_triangles on the crate: the same id, the old triangles gone;
  (d) the same on the terrain, every vertex moved (another octree than the one (a) builds), and (d0) with the vertices it has (the octree of (a));
  (e) as (c) on a scene whose crate is mesh 0: the terrain's part of every array lies behind it and moves.
Each on a host-only scene (device -1, measurable on any machine) and, where a GPU is visible, on device 0 (the upload included).  Medians of
`reps` runs, milliseconds.  Asserted, on the product's own host-side code (tests/mesh_edit's checker library): (c) and (d) build exactly one
mesh octree, and the bytes of the host arrays after ten replacements of equal size are those after one.  Prints one JSON line.
    python tools/mesh_edit_bench.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib

import numpy as np

xrt = importlib.import_module("xna-ray-trace_amd")
api = xrt.api
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
M = int(os.environ.get("MESH_EDIT_BENCH_M", "707"))   # (a smaller terrain for a quick look)


def sync(device):
    if device >= 0:
        import torch
        torch.cuda.synchronize()


def timed(fn, device):
    a = time.perf_counter()
    fn()
    sync(device)
    return 1e3 * (time.perf_counter() - a)


def moved(data, seed):
    """Every vertex of the terrain moved a little in y: the same triangle count, another octree."""
    rng = np.random.default_rng(seed)
    v = data.v.copy()
    v[:, :, 1] += rng.uniform(-0.05, 0.05, size=v.shape[:2]).astype(np.float32)
    out = xrt.fixtures.MeshData(v, data.n, data.uv, data.color)
    out.bbox = data.bbox.copy()
    return out


def crate_variant(i):
    """The crate with its vertices moved inside its box (the same twelve triangles)."""
    d = xrt.fixtures.crate(1)
    lo, hi = d.bbox[:3], d.bbox[3:]
    f = np.float32(1.0 - 0.01 * (1 + i % 5))
    out = xrt.fixtures.MeshData((d.v - 0.5 * (lo + hi)) * f + 0.5 * (lo + hi), d.n, d.uv, d.color)
    out.bbox = d.bbox.copy()
    return out


def structure():
    """The structural facts, on HostScene itself."""
    import mesh_edit_py
    spec = xrt.configs.heightfield_scene(64, 36, m=M)
    spec.meshes.append((xrt.fixtures.crate(1), xrt.configs.material(0.5)))
    spec.objects.append(([1], (0.0, 40.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    emu = mesh_edit_py.MeshEditEmul(spec)
    built = emu.trees_built()
    assert emu.set_mesh_triangles(1, crate_variant(0)) == 0 and emu.trees_built() == built + 1      # (c): one octree
    one = emu.bytes()
    for i in range(1, 10):
        assert emu.set_mesh_triangles(1, crate_variant(i)) == 0
    assert emu.bytes() == one and emu.trees_built() == built + 10
    terrain = spec.meshes[0][0]
    assert emu.set_mesh_triangles(0, moved(terrain, 1)) == 0 and emu.trees_built() == built + 11    # (d): one octree
    first = emu.bytes()
    assert emu.set_mesh_triangles(0, moved(terrain, 2)) == 0 and emu.set_mesh_triangles(0, moved(terrain, 1)) == 0 and emu.bytes() == first   # (another octree between: nothing of it stays)
    return {"c_octrees_built": 1, "d_octrees_built": 1, "host_array_bytes_after_1_and_10_crates": one, "host_array_bytes_after_1_and_3_terrains": first}


def measure(device):
    spec = xrt.configs.heightfield_scene(1920, 1080, m=M)
    terrain = api.Mesh(spec.meshes[0][0], api.Material(0.3), device=device)
    crate = api.Mesh(xrt.fixtures.crate(1), api.Material(0.5), device=device)
    ground, box = api.SceneObject([terrain]), api.SceneObject([crate], (0.0, 40.0, 0.0))
    sm = api.OctreeSpatialManager(device)
    sm.Bodies[:] = [ground, box]
    base = timed(sm.Build, device)
    a, b, c, d, d0, e = [], [], [], [], [], []
    for i in range(reps):   # (a) everything again: another mesh threshold makes Build() take the full way (a new scene)
        sm.meshItemTreshold = 50 + (i + 1) % 2
        a.append(timed(sm.Build, device))
        assert sm.last_build_meshes == 2
    handle = sm.handle.value
    terrains = [moved(spec.meshes[0][0], 10 + i) for i in range(reps)]
    for i in range(reps):
        c.append(timed(lambda: sm.SetMeshTriangles(crate, crate_variant(i)), device))              # (c)
        d0.append(timed(lambda: sm.SetMeshTriangles(sm.mesh_id(terrain), spec.meshes[0][0]), device))   # (d0)
        d.append(timed(lambda: sm.SetMeshTriangles(terrain, terrains[i]), device))                 # (d)
        assert sm.handle.value == handle and sm.last_build_meshes == 2
    for i in range(reps):   # (b) a body of a new crate mesh in the old one's place (the scene grows by a mesh every time)
        sm.Bodies[:] = [ground, api.SceneObject([api.Mesh(crate_variant(i), api.Material(0.5), device=device)], (0.0, 40.0, 0.0))]
        b.append(timed(sm.Build, device))
        assert sm.last_build_meshes == 1 and sm.handle.value == handle
    del sm
    sm = api.OctreeSpatialManager(device)   # (e) the crate first
    sm.Bodies[:] = [box, ground]
    sm.Build()
    assert sm.mesh_id(crate) == 0
    for i in range(reps):
        e.append(timed(lambda: sm.SetMeshTriangles(crate, crate_variant(i)), device))
    med = lambda v: round(float(np.median(v)), 3)
    return {"first_build_ms": round(base, 3), "a_build_everything_ms": med(a), "b_add_mesh_set_bodies_ms": med(b), "c_set_mesh_triangles_crate_ms": med(c),
            "d_set_mesh_triangles_terrain_ms": med(d), "d0_set_mesh_triangles_terrain_same_vertices_ms": med(d0), "e_set_mesh_triangles_crate_first_ms": med(e)}


out = {"reps": reps, "triangles": int(xrt.fixtures.heightfield(M).ntri), "structure": structure(), "host_only": measure(-1)}
try:
    import torch
    gpu = torch.cuda.is_available()
except Exception:
    gpu = False
if gpu:
    out["gpu"] = measure(0)
    out["c_upload_ms"] = round(out["gpu"]["c_set_mesh_triangles_crate_ms"] - out["host_only"]["c_set_mesh_triangles_crate_ms"], 3)
print(json.dumps(out))
