"""xrt_cast_rays_paths next to xrt_cast_rays on the same rays -- the primary rays of a configuration's camera (default G1: the reference's glass
spheres, 512x512, depth 8) -- in the host and the device form, runs interleaved.  The paths call is timed counting only (no vertex array) and
with a vertex array of exactly the size the batch needs; its colours are checked against the plain call's.  Prints one JSON line.
    python tools/paths_bench.py [config] [reps] [iteration]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib

import numpy as np
import torch

xrt = importlib.import_module("xna-ray-trace_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "G1"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
iteration = int(sys.argv[3]) if len(sys.argv) > 3 else 0
spec = xrt.configs.config(name)
scene, tracer = xrt.configs.build_product(spec)
lib, abi = xrt.abi.lib(), xrt.abi
rays = tracer.GeneratePrimaryRays()
n = len(rays)
opts, lights = tracer._opts_abi(shard_count=0), tracer._lights_abi()
opts.n_gpus = 0
st, need = abi.xrt_stats(), C.c_int64(0)
PR, PU, PV = C.POINTER(abi.xrt_ray), C.POINTER(C.c_uint32), C.POINTER(abi.xrt_path_vertex)

h_rgba, h_rgba2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
h_start, h_back = np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=xrt.RAY_DTYPE)
d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
d_rgba, d_rgba2 = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
d_start, d_back = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros((n, 8), dtype=torch.float32, device="cuda")


def host_plain():
    abi.check(lib.xrt_cast_rays(scene.handle, rays.ctypes.data_as(PR), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts), h_rgba.ctypes.data_as(PU), None, C.byref(st)))


def host_paths(verts, cap):
    abi.check(lib.xrt_cast_rays_paths(scene.handle, rays.ctypes.data_as(PR), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts), h_rgba2.ctypes.data_as(PU), None,
                                      h_back.ctypes.data_as(PR), h_start.ctypes.data_as(C.POINTER(C.c_int64)), verts.ctypes.data_as(PV) if cap else None, cap, C.byref(need), C.byref(st)))


def dev_plain():
    abi.check(lib.xrt_cast_rays_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts), C.c_void_p(d_rgba.data_ptr()),
                                       None, None, C.byref(st)))


def dev_paths(verts, cap):
    abi.check(lib.xrt_cast_rays_paths_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, iteration, 1.0, lights, len(tracer.Lights), C.byref(opts), C.c_void_p(d_rgba2.data_ptr()),
                                             None, C.c_void_p(d_back.data_ptr()), C.c_void_p(d_start.data_ptr()), C.c_void_p(verts.data_ptr()) if cap else None, cap, None,
                                             C.byref(need), C.byref(st)))


host_paths(None, 0)
total = need.value
h_verts = np.zeros(max(total, 1), dtype=xrt.VERTEX_DTYPE)
d_verts = torch.zeros((max(total, 1), 4), dtype=torch.float32, device="cuda")
runs = {"host_plain": host_plain, "host_paths_count": lambda: host_paths(None, 0), "host_paths": lambda: host_paths(h_verts, total),
        "device_plain": dev_plain, "device_paths_count": lambda: dev_paths(None, 0), "device_paths": lambda: dev_paths(d_verts, total)}
times = {k: [] for k in runs}
for rep in range(reps + 3):   # interleaved: every repetition runs every variant once; three warm-up repetitions
    for k, fn in runs.items():
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= 3:
            times[k].append(time.perf_counter() - a)
out = {"config": name, "rays": n, "depth": spec.max_reflections, "iteration": iteration, "reps": reps, "vertices": total,
       "same_colours": bool(np.array_equal(h_rgba, h_rgba2) and torch.equal(d_rgba, d_rgba2) and np.array_equal(d_rgba.cpu().numpy().view(np.uint32), h_rgba)),
       "same_vertices_host_device": bool(np.array_equal(d_verts.cpu().numpy().view(np.uint32).reshape(-1), h_verts.view(np.uint32).reshape(-1)))}
for k, t in times.items():
    out[k] = {"ms": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * float(np.min(t)), 3)}
for form in ("host", "device"):
    out[form + "_paths_vs_plain"] = round(out[form + "_paths"]["ms"] / out[form + "_plain"]["ms"], 3)
    out[form + "_count_vs_plain"] = round(out[form + "_paths_count"]["ms"] / out[form + "_plain"]["ms"], 3)
print(json.dumps(out))
