"""xrt_cast_rays_device on the primary rays of a configuration's camera (default C5_1spp: 2.07 M rays, depth 3) in three orders --
row-major, 64x8-tile order (the order a frame traces its pixels in) and shuffled -- next to the blocking frame of the same camera
(xrt_render_device).  Every order's colours are checked against the frame's.  Prints one JSON line.
    python tools/cast_rays_bench.py [config] [reps]"""
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
name = sys.argv[1] if len(sys.argv) > 1 else "C5_1spp"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
spec = xrt.configs.config(name)
scene, tracer = xrt.configs.build_product(spec)
W, H = spec.width, spec.height
n = W * H
lib, abi = xrt.abi.lib(), xrt.abi

frame = torch.zeros(n, dtype=torch.int32, device="cuda")
render = tracer.PrepareDevice(frame.data_ptr())


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - a)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


frame_ms, frame_min = timed(render)
ref = frame.cpu().numpy().view(np.uint32)

rays = tracer.GeneratePrimaryRays()   # row-major, RT:410-421
ys, xs = np.divmod(np.arange(n), W)
tile = (ys // 8) * ((W + 63) // 64) + xs // 64
orders = {"row_major": np.arange(n), "tile_64x8": np.lexsort((xs % 64, ys % 8, tile)), "shuffled": np.random.default_rng(1).permutation(n)}
opts, lights = tracer._opts_abi(shard_count=0), tracer._lights_abi()
st = abi.xrt_stats()
out = {"config": name, "rays": n, "depth": spec.max_reflections, "reps": reps, "frame_ms": round(frame_ms, 3), "frame_ms_min": round(frame_min, 3)}
for key, perm in orders.items():
    d_rays = torch.from_numpy(rays[perm].view(np.float32).reshape(-1, 8).copy()).cuda()
    d_out = torch.zeros(n, dtype=torch.int32, device="cuda")

    def cast():
        abi.check(lib.xrt_cast_rays_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, 0, 1.0, lights, len(tracer.Lights), C.byref(opts),
                                           C.c_void_p(d_out.data_ptr()), None, None, C.byref(st)))
    ms, ms_min = timed(cast)
    got = np.empty(n, dtype=np.uint32)
    got[perm] = d_out.cpu().numpy().view(np.uint32)
    out[key] = {"ms": round(ms, 3), "ms_min": round(ms_min, 3), "mrays_per_s": round(n / ms / 1e3, 1), "vs_frame": round(ms / frame_ms, 3),
                "ms_intersect": round(st.ms_intersect, 3), "launches": int(st.intersect_launches), "same_as_frame": bool(np.array_equal(got, ref))}
print(json.dumps(out))
