"""xrt_shade_hits_device next to xrt_cast_rays_device on a configuration's primary rays (profiles/shade_hits/README.md): the frame's rays go
to the device once, xrt_scene_intersect_device traces them once, then medians of `reps` blocking calls after 3 warm-up calls of
xrt_cast_rays_device (rays -> colours, generation 0 traced) and of xrt_shade_hits_device (rays + hits -> colours, generation 0 ingested) on
the same rays.  One sample per ray whatever the configuration's multisampling mode.  The colours are compared row by row.  Run from the
tree of a library that has no xrt_shade_hits (the parent commit's) it times xrt_cast_rays_device alone.  Prints one JSON line.
    python tools/shade_hits_bench.py [config] [reps]"""
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
n = spec.width * spec.height
rays = tracer.GeneratePrimaryRays()
d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
d_hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda")
xrt.abi.check(xrt.abi.lib().xrt_scene_intersect_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()), None))
torch.cuda.synchronize()


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
    return round(1e3 * float(np.median(t)), 3), round(1e3 * float(np.min(t)), 3)


def row(t, tmin, st):
    return {"ms": t, "ms_min": tmin, "device_ms": round(st["ms_total"], 3), "ms_intersect": round(st["ms_intersect"], 3),
            "launches": int(st["intersect_launches"]), "rays_closest": int(st["rays_closest"]), "rays_shadow": int(st["rays_shadow"]),
            "rays_traversed": int(st["rays_traversed"])}


got = {}
out = {"config": name, "width": spec.width, "height": spec.height, "depth": spec.max_reflections, "lights": len(spec.lights), "reps": reps, "n": n,
       "hits": int((d_hits[:, 0] != 0).sum().item())}


def cast():
    got["cast"] = tracer.CastRays(d_rays, device=True)


t, tmin = timed(cast)
out["cast_rays"] = row(t, tmin, tracer.last_stats)
if hasattr(tracer, "ShadeHits"):
    def shade():
        got["shade"] = tracer.ShadeHits(d_rays, d_hits, device=True)
    t, tmin = timed(shade)
    out["shade_hits"] = row(t, tmin, tracer.last_stats)
    out["shade_vs_cast"] = round(t / out["cast_rays"]["ms"], 3)
    out["same_colours"] = bool(torch.equal(got["cast"], got["shade"]))
print(json.dumps(out))
