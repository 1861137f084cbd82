"""xrt_light_hits_device on a configuration's device-resident primary hits (profiles/lights/README.md), next to two baselines: the frame's
rays go to the device once, xrt_scene_intersect_device traces them once, then medians of `reps` blocking calls after 3 warm-up calls of
  shade_hits   xrt_shade_hits_device with max_reflections = 0 (rays + hits -> colours): the nearest equivalent a library without
               xrt_light_hits has -- the same shadow rays, and around them the ingest, the level records and the compose;
  light_hits   xrt_light_hits_device, the light sum alone, and light_hits_amounts, the light sum and the per-light amounts;
  intersect    xrt_scene_intersect_device on the shadow rays of the live hits, formed beforehand (the seam-1 host's way: a 32-byte ray in
               and a 48-byte hit out per shadow ray; the forming is not timed).
One sample per ray whatever the configuration's multisampling mode.  Run from the tree of a library that has no xrt_light_hits (the parent
commit's) it times shade_hits alone.  Prints one JSON line.
    python tools/lights_bench.py [config] [reps]"""
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
tracer.MaxReflections = 0
n = spec.width * spec.height
rays = tracer.GeneratePrimaryRays()
d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
d_hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda")
lib = xrt.abi.lib()
xrt.abi.check(lib.xrt_scene_intersect_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()), None))
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


def row(t, tmin, st=None):
    out = {"ms": t, "ms_min": tmin}
    if st is not None:
        out.update({"device_ms": round(st["ms_total"], 3), "ms_intersect": round(st["ms_intersect"], 3), "launches": int(st["intersect_launches"]),
                    "rays_shadow": int(st["rays_shadow"]), "rays_traversed": int(st["rays_traversed"])})
    return out


got = {}
live = d_hits[:, 0] != 0
out = {"config": name, "width": spec.width, "height": spec.height, "lights": len(spec.lights), "reps": reps, "n": n, "hits": int(live.sum().item())}


def shade():
    got["shade"] = tracer.ShadeHits(d_rays, d_hits, want_float=True, device=True)


t, tmin = timed(shade)
out["shade_hits"] = row(t, tmin, tracer.last_stats)
if hasattr(tracer, "LightHits"):
    def light():
        got["light"] = tracer.LightHits(d_hits, device=True)

    def both():
        got["both"] = tracer.LightHits(d_hits, want_amounts=True, device=True)
    t, tmin = timed(light)
    out["light_hits"] = row(t, tmin, tracer.last_stats)
    out["light_vs_shade"] = round(t / out["shade_hits"]["ms"], 3)
    t, tmin = timed(both)
    out["light_hits_amounts"] = row(t, tmin, tracer.last_stats)
    # the seam-1 way: the shadow rays of the live hits, light by light (RT:469-479), through the closest-hit query
    h = d_hits[live]
    w = h[:, 8:11].view(torch.float32)
    parts = []
    for l in spec.lights:
        if l["kind"] == xrt.abi.LIGHT_SPOT:
            d = torch.tensor(l["position"], dtype=torch.float32, device="cuda") - w
            d = d / d.norm(dim=1, keepdim=True)
        else:
            d = (-torch.tensor(l["direction"], dtype=torch.float32, device="cuda")).expand_as(w)
        parts.append(torch.cat([w, d, h[:, 2:4].view(torch.float32)], dim=1))
    if parts:
        s_rays = torch.cat(parts).contiguous()
        s_hits = torch.zeros((s_rays.shape[0], 12), dtype=torch.int32, device="cuda")

        def seam1():
            xrt.abi.check(lib.xrt_scene_intersect_device(scene.handle, C.c_void_p(s_rays.data_ptr()), s_rays.shape[0], C.c_void_p(s_hits.data_ptr()), None))
        t, tmin = timed(seam1)
        out["intersect"] = row(t, tmin)
        out["intersect"]["rays"] = int(s_rays.shape[0])
        out["light_amounts_vs_intersect"] = round(out["light_hits_amounts"]["ms"] / t, 3)
        # the closest-hit answers say "obstructed or not" as the amounts do wherever no blocker lies beyond a light
        out["obstructed_by_intersect"] = int((s_hits[:, 0] != 0).sum().item())
        out["amounts_nonzero"] = int((got["both"][1] != 0).sum().item())
print(json.dumps(out))
