"""xrt_trace_pixels_device on a configuration's row-major frame (profiles/trace_pixels/README.md), one sample per pixel whatever the configuration's
multisampling mode.  Medians of `reps` blocking calls after 3 warm-up calls, host wall clock around each call, the device synchronised.
  (a) primary hits: "today's way" -- xrt_generate_primary_rays (host), the upload of its rays, xrt_scene_intersect_device -- next to
      xrt_trace_pixels_device unhinted and hinted (XRT_LIST_COHERENT), rays and hits both wanted, and hinted with hits alone.  The hits of all ways
      are compared field by field without `reserved`.
  (b) the relight loop: one xrt_trace_pixels_device (hinted), then K xrt_shade_hits_device calls on its rays and hits with a light that moves between
      the calls, next to K xrt_cast_rays_device calls on the same rays with the same lights.  The colours of the last step are compared.
Run from the tree of a library that has no xrt_trace_pixels (the parent commit's) it times today's way and the K xrt_cast_rays_device calls alone.
Prints one JSON line.
    python tools/trace_pixels_bench.py [config] [reps] [K]"""
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
name = sys.argv[1] if len(sys.argv) > 1 else "C3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
K = int(sys.argv[3]) if len(sys.argv) > 3 else 8
spec = xrt.configs.config(name)
scene, tracer = xrt.configs.build_product(spec)
tracer.UseMultisampling = False
n = spec.width * spec.height
lib = xrt.abi.lib()


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
    r = {"ms": t, "ms_min": tmin}
    if st is not None:
        r.update({"device_ms": round(st["ms_total"], 3), "ms_intersect": round(st["ms_intersect"], 3), "launches": int(st["intersect_launches"]),
                  "rays_closest": int(st["rays_closest"]), "rays_traversed": int(st["rays_traversed"]), "hits_closest": int(st["hits_closest"])})
    return r


got = {}
out = {"config": name, "width": spec.width, "height": spec.height, "depth": spec.max_reflections, "lights": len(spec.lights), "reps": reps, "n": n, "K": K}
d_hits_today = torch.zeros((n, 12), dtype=torch.int32, device="cuda")


def today():
    rays = tracer.GeneratePrimaryRays()
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).cuda()
    xrt.abi.check(lib.xrt_scene_intersect_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits_today.data_ptr()), None))
    got["today_rays"] = d_rays


t, tmin = timed(today)
out["today"] = row(t, tmin)
torch.cuda.synchronize()
out["hits"] = int((d_hits_today[:, 0] != 0).sum().item())
d_rays = got["today_rays"]
has = hasattr(tracer, "TracePixels")
if has:
    y, x = np.mgrid[0:spec.height, 0:spec.width]
    d_c = torch.from_numpy(np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float32)).cuda()
    for key, kw in (("trace_unhinted", dict(coherent=False)), ("trace_hinted", dict(coherent=True)), ("trace_hinted_hits_only", dict(coherent=True, want_rays=False))):
        def trace():
            got[key] = tracer.TracePixels(d_c, device=True, **kw)
        t, tmin = timed(trace)
        out[key] = row(t, tmin, tracer.last_stats)
        out[key]["vs_today"] = round(t / out["today"]["ms"], 3)
    same = True
    for key in ("trace_unhinted", "trace_hinted"):
        r, h = got[key]
        same = same and bool(torch.equal(r.view(torch.int32).reshape(-1, 8), d_rays.view(torch.int32).reshape(-1, 8))) and bool(torch.equal(h[:, :11], d_hits_today[:, :11]))
    same = same and bool(torch.equal(got["trace_hinted_hits_only"][:, :11], d_hits_today[:, :11]))
    out["same_rays_and_hits"] = same

# (b) the relight loop: the first light circles the scene, one step per call
base = [(l.Position if hasattr(l, "Position") else None) for l in tracer.Lights]


def move(step):
    l = tracer.Lights[0]
    if base[0] is not None:
        px_, py_, pz_ = (float(v) for v in base[0])
        a = 0.2 * step
        l.Position = (px_ * np.cos(a) - pz_ * np.sin(a), py_, px_ * np.sin(a) + pz_ * np.cos(a))


def cast_loop():
    for k in range(K):
        move(k)
        got["cast"] = tracer.CastRays(d_rays, device=True)


t, tmin = timed(cast_loop)
out["relight_cast_rays"] = row(t, tmin)
if has:
    def shade_loop():
        r, h = tracer.TracePixels(d_c, device=True, coherent=True)
        for k in range(K):
            move(k)
            got["shade"] = tracer.ShadeHits(r, h, device=True)
    t, tmin = timed(shade_loop)
    out["relight_trace_then_shade_hits"] = row(t, tmin)
    out["relight_vs_cast"] = round(t / out["relight_cast_rays"]["ms"], 3)
    out["same_colours"] = bool(torch.equal(got["cast"], got["shade"]))
print(json.dumps(out))
