"""xrt_surface_hits_device on a configuration's device-resident primary hits (profiles/surface/README.md): the frame's rays go to the device
once, xrt_scene_intersect_device traces them once, then, in one process, medians of `reps` blocking calls after 3 warm-up calls of
  surface_all    xrt_surface_hits_device with the three outputs (surface record, reflected ray, refracted ray);
  surface_only   the surface record alone -- and its achieved bytes per second, from the bytes the kernel must move: per miss the first
                 quarter of the hit (16) and the zero record (64); per live entry two quarters of the hit (32), the triangle's shade words
                 (s0..s4, and s5 for a flat normal: 16 each), a texel where the material is textured and point-filtered (4) and the record
                 (64).  The 128-byte mesh record and the 32-byte material are shared by many entries and not counted;
  shade_hits     xrt_shade_hits_device with no lights and max_reflections = 0 on the same hits (rays + hits -> RGBA8): the existing call that
                 does the same gathers and writes 4 bytes per entry.
`expected_ms` is shade_hits plus the time the call's extra bytes take at surface_only's achieved rate; `within_expectation` says whether
the call's device time stays below it.  Device times are the calls' own (xrt_stats.ms_total: events around the kernels); `ms` is the host
clock around the blocking call.  One sample per ray whatever the configuration's multisampling mode.  Prints one JSON line per configuration.
    python tools/surface_bench.py [reps] [config ...]        (default: 20 C3 C5_1spp)"""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
names = sys.argv[2:] or ["C3", "C5_1spp"]
lib = xrt.abi.lib()


def timed(fn, tracer):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t, dev = [], []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - a)
        dev.append(tracer.last_stats["ms_total"])
    return {"ms": round(1e3 * float(np.median(t)), 4), "ms_min": round(1e3 * float(np.min(t)), 4), "device_ms": round(float(np.median(dev)), 4),
            "device_ms_min": round(float(np.min(dev)), 4)}


for name in names:
    spec = xrt.configs.config(name)
    scene, tracer = xrt.configs.build_product(spec)
    tracer.MaxReflections = 0
    del tracer.Lights[:]
    n = spec.width * spec.height
    rays = tracer.GeneratePrimaryRays()
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda")
    xrt.abi.check(lib.xrt_scene_intersect_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()), None))
    torch.cuda.synchronize()
    got = {}

    def surface_all():
        got["all"] = tracer.SurfaceHits(d_hits, d_rays, want_reflect=True, want_refract=True, device=True)

    def surface_only():
        got["surface"] = tracer.SurfaceHits(d_hits, device=True)

    def shade():
        got["shade"] = tracer.ShadeHits(d_rays, d_hits, device=True)

    out = {"config": name, "width": spec.width, "height": spec.height, "reps": reps, "n": n}
    out["shade_hits"] = timed(shade, tracer)
    out["surface_only"] = timed(surface_only, tracer)
    out["surface_all"] = timed(surface_all, tracer)
    out["shade_hits_again"] = timed(shade, tracer)   # (the spread of the baseline within the process)
    flags = got["surface"][:, 12].view(torch.int32)
    live = int((flags & 1).ne(0).sum().item())
    flat = int(((flags & 1).ne(0) & (flags & 4).eq(0)).sum().item())
    textured = int((flags & 8).ne(0).sum().item())
    point = int(tracer.TextureFiltering) == xrt.abi.FILTER_POINT
    moved = (n - live) * (16 + 64) + live * (32 + 5 * 16 + 64) + flat * 16 + (textured * 4 if point else 0)
    rate = moved / (out["surface_only"]["device_ms"] * 1e-3)
    transparent = int((flags & 2).ne(0).sum().item())
    out.update(hits=live, flat=flat, textured=textured, transparent=transparent, surface_only_bytes=moved, surface_only_GBps=round(rate / 1e9, 1))
    base = out["shade_hits"]["device_ms"]
    extra_only = n * (64 - 4)
    extra_all = extra_only + 2 * 32 * n + live * (16 + 32)   # the two ray records of every entry; the position quarter and the ray of a live one
    out["surface_only"]["expected_ms"] = round(base + 1e3 * extra_only / rate, 4)
    out["surface_all"]["expected_ms"] = round(base + 1e3 * extra_all / rate, 4)
    for k in ("surface_only", "surface_all"):
        out[k]["within_expectation"] = bool(out[k]["device_ms"] <= out[k]["expected_ms"])
        out[k]["vs_shade_hits"] = round(out[k]["device_ms"] / base, 3)
    print(json.dumps(out), flush=True)
