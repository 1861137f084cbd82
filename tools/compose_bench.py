"""xrt_compose_hits_device on a configuration's device-resident primary hits (profiles/compose/README.md): the frame's rays go to the device
once, xrt_scene_intersect_device traces them once, xrt_surface_hits_device and xrt_light_hits_device (the configuration's lights) run once,
then, in one process, medians of `reps` blocking calls after 3 warm-up calls of
  compose_last   xrt_compose_hits_device without reflect_rgba (RT:726), both outputs;
  compose_step   with reflect_rgba and refract_rgba (RT:584, RT:699 on the Transparent entries), both outputs;
  copy           hipMemcpyAsync device to device of as many bytes as compose_last / compose_step must move, timed with events;
  shade_hits     xrt_shade_hits_device with no lights and max_reflections = 0 on the same hits (rays + hits -> RGBA8), for scale.
The bytes the kernel must move, counted from the flags: per entry the flags quarter of the record (16) and the two outputs (4 + 12); per hit
the colour quarter (16) and the light (12); with a reflection per hit the reflectiveness quarter (16) and the colour (4); per Transparent hit
the refraction's colour (4).  Four consecutive lanes share one 64-byte record, so a line of the record array is fetched whole wherever a
wave has a hit: the bytes that travel are more than the bytes counted.  Device times are the calls' own (xrt_stats.ms_total: events around
the kernel and the memset of the counter word); `ms` is the host clock around the blocking call.  Prints one JSON line per configuration.
    python tools/compose_bench.py [reps] [config ...]        (default: 20 C3 C5_1spp)"""
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


def copy_ms(nbytes):
    """Median device ms of a device-to-device copy of nbytes (torch's copy_ of a contiguous tensor is hipMemcpyAsync), events around it."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4)


for name in names:
    spec = xrt.configs.config(name)
    scene, tracer = xrt.configs.build_product(spec)
    n = spec.width * spec.height
    rays = tracer.GeneratePrimaryRays()
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.zeros((n, 12), dtype=torch.int32, device="cuda")
    xrt.abi.check(lib.xrt_scene_intersect_device(scene.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_hits.data_ptr()), None))
    torch.cuda.synchronize()
    d_surf = tracer.SurfaceHits(d_hits, device=True)
    d_light = tracer.LightHits(d_hits, device=True)
    # colours to blend with: any will do for the time; these are the RT:726 colours of the hits themselves
    d_below = tracer.ComposeHits(d_surf, d_light, device=True)
    got = {}

    def compose_last():
        got["last"] = tracer.ComposeHits(d_surf, d_light, want_float=True, device=True)

    def compose_step():
        got["step"] = tracer.ComposeHits(d_surf, d_light, d_below, d_below, want_float=True, device=True)

    out = {"config": name, "width": spec.width, "height": spec.height, "reps": reps, "n": n, "lights": len(tracer.Lights)}
    out["compose_last"] = timed(compose_last, tracer)
    out["compose_step"] = timed(compose_step, tracer)
    flags = d_surf[:, 12].contiguous().view(torch.int32)
    live = int((flags & 1).ne(0).sum().item())
    transparent = int((flags & 3).eq(3).sum().item())
    moved = {"compose_last": n * (16 + 4 + 12) + live * (16 + 12), "compose_step": n * (16 + 4 + 12) + live * (16 + 12 + 16 + 4) + transparent * 4}
    out.update(hits=live, transparent=transparent)
    for k, b in moved.items():
        out[k]["bytes"] = b
        out[k]["GBps"] = round(b / (out[k]["device_ms"] * 1e-3) / 1e9, 1)
        c = copy_ms(b // 2)   # (a copy of b / 2 bytes reads b / 2 and writes b / 2: b bytes moved)
        out[k]["copy_device_ms"] = c
        out[k]["copy_GBps"] = round(b / (c * 1e-3) / 1e9, 1)
    kept = tracer.MaxReflections, list(tracer.Lights)
    tracer.MaxReflections = 0
    del tracer.Lights[:]

    def shade():
        got["shade"] = tracer.ShadeHits(d_rays, d_hits, device=True)

    out["shade_hits"] = timed(shade, tracer)
    tracer.MaxReflections = kept[0]
    tracer.Lights.extend(kept[1])
    out["compose_last_again"] = timed(compose_last, tracer)   # (the spread within the process)
    print(json.dumps(out), flush=True)
