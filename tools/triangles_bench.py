"""Triangle colours edited on the headline scene (xrt_scene_set_triangle_shading): the 999,698-triangle heightfield (m = 707) as one body,
and what it costs to recolour ALL its triangles, wall time until the device is idle again:
  (a) a new scene of the terrain with the new colours, built from scratch -- the only way before these entry points;
  (b) the host form (host copy edited, arrays staged through page-locked memory, one copy, one k_tri_shading) with no ticket open;
  (c) the host form with one ticket open: the edit goes into a free version, made a copy of the current one on the device first;
  (d), (e) the device form (the colours already in HBM) without and with an open ticket.
For (c) and (e) the ticket's frame is rendered to its end before the clock starts and stays open (its version must not be overwritten),
so the clock sees the edit alone.  On device 0; medians of `reps` runs, milliseconds.  Prints one JSON line.
    python tools/triangles_bench.py [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib

import numpy as np
import torch

xrt = importlib.import_module("xna-ray-trace_amd")
api = xrt.api
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3


def timed(fn):
    torch.cuda.synchronize()
    a = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - a)


spec = xrt.configs.heightfield_scene(192, 108, m=707)
data = spec.meshes[0][0]
nt = data.ntri
rng = np.random.default_rng(0)
palette = [np.ascontiguousarray(rng.uniform(0, 1, size=(nt, 4)), dtype=np.float32) for _ in range(reps + 1)]

a = []
for r in range(reps):   # (a) from scratch
    data.color[...] = palette[r]
    a.append(timed(lambda: xrt.configs.build_product(spec)))
scene, tracer = xrt.configs.build_product(spec)
out_buf = torch.zeros(spec.width * spec.height, dtype=torch.int32, device="cuda")
frame = tracer.PrepareDevice(out_buf.data_ptr())
frame.end(frame.begin())
dev = [torch.tensor(p, device="cuda") for p in palette]
res = {}
for name, device, ticket in (("b_host_no_ticket", False, False), ("c_host_one_ticket", False, True), ("d_device_no_ticket", True, False), ("e_device_one_ticket", True, True)):
    v = []
    for r in range(reps + 1):   # (the first run allocates the staging and, with a ticket, the version: not counted)
        t = None
        if ticket:
            t = frame.begin()
            torch.cuda.synchronize()
        if device:
            v.append(timed(lambda: scene.SetTriangleShadingDevice(0, range(0, nt), color=dev[r])))
        else:
            v.append(timed(lambda: scene.SetTriangleShading(0, range(0, nt), color=palette[r])))
        if ticket:
            frame.end(t)
    res[name + "_first_ms"] = round(v[0], 3)
    res[name + "_ms"] = round(float(np.median(v[1:])), 3)
# where the time goes: the calls of the mirror above also keep its MeshData in step (the device form copies the colours to the host for
# that); the library calls alone, without the mirror:
lib, C = xrt.abi.lib(), api.C
for name, ticket in (("no_ticket", False), ("one_ticket", True)):
    host, device = [], []
    for r in range(reps):
        t = None
        if ticket:
            t = frame.begin()
            torch.cuda.synchronize()
        c, d = palette[r], dev[r]
        host.append(timed(lambda: xrt.abi.check(lib.xrt_scene_set_triangle_shading(scene.handle, 0, None, 0, nt, None, None, api._fp(c)))))
        if ticket:   # (the host form moved the current version on: a new ticket for the device form)
            frame.end(t)
            t = frame.begin()
            torch.cuda.synchronize()
        device.append(timed(lambda: xrt.abi.check(lib.xrt_scene_set_triangle_shading_device(scene.handle, 0, None, 0, nt, None, None, C.c_void_p(d.data_ptr()), None))))
        if ticket:
            frame.end(t)
    res["library_host_form_%s_ms" % name] = round(float(np.median(host)), 3)
    res["library_device_form_%s_ms" % name] = round(float(np.median(device)), 3)
res["a_build_from_scratch_ms"] = round(float(np.median(a)), 3)
print(json.dumps({"reps": reps, "triangles": int(nt), "shade_bytes": int(nt) * 96, **res}))
