"""xrt_render_pixels_device next to xrt_render_device on one configuration and multisampling mode (profiles/pixels/README.md):
  - the listed frame: all W*H integer centres in row-major order, against the blocking frame of the same camera on the same build (the list's
    colours are checked against the frame's);
  - small lists: one centre, 4096 random pixels, a 128x128 rectangle -- the latency a pixel inspector or a region re-render sees.
One process, warm-up, medians of `reps` blocking calls.  Prints one JSON line.
    python tools/pixels_bench.py [config] [off|fixed16|adaptive] [reps] [coherent]
coherent (profiles/coherent_lists/README.md): 0 every list unhinted (the default, the rows as they were), 1 every list with XRT_LIST_COHERENT, both: each
list unhinted under its key and hinted under <key>_coherent, in that order in one process."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib

import numpy as np
import torch

xrt = importlib.import_module("xna-ray-trace_amd")
name = sys.argv[1] if len(sys.argv) > 1 else "C5"
mode = sys.argv[2] if len(sys.argv) > 2 else "fixed16"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
coherent = sys.argv[4] if len(sys.argv) > 4 else "0"
hints = {"0": [(False, "")], "1": [(True, "")], "both": [(False, ""), (True, "_coherent")]}[coherent]
abi = xrt.abi
spec = xrt.configs.config(name)
scene, tracer = xrt.configs.build_product(spec)
ms = {"off": abi.MS_OFF, "fixed16": abi.MS_FIXED16, "adaptive": abi.MS_ADAPTIVE}[mode]
tracer.UseMultisampling = ms != abi.MS_OFF
tracer.MultisampleMode = ms if ms != abi.MS_OFF else None
W, H = spec.width, spec.height
n = W * H

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
    return round(1e3 * float(np.median(t)), 3), round(1e3 * float(np.min(t)), 3)


out = {"config": name, "mode": mode, "width": W, "height": H, "depth": spec.max_reflections, "reps": reps, "coherent": coherent}
out["frame_ms"], out["frame_ms_min"] = timed(render)
ref = frame.cpu().numpy().view(np.uint32)

ys, xs = np.divmod(np.arange(n), W)
rng = np.random.default_rng(1)
x0, y0 = (W - 128) // 2, (H - 128) // 2
ry, rx = np.mgrid[y0:y0 + 128, x0:x0 + 128]
lists = {"listed_frame": np.arange(n), "one": np.array([(H // 2) * W + W // 2]), "random_4096": rng.permutation(n)[:4096],
         "rect_128x128": (ry * W + rx).ravel()}
for key, at in lists.items():
    centers = torch.from_numpy(np.stack([xs[at], ys[at]], axis=1).astype(np.float32)).cuda()
    for hinted, suffix in hints:
        got = {}

        def call():
            got["rgba"] = tracer.RenderPixels(centers, device=True, coherent=hinted)
        t, tmin = timed(call)
        st = tracer.last_stats
        out[key + suffix] = {"n": int(len(at)), "ms": t, "ms_min": tmin, "vs_frame": round(t / out["frame_ms"], 3), "device_ms": round(st["ms_total"], 3),
                             "ms_intersect": round(st["ms_intersect"], 3), "launches": int(st["intersect_launches"]), "rays": int(st["rays_closest"] + st["rays_shadow"]),
                             "same_as_frame": bool(np.array_equal(got["rgba"].cpu().numpy().view(np.uint32), ref[at]))}
print(json.dumps(out))
