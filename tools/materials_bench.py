"""Materials changing between frames (xrt_scene_set_materials): the pipelined frame period of C3 (64 crates sharing one textured mesh) and
G1 (four glass spheres), two tickets in flight (xrt_render_device_begin / _end on library streams), in three cases: static; one material's
scalars set before every _begin; one texture of the crate's size (512 x 512) replaced before every _begin.  The picture must not change
with the case, or the periods would compare different frames: the scalars set are the ones the material has, and the texture
"replaced" is the one the mesh has, handed over again (G1's spheres carry no texture: they are given one with use_texture 0, which the
kernels never read).  Also the host time of the call, and the cost of the only alternative before this entry point (a new scene).
Prints one JSON line.
    python tools/materials_bench.py [frames]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib

import numpy as np
import torch

xrt = importlib.import_module("xna-ray-trace_amd")
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def period(scene, tracer, update, n):
    """Steady-state period: n pipelined frames (two tickets), wall time / n; update(): called before every _begin (None: static)."""
    px = tracer.CurrentTarget.Width * tracer.CurrentTarget.Height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    set_ms = []

    def step(k, open_):
        slot = k % 2
        if slot in open_:
            fr[slot].end(open_.pop(slot))
        if update is not None:
            a = time.perf_counter()
            update()
            set_ms.append(1e3 * (time.perf_counter() - a))
        open_[slot] = fr[slot].begin()
    open_ = {}
    for k in range(10):
        step(k, open_)
    for s, t in open_.items():
        fr[s].end(t)
    torch.cuda.synchronize()
    open_, set_ms[:] = {}, []
    a = time.perf_counter()
    for k in range(n):
        step(k, open_)
    for s, t in sorted(open_.items()):
        fr[s].end(t)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - a) / n
    return round(ms, 4), (round(float(np.median(set_ms)) * 1e3, 1) if set_ms else None)


def rebuild_ms(spec, reps=3):
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        xrt.configs.build_product(spec)
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - a))
    return round(float(np.median(t)), 2)


out = {"frames": frames}
for name in ("C3", "G1"):
    spec = xrt.configs.config(name)
    scene, tracer = xrt.configs.build_product(spec)
    mat = scene.meshes[0].MeshMaterial
    tex = mat.Texture if mat.Texture is not None else xrt.fixtures.crate_texture()
    with_tex = xrt.api.Material(mat.Reflectiveness, mat.UseTexture, mat.Transparent, mat.RefractionIndex, tex, mat.TexturePArgb)
    with_tex.InterpolateNormals = mat.InterpolateNormals
    scalars = mat._to_abi_update(False)      # NULL texels: the library keeps the ones it has
    texels = with_tex._to_abi_update(True)   # the same picture, 512 x 512 texels on their way again
    r = {"texels": int(tex.size)}
    r["static_ms"], _ = period(scene, tracer, None, frames)
    r["set_scalars_ms"], r["set_scalars_call_us"] = period(scene, tracer, lambda: scene.SetMaterials([0], [scalars]), frames)
    r["set_texture_ms"], r["set_texture_call_us"] = period(scene, tracer, lambda: scene.SetMaterials([0], [texels]), frames)
    r["static_again_ms"], _ = period(scene, tracer, None, frames)
    r["scalars_overhead"] = round(r["set_scalars_ms"] / r["static_ms"], 4)
    r["texture_overhead"] = round(r["set_texture_ms"] / r["static_ms"], 4)
    r["rebuild_scene_ms"] = rebuild_ms(spec)
    out[name] = r
print(json.dumps(out))
