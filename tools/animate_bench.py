"""Bodies moving between frames (xrt_scene_set_poses[_device]): the pipelined frame period of C3 (64 crates, two tickets in flight,
xrt_render_device_begin / _end on library streams) with static poses, with all 64 crates re-posed before every _begin (host arrays, and
device arrays from torch), the cost of the only alternative before these entry points (create, add every mesh and body, xrt_scene_build),
and the same for G1 running the reference's video loop (spheres on circles, Game1.cs:152-189).  A moving scene is a different picture
every frame (G1's spheres spread out and get cheaper), so the update's own cost is measured as the same pose set again before every
frame against that pose left alone (update_overhead).  Prints one JSON line.
    python tools/animate_bench.py [frames]
k_pose's device time: run under `rocprofv3 --kernel-trace --stats -- python tools/animate_bench.py` (profiles/poses)."""
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


def grid_poses(spec, k):
    """Every body of spec, shifted and turned a little by frame k: (ids, world, inv, wbb) as float32 arrays."""
    ids = np.arange(len(spec.objects), dtype=np.int32)
    w, iw, bb = [], [], []
    for b, (mids, pos, rot, scale) in enumerate(spec.objects):
        bbox = np.zeros(6, dtype=np.float32)
        for i in mids:
            bbox[:3] = np.minimum(bbox[:3], spec.meshes[i][0].bbox[:3])
            bbox[3:] = np.maximum(bbox[3:], spec.meshes[i][0].bbox[3:])
        a = 0.01 * k + 0.1 * b
        world, inv, wbb = xrt.xna.build_world(scale, (rot[0], rot[1] + a, rot[2]), (pos[0] + 2.0 * np.sin(a), pos[1], pos[2] + 2.0 * np.cos(a)), bbox)
        w.append(xrt.xna.as_array(world)); iw.append(xrt.xna.as_array(inv)); bb.append(xrt.xna.as_array(wbb))
    return ids, np.concatenate(w), np.concatenate(iw), np.concatenate(bb)


def video_poses(spec, k):
    """G1's four spheres on a circle of radius 10 (the reference's video loop), frame k."""
    ids = np.arange(4, dtype=np.int32)
    w, iw, bb = [], [], []
    for i in range(4):
        bbox = np.zeros(6, dtype=np.float32)
        bbox[:3] = np.minimum(bbox[:3], spec.meshes[0][0].bbox[:3]); bbox[3:] = np.maximum(bbox[3:], spec.meshes[0][0].bbox[3:])
        rot = 0.05 * k + i * (np.pi / 2)
        world, inv, wbb = xrt.xna.build_world((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (float(np.sin(rot) * 10), 3.0, float(np.cos(rot) * 10)), bbox)
        w.append(xrt.xna.as_array(world)); iw.append(xrt.xna.as_array(inv)); bb.append(xrt.xna.as_array(wbb))
    return ids, np.concatenate(w), np.concatenate(iw), np.concatenate(bb)


def period(scene, tracer, poses_of, mode, n):
    """Steady-state period: n pipelined frames (two tickets), wall time / n.  mode: static | host | device (a new pose every frame) |
    host_same (the same pose set again before every frame: the update's cost alone, the picture does not change)."""
    px = tracer.CurrentTarget.Width * tracer.CurrentTarget.Height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    pre = [poses_of(k) for k in range(16)]
    dev = [tuple(torch.from_numpy(a).cuda() for a in p) for p in pre]
    set_ms = []

    def step(k, open_):
        slot = k % 2
        if slot in open_:
            fr[slot].end(open_.pop(slot))
        if mode != "static":
            a = time.perf_counter()
            if mode == "host":
                scene.SetPoses(*pre[k % 16])
            elif mode == "host_same":
                scene.SetPoses(*pre[0])
            else:
                scene.SetPosesDevice(*dev[k % 16])
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
for name, poses in (("C3", grid_poses), ("G1", video_poses)):
    spec = xrt.configs.config(name)
    scene, tracer = xrt.configs.build_product(spec)
    r = {}
    r["static_ms"], _ = period(scene, tracer, lambda k: poses(spec, k), "static", frames)
    r["set_poses_ms"], r["set_poses_call_us"] = period(scene, tracer, lambda k: poses(spec, k), "host", frames)
    r["set_poses_device_ms"], r["set_poses_device_call_us"] = period(scene, tracer, lambda k: poses(spec, k), "device", frames)
    scene.SetPoses(*poses(spec, 0))
    r["static_posed_ms"], _ = period(scene, tracer, lambda k: poses(spec, k), "static", frames)     # the scene at pose 0, not moving
    r["same_pose_every_frame_ms"], _ = period(scene, tracer, lambda k: poses(spec, k), "host_same", frames)
    r["update_overhead"] = round(r["same_pose_every_frame_ms"] / r["static_posed_ms"], 4)
    r["animated_vs_static"] = round(r["set_poses_ms"] / r["static_ms"], 4)
    r["bodies_posed_per_frame"] = len(poses(spec, 0)[0])
    r["rebuild_scene_ms"] = rebuild_ms(spec)
    out[name] = r
print(json.dumps(out))
