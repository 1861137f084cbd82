"""xrt_scene_set_poses / xrt_scene_set_poses_device / xrt_scene_build_tree on the MI355X: frames, seam-1 answers and ray batches of
scenes whose bodies move between frames, bit for bit against the checker (tests/poses: the oracle with moved bodies, RGBA8 and the
fp32 colour vectors) -- with the stale scene octree of the reference's game loop, after the tree is built again, pipelined, from device
arrays, on replicas and through the scene file."""
import ctypes as C

import numpy as np
import pytest

import poses_py
from poses_py import PoseOracle, hits_equal, moved, pose_arrays

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def frame_equal(got_rgba, got_f, want, what):
    rgba, rgbf = want
    bad = int((np.asarray(got_rgba).reshape(-1) != rgba).sum())
    assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, rgba.size)
    if got_f is not None:
        assert np.array_equal(_bits(got_f).reshape(-1), _bits(rgbf).reshape(-1)), what


def render(tracer):
    rgba, rgbf = tracer.Render(want_float=True)
    return rgba.copy(), rgbf.copy()


def move(body, pos, rot, scale=(1.0, 1.0, 1.0)):
    body.Position, body.Rotation, body.Scale = pos, rot, scale


def f32_turns(start, k, step=0.02):
    """prism.Rotation += (0, 0.02f, 0), k times in binary32 (Game1.cs:281-288)."""
    r = np.float32(start)
    for _ in range(k):
        r = np.float32(r + np.float32(step))
    return float(r)


def test_prism_turned_by_the_n_key(xrt):
    """Game1's N key turns the glass prism by 0.02 rad about y; the next frame renders the turned prism (ray trees through glass)."""
    spec = xrt.configs.content_scene2(96, 54, max_reflections=3)
    scene, tracer = xrt.configs.build_product(spec)
    ref = PoseOracle(spec)
    prism = scene.Bodies[1]
    pos, rot, scale = spec.objects[1][1:]
    before = render(tracer)
    for presses in (1, 25):
        r = (rot[0], f32_turns(rot[1], presses), rot[2])
        move(prism, pos, r, scale)
        ref.set_pose(1, pos, r, scale)
        got = render(tracer)
        frame_equal(*got, ref.render(), "prism after %d presses" % presses)
        assert not np.array_equal(got[0], before[0])


def test_a_body_moved_out_of_the_root_box_appears_after_build_tree(xrt):
    spec = xrt.configs.default_game_scene(96, 96, max_reflections=4)
    spec.scene_threshold = 2
    scene, tracer = xrt.configs.build_product(spec)
    ref = PoseOracle(spec)
    out = ((-7.5, 9.0, 4.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))   # above and in front of the four: outside the build-time root box
    move(scene.Bodies[0], *out)
    ref.set_pose(0, *out)
    stale = render(tracer)
    frame_equal(*stale, ref.render(), "stale tree")
    scene.Build()                     # same bodies: xrt_scene_build_tree
    ref.build_tree()
    rebuilt = render(tracer)
    frame_equal(*rebuilt, ref.render(), "new tree")
    assert not np.array_equal(stale[0], rebuilt[0])   # (the sphere appeared)
    _, fresh_tracer = xrt.configs.build_product(moved(spec, {0: out}))
    frame_equal(*rebuilt, render(fresh_tracer), "fresh scene")


C3_MOVES = {0: ((-130.0, 10.0, -140.0), (0.3, 0.9, -0.4), (1.5, 0.6, 1.0)), 9: ((-90.0, 0.0, -100.0), (0.0, 2.0, 0.0), (1.0, 1.0, 1.0)),
            27: ((5.0, 3.0, -15.0), (1.0, 0.0, 0.5), (0.8, 0.8, 2.0)), 36: ((20.0, 0.0, 25.0), (0.0, 0.0, 0.0), (1.0, 0.0, 1.0)),
            63: ((140.0, -5.0, 140.0), (0.0, -0.5, 0.2), (2.0, 1.0, 1.0))}


@pytest.mark.parametrize("name", ["C3", "C2"])
def test_crates_moved_rotated_and_scaled(xrt, name):
    spec = xrt.configs.config(name, scale=0.08)
    moves = C3_MOVES if name == "C3" else {0: ((2.0, 1.0, -3.0), (0.4, 0.7, 0.1), (1.2, 0.8, 1.0))}
    scene, tracer = xrt.configs.build_product(spec)
    ref = PoseOracle(spec)
    for b, p in moves.items():
        move(scene.Bodies[b], *p)
        ref.set_pose(b, *p)
    frame_equal(*render(tracer), ref.render(), name)
    rng = np.random.default_rng(3)
    o = rng.normal(size=(4000, 3)) * 150.0
    d = rng.uniform(-60, 60, size=(4000, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([tracer.GeneratePrimaryRays(), xrt.rays_array(o.astype(np.float32), d.astype(np.float32))])
    msg = hits_equal(scene.IntersectBatch(rays), ref.intersect(rays))
    assert msg is None, msg


def test_pipelined_tickets_render_their_own_poses(xrt):
    import torch
    spec = xrt.configs.config("C3", scale=0.08)
    scene, tracer = xrt.configs.build_product(spec)
    ref0, ref1 = PoseOracle(spec), PoseOracle(spec)
    p1 = {b: p for b, p in C3_MOVES.items() if b != 36}
    for b, p in p1.items():
        ref1.set_pose(b, *p)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    f0, f1 = tracer.PrepareDevice(outs[0].data_ptr()), tracer.PrepareDevice(outs[1].data_ptr())
    t0 = f0.begin()                                  # pose 0
    for b, p in p1.items():
        move(scene.Bodies[b], *p)
    t1 = f1.begin()                                  # set_poses while ticket 0 is open, then pose 1
    f0.end(t0)
    f1.end(t1)
    frame_equal(outs[0].cpu().numpy().view(np.uint32), None, ref0.render(), "ticket of pose 0")
    frame_equal(outs[1].cpu().numpy().view(np.uint32), None, ref1.render(), "ticket of pose 1")


def test_video_loop_through_prepare_device(xrt):
    """The reference's video loop (Game1.cs:152-189, 343-361): the spheres on circles, one pose per frame, two frames in flight."""
    import torch
    spec = xrt.configs.default_game_scene(64, 64, max_reflections=3)
    scene, tracer = xrt.configs.build_product(spec)
    ref = PoseOracle(spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    want, open_ = [], {}
    space = 2.0 * np.pi / 4.0
    for k in range(8):
        rot = np.float32(0.1) * k
        poses = {i: ((float(np.sin(rot + i * space) * 10), 3.0, float(np.cos(rot + i * space) * 10)), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) for i in range(4)}
        for i, p in poses.items():
            move(scene.Bodies[i], *p)
            ref.set_pose(i, *p)
        want.append(ref.render()[0])
        slot = k % 2
        if slot in open_:
            kk, t = open_.pop(slot)
            fr[slot].end(t)
            frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (want[kk], None), "video frame %d" % kk)
        open_[slot] = (k, fr[slot].begin())
    for slot, (kk, t) in sorted(open_.items(), key=lambda x: x[1][0]):
        fr[slot].end(t)
        frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (want[kk], None), "video frame %d" % kk)


def _pose_tensors(spec, moves, device="cuda"):
    import torch
    ids = sorted(moves)
    w, iw, bb = zip(*(pose_arrays(spec, b, *moves[b]) for b in ids))
    return (torch.tensor(ids, dtype=torch.int32, device=device), torch.tensor(np.concatenate(w), device=device),
            torch.tensor(np.concatenate(iw), device=device), torch.tensor(np.concatenate(bb), device=device))


def test_set_poses_device_from_tensors_on_a_side_stream(xrt):
    import torch
    spec = xrt.configs.config("C3", scale=0.08)
    scene, tracer = xrt.configs.build_product(spec)
    _, host_tracer = xrt.configs.build_product(spec)
    ids, w, iw, bb = _pose_tensors(spec, C3_MOVES)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scene.SetPosesDevice(ids, w, iw, bb, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    hs = host_tracer.CurrentScene
    hs.SetPoses(ids.cpu().numpy(), w.cpu().numpy(), iw.cpu().numpy(), bb.cpu().numpy())
    frame_equal(*render(tracer), render(host_tracer), "device form vs host form")
    ref = PoseOracle(spec)
    for b, p in C3_MOVES.items():
        ref.set_pose(b, *p)
    frame_equal(*render(tracer), ref.render(), "device form vs checker")
    lib, abi = xrt.abi.lib(), xrt.abi
    assert lib.xrt_scene_set_poses_device(scene.handle, C.c_void_p(ids.data_ptr()), 1, C.c_void_p(w.data_ptr() + 4), C.c_void_p(iw.data_ptr()),
                                          C.c_void_p(bb.data_ptr()), None) == abi.XRT_E_INVALID_ARG
    # the poses set on the device are what the scene file and build_tree read
    scene.Build()
    frame_equal(*render(tracer), render(xrt.configs.build_product(moved(spec, C3_MOVES))[1]), "build_tree after the device form")


def test_cast_rays_after_a_pose_change(xrt):
    spec = xrt.configs.default_game_scene(32, 32, max_reflections=4)
    scene, tracer = xrt.configs.build_product(spec)
    ref = PoseOracle(spec)
    p = ((-6.0, 2.5, -4.0), (0.2, 0.0, 0.3), (1.3, 1.0, 0.8))
    move(scene.Bodies[2], *p)
    ref.set_pose(2, *p)
    rays = tracer.GeneratePrimaryRays()
    rgba, rgbf = tracer.CastRays(rays, want_float=True)
    o_rgba, o_rgbf = ref.cast_rays(rays)
    assert np.array_equal(rgba, o_rgba)
    assert np.array_equal(_bits(rgbf), _bits(o_rgbf))


def test_replicas_render_the_moved_poses(xrt, monkeypatch):
    monkeypatch.setenv("XRT_FAKE_GPUS", "1")
    spec = xrt.configs.crate_grid_scene(200, 120)
    scene, tracer = xrt.configs.build_product(spec)
    tracer.NumGpus = 2
    tracer.Render()                      # (the replicas exist before the move)
    tracer.NumGpus = 1
    for b, p in C3_MOVES.items():
        move(scene.Bodies[b], *p)
    want = tracer.Render().copy()
    for n in (2, 3):
        tracer.NumGpus = n
        got = tracer.Render().copy()
        assert np.array_equal(got, want), "n_gpus %d" % n
    tracer.NumGpus = 1


def test_save_load_build_after_set_poses(xrt, tmp_path):
    spec = xrt.configs.config("C3", scale=0.08)
    scene, tracer = xrt.configs.build_product(spec)
    for b, p in C3_MOVES.items():
        move(scene.Bodies[b], *p)
    tracer.Render()                      # (pushes the poses)
    scene.Save(tmp_path / "moved.xrts")
    loaded = xrt.api.OctreeSpatialManager.Load(tmp_path / "moved.xrts")
    tracer.CurrentScene = loaded
    got = render(tracer)
    _, fresh = xrt.configs.build_product(moved(spec, C3_MOVES))
    frame_equal(*got, render(fresh), "loaded")


def test_build_tree_while_a_ticket_is_open_is_busy(xrt):
    spec = xrt.configs.config("C3", scale=0.05)
    scene, tracer = xrt.configs.build_product(spec)
    host = np.zeros(spec.width * spec.height, dtype=np.uint32)
    fr = tracer.PrepareHost(host)
    t = fr.begin()
    assert xrt.abi.lib().xrt_scene_build_tree(scene.handle, 0) == xrt.abi.XRT_E_BUSY
    fr.end(t)
    assert xrt.abi.lib().xrt_scene_build_tree(scene.handle, 0) == xrt.abi.XRT_OK


def test_python_position_after_build_changes_the_next_frame(xrt):
    spec = xrt.configs.crate_scene(64, 48, max_reflections=2)
    scene, tracer = xrt.configs.build_product(spec)
    before = render(tracer)
    scene.Bodies[0].Position = (3.0, 2.0, -4.0)
    ref = PoseOracle(spec)
    ref.set_pose(0, (3.0, 2.0, -4.0), (0.0, 0.0, 0.0))
    after = render(tracer)
    assert not np.array_equal(before[0], after[0])
    frame_equal(*after, ref.render(), "Position setter")
