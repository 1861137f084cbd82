"""The table of screen boxes of a camera frame's primary packets (csrc/screen_rects.h, XRT_PK_SCREEN): in a one-body scene, k_screen_rects writes
every frame one entry per leaf reference -- the screen box outside which no primary ray of the frame can be accepted by the reference's triangle --
and launch #0 of k_packet gives no triangle step to a triangle whose entry misses the packet's screen rectangle.

Nothing a caller can see may change.  For every case the frame with the switch on, the frame with it off and the oracle are equal bit for bit, with
equal ray statistics where the oracle's mirror reports them; the table the device wrote
(xrt_debug_screen_table) equals the host's evaluation of the same functions word for word; with the switch off, and for a viewport the fields cannot
hold, there is no table.  fixtures.heightfield(64) at 96x54 with 16 samples unless a case says otherwise."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 96, 54
BENCH = ((0, 60, 110), (0, 0, 0))
GRAZING = ((0, 4.2, 70), (0, 0, 0))          # just above the terrain (y in [-4, 4]), looking along it
INSIDE = ((5, 1.5, 10), (-20, 0, -30))       # inside the mesh's box: triangles behind the eye and across the near plane
OTHER = ((40, 50, 90), (-10, 0, 10))
NO_CULL = 0xFFFFFFFF


def spec_of(xrt, cam=BENCH, ms=None, size=(W, H), body=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), near=1.0):
    s = xrt.configs.SceneSpec("heightfield_m64")
    s.meshes.append((xrt.fixtures.heightfield(64), xrt.configs.material(0.3)))
    s.objects.append(([0],) + tuple(body))
    s.lights = [xrt.configs.spot((0.0, 120.0, 160.0))]
    s.max_reflections = 1
    s.multisampling, s.multisample_quality = (xrt.abi.MS_FIXED16 if ms is None else ms), 0
    s.camera = xrt.configs.camera(cam[0], cam[1], near=near)
    return s.with_size(*size)


def build(xrt, monkeypatch, spec, env):
    with monkeypatch.context() as m:   # (xrt_scene_create reads the switches)
        for k, v in env.items():
            m.setenv(k, v)
        return xrt.configs.build_product(copy.deepcopy(spec))


_ORACLE = {}


def oracle(orc, key, spec):
    if key not in _ORACLE:
        rgba, _, st = orc.OracleScene(copy.deepcopy(spec)).render(nthreads=8, want_float=False)
        rgba.setflags(write=False)
        _ORACLE[key] = (rgba, st)
    return _ORACLE[key]


def check_tables(scene, expect, what):
    """The device's table against the host's evaluation; returns the share of entries that cull."""
    dev = scene.ScreenTable()
    if not expect:
        assert dev.shape[0] == 0, (what, "a table where none is expected", dev.shape)
        return 0.0
    assert dev.shape[0] > 0, (what, "launch #0 took no table")
    host = scene.ScreenTable(host_eval=True)
    assert np.array_equal(dev, host), (what, "%d entries differ from the host's" % int((dev != host).any(axis=1).sum()))
    culls = dev[:, 0] != NO_CULL
    c = dev[culls]
    assert np.all((c[:, 0] & 0xFFFF) <= (c[:, 0] >> 16)) and np.all((c[:, 1] & 0xFFFF) <= (c[:, 1] >> 16)), (what, "an entry with x0 > x1 or y0 > y1")
    return float(culls.mean())


STAT_KEYS = ("rays_closest", "rays_shadow", "rays_traversed", "shaded_hits", "pixels")

CASES = {
    # name: (spec arguments, environment, smallest share of culling entries expected)
    "bench": (dict(), {}, 0.9),
    "grazing": (dict(cam=GRAZING), {}, 0.0),
    "eye_inside": (dict(cam=INSIDE, near=0.5), {}, 0.0),
    "transformed_body": (dict(body=((3.0, -2.0, 5.0), (0.3, 0.5, 0.2), (1.5, 0.6, 2.0))), {}, 0.5),
    "adaptive_level0": (dict(ms="adaptive"), {"XRT_PACKET": "1"}, 0.9),
    "one_sample": (dict(ms="off"), {"XRT_PACKET": "1"}, 0.9),
}


def case_spec(xrt, kw):
    kw = dict(kw)
    if kw.get("ms") == "adaptive":
        kw["ms"] = xrt.abi.MS_ADAPTIVE
    elif kw.get("ms") == "off":
        kw["ms"] = xrt.abi.MS_OFF
    return spec_of(xrt, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_on_off_oracle(xrt, orc, monkeypatch, name):
    kw, env, min_share = CASES[name]
    spec = case_spec(xrt, kw)
    o_rgba, o_st = oracle(orc, name, spec)
    assert float(((o_rgba & 0xffffff) != 0).mean()) > 0.01, "the camera should see the terrain"
    seen = {}
    for on in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, dict(env, XRT_PK_SCREEN=on))
        for rep in range(2):
            rgba = tracer.Render().copy()
            assert np.array_equal(rgba, o_rgba), (name, on, rep, "%d RGBA8 pixels differ from the oracle" % int((rgba != o_rgba).sum()))
            for k in ("rays_closest", "rays_shadow"):
                assert tracer.last_stats[k] == o_st[k], (name, on, k, tracer.last_stats[k], o_st[k])
        share = check_tables(scene, on == "1", (name, on))
        if on == "1":
            print("screen table", name, "share of culling entries %.3f" % share)
            assert share >= min_share, (name, share)
        seen[on] = (rgba, {k: tracer.last_stats[k] for k in STAT_KEYS})
    assert np.array_equal(seen["1"][0], seen["0"][0]) and seen["1"][1] == seen["0"][1]


def test_offset_viewport(xrt, orc, monkeypatch):
    """A viewport that does not start at (0, 0): the frame looks at a shifted window of the projection.  The reference is the oracle's frame with the same
    viewport origin (tests/pixels_py.oracle_frame: the oracle takes vp_x / vp_y, its Python mirror pins them to 0)."""
    import pixels_py
    spec = spec_of(xrt)
    vp = (-29, 11)
    want = np.asarray(pixels_py.oracle_frame(orc, orc.OracleScene(copy.deepcopy(spec)), spec, vp=vp)[0]).reshape(-1)
    assert 0.01 < float(((want & 0xffffff) != 0).mean())
    assert not np.array_equal(want, oracle(orc, "bench", spec)[0].reshape(-1))
    for on in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, {"XRT_PK_SCREEN": on})
        plain = tracer._camera_abi

        def shifted(plain=plain):
            cam = plain()
            cam.vp_x, cam.vp_y = vp
            return cam
        tracer._camera_abi = shifted
        for rep in range(2):
            got = tracer.Render().copy().reshape(-1)
            assert np.array_equal(got, want), (on, rep, "%d RGBA8 pixels differ from the oracle" % int((got != want).sum()))
        share = check_tables(scene, on == "1", ("offset viewport", on))
        if on == "1":
            assert share > 0.9


def test_shard_one_of_three(xrt, orc, monkeypatch):
    import torch
    spec = spec_of(xrt)
    o_rgba, _ = oracle(orc, "bench", spec)
    tx, ty, tpr = xrt.dist.shard_layout(W, H, 3)
    n = tpr * 512
    for on in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec, {"XRT_PK_SCREEN": on})
        gathered = torch.full((3 * n,), 0x55, dtype=torch.int32, device="cuda")
        for rank in (0, 2, 1):
            tracer.RenderDevice(gathered[rank * n:(rank + 1) * n].data_ptr(), shard_rank=rank, shard_count=3)
        check_tables(scene, on == "1", ("shard 1 of 3", on))   # shard 1: the last one rendered
        out = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        xrt.dist.detile_device(gathered, W, H, 3, out)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32).reshape(o_rgba.shape)
        assert np.array_equal(got, o_rgba), (on, int((got != o_rgba).sum()))


def test_two_cameras_in_flight(xrt, orc, monkeypatch):
    """Two frames in flight with two different cameras, alternating: every frame context has the table of its own camera."""
    import torch
    specs = [spec_of(xrt), spec_of(xrt, cam=OTHER)]
    want = [oracle(orc, "bench", specs[0])[0], oracle(orc, "other", specs[1])[0]]
    assert not np.array_equal(want[0], want[1])
    for on in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, specs[0], {"XRT_PK_SCREEN": on})
        outs = [torch.zeros(W * H, dtype=torch.int32, device="cuda") for _ in range(2)]
        frames = []
        for i in range(2):
            c = specs[i].camera
            tracer.CurrentCamera = xrt.Camera(c["pos"], c["target"], c["up"], c["fov"], xrt.xna.aspect_ratio(W, H), c["near"], c["far"])
            frames.append(tracer.PrepareDevice(outs[i].data_ptr()))   # (the camera is marshalled here)
        tickets = [None, None]
        for f in range(5):
            cur = f & 1
            if f < 4:
                tickets[cur] = frames[cur].begin()
            if f >= 1:
                prv = cur ^ 1
                frames[prv].end(tickets[prv])
                torch.cuda.synchronize()
                got = outs[prv].cpu().numpy().view(np.uint32).reshape(want[prv].shape)
                assert np.array_equal(got, want[prv]), (on, "in flight", f, int((got != want[prv]).sum()))
                outs[prv].zero_()
                torch.cuda.synchronize()
        check_tables(scene, on == "1", ("two in flight", on))


def test_pose_change_between_frames(xrt, orc, monkeypatch):
    """The body moves between two frames (SceneObject.Position / Rotation / Scale -> xrt_scene_set_poses): the second frame's table is made from the new pose.
    The reference is the oracle with the moved body under the scene octree of the build (tests/poses: the reference's game loop does not rebuild it)."""
    from poses_py import PoseOracle
    moved = ((3.0, -2.0, 5.0), (0.3, 0.5, 0.2), (1.5, 0.6, 2.0))
    spec0 = spec_of(xrt)
    want0 = oracle(orc, "bench", spec0)[0]
    ref = PoseOracle(copy.deepcopy(spec0))
    ref.set_pose(0, *moved)
    want1 = np.asarray(ref.render()[0]).reshape(-1)
    assert not np.array_equal(want0.reshape(-1), want1)
    for on in ("1", "0"):
        scene, tracer = build(xrt, monkeypatch, spec0, {"XRT_PK_SCREEN": on})
        assert np.array_equal(tracer.Render(), want0)
        first = scene.ScreenTable()
        body = scene.Bodies[0]
        body.Position, body.Rotation, body.Scale = moved
        got = tracer.Render().copy().reshape(-1)
        assert np.array_equal(got, want1), (on, int((got != want1).sum()))
        check_tables(scene, on == "1", ("pose change", on))
        if on == "1":
            assert not np.array_equal(first, scene.ScreenTable())


def test_viewport_too_wide_for_the_fields(xrt, orc, monkeypatch):
    """4100 pixels do not fit the 16-bit fields (sixteenths of a pixel): the frame takes no table and today's path."""
    spec = spec_of(xrt, size=(4100, 8))
    o_rgba, _ = oracle(orc, "wide", spec)
    scene, tracer = build(xrt, monkeypatch, spec, {"XRT_PK_SCREEN": "1"})
    got = tracer.Render().copy()
    assert np.array_equal(got, o_rgba), int((got != o_rgba).sum())
    check_tables(scene, False, "wide")
