"""k_shade finishes a hit in part A when none of its shadow rays has to be emitted (kernels.h ShadeArgs::finish, XRT_AE_FINISH): such a hit takes
no slot, writes no slot record and no shadow words, and forms its light sum at once instead of in part B of the next step.  Nothing a caller can
see may change: every case renders with the switch on and off (xrt_scene_create reads it, so one scene per setting) and requires the RGBA8 frame
and the fp32 colour vectors to be bit-equal to each other and to the oracle, and xrt_stats to be equal field by field.

The path needs `answered at emission` (ShadeArgs::ae): a scene of one body with one mesh whose surface normals all lie on one side of a
coordinate plane.  tilted_soup() is such a mesh with mixed facings inside that half space; which hits finish is then a matter of where the
lights are.  How many shadow queries part A answered is xrt_stats.rays_traversed with XRT_AE=0 minus the same with XRT_AE=1 (MaxReflections 0:
no reflections among them), which is how the cases check that they exercise what their names say.

What these tests cannot see is whether the path engages: a finished hit changes nothing a caller can read, xrt_stats included (that is the
point of it), and the library exports no other counter.  A host condition that left ShadeArgs::finish off would pass this file; that the path runs
shows only in a kernel trace (the k_shade<true> instantiation) or in a `make DEV=1` build's XRT_FINISH_COUNTS=1 print, both recorded under
profiles/shade_finish."""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNTS = ("rays_closest", "rays_shadow", "shaded_hits", "pixels")   # what the oracle accounts for without its counting pass


def tilted_soup(xrt, n, seed, size=0.5, slope=0.5):
    """n small triangles in [-1,1]^3, every one tilted out of the horizontal by random slopes in [-slope, slope] along x and z and wound so that
    its surface normal points up: facings mixed, but the mesh's normal box stays clear of y = 0."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, size=(n, 1, 3))
    xz = rng.uniform(-size, size, size=(n, 3, 2))
    a, b = rng.uniform(-slope, slope, size=(n, 1)), rng.uniform(-slope, slope, size=(n, 1))
    v = np.stack([c[:, :, 0] + xz[:, :, 0], c[:, :, 1] + a * xz[:, :, 0] + b * xz[:, :, 1], c[:, :, 2] + xz[:, :, 1]], axis=2).astype(np.float32)
    down = xrt.fixtures.surface_normals(v)[:, 1] < 0
    v[down] = v[down][:, [0, 2, 1]]
    md = xrt.fixtures.MeshData(v, np.zeros((n, 3, 3), dtype=np.float32), rng.uniform(0, 1, size=(n, 3, 2)).astype(np.float32),
                               rng.uniform(0, 1, size=(n, 4)).astype(np.float32))
    assert (md.surface_normal[:, 1] > 0).all()
    md.n = np.repeat(md.surface_normal[:, None, :], 3, axis=1).copy()
    return md


def soup_spec(xrt, lights, n=60, seed=3, R=2):
    s = xrt.configs.SceneSpec("tilted_soup")
    s.meshes.append((tilted_soup(xrt, n, seed), xrt.configs.material(0.5)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera((0, 3, 3), (0, 0, 0))
    s.lights = lights
    s.mesh_threshold = 2
    s.max_reflections = R
    return s.with_size(64, 64)


NEAR_ABOVE = (0.5, 0.8, 0.0)    # inside the soup's box: the way to it is steep from the hits below it and flat from the hits at the rim
FAR_ABOVE = (0.0, 60.0, 0.0)    # every hit sees it straight above: always answered
LOW_ASIDE = (4.0, 0.05, 0.0)    # the way to it is nearly horizontal: never answered


def build(xrt, monkeypatch, spec, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return xrt.configs.build_product(copy.deepcopy(spec))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def both(xrt, monkeypatch, spec):
    """(scene, tracer) with the switch on and off"""
    return [build(xrt, monkeypatch, spec, {"XRT_AE_FINISH": f}) for f in ("1", "0")]


def same_stats(a, b):
    return {k: (a[k], b[k]) for k in a if not k.startswith("ms_") and a[k] != b[k]}


def frames_equal(rgba, rgbf, o_rgba, o_rgbf):
    assert np.array_equal(rgba, o_rgba), "%d RGBA8 pixels differ" % int((rgba != o_rgba).sum())
    assert np.array_equal(rgbf.view(np.uint32), o_rgbf.view(np.uint32)), "fp32 colour vectors not bit-identical"


def check_on_off_oracle(xrt, orc, monkeypatch, spec):
    """Blocking frames with the switch on and off: both equal to the oracle, stats equal to each other and to the oracle's accounting."""
    o_rgba, o_rgbf, o_st = orc.OracleScene(spec).render(nthreads=8)
    got = []
    for scene, tracer in both(xrt, monkeypatch, spec):
        rgba, rgbf = tracer.Render(want_float=True)
        frames_equal(rgba, rgbf, o_rgba, o_rgbf)
        for k in COUNTS:
            assert tracer.last_stats[k] == o_st[k], (k, tracer.last_stats[k], o_st[k])
        got.append((rgba.copy(), rgbf.copy(), dict(tracer.last_stats)))
    frames_equal(got[0][0], got[0][1], got[1][0], got[1][1])
    assert same_stats(got[0][2], got[1][2]) == {}
    return o_rgba, o_rgbf, o_st


def answered_at_emission(xrt, monkeypatch, spec):
    """(shadow queries part A answers, shaded hits) of the generation-0 hits of `spec`"""
    s0 = copy.deepcopy(spec)
    s0.max_reflections = 0
    st = []
    for ae in ("0", "1"):
        scene, tracer = build(xrt, monkeypatch, s0, {"XRT_AE": ae})
        tracer.Render()
        st.append(dict(tracer.last_stats))
    assert st[0]["shaded_hits"] == st[1]["shaded_hits"]
    return st[0]["rays_traversed"] - st[1]["rays_traversed"], st[0]["shaded_hits"]


def test_mixed_wave(xrt, orc, monkeypatch):
    """One spot light among the triangles: in most waves some hits finish and others emit their shadow ray.  Then again under XRT_GUARD=1
    (every work buffer ends in a checked pattern: a slot or a shadow word written for a hit that took no slot would land outside)."""
    spec = soup_spec(xrt, [xrt.configs.spot(NEAR_ABOVE)])
    answered, hits = answered_at_emission(xrt, monkeypatch, spec)
    assert hits > 500 and hits // 10 < answered < hits - hits // 10, (answered, hits)
    check_on_off_oracle(xrt, orc, monkeypatch, spec)
    monkeypatch.setenv("XRT_GUARD", "1")
    try:
        check_on_off_oracle(xrt, orc, monkeypatch, spec)
    finally:
        monkeypatch.setenv("XRT_GUARD", "0")
        xrt.configs.build_product(xrt.configs.crate_scene(32, 32, 0))   # (xrt_scene_create reads the switch: guards off for the tests that follow)
        monkeypatch.delenv("XRT_GUARD")


def test_two_lights_one_answered(xrt, orc, monkeypatch):
    """A light every hit sees straight above and one whose shadow ray is always emitted: every hit has one answer and one ray, none may finish.
    And with the near light in place of the far one: hits with one, and hits with no answered light side by side."""
    spec = soup_spec(xrt, [xrt.configs.spot(FAR_ABOVE), xrt.configs.spot(LOW_ASIDE)])
    answered, hits = answered_at_emission(xrt, monkeypatch, spec)
    assert hits > 500 and answered == hits, (answered, hits)   # one of the two queries of every hit
    check_on_off_oracle(xrt, orc, monkeypatch, spec)
    check_on_off_oracle(xrt, orc, monkeypatch, soup_spec(xrt, [xrt.configs.spot(LOW_ASIDE), xrt.configs.spot(NEAR_ABOVE)]))


def test_every_hit_finishes(xrt, orc, monkeypatch):
    """The m=224 terrain at 48x27 with 16 sub-rays, the fixture frame (golden) and the same lit from straight above, where every shadow query of
    generation 0 is answered at emission: no slot is taken at all, part B has nothing to do."""
    spec = xrt.configs.heightfield_scene(48, 27, m=224, multisampling=xrt.abi.MS_FIXED16)
    o_rgba, _, _ = check_on_off_oracle(xrt, orc, monkeypatch, spec)
    assert np.array_equal(o_rgba, np.load(os.path.join(GOLDEN, "h224_48x27_ms16_rgba.npy")))
    above = copy.deepcopy(spec)
    above.lights = [xrt.configs.spot((0.0, 5000.0, 0.0))]
    answered, hits = answered_at_emission(xrt, monkeypatch, above)
    assert hits > 0 and answered == hits, (answered, hits)
    check_on_off_oracle(xrt, orc, monkeypatch, above)


def test_no_lights(xrt, orc, monkeypatch):
    """nLights == 0: every hit is finished, with a light sum of zero."""
    check_on_off_oracle(xrt, orc, monkeypatch, soup_spec(xrt, []))


def test_blocking_and_two_in_flight(xrt, orc, monkeypatch):
    """The mixed frame blocking, then eight frames with two in flight on two render objects: every frame is compared, and so are its counters."""
    import torch
    spec = soup_spec(xrt, [xrt.configs.spot(NEAR_ABOVE)])
    o_rgba, o_rgbf, o_st = check_on_off_oracle(xrt, orc, monkeypatch, spec)
    stats = []
    for scene, tracer in both(xrt, monkeypatch, spec):
        outs = [torch.zeros(spec.width * spec.height, dtype=torch.int32, device="cuda") for _ in range(2)]
        frs = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
        tickets = [None, None]
        mine = []
        for f in range(8 + 1):
            cur = f & 1
            if f >= 1:   # the frame begun one step ago is still open while this one is enqueued
                prv = cur ^ 1
                if f < 8:
                    tickets[cur] = frs[cur].begin()
                st = frs[prv].end(tickets[prv])
                torch.cuda.synchronize()
                assert np.array_equal(outs[prv].cpu().numpy().view(np.uint32), o_rgba), f
                for k in COUNTS:
                    assert st[k] == o_st[k], (f, k, st[k], o_st[k])
                mine.append(dict(st))
                outs[prv].zero_()
                torch.cuda.synchronize()   # (the next frame into this buffer runs on the library's own stream)
            else:
                tickets[cur] = frs[cur].begin()
        stats.append(mine)
    for a, b in zip(*stats):
        assert same_stats(a, b) == {}


def test_ray_tree_frame_does_not_engage(xrt, orc, monkeypatch):
    """Transparent materials (the glass spheres at 64x64): a ray-tree frame keeps every hit's slot; same results and counters either way."""
    check_on_off_oracle(xrt, orc, monkeypatch, xrt.configs.default_game_scene(64, 64, 4))


def test_cast_rays_paths_unchanged(xrt, monkeypatch):
    """xrt_cast_rays_paths takes every hit's position from its slot record: the pass keeps the slots.  The soup's primary rays, switch on and off."""
    spec = soup_spec(xrt, [xrt.configs.spot(NEAR_ABOVE)])
    got = []
    for scene, tracer in both(xrt, monkeypatch, spec):
        rays = tracer.GeneratePrimaryRays()
        plain = tracer.CastRays(rays, want_float=True)
        st_plain = dict(tracer.last_stats)
        rgba, rgbf, vertices, vstart, back = tracer.CastRays(rays, want_float=True, paths=True)
        frames_equal(plain[0], plain[1], rgba, rgbf)   # (the pass without paths may finish hits in part A, the one with paths may not)
        got.append((rgba, rgbf, vertices, vstart, back, st_plain, dict(tracer.last_stats)))
    on, off = got
    frames_equal(on[0], on[1], off[0], off[1])
    assert on[2].tobytes() == off[2].tobytes() and len(on[2]) > 0
    assert np.array_equal(on[3], off[3]) and on[4].tobytes() == off[4].tobytes()
    assert same_stats(on[5], off[5]) == {} and same_stats(on[6], off[6]) == {}


def test_adaptive_frame_unchanged(xrt, orc, monkeypatch):
    """An adaptive-supersampling frame (RT:170-311) at 64x64: its passes are not answered at emission, so nothing finishes in part A."""
    spec = xrt.configs.heightfield_scene(64, 64, m=48, multisampling=xrt.abi.MS_ADAPTIVE)
    spec.multisample_quality = 2
    check_on_off_oracle(xrt, orc, monkeypatch, spec)
