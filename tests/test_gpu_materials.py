"""xrt_scene_set_materials on the MI355X: frames and ray batches of scenes whose materials change between frames, bit for bit (RGBA8 words
and the uint32 view of the fp32 colour vectors) against the oracle of the spec with the new material dicts -- the frame the reference
renders after Material's setters ran.  Scalars, the switch between the plain and the ray-tree pipeline in both directions, the depth limit
that follows it, textures replaced / switched off / brought back, tickets that render their own materials, a pipelined loop, ray batches
and their paths, replicas, the scene file, and seam 1, which must not notice."""
import numpy as np
import pytest

from materials_py import gen_texture, with_materials
from poses_py import hits_equal

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle(orc, spec):
    rgba, rgbf, _ = orc.OracleScene(spec).render(nthreads=16)
    return rgba, rgbf


def frame_equal(got_rgba, got_f, want, what):
    rgba, rgbf = want
    bad = int((np.asarray(got_rgba).reshape(-1) != rgba).sum())
    assert bad == 0, "%s: %d of %d pixels differ" % (what, bad, rgba.size)
    if got_f is not None:
        assert np.array_equal(_bits(got_f).reshape(-1), _bits(rgbf).reshape(-1)), what


def render(tracer):
    rgba, rgbf = tracer.Render(want_float=True)
    return rgba.copy(), rgbf.copy()


def apply(scene, changes):
    """The material dict changes of with_materials, made through the mirror's Material properties."""
    names = dict(reflectiveness="Reflectiveness", transparent="Transparent", refraction_index="RefractionIndex", interpolate_normals="InterpolateNormals",
                 use_texture="UseTexture", texture="Texture", texture_pargb="TexturePArgb")
    for m, ch in changes.items():
        mat = scene.meshes[m].MeshMaterial
        if "texture" in ch and "texture_pargb" not in ch:
            mat.TexturePArgb = None
        for k, v in ch.items():
            setattr(mat, names[k], v)
        if "texture" in ch and "use_texture" not in ch:
            mat.UseTexture = ch["texture"] is not None


def test_scalars_on_the_reference_content(xrt, orc):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)   # 0 plane, 1 monkey, 2 torus, 3 sphere, 4 cube
    scene, tracer = xrt.configs.build_product(spec)
    f0 = render(tracer)
    ch1 = {2: dict(reflectiveness=0.2), 4: dict(interpolate_normals=False)}
    apply(scene, ch1)
    s1 = with_materials(spec, ch1)
    f1 = render(tracer)
    frame_equal(*f1, oracle(orc, s1), "torus reflectiveness, cube flat normals")
    assert not np.array_equal(f0[0], f1[0])
    ch2 = {1: dict(refraction_index=float(np.float32(1.1)))}
    apply(scene, ch2)
    f2 = render(tracer)
    frame_equal(*f2, oracle(orc, with_materials(s1, ch2)), "monkey refraction index")
    assert not np.array_equal(f1[0], f2[0])


def test_pipeline_switch_both_ways(xrt, orc):
    spec = xrt.configs.default_game_scene(64, 64, max_reflections=4)
    scene, tracer = xrt.configs.build_product(spec)
    first = render(tracer)
    frame_equal(*first, oracle(orc, spec), "glass spheres")
    opaque = with_materials(spec, {0: dict(transparent=False)})
    apply(scene, {0: dict(transparent=False)})
    got = render(tracer)
    frame_equal(*got, oracle(orc, opaque), "spheres turned opaque")
    frame_equal(*got, render(xrt.configs.build_product(opaque)[1]), "spheres turned opaque vs a scene built opaque")
    assert not np.array_equal(got[0], first[0])
    apply(scene, {0: dict(transparent=True)})
    frame_equal(*render(tracer), first, "glass again")
    # the reference's content: both glass meshes opaque -- no Transparent material is left --, then one of them glass again
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = xrt.configs.build_product(spec)
    none = {1: dict(transparent=False), 3: dict(transparent=False)}
    apply(scene, none)
    frame_equal(*render(tracer), oracle(orc, with_materials(spec, none)), "no Transparent material left")
    one = {1: dict(transparent=False), 3: dict(transparent=True)}
    apply(scene, one)
    frame_equal(*render(tracer), oracle(orc, with_materials(spec, one)), "only the sphere is glass")


def test_the_depth_limit_follows_the_flag(xrt, orc):
    spec = with_materials(xrt.configs.default_game_scene(32, 32, max_reflections=13), {0: dict(transparent=False)})
    scene, tracer = xrt.configs.build_product(spec)
    first = render(tracer)
    frame_equal(*first, oracle(orc, spec), "opaque, MaxReflections 13")
    apply(scene, {0: dict(transparent=True)})
    with pytest.raises(xrt.abi.XrtError) as e:
        tracer.Render()
    assert e.value.code == xrt.abi.XRT_E_UNSUPPORTED
    apply(scene, {0: dict(transparent=False)})
    frame_equal(*render(tracer), first, "opaque again")


@pytest.mark.parametrize("filtering", ["point", "bilinear"])
def test_textures_replaced_switched_off_and_brought_back(xrt, orc, filtering):
    spec = xrt.configs.crate_scene(64, 48, 2)
    spec.filtering = xrt.abi.FILTER_POINT if filtering == "point" else xrt.abi.FILTER_BILINEAR
    scene, tracer = xrt.configs.build_product(spec)
    before = render(tracer)
    argb, pargb = gen_texture(5, 3, 11)   # another size, non-square, with alpha and its premultiplied copy
    ch = {0: dict(texture=argb, texture_pargb=pargb)}
    apply(scene, ch)
    textured = render(tracer)
    frame_equal(*textured, oracle(orc, with_materials(spec, ch)), "texture replaced")
    assert not np.array_equal(textured[0], before[0])
    apply(scene, {0: dict(use_texture=False)})
    plain = render(tracer)
    frame_equal(*plain, oracle(orc, with_materials(spec, {0: dict(use_texture=False, texture=None)})), "use_texture off: the triangle colours")
    assert not np.array_equal(plain[0], textured[0])
    sent = scene._pushed_tex[0]
    apply(scene, {0: dict(use_texture=True)})
    frame_equal(*render(tracer), textured, "use_texture on again, no texels given")
    assert scene._pushed_tex[0] == sent   # (the mirror sent NULL texels: the library kept them)


def _two_tickets(xrt, orc, spec, changes):
    import torch
    scene, tracer = xrt.configs.build_product(spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    f0, f1 = tracer.PrepareDevice(outs[0].data_ptr()), tracer.PrepareDevice(outs[1].data_ptr())
    t0 = f0.begin()                                  # the materials as built
    apply(scene, changes)
    t1 = f1.begin()                                  # set_materials while ticket 0 is open, then the new materials
    f0.end(t0)
    f1.end(t1)
    frame_equal(outs[0].cpu().numpy().view(np.uint32), None, oracle(orc, spec), "ticket of the old materials")
    frame_equal(outs[1].cpu().numpy().view(np.uint32), None, oracle(orc, with_materials(spec, changes)), "ticket of the new materials")
    assert not np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy())


def test_pipelined_tickets_render_their_own_materials(xrt, orc):
    argb, _ = gen_texture(37, 21, 5, alpha=False)
    _two_tickets(xrt, orc, xrt.configs.config("C3", scale=0.08), {0: dict(reflectiveness=0.125, texture=argb)})


def test_pipelined_tickets_take_their_own_pipeline(xrt, orc):
    _two_tickets(xrt, orc, xrt.configs.default_game_scene(64, 64, 3), {0: dict(transparent=False)})


def test_two_tickets_opened_after_one_update_both_render_it(xrt, orc):
    """One update, then two tickets: the first frame that reads the new version puts its copies on its own stream, the second -- on another
    stream, with a megabyte of texels on its way -- has to wait for them."""
    import torch
    spec = xrt.configs.config("C3", scale=0.08)
    scene, tracer = xrt.configs.build_product(spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    for k in range(4):                                # (frames in flight before the update, so that the tickets are on streams of their own)
        fr[k % 2].end(fr[k % 2].begin())
    h, w = spec.meshes[0][1]["texture"].shape
    ch = {0: dict(reflectiveness=0.75, texture=gen_texture(w, h, 31, alpha=False)[0])}
    apply(scene, ch)
    t0 = fr[0].begin()
    t1 = fr[1].begin()
    fr[0].end(t0)
    fr[1].end(t1)
    want = oracle(orc, with_materials(spec, ch))
    for k in range(2):
        frame_equal(outs[k].cpu().numpy().view(np.uint32), None, want, "ticket %d" % k)


def _loop(xrt, orc, spec, frames):
    """frames: one material change of mesh 0 per frame.  Two frames in flight; every frame against the oracle of its own materials."""
    import torch
    scene, tracer = xrt.configs.build_product(spec)
    px = spec.width * spec.height
    outs = [torch.zeros(px, dtype=torch.int32, device="cuda") for _ in range(2)]
    fr = [tracer.PrepareDevice(o.data_ptr()) for o in outs]
    want, open_, cache, cur = [], {}, {}, spec
    for k, (key, ch) in enumerate(frames):
        apply(scene, {0: ch})
        cur = with_materials(cur, {0: ch})
        if key not in cache:
            cache[key] = oracle(orc, cur)[0]
        want.append(cache[key])
        slot = k % 2
        if slot in open_:
            kk, t = open_.pop(slot)
            fr[slot].end(t)
            frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (want[kk], None), "frame %d" % kk)
        open_[slot] = (k, fr[slot].begin())
    for slot, (kk, t) in sorted(open_.items(), key=lambda x: x[1][0]):
        fr[slot].end(t)
        frame_equal(outs[slot].cpu().numpy().view(np.uint32), None, (want[kk], None), "frame %d" % kk)
    assert len({w.tobytes() for w in want}) == len(cache) > 1


REFLECTIVENESS = (0.1, 0.9, 0.5, 0.3)


def test_a_loop_of_reflectiveness_with_two_frames_in_flight(xrt, orc):
    frames = [(REFLECTIVENESS[k % 4], dict(reflectiveness=REFLECTIVENESS[k % 4])) for k in range(12)]
    _loop(xrt, orc, xrt.configs.default_game_scene(48, 48, 3), frames)


def test_a_loop_that_replaces_a_texture_of_the_same_size(xrt, orc):
    spec = xrt.configs.crate_scene(48, 36, 1)
    h, w = spec.meshes[0][1]["texture"].shape
    tex = [gen_texture(w, h, 20 + i, alpha=False)[0] for i in range(2)]
    frames, t = [], -1
    for k in range(12):
        ch = dict(reflectiveness=REFLECTIVENESS[k % 2])
        if k % 3 == 0:
            t += 1
            ch["texture"] = tex[t % 2]
        frames.append(((k % 2, t % 2), ch))
    _loop(xrt, orc, spec, frames)


def test_cast_rays_after_a_change(xrt):
    import castray_py
    import paths_py
    spec = xrt.configs.default_game_scene(32, 32, max_reflections=4)
    scene, tracer = xrt.configs.build_product(spec)
    rays = tracer.GeneratePrimaryRays()
    ch = {0: dict(reflectiveness=0.25, refraction_index=float(np.float32(1.5)))}
    apply(scene, ch)
    rgba, rgbf = tracer.CastRays(rays, want_float=True)
    o_rgba, o_rgbf, _ = castray_py.CastRayScene(with_materials(spec, ch)).cast_rays(rays)
    assert np.array_equal(rgba, o_rgba) and np.array_equal(_bits(rgbf), _bits(o_rgbf))
    glass = tracer.CastRays(rays, paths=True)
    assert (glass[1]["color"] == paths_py.RED).any()           # (refraction segments while the spheres are glass)
    ch[0]["transparent"] = False
    apply(scene, ch)
    rgba, rgbf, vertices, vstart, back = tracer.CastRays(rays, want_float=True, paths=True)
    want = paths_py.PathsScene(with_materials(spec, ch)).cast_rays_paths(rays)
    assert np.array_equal(rgba, want.rgba) and np.array_equal(_bits(rgbf), _bits(want.rgbf))
    assert np.array_equal(vstart, want.vertex_start) and paths_py.same_bits(vertices, want.vertices) and paths_py.same_bits(back, want.rays_back)
    assert len(vertices) > 0 and not (vertices["color"] == paths_py.RED).any()


def test_replicas_render_the_changed_materials(xrt, monkeypatch):
    monkeypatch.setenv("XRT_FAKE_GPUS", "1")
    spec = xrt.configs.crate_grid_scene(200, 120)
    scene, tracer = xrt.configs.build_product(spec)
    tracer.NumGpus = 2
    before = tracer.Render().copy()      # (the replicas exist before the change)
    tracer.NumGpus = 1
    apply(scene, {0: dict(reflectiveness=0.9, texture=gen_texture(64, 48, 9, alpha=False)[0])})
    want = tracer.Render().copy()
    assert not np.array_equal(want, before)
    for n in (2, 3):
        tracer.NumGpus = n
        assert np.array_equal(tracer.Render(), want), "n_gpus %d" % n
    tracer.NumGpus = 1
    assert np.array_equal(tracer.Render(), want)


def test_save_load_after_set_materials(xrt, tmp_path):
    spec = xrt.configs.content_scene(96, 54, max_reflections=3)
    scene, tracer = xrt.configs.build_product(spec)
    argb, pargb = gen_texture(9, 4, 3)
    ch = {0: dict(texture=argb, texture_pargb=pargb), 1: dict(transparent=False, reflectiveness=0.75), 4: dict(interpolate_normals=False)}
    apply(scene, ch)
    scene.Save(tmp_path / "changed.xrts")
    tracer.CurrentScene = xrt.api.OctreeSpatialManager.Load(tmp_path / "changed.xrts")
    got = render(tracer)
    frame_equal(*got, render(xrt.configs.build_product(with_materials(spec, ch))[1]), "loaded")


def test_seam_1_does_not_notice(xrt):
    spec = xrt.configs.config("C3", scale=0.08)
    scene, tracer = xrt.configs.build_product(spec)
    rng = np.random.default_rng(3)
    o = rng.normal(size=(4000, 3)) * 150.0
    d = rng.uniform(-60, 60, size=(4000, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([tracer.GeneratePrimaryRays(), xrt.rays_array(o.astype(np.float32), d.astype(np.float32))])
    before = scene.IntersectBatch(rays)
    apply(scene, {0: dict(reflectiveness=0.0, transparent=True, refraction_index=1.2, texture=gen_texture(3, 3, 1)[0])})
    after = scene.IntersectBatch(rays)
    assert hits_equal(before, after) is None, hits_equal(before, after)
    assert (before["hit"] != 0).sum() > 1000
