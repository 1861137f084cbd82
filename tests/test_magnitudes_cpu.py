"""Parity across magnitudes on the CPU: the oracle against the single-stepper of the product's traversal (tests/emul) on scenes scaled by
2^k and rays whose directions have length 2^j -- the cells of tests/magnitudes.py, at which the guards of the hot path's shortcuts flip
(DESIGN.md §3 "Range of validity"): certainly_negative, make_ray_cull, the tight leaf boxes, all_back_facing, the 1e-6 parallel branch of
the slab test, the reference's own under- and overflows.  tests/test_gpu_magnitudes.py runs the same cells on the device; a cell that fails
there and passes here is a fault of the device-only code.

Three things per cell: (a) oracle == single-stepper, bit for bit, at the scene seam and at the mesh seam; (b) a pin of the oracle that does
not involve the product: MO:259-353 and RE:42-75 use + - * / and comparisons only, so a power-of-two scale leaves every decision and u, v
alone and multiplies d and w exactly -- until something under- or overflows; (c) the oracle alone finds at least FLOOR hits, so no cell
passes because every ray missed."""
import numpy as np
import pytest

import poses_py
from magnitudes import (CELLS, FLOOR, FRAME_FLOOR, FRAMES, POSES, SECONDARY, cell_floors, cell_id, cell_spec_and_rays, frame_id, oracle_frame, oracle_of,
                        pose_floors, pose_id, secondary_case, secondary_id)
from util import hits_equal, magnitude_fixture, magnitude_pose_case, scaled_rays


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_oracle_equals_single_stepper(xrt, orc, emul, cell):
    spec, rays = cell_spec_and_rays(xrt, cell)
    o = oracle_of(xrt, orc, cell[0], cell[1])
    e = emul.EmulScene(spec)
    floor_scene, floor_mesh = cell_floors(cell)
    if floor_scene is not None:
        want = o.intersect(rays)
        print("%s: oracle hits %d at the scene seam" % (cell_id(cell), int(want["hit"].sum())))
        assert int(want["hit"].sum()) >= floor_scene
        assert hits_equal(want, e.intersect(rays)) == {}
    want = o.mesh_intersect(0, rays)
    print("%s: oracle hits %d at the mesh seam" % (cell_id(cell), int(want["hit"].sum())))
    assert int(want["hit"].sum()) >= floor_mesh
    assert hits_equal(want, e.intersect(rays, mode=1, mesh=0)) == {}


def scale_exact(xrt, orc, name, k):
    """Is the oracle's mesh-seam answer at scale 2^k the unit answer with d and w multiplied by 2^k, and the tree's reference list the same?"""
    md, spec, rays, _ = magnitude_fixture(xrt, name)
    o0, ok = oracle_of(xrt, orc, name, 0), oracle_of(xrt, orc, name, k)
    h0, hk = o0.mesh_intersect(0, rays), ok.mesh_intersect(0, scaled_rays(rays, k, 0))
    want = h0.copy()
    with np.errstate(all="ignore"):
        want["d"] = h0["d"] * np.ldexp(np.float32(1), k)
        want["w"] = h0["w"] * np.ldexp(np.float32(1), k)
    return hits_equal(want, hk) == {} and np.array_equal(o0.tree(0)[1], ok.tree(0)[1]), int(h0["hit"].sum())


@pytest.mark.parametrize("name", ["soup", "hf"])
@pytest.mark.parametrize("k", [-31, -20, 20, 29])
def test_oracle_is_exact_under_power_of_two_scales(xrt, orc, name, k):
    same, hits = scale_exact(xrt, orc, name, k)
    assert hits >= FLOOR
    assert same


@pytest.mark.parametrize("name", ["soup", "hf"])
def test_the_sweep_leaves_the_exact_regime(xrt, orc, name):
    """At 2^-40 squares of edges underflow: the oracle's answers are no longer the scaled unit answers."""
    same, hits = scale_exact(xrt, orc, name, -40)
    assert hits >= FLOOR
    assert not same


@pytest.mark.parametrize("case", SECONDARY, ids=secondary_id)
def test_secondary_rays_oracle_equals_single_stepper(xrt, orc, emul, case):
    spec, rays, floor = secondary_case(xrt, orc, case)
    want = oracle_of(xrt, orc, case[0], case[1]).intersect(rays)
    print("%s: %d rays, oracle hits %d" % (secondary_id(case), len(rays), int(want["hit"].sum())))
    assert len(rays) >= FLOOR and int(want["hit"].sum()) >= floor
    assert hits_equal(want, emul.EmulScene(spec).intersect(rays)) == {}


@pytest.mark.parametrize("case", FRAMES, ids=frame_id)
def test_the_oracle_shades_the_frames(xrt, orc, case):
    spec, rgba, rgbf, st = oracle_frame(xrt, orc, *case)
    print("%s: shaded %d, %d colours" % (frame_id(case), st["shaded_hits"], len(np.unique(rgba))))
    assert st["shaded_hits"] >= FRAME_FLOOR
    if case[1] <= -40:
        assert len(np.unique(rgba)) <= 8   # the light vectors underflow: a handful of colours is left, which is the point
    else:
        assert len(np.unique(rgba)) >= 100


@pytest.mark.filterwarnings("ignore::RuntimeWarning")   # (the inverse of a singular world matrix: infinities and NaNs, as in the reference)
@pytest.mark.parametrize("case", POSES, ids=pose_id)
def test_poses_oracle_equals_single_stepper(xrt, case):
    """HostScene::set_pose / build_tree (the cull record of pose.h on the host) under the single-stepper against the oracle with the body moved."""
    spec, pose0, rays0, rays1 = magnitude_pose_case(xrt, case[0], case[1])
    ref, emu = poses_py.PoseOracle(spec), poses_py.PoseEmul(spec)
    ref.set_pose(0, *pose0)
    emu.set_pose(0, *pose0)
    floors = pose_floors(case)
    for i, tree in enumerate(("stale", "built")):
        if tree == "built":
            ref.build_tree()
            emu.build_tree()
        for b, rays in enumerate((rays0, rays1)):
            want = ref.intersect(rays)
            print("%s %s tree, body %d: oracle hits %d" % (pose_id(case), tree, b, int(want["hit"].sum())))
            assert int(want["hit"].sum()) >= floors[2 * i + b]
            msg = poses_py.hits_equal(want, emu.intersect(rays))
            assert msg is None, msg
