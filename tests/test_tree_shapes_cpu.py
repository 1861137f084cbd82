"""Tree shapes on the CPU: the cases of tests/tree_shapes.py -- mesh octrees up to the 20 levels the builder accepts, scene octrees up to 24,
both at once up to the 40 stack words the per-lane kernel is compiled for, scene leaves of 32, 33 and 65 bodies -- with the oracle against the
single-stepper of the product's traversal (tests/emul), bit for bit.  tests/test_gpu_tree_shapes.py runs the same cases on the device; this
module goes first and says that the first device run of a deep tree is a test and not a gamble:

  (a) every case's trees have the shape its table row claims, and the oracle, the single-stepper's host build and the library's host-only build
      agree on them;
  (b) the oracle alone meets the coverage conditions: the deep levels, the pops and the ties are reached, not just built;
  (c) the single-stepper, on a stack bounded by the capacity the library picks for the device (traverse.h intersect_stack_capacity, read through
      the single-stepper: the table is typed nowhere here), never touches a word at or beyond what the scene is said to need;
  (d) one word more is refused by xrt_scene_build."""
import copy

import numpy as np
import pytest

from tree_shapes import (CASE_IDS, CASES, REFUSED, all_rays, case, case_spec, family_slice, nested_bodies, oracle_of, staircase, staircase_scene, wanted,
                         wanted_mesh)
from util import hits_equal


def _tree_shape(e, spec):
    """(scene depth, deepest mesh depth, largest scene leaf) of a built single-stepper scene, from its trees."""
    sn, _ = e.tree(-1)
    return (int(sn["depth"].max()), max(e.tree_stats(i)["max_depth"] for i in range(len(spec.meshes))), int(sn["count"][sn["is_leaf"] == 1].max()))


@pytest.mark.parametrize("name", CASE_IDS + [REFUSED["name"]])
def test_shape(xrt, orc, emul, name):
    """The built trees have the depths and the leaf size of the case's row; oracle, single-stepper and the library's host-only scene build the same."""
    c, spec = case(name), case_spec(xrt, name)
    o, e = oracle_of(xrt, orc, name), emul.EmulScene(spec)
    sd, md, leaf = _tree_shape(e, spec)
    print("%s: scene depth %d, mesh depth %d, largest scene leaf %d, %d stack words" % (name, sd, md, leaf, sd + md + 2))
    assert (sd, md, leaf) == (c["sd"], c["md"], c["leaf"]) and c["words"] == sd + md + 2
    for m in range(len(spec.meshes)):
        assert int(e.tree(m)[0]["depth"].max()) == e.tree_stats(m)["max_depth"]
    product = None
    if name != REFUSED["name"]:
        product, _ = xrt.configs.build_product(spec, device=-1)
    for mesh in [-1] + list(range(len(spec.meshes))):
        no, ro = o.tree(mesh)
        ne, re_ = e.tree(mesh)
        assert no.tobytes() == ne.tobytes() and np.array_equal(ro, re_)
        if product is not None:
            np_, rp = xrt.api._get_tree(product._scene, mesh)
            assert no.tobytes() == np_.tobytes() and np.array_equal(ro, rp)


@pytest.mark.parametrize("name", CASE_IDS)
def test_oracle_equals_single_stepper(xrt, orc, emul, name):
    """Every ray family at the scene seam, and at the mesh seam of the one-body cases."""
    spec, rays = case_spec(xrt, name), all_rays(xrt, orc, name)
    want, _ = wanted(xrt, orc, name)
    e = emul.EmulScene(spec)
    print("%s: %d rays, oracle hits %d" % (name, len(rays), int(want["hit"].sum())))
    assert hits_equal(want, e.intersect(rays)) == {}
    if case(name)["kind"] == "mesh":
        want = wanted_mesh(xrt, orc, name)
        assert int(want["hit"].sum()) > 0
        assert hits_equal(want, e.intersect(rays, mode=1, mesh=0)) == {}


def _leaf_depths(nodes):
    """DFS index -> depth of the leaves of a tree (xrt_node_info records)."""
    leaves = nodes[nodes["is_leaf"] == 1]
    return dict(zip(leaves["dfs_index"].tolist(), leaves["depth"].tolist()))


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_oracle_reaches_what_the_case_is_about(xrt, orc, name):
    """Coverage, by the oracle alone (no tolerance, nothing of the product): every triangle of a staircase, every nested body, every body of a crowd
    is the answer of some ray; some answer lies in a leaf of the tree's greatest depth; some outward ray is answered at least md - 2 levels above
    the leaf it starts in (the walk popped that far); the coincident pair of a crowd ties exactly and its lower-listed body is the answer."""
    c, spec, rays = case(name), case_spec(xrt, name), all_rays(xrt, orc, name)
    o = oracle_of(xrt, orc, name)
    want, _ = wanted(xrt, orc, name)
    hit = want[want["hit"] == 1]
    bodies = set(range(len(spec.objects))) - ({1} if c["kind"] == "crowd" else set())   # (the upper of the coincident pair never wins)
    assert set(hit["object"].tolist()) == bodies
    if c["md"] > 0:
        ntri = spec.meshes[0][0].ntri
        assert ntri == c["md"] + 2 and set(hit["tri"].tolist()) == set(range(ntri))
        depth = _leaf_depths(o.tree(0)[0])
        hd = np.array([depth[l] for l in hit["leaf"].tolist()])
        assert int(hd.max()) == c["md"]
        # outward rays: the leaf of the origin (object space of the innermost body, whose pose is a translation and a uniform scale) against the leaf of the answer
        nodes = o.tree(0)[0]
        leaves = nodes[nodes["is_leaf"] == 1]
        sl = family_slice(xrt, name, "outward")
        ids, pos, rot, scale = spec.objects[-1]
        org = (rays["o"][sl].astype(np.float64) - np.array(pos)) / scale[0]
        inside = ((org[:, None, :] >= leaves["bmin"][None]) & (org[:, None, :] <= leaves["bmax"][None])).all(axis=2)
        origin_depth = np.where(inside, leaves["depth"][None], -1).max(axis=1)
        w = want[sl]
        ok = (w["hit"] == 1) & (w["object"] == len(spec.objects) - 1)
        rise = origin_depth[ok] - np.array([depth[l] for l in w["leaf"][ok].tolist()])
        print("%s: outward rays start at depth %d..%d, greatest rise to the answer %d" % (name, origin_depth.min(), origin_depth.max(), rise.max()))
        assert int(origin_depth.min()) == c["md"] and int(rise.max()) >= c["md"] - 2
    if c["sd"] > 0:
        sn, sr = o.tree(-1)
        deepest = sn[(sn["is_leaf"] == 1) & (sn["depth"] == c["sd"]) & (sn["count"] > 0)]
        there = set(int(b) for n in deepest for b in sr[n["first_ref"]: n["first_ref"] + n["count"]])
        assert there & set(hit["object"].tolist())
    if c["kind"] == "crowd":
        assert spec.objects[0] == spec.objects[1] and max(len(ob[0]) for ob in spec.objects) == 6
        assert 6 in set(len(spec.objects[b][0]) for b in hit["object"].tolist())
        first = want["hit"].astype(bool) & (want["object"] == 0)
        assert first.sum() > 0 and not (want["object"][want["hit"] == 1] == 1).any()
        alone = copy.copy(spec)          # the same scene without body 0: body 1, now listed first, gives the very same answers, so the two tied exactly
        alone.objects = spec.objects[1:]
        twin = orc.OracleScene(alone).intersect(rays[first])
        assert hits_equal(want[first], twin) == {}


@pytest.mark.parametrize("name", CASE_IDS)
def test_the_stack_stays_inside_the_device_capacity(xrt, orc, emul, name):
    """The single-stepper on a stack of the capacity k_intersect would get: no access at or beyond (sd + 1) + (md + 1), which is at most that
    capacity, and the oracle's answers."""
    c, spec, rays = case(name), case_spec(xrt, name), all_rays(xrt, orc, name)
    cap = emul.stack_capacity(c["words"])
    e = emul.EmulScene(spec)
    got, info = e.intersect_bounded(rays, cap)
    print("%s: %d words needed, capacity %d, highest index touched %d" % (name, c["words"], cap, info["high"]))
    assert info["scene_words"] + info["mesh_words"] == c["words"] <= cap
    assert info["outside"] == 0 and info["high"] < c["words"]
    assert hits_equal(wanted(xrt, orc, name)[0], got) == {}
    if c["kind"] == "mesh":
        got, info = e.intersect_bounded(rays, cap, mode=1, mesh=0)
        assert info["outside"] == 0 and info["high"] < c["words"]
        assert hits_equal(wanted_mesh(xrt, orc, name), got) == {}
    if c["md"] > 0:   # (the walk does use its deep words: a bound nothing comes near would say little)
        assert info["high"] >= c["words"] - 3


def test_the_bounded_stack_notices_a_word_too_many(xrt, orc, emul):
    """The instrument itself: on a stack one word shorter than the deepest index the walk touches, the access is recorded and refused."""
    name = "both_sd18_md20"
    e, rays = emul.EmulScene(case_spec(xrt, name)), all_rays(xrt, orc, name)
    high = e.intersect_bounded(rays, 256)[1]["high"]
    assert e.intersect_bounded(rays, high + 1)[1]["outside"] == 0
    assert e.intersect_bounded(rays, high)[1]["outside"] > 0


def test_the_cases_stand_on_both_sides_of_every_capacity_seam(emul):
    """Each pair needs the last word of one compiled capacity and the first of the next (the capacities themselves are the library's)."""
    cap = lambda name: emul.stack_capacity(case(name)["words"])
    for last, first in (("mesh_md6", "mesh_md7"), ("mesh_md10", "mesh_md11"), ("mesh_md14", "mesh_md15")):
        assert case(first)["words"] == case(last)["words"] + 1
        assert cap(last) == case(last)["words"] < cap(first)
    assert cap("mesh_md15") == cap("mesh_md20") < cap("both_sd4_md20") == cap("both_sd18_md20") == case("both_sd18_md20")["words"]
    assert emul.stack_capacity(REFUSED["words"]) == -1 and REFUSED["words"] == case("both_sd18_md20")["words"] + 1


def test_one_word_more_is_refused(xrt, emul):
    """41 words: xrt_scene_build refuses the host-only scene with XRT_E_UNSUPPORTED; 40 words are accepted.  And the builders' own limits: a mesh
    tree of 21 levels, a scene tree of 25."""
    xrt.configs.build_product(case_spec(xrt, "both_sd18_md20"), device=-1)
    with pytest.raises(xrt.abi.XrtError, match="too deep for the LDS stack") as err:
        xrt.configs.build_product(case_spec(xrt, REFUSED["name"]), device=-1)
    assert err.value.code == xrt.abi.XRT_E_UNSUPPORTED
    for spec, msg in ((staircase_scene(xrt, 21), "deeper than 20 levels"), (nested_bodies(xrt, 25), "OctreeSpatialManager.BuildTree would not terminate")):
        with pytest.raises(xrt.abi.XrtError, match=msg):
            xrt.configs.build_product(spec, device=-1)
        with pytest.raises(RuntimeError, match=msg):
            emul.EmulScene(spec)
    xrt.configs.build_product(staircase_scene(xrt, 20), device=-1)
    xrt.configs.build_product(nested_bodies(xrt, 24), device=-1)
