"""The runs of a big leaf tested against their vertex box grown by the LEAF's margin (packet.hip pk_walk): the host program
tests/run_margin/run_margin.cpp, built with host ASan + UBSan (csrc/Makefile `run_margin`), checks by brute force that the rule skips no (ray, run)
pair in which RE:42-75 accepts a triangle -- on a 64 x 64-quad heightfield, a tessellated crate and a triangle soup, with rays on the decision
boundary --, that axis-parallel rays, rays with a tiny direction component and non-finite rays take the fallback, and that leaf_certainly_missed
composed of leaf_margin and grown_box_missed answers like its body before the split.  It also reports the rule's culling power on coherent camera
rays (profiles/run_margin/README.md quotes the figures); no threshold is set on those."""
import re
import subprocess

import numpy as np
import pytest

import run_margin_py


@pytest.fixture(scope="module")
def output():
    exe = run_margin_py.build_checked()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def _checks(output):
    rows = {}
    for line in output.splitlines():
        w = line.split()
        if w and w[0] == "check":
            rows[(w[1], w[2])] = {w[i]: int(w[i + 1]) for i in range(3, len(w), 2)}
    return rows


def test_runs_under_the_leaf_margin_are_sound(output):
    assert "run_margin: ok" in output
    rows = _checks(output)
    assert len(rows) == 3 * len(run_margin_py.CATEGORIES)
    for (scene, cat), r in rows.items():
        assert r["unsound_new"] == 0 and r["unsound_old"] == 0, (scene, cat, r)
        assert r["pairs"] > 0 and r["rays"] > 0, (scene, cat)
        if cat != "non_finite":
            assert r["accepted"] > 0, (scene, cat)   # the rays do hit triangles of the runs: the check is not empty
    for scene in ("heightfield", "crate"):   # smooth surfaces: the cheap rule decides, and it is not far behind the run's own test
        for cat in ("graze", "in_plane", "vertex_edge"):
            r = rows[(scene, cat)]
            assert 0 < r["new_skips"] < r["pairs"] and r["both"] == r["new_skips"], (scene, cat, r)
    for cat in ("graze", "in_plane", "vertex_edge"):   # the soup's leaves hold normals of every direction: no usable leaf margin, the fallback decides
        r = rows[("soup", cat)]
        assert r["usable_leaf_margins"] == 0 and r["new_skips"] == 0 and r["old_skips"] > 0, (cat, r)


def test_rays_without_a_margin_take_the_fallback(output):
    rows = _checks(output)
    for (scene, cat), r in rows.items():
        assert r["fallback_wrong"] == 0, (scene, cat)
        if cat in ("axis_parallel", "tiny_component", "non_finite"):
            assert r["usable_leaf_margins"] == 0 and r["new_skips"] == 0, (scene, cat, r)


def test_the_split_functions_compose_to_the_old_test(output):
    for key, r in _checks(output).items():
        assert r["composition_mismatch"] == 0, key


def test_culling_power_report(output):
    """Figures (a) and (b) of the coherent samples are printed (pytest -s shows them); they explain the GPU timing and carry no threshold."""
    got = dict(re.findall(r"^report (\w+ \w+) ([0-9.]+)$", output, flags=re.M))
    for view in ("grazing", "bench_camera"):
        for k in ("a_share_literal", "a_share_shipped", "b_fallback_share"):
            v = float(got["%s %s" % (view, k)])
            print(view, k, v)
            assert 0.0 <= v <= 1.0


def test_the_programs_heightfield_is_the_fixture(xrt):
    """The GPU test renders fixtures.heightfield(64) and casts the program's rays at it: the two meshes are the same bits."""
    v = run_margin_py.heightfield_vertices()
    assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(xrt.fixtures.heightfield(64).v, dtype=np.float32).reshape(-1, 3, 3).view(np.uint32))
