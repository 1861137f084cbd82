"""The mesh-level test "every triangle faces away from this ray" with the normals bounded in a diagonal frame as well as in their axis-aligned box
(traverse.h mesh_faces_away): the host program tests/normal_diag/normal_diag.cpp, built with host ASan + UBSan (csrc/Makefile
`normal_diag`), checks by brute force that whenever the test answers, RE:49-50 in binary32 rejects EVERY triangle of the mesh -- on a 64 x 64-quad
heightfield, a tessellated crate, a triangle soup, a flat tilted grid, a cone of normals about (1, 1, 1) and a fan of normals about (1, 1, 0), for seeded
directions, the benchmark camera's reflections, directions on the decision boundary and a few ulps to either side, axis-parallel directions, components
of 1e-30 and 1e30, NaNs and infinities -- and that it answers whatever the axis-aligned box alone answers.  It also reports the share of the camera's
reflections each test leaves to be traced (profiles/normal_diag/README.md quotes the figures)."""
import re
import subprocess

import pytest

import normal_diag_py


@pytest.fixture(scope="module")
def output():
    exe = normal_diag_py.build_checked()
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


def _scenes(output):
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^scene (\w+) .* axis (\d) can_face_away (\d) ", output, flags=re.M)}


def test_an_answer_is_never_wrong_and_none_is_lost(output):
    assert "normal_diag: ok" in output
    rows = _checks(output)
    assert len(rows) == len(normal_diag_py.SCENES) * len(normal_diag_py.CATEGORIES)
    for (scene, cat), r in rows.items():
        assert r["unsound"] == 0 and r["unsound_old"] == 0, (scene, cat, r)
        assert r["lost"] == 0 and r["new_yes"] >= r["old_yes"], (scene, cat, r)
        if cat == "non_finite":
            assert r["dirs"] > 0 and r["new_yes"] == 0, (scene, r)
    for scene in ("heightfield", "cone111", "fan110", "plane"):   # the checks are not empty: the test answers, on its boundary too, and at 1e-30 and 1e30
        for cat in ("seeded", "boundary", "scaled"):
            assert 0 < rows[(scene, cat)]["new_yes"] < rows[(scene, cat)]["dirs"], (scene, cat)
    for scene in ("crate", "soup"):   # normals of every direction: nothing to answer, by either bound
        assert all(rows[(scene, cat)]["new_yes"] == 0 for cat in normal_diag_py.CATEGORIES), scene


def test_the_axis_rule(output):
    """The terrain's diagonal frame is the one about y (the issue's measurement: about x it answers nothing new); crate and soup get none."""
    sc = _scenes(output)
    assert sc["heightfield"] == (2, 1)
    assert sc["crate"] == (0, 0) and sc["soup"] == (0, 0)
    assert sc["cone111"][0] in (1, 2, 3) and sc["cone111"][1] == 1
    assert sc["fan110"] == (3, 1)   # N_x + N_y is the interval that excludes 0: the frame about z


def test_the_diagonal_frame_answers_more(output):
    rows = _checks(output)
    # the cone about (1, 1, 1): every axis interval excludes 0, the box answers, and the diagonal box answers directions it cannot
    assert rows[("cone111", "seeded")]["new_yes"] > rows[("cone111", "seeded")]["old_yes"] > 0
    # the fan about (1, 1, 0): the axis-aligned box holds the origin on every axis and answers nothing at all
    assert rows[("fan110", "seeded")]["old_yes"] == 0 and rows[("fan110", "seeded")]["new_yes"] > 0
    got = dict(re.findall(r"^report (\w+ \w+) ([0-9.]+)$", output, flags=re.M))
    old, new = float(got["heightfield not_answered_old"]), float(got["heightfield not_answered_new"])
    print("heightfield, benchmark camera: reflections not answered at the mesh level, old %.4f new %.4f" % (old, new))
    assert int(float(got["heightfield reflections"])) > 1000
    assert new <= old
