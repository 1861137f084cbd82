"""plan_frame (csrc/frame_plan.h): what a frame launches is decided once, by a function that calls no HIP function and only reads the scene.  The
host program tests/frame_plan/host_plan.cpp, built with host ASan + UBSan from the library's own sources (csrc/Makefile `hostcheck_plan`), plans
every combination of scene kind, sampling, Transparent materials, collect_stats, batch, light count, float output, parts, shards / tile table,
MaxReflections and frame size on hand-filled host-only scenes and checks on each plan what the planner's comments state: what `fast`, `ae`,
`finishA`, `endEarly`, `skipTiles` and `fuseResolve` imply, the level map and the buffer sizes, the many-lights bounds, the shape of a batch; then
the switches of Settings one at a time, every refusal with its code and message, and that planning twice gives the same plan."""
import os
import re
import subprocess

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
FLAGS = ("fast", "heapFast", "adaptiveFast", "ae", "finishA", "endEarly", "skipTiles", "fuseResolve", "levelMap", "wantFeedback", "multiChunk", "tabled", "wantF32")


@pytest.fixture(scope="module")
def output():
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_plan"])
    p = subprocess.run([os.path.join(CSRC, "hostcheck_plan")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_every_plan_of_the_sweep_keeps_what_the_planner_states(output):
    assert "host_plan: ok" in output
    plans, refused = map(int, re.search(r"^plans (\d+) refused (\d+)$", output, flags=re.M).groups())
    # 3 scene kinds x 2 (Transparent) x 2 sizes x 3 (shards, table) x 4 samplings x 2 (collect) x 3 (batch) x 4 light counts x 2 (float) x 2 (parts) x 2 (R)
    assert plans + refused == 3 * 2 * 2 * 3 * 4 * 2 * 3 * 4 * 2 * 2 * 2
    assert plans >= 6000   # every combination that is a frame or a batch the library renders


def test_the_sweep_reaches_both_sides_of_every_flag(output):
    rows = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^check (\w+) plans (\d+) on (\d+)$", output, flags=re.M)}
    assert set(rows) == set(FLAGS)
    for name, (plans, on) in rows.items():
        assert 0 < on < plans, name
