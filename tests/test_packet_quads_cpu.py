"""How a frame's primary rays are grouped into packets (kernels.h QuadTable): the host program tests/packet_quads/packet_quads.cpp, built with host
ASan + UBSan (csrc/Makefile `packet_quads`), is a host model of the packet walk (packet.hip pk_walk: the same tests in the same order, with the
library's own functions) on fixtures.heightfield(256) at 480x270 with 16 sub-rays per pixel.  It walks the frame's live rays once as packets of 64
consecutive slots and once as one packet per aligned unit of 64 paths (a 2x2 pixel quad: one wave of k_raygen), prints blocks, child visits, run
tests and triangle steps of both, and fails if the per-quad grouping needs more triangle steps or more run tests.  A lane's answer does not depend on
who shares its packet: both groupings find the same hits."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")


@pytest.fixture(scope="module")
def output():
    subprocess.check_call(["make", "-s", "-C", CSRC, "packet_quads"])
    p = subprocess.run([os.path.join(CSRC, "packet_quads")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def _groupings(output):
    rows = {}
    for line in output.splitlines():
        w = line.split("|")[0].split()
        if w and w[0] == "grouping":
            rows[w[1]] = {w[i]: float(w[i + 1]) for i in range(2, len(w), 2)}
    return rows


def test_per_quad_packets_do_less_work(output):
    assert "packet_quads: ok" in output
    g = _groupings(output)
    c, q = g["consecutive"], g["per_quad"]
    for k in ("packets", "blocks", "child_visits", "run_tests", "triangle_steps"):
        print(k, int(c[k]), int(q[k]))
    assert q["triangle_steps"] <= c["triangle_steps"] and q["run_tests"] <= c["run_tests"]
    assert c["triangle_steps"] > 0 and c["run_tests"] > 0 and c["blocks"] > c["packets"] > 1000   # the walk is not empty
    assert q["packets"] >= c["packets"]   # partly dead quads are packets of their own


def test_both_groupings_find_the_same_hits(output):
    m = re.search(r"^hits consecutive (\d+) per_quad (\d+) paths_with_different_answers (\d+)$", output, flags=re.M)
    assert m, output[-500:]
    a, b, differ = (int(x) for x in m.groups())
    g = _groupings(output)
    assert a == b == int(g["consecutive"]["hits"]) == int(g["per_quad"]["hits"]) and a > 0 and differ == 0
