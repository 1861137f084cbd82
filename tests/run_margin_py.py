"""TEST INFRASTRUCTURE -- tests/run_margin/run_margin.cpp (the runs of a big leaf under the leaf's margin, checked by brute force on the host).
The checks themselves run in the sanitizer build of csrc/Makefile `run_margin` (tests/test_run_margin_cpu.py); build() here makes a plain copy,
tests/run_margin/run_margin_plain, whose only use is to write out the program's heightfield and its adversarial rays for the GPU test."""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
SRC = os.path.join(_HERE, "run_margin", "run_margin.cpp")
PLAIN = os.path.join(_HERE, "run_margin", "run_margin_plain")
CATEGORIES = ("graze", "in_plane", "vertex_edge", "axis_parallel", "tiny_component", "non_finite")


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(d) for d in deps)


def _deps():
    return [SRC, os.path.join(CSRC, "scene_build.cpp"), os.path.join(CSRC, "scene_host.cpp")] + \
           [os.path.join(CSRC, h) for h in ("traverse.h", "xrt_core.h", "scene_host.h", "scene_build.h")]


def build():
    if _stale(PLAIN, _deps()):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-o", PLAIN] + _deps()[:3])
    return PLAIN


def build_checked():
    """The sanitizer build (host ASan + UBSan), csrc/run_margin."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "run_margin"])
    return os.path.join(CSRC, "run_margin")


def heightfield_vertices():
    """The program's 64 x 64-quad heightfield, (ntri, 3, 3) float32."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "mesh.bin")
        subprocess.check_call([build(), "--dump-mesh", p])
        return np.fromfile(p, dtype=np.float32).reshape(-1, 3, 3)


def adversarial_rays(per_category):
    """{category: (origins, directions)} of the program's adversarial rays at the runs of the heightfield's big leaves, at least per_category each."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "rays.bin")
        subprocess.check_call([build(), "--dump-rays", p, str(int(per_category))])
        a = np.fromfile(p, dtype=np.float32).reshape(-1, 7)
    return {name: (a[a[:, 6] == k, 0:3].copy(), a[a[:, 6] == k, 3:6].copy()) for k, name in enumerate(CATEGORIES)}
