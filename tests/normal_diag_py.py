"""TEST INFRASTRUCTURE -- tests/normal_diag/normal_diag.cpp ("the whole mesh faces away" with the normals bounded in a diagonal frame too, checked by brute
force on the host).  The checks themselves run in the sanitizer build of csrc/Makefile `normal_diag` (tests/test_normal_diag_cpu.py); build() here makes a
plain copy, tests/normal_diag/normal_diag_plain, which answers world-space rays with the library's own host code: the scene build of scene_host.cpp and
traverse.h mesh_faces_away, the function the kernels call (tests/test_gpu_normal_diag.py counts with it what the device must have answered)."""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
SRC = os.path.join(_HERE, "normal_diag", "normal_diag.cpp")
PLAIN = os.path.join(_HERE, "normal_diag", "normal_diag_plain")
CATEGORIES = ("seeded", "reflections", "boundary", "axis", "scaled", "non_finite")
SCENES = ("heightfield", "crate", "soup", "cone111", "fan110", "plane")


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
    """The sanitizer build (host ASan + UBSan), csrc/normal_diag."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "normal_diag"])
    return os.path.join(CSRC, "normal_diag")


def answers(vertices, mesh_threshold, inv_world, kind, records):
    """For a one-body scene of the mesh `vertices` (ntri, 3, 3) under the row-major 4x4 `inv_world`: per world-space ray whether the library's emission
    test answers it "nothing there" (bool array), the axis of the mesh record's diagonal frame (0: none, 1..3 = x, y, z) and whether the mesh can face away
    from any ray at all.  kind "rays": records (n, 6) = origin, direction; "hits": (n, 9) = hit position, direction of the ray that hit, fragment normal
    (the reflection from the hit); "light": (n, 6) = hit position, light position (the shadow ray from the hit)."""
    r = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 9 if kind == "hits" else 6)
    with tempfile.TemporaryDirectory() as t:
        p = [os.path.join(t, n) for n in ("mesh.bin", "inv.bin", "rays.bin", "out.bin")]
        np.ascontiguousarray(vertices, dtype=np.float32).tofile(p[0])
        np.ascontiguousarray(inv_world, dtype=np.float32).reshape(16).tofile(p[1])
        r.tofile(p[2])
        subprocess.check_call([build(), "--answer", p[0], str(int(mesh_threshold)), p[1], kind, p[2], p[3]])
        out = np.fromfile(p[3], dtype=np.uint8)
    assert out.size == r.shape[0] + 4
    return out[:-4].astype(bool), int(out[-4]), bool(out[-3])
