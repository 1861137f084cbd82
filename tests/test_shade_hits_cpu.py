"""xrt_shade_hits (what CastRay does with an IntersectionResult, RT:514-737, on caller-given hits) without a GPU: the exports in every
binding, the checker's restatement pinned against the oracle's own CastRay -- orc_shade_hits(R, orc_scene_intersect(R)) is orc_cast_rays(R)
in colours, in the bits of the colour vectors and in counters --, and tests/shade_hits/host_shade_hits.cpp (the order of the argument
errors and every kind of invalid hit entry on a host-only scene) as a program of its own under ASan and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import shade_hits_py as sh
from test_gpu_cast_rays import scenes
from util import secondary_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")
EXPORTS = ("xrt_shade_hits", "xrt_shade_hits_device")


def test_exports_are_in_the_library_the_header_and_every_binding(xrt):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    raw = C.CDLL(xrt.abi.LIB_PATH)
    for name in EXPORTS:
        assert hasattr(raw, name), name
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in xrt.abi.SYMBOLS, name
        assert re.search(r"CallingConvention = CallingConvention\.Cdecl\)\] public static extern (?:unsafe )?int %s\(" % name, cs), name
    assert "#define XRT_VERSION 203" in hdr and xrt.abi.lib().xrt_version() == 203
    assert callable(getattr(xrt.RayTracer, "ShadeHits", None))
    # the kernel's paths-per-block-group constant the GPU test sizes its lists around
    src = open(os.path.join(CSRC, "hits.h")).read()
    assert int(re.search(r"INGEST_HITS_SPAN = (\d+);", src).group(1)) == 4096


def glass_index(xrt):
    return [m["refraction_index"] for _, m in scenes(xrt)["glass"].meshes if m["transparent"]][0]


def expected_stats(cast, query, hits):
    """What xrt_shade_hits counts, from the counters of CastRay on the same rays and of the n queries alone: the n skipped queries and
    their work are not counted; the shaded hits and the shadow rays are."""
    out = dict(cast)
    for k in ("rays_closest", "hits_closest", "scene_node_tests", "instance_visits", "mesh_aabb_tests", "mesh_queries", "node_tests", "leaf_refs", "tri_tests"):
        out[k] = cast[k] - query[k]
    assert query["rays_closest"] == len(hits) and query["hits_closest"] == int((hits["hit"] != 0).sum())
    rays, nhits = out["rays_closest"] + out["rays_shadow"], out["hits_closest"] + out["hits_shadow"]   # (oracle.cpp FillStats)
    out["algorithmic_bytes"] = (rays * 80 + 32 * out["node_tests"] + 4 * out["leaf_refs"] + 48 * out["tri_tests"] + 32 * out["scene_node_tests"] +
                                64 * out["instance_visits"] + 24 * out["mesh_aabb_tests"] + 64 * nhits + 80 * out["shaded_hits"] + 4 * out["pixels"])
    return out


@pytest.mark.parametrize("name", ["crate", "crate_grid", "glass", "heightfield", "content"])
def test_the_restatement_is_the_oracles_castray(xrt, name):
    """Primary rays and secondary rays off their hits; iterations 0, 1, M, M + 1; currentRefIndex 1.0 and the glass's index."""
    spec = scenes(xrt)[name]
    cs = sh.ShadeHitsScene(spec)
    primary = cs.primary_rays()
    p_hits, _ = cs.intersect(primary)
    assert 0 < int(p_hits["hit"].sum()) < len(primary), "the camera sees hits and misses"
    secondary = secondary_rays(xrt, p_hits, seed=3)
    M = spec.max_reflections
    for what, rays in (("primary", primary), ("secondary", secondary)):
        hits, q_st = cs.intersect(rays)
        for it in (0, 1, M, M + 1):
            for ref in (1.0, glass_index(xrt)):
                tag = (name, what, it, ref)
                o_rgba, o_rgbf, o_st = cs.cast_rays(rays, iteration=it, ref_index=ref)
                rgba, rgbf, st = cs.shade_hits(rays, hits, iteration=it, ref_index=ref)
                assert np.array_equal(rgba, o_rgba), tag
                assert sh.same_bits(rgbf, o_rgbf), tag
                want = expected_stats(o_st, q_st, hits)
                for k, v in want.items():
                    if not k.startswith("ms_"):
                        assert st[k] == v, (tag, k, st[k], v)


def test_what_castray_does_not_read_is_not_read(xrt):
    """Garbage origins, origin triangles, d, leaf, reserved and object leave the checker's colours alone; a hit word other than 1 is a hit;
    an entry whose mesh or triangle does not exist is a miss."""
    spec = scenes(xrt)["glass"]
    cs = sh.ShadeHitsScene(spec)
    rays = cs.primary_rays()
    hits, _ = cs.intersect(rays)
    want = cs.shade_hits(rays, hits)
    r2, h2 = rays.copy(), hits.copy()
    rng = np.random.default_rng(1)
    r2["o"] = rng.normal(size=r2["o"].shape).astype(np.float32) * 1e6
    r2["o"][::7] = np.nan
    r2["ignore_mesh"], r2["ignore_tri"] = 123456, -98765
    h2["d"], h2["leaf"], h2["reserved"], h2["object"] = np.float32(np.nan), -3, 0x12345678, 77
    h2["hit"][h2["hit"] != 0] = -1234
    got = cs.shade_hits(r2, h2)
    assert np.array_equal(got[0], want[0]) and sh.same_bits(got[1], want[1])
    live = np.flatnonzero(hits["hit"] != 0)
    h3 = hits.copy()
    h3["mesh"][live[0]], h3["mesh"][live[1]], h3["tri"][live[2]], h3["tri"][live[3]] = -1, 10 ** 6, -1, 2 ** 31 - 1
    got = cs.shade_hits(rays, h3)
    black = cs.shade_hits(rays[:1], np.zeros(1, dtype=hits.dtype))[0][0]
    bad = live[:4]
    assert (got[0][bad] == black).all() and not (want[0][bad] == black).all()
    keep = np.ones(len(rays), dtype=bool); keep[bad] = False
    assert np.array_equal(got[0][keep], want[0][keep]) and sh.same_bits(got[1][keep], want[1][keep])


def test_host_program_under_the_sanitizers():
    """tests/shade_hits/host_shade_hits.cpp, host code under ASan and UBSan, a program of its own (nothing is preloaded, no GPU)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_shade_hits"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CSRC, "hostcheck_shade_hits")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and "host_shade_hits: ok" in p.stdout, p.stdout + p.stderr
