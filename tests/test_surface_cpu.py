"""xrt_surface_hits (what CastRay computes at a hit without asking the scene anything: RT:520-531, 547-559, 568-581, 656-694) without a GPU:
the exports in every binding, the checker's restatement pinned against the oracle's own CastRay -- its colour times the light sum is the
colour vector of orc_cast_rays at MaxReflections 0, its reflected ray ends where orc_paths_run's reflection segment ends, its refracted ray
is the ray CastRay leaves behind --, the branch counts the GPU tests rely on, the argument checks on a host-only scene in a host program
under ASan and UBSan, and the numerical contract (no contracted multiply-add) on the ISA of surface.hip.
Every comparison is bit for bit; a NaN equals a NaN of any payload."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lights_py as lp
import paths_py
import surface_py as sp
from test_gpu_cast_rays import scenes, two_mesh_spec
from test_numerics_contract import check_no_contracted_fma, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")
EXPORTS = ("xrt_surface_hits", "xrt_surface_hits_device")
NAMES = ["crate", "crate_grid", "glass", "heightfield", "content", "two_mesh"]
_CTX = {}


def _specs(xrt):
    out = dict(scenes(xrt))
    out["two_mesh"] = two_mesh_spec(xrt)
    return out


def ctx(xrt, name):
    """(spec, checker scene, the camera's rays, the oracle's hits of them, the checker's outputs), made once."""
    if name not in _CTX:
        spec = _specs(xrt)[name]
        cs = sp.SurfaceScene(spec)
        rays = cs.primary_rays()
        hits, _ = cs.intersect(rays)
        _CTX[name] = (spec, cs, rays, hits, cs.surface_hits(hits, rays))
    return _CTX[name]


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
    assert "public struct XrtSurface" in cs
    assert callable(getattr(xrt.RayTracer, "SurfaceHits", None))
    # the record in the header, in ctypes, in numpy and in the checker: 64 bytes, the same fields at the same offsets
    assert C.sizeof(xrt.abi.xrt_surface) == 64 == xrt.SURFACE_DTYPE.itemsize
    for name, _ in xrt.abi.xrt_surface._fields_:
        assert getattr(xrt.abi.xrt_surface, name).offset == xrt.SURFACE_DTYPE.fields[name][1] == sp.SURFACE_DTYPE.fields[name][1], name
    body = re.search(r"typedef struct xrt_surface \{(.*?)\} xrt_surface;", hdr, re.S).group(1)
    assert re.findall(r"^\s*(?:float|int32_t)\s+(\w+)", body, flags=re.M) == [n for n, _ in xrt.abi.xrt_surface._fields_]
    for flag, value in (("HIT", 1), ("TRANSPARENT", 2), ("INTERPOLATED", 4), ("TEXTURED", 8)):
        assert re.search(r"#define XRT_SURF_%s\s+%d\b" % (flag, value), hdr) and getattr(xrt.abi, "SURF_" + flag) == value == getattr(sp, "SURF_" + flag)
    # the kernel's block size and block cap, which the GPU test sizes its lists around
    src = open(os.path.join(CSRC, "surface.h")).read()
    assert int(re.search(r"SURFACE_BLOCK = (\d+);", src).group(1)) % 64 == 0 and int(re.search(r"SURFACE_MAX_BLOCKS = (\d+);", src).group(1)) > 0


@pytest.mark.parametrize("name", NAMES)
def test_colour_times_light_is_the_oracles_colour_vector(xrt, name):
    """On the oracle's own hits of the camera rays: surface colour * light sum (orc_light_hits) is the vector CastRay hands to `new Color` at
    MaxReflections 0 (RT:726) -- on textured and untextured scenes --, and a miss is the zero record and the null rays."""
    spec, cs, rays, hits, (surf, refl, refr, counts) = ctx(xrt, name)
    nhit = int((hits["hit"] != 0).sum())
    assert 0 < nhit < len(rays) and counts["live"] == nhit
    light = lp.LightsScene(spec).light_hits(hits)[0]
    _, o_rgbf, o_st = cs.cast_rays(rays, max_reflections=0)
    assert o_st["shaded_hits"] == nhit
    assert (sp.bits(o_rgbf) != 0).any()
    assert sp.same_floats(surf["color"] * light, o_rgbf), name
    miss = hits["hit"] == 0
    assert (sp.bits(surf[miss]) == 0).all()
    for out in (refl, refr):
        assert (sp.bits(out["o"][miss]) == 0).all() and (sp.bits(out["d"][miss]) == 0).all()
        assert (out["ignore_mesh"][miss] == -1).all() and (out["ignore_tri"][miss] == -1).all()
    live = ~miss
    assert np.array_equal(surf["flags"][live] & 1, np.ones(nhit, dtype=np.int32)) and (surf["reserved"] == 0).all()
    assert np.array_equal(refl["ignore_mesh"][live], hits["mesh"][live]) and np.array_equal(refl["ignore_tri"][live], hits["tri"][live])
    # each output does not depend on the others being asked, and entries do not depend on their neighbours
    assert sp.same_surface(cs.surface_hits(hits)[0], surf)
    perm = np.random.default_rng(2).permutation(len(rays))
    s2, r2, t2, _ = cs.surface_hits(hits[perm], rays[perm])
    assert sp.same_outputs((s2, r2, t2), (surf[perm], refl[perm], refr[perm]))


@pytest.mark.parametrize("name", ["crate_grid", "glass", "content", "two_mesh"])
def test_next_rays_are_the_rays_castray_casts(xrt, name):
    """orc_paths_run at MaxReflections 1 keeps CastRay's segments and its `ref ray`: the oracle's hit of the checker's reflected ray is the end
    vertex of the reflection's white segment (and the reflection has no segment where that ray hits nothing), and the checker's refracted ray
    is the ray CastRay leaves behind for a Transparent root; any other root leaves its ray as it was."""
    spec, cs, rays, hits, (surf, refl, refr, counts) = ctx(xrt, name)
    res = paths_py.PathsScene(spec).cast_rays_paths(rays, max_reflections=1)
    rec_ray, rec_node, rec_kind, rec_v = res.recs
    n = len(rays)
    live = np.flatnonzero(hits["hit"] != 0)
    # node 0 of every ray: the root's own hit, which is the hit the checker was given
    root = (rec_node == 0) & (rec_kind == 0)
    assert np.array_equal(rec_ray[root], live) and sp.same_floats(rec_v[root], hits["w"][live])
    # node 1: the reflection (ray trees: 2 * 0 + 1, chains: generation 1)
    at = (rec_node == 1) & (rec_kind == 0)
    has = np.zeros(n, dtype=bool); has[rec_ray[at]] = True
    end = np.zeros((n, 3), dtype=np.float32); end[rec_ray[at]] = rec_v[at]
    r_hits, _ = cs.intersect(refl[live])
    assert np.array_equal(has[live], r_hits["hit"] != 0), name
    assert has.sum() > 0 and not has[hits["hit"] == 0].any()
    assert sp.same_floats(r_hits["w"][r_hits["hit"] != 0], end[live][has[live]]), name
    # the `ref ray`
    t = (surf["flags"] & sp.SURF_TRANSPARENT) != 0
    assert int(t.sum()) == counts["transparent"]
    if name in ("glass", "content"):
        assert counts["transparent"] > 0
    back = res.rays_back
    assert sp.same_floats(back["o"][t], refr["o"][t]) and sp.same_floats(back["d"][t], refr["d"][t]), name
    assert sp.same_bits(back["o"][~t], rays["o"][~t]) and sp.same_bits(back["d"][~t], rays["d"][~t])
    # ... and the refraction's own node (2) was cast with that direction
    cast = (rec_node == 2) & (rec_kind == 1)
    assert np.array_equal(rec_ray[cast], np.flatnonzero(t)) and sp.same_floats(rec_v[cast], refr["d"][t])
    # currentRefIndex 1.0 is not the material's index: the nested call receives n2 = 1 (RT:663-667); an opaque hit keeps the caller's index
    assert (surf["refraction_index"][t] != 1.0).all() and sp.same_floats(surf["next_ref_index"][hits["hit"] != 0], np.ones(len(live), dtype=np.float32))


def test_the_scenes_cover_every_kind_of_entry(xrt):
    """What the GPU parity test asserts of its scenes as a whole, from the checker's counts alone: hits and misses, interpolated and flat
    normals, textured and untextured, Transparent and opaque entries."""
    total = dict.fromkeys(sp.COUNTS, 0)
    n = 0
    for name in NAMES:
        spec, cs, rays, hits, out = ctx(xrt, name)
        n += len(rays)
        for k, v in out[3].items():
            total[k] += v
    live = total["live"]
    assert 0 < live < n
    for k in ("interpolated", "textured", "transparent"):
        assert 0 < total[k] < live, (k, total)
    assert total["index_equal"] + total["index_differs"] == total["transparent"] == total["cos_nonneg"] + total["cos_neg"]


@pytest.mark.parametrize("name", ["glass", "content"])
def test_every_refraction_branch_occurs(xrt, name):
    """The batches the GPU test uses for RT:656-694: rays from outside and from inside, current index equal to the material's and not, and a
    total internal reflection (a NaN direction, written as it is)."""
    spec, cs, rays, hits, (surf, refl, refr, counts) = ctx(xrt, name)
    total = dict.fromkeys(sp.COUNTS, 0)
    for what, r, h, cur in sp.refraction_cases(rays, hits, surf):
        s2, r2, t2, c = cs.surface_hits(h, r, ref_index=cur)
        for k, v in c.items():
            total[k] += v
        assert c["transparent"] == len(h) == c["live"]
        equal = cur != 1.0
        assert (c["index_equal"], c["index_differs"]) == ((len(h), 0) if equal else (0, len(h))), what
        assert sp.same_floats(s2["next_ref_index"], np.full(len(h), cur if equal else 1.0, dtype=np.float32)), what
        nan = np.isnan(t2["d"]).any(axis=1)
        assert int(nan.sum()) == c["nan_direction"] and (c["nan_direction"] == 0) == equal, what   # (n1 / n2 = 1 / index < 1 never reflects totally)
        assert np.isnan(t2["d"][nan]).all() and sp.same_bits(t2["o"][nan], h["w"][nan])
    for k in ("index_equal", "index_differs", "cos_nonneg", "cos_neg", "nan_direction"):
        assert total[k] > 0, (k, total)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("filtering", [0, 1])
def test_address_modes_and_filters_reach_the_lookup(xrt, mode, filtering):
    """The checker's colour on the textured crate is the oracle's SurfaceColor under every address mode and filter: colour * light is
    orc_cast_rays' vector with the same options, with uv pushed outside [0, 1] so that the modes differ."""
    import copy
    base = _specs(xrt)["crate"]
    spec = copy.copy(base)
    spec.address_mode, spec.filtering = mode, filtering
    cs = sp.SurfaceScene(spec)
    rays = cs.primary_rays()
    hits, _ = cs.intersect(rays)
    surf = cs.surface_hits(hits)[0]
    assert (surf["flags"][hits["hit"] != 0] & sp.SURF_TEXTURED).all()
    light = lp.LightsScene(spec).light_hits(hits)[0]
    assert sp.same_floats(surf["color"] * light, cs.cast_rays(rays, max_reflections=0)[1])
    assert sp.same_surface(cs.surface_hits(hits, address_mode=mode, filtering=filtering)[0], surf)
    # u, v beyond the triangle: uv leaves [0, 1] and the address modes part ways
    wide = hits.copy()
    wide["u"] = wide["u"] * np.float32(3.0) - np.float32(1.0)
    wide["v"] = wide["v"] * np.float32(-2.5) + np.float32(0.75)
    got = {m: cs.surface_hits(wide, address_mode=m, filtering=filtering)[0] for m in (0, 1, 2)}
    assert sp.same_floats(got[0]["uv"], got[1]["uv"]) and sp.same_floats(got[0]["normal"], got[2]["normal"])
    assert not sp.same_floats(got[0]["color"], got[1]["color"]) and not sp.same_floats(got[1]["color"], got[2]["color"])


def test_host_program_under_the_sanitizers():
    """tests/surface/host_surface.cpp on a host-only scene, host code under ASan and UBSan, a program of its own (nothing is preloaded, no
    GPU): every XRT_E_INVALID_ARG case in the header's order, the first offending index in the message, n == 0, then XRT_E_NO_DEVICE, nothing
    written on failure."""
    exe = sp.build_checked()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and "host_surface: ok" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]


def test_python_binding_checks_its_arguments(xrt):
    spec = xrt.configs.crate_scene(8, 8, max_reflections=1)
    scene, tracer = xrt.configs.build_product(spec, device=-1)
    hits = np.zeros(4, dtype=xrt.HIT_DTYPE)
    rays = np.zeros(4, dtype=xrt.RAY_DTYPE)
    with pytest.raises(ValueError):
        tracer.SurfaceHits(hits, want_surface=False)
    with pytest.raises(ValueError):
        tracer.SurfaceHits(hits, want_reflect=True)            # a ray output without rays
    with pytest.raises(ValueError):
        tracer.SurfaceHits(hits, rays[:3], want_refract=True)
    out = tracer.SurfaceHits(hits[:0])
    assert out.dtype == xrt.SURFACE_DTYPE and out.shape == (0,)
    s, r, t = tracer.SurfaceHits(hits[:0], rays[:0], want_reflect=True, want_refract=True)
    assert r.dtype == xrt.RAY_DTYPE and t.shape == (0,)
    hits["hit"][2] = 1
    hits["tri"][2] = spec.meshes[0][0].ntri
    with pytest.raises(ValueError) as e:
        tracer.SurfaceHits(hits)
    assert "hit 2 " in str(e.value)


def test_no_contracted_multiply_add_in_the_kernel(tmp_path):
    """The rule of test_numerics_contract.py (check_no_contracted_fma) on the ISA of surface.hip, compiled with the Makefile's flags, and what
    this kernel adds to it: its f32 fmas are divisions' and square roots' alone, its doubles the square root of RT:676-679 and the two
    remainders of MAT:168-169.  And the kernel's resources: no scratch, 16 bytes of LDS (the count cells)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bsurface\.hip\b", mk, flags=re.M) and re.search(r"for k in [^;]*\bsurface\b", mk)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    flags = [f for f in flags if not f.startswith("$(") and not f.startswith("--offload-arch")] + ["--offload-arch=gfx950"]
    assert "-ffp-contract=off" in flags
    out = str(tmp_path / "surface.s")
    p = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-x", "hip", os.path.join(CSRC, "surface.hip"), "--cuda-device-only", "-S", "-o", out,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    ks = kernels(open(out).read())
    assert [k for k in ks if "k_surface" in k] and len(ks) == 1
    for name, lines in ks.items():
        got = check_no_contracted_fma(name, "\n".join(lines))
        assert got["div"] > 0 and got["sqrt"] > 0 and got["idiv"] == 0, (name, got)   # (no 64-bit integer division here: every f32 fma is a division's or a square root's)
        assert got["f64"] == (0, 1, 2), got   # Snell's square root and the two IEEERemainders; no light, so no SPOT:54 division
    usage = p.stderr
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", usage) and re.search(r"LDS Size \[bytes/block\]: 16\b", usage), usage[-2000:]
