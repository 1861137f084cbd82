"""xrt_compose_hits (the return path of CastRay, one level: RT:584, 699, 705, 726, 732) and xrt_fold_samples (RT:309) without a GPU: the
exports in every binding, the checker (tests/compose) pinned against the oracle's own CastRay -- one level composed by hand from the
checkers' surface records, light sums and the colours of CastRay on the next rays is CastRay on the rays, and so is the whole recursion
driven by hand -- and against the oracle's XRT_MS_FIXED16 frames, the synthetic table the GPU test feeds, the argument checks on a
host-only scene in a host program under ASan and UBSan, the numerical contract on the ISA of compose.hip, and the one home of the shared
statements.  Every comparison is bit for bit; a NaN equals a NaN of any payload."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compose_py as cp
import lights_py as lp
import pixels_py as px
import surface_py as sp
import trace_py as tp
from test_gpu_cast_rays import scenes, two_mesh_spec
from test_numerics_contract import check_no_contracted_fma, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")
EXPORTS = ("xrt_compose_hits", "xrt_compose_hits_device", "xrt_fold_samples", "xrt_fold_samples_device")
NAMES = ["crate", "crate_grid", "glass", "heightfield", "content", "two_mesh"]
LEVELS = [(0, 0), (0, 1), (0, 3), (1, 3), (2, 2)]   # (iteration, max_reflections)
_CTX = {}


def _specs(xrt):
    out = dict(scenes(xrt))
    out["two_mesh"] = two_mesh_spec(xrt)
    return out


def ctx(xrt, name):
    """(spec, the surface checker's scene, the light checker's scene, the camera's rays), made once."""
    if name not in _CTX:
        spec = _specs(xrt)[name]
        cs = sp.SurfaceScene(spec)
        _CTX[name] = (spec, cs, lp.LightsScene(spec), cs.primary_rays())
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
    assert callable(getattr(xrt.RayTracer, "ComposeHits", None)) and callable(getattr(xrt.RayTracer, "FoldSamples", None))
    # the header no longer sends the host off to do the arithmetic itself
    assert "compose as RT:584/699/726 do" not in hdr and "folded by the RT:309 mean of means" not in hdr
    # the kernel's block size and block cap, which the GPU test sizes its lists around
    src = open(os.path.join(CSRC, "compose.h")).read()
    assert int(re.search(r"COMPOSE_BLOCK = (\d+);", src).group(1)) % 64 == 0 and int(re.search(r"COMPOSE_MAX_BLOCKS = (\d+);", src).group(1)) > 0


@pytest.mark.parametrize("name", NAMES)
def test_one_level_by_hand_is_the_oracles_castray(xrt, name):
    """One level composed from SurfaceScene.surface_hits, LightsScene.light_hits and orc_cast_rays on reflect_out / refract_out at
    iteration + 1 (the refraction grouped by next_ref_index and cast with it) equals orc_cast_rays on the rays, in packed colours and in
    colour vectors, at every (iteration, max_reflections) pair."""
    spec, cs, ls, rays = ctx(xrt, name)
    for iteration, m in LEVELS:
        ops = cp.OracleOps(spec, m, cs, ls)
        rgba, rgbf = cp.cast_by_hand(ops, rays, iteration, m)
        o_rgba, o_rgbf, _ = cs.cast_rays(rays, iteration=iteration, max_reflections=m)
        assert np.array_equal(rgba, o_rgba) and cp.same_floats(rgbf, o_rgbf), (name, iteration, m)
        assert (ops.cast_calls > 0) == (iteration < m)
        assert len(np.unique(o_rgba)) > 3, (name, iteration, m)


@pytest.mark.parametrize("name,m", [("glass", 2), ("content", 1)])
def test_the_whole_recursion_by_hand(xrt, name, m):
    """The same recursion driven to the bottom: no orc_cast_rays call below the top."""
    spec, cs, ls, rays = ctx(xrt, name)
    ops = cp.OracleOps(spec, m, cs, ls)
    rgba, rgbf = cp.cast_by_hand(ops, rays, 0, m, hand_levels=99)
    assert ops.cast_calls == 0
    o_rgba, o_rgbf, _ = cs.cast_rays(rays, max_reflections=m)
    assert np.array_equal(rgba, o_rgba) and cp.same_floats(rgbf, o_rgbf), name


def test_the_scenes_cover_every_kind_of_entry(xrt):
    """What the GPU test relies on: misses, opaque hits and Transparent hits over the scenes, NaN refraction directions on `glass` and
    `content`, and entries that take RT:699."""
    miss = opaque = glassy = 0
    for name in NAMES:
        spec, cs, ls, rays = ctx(xrt, name)
        hits, _ = cs.intersect(rays)
        surf, refl, refr, _ = cs.surface_hits(hits, rays)
        t = (surf["flags"] & cp.SURF_TRANSPARENT) != 0
        miss += int((surf["flags"] == 0).sum())
        glassy += int(t.sum())
        opaque += int(((surf["flags"] & cp.SURF_HIT) != 0).sum() - t.sum())
        if name in ("glass", "content"):
            assert t.sum() > 0 and np.isnan(refr["d"][t]).any(axis=1).sum() > 0, name
            light = ls.light_hits(hits)[0]
            colours = np.arange(len(rays), dtype=np.uint32) * np.uint32(2654435761)
            _, _, counts = cp.compose_hits(surf, light, colours, colours[::-1].copy())
            assert counts["refracted"] == int(t.sum()) and counts["miss"] == int((surf["flags"] == 0).sum())
    assert miss > 0 and opaque > 0 and glassy > 0


@pytest.mark.parametrize("name", ["crate_grid", "glass"])
def test_fold_is_the_oracles_fixed16_frame(xrt, orc, name):
    """orc_fold_samples of orc_cast_rays colours at the sixteen positions of a pixel equals the oracle's XRT_MS_FIXED16 frame there, on pixels
    across an edge; samples == 4 equals pixels_py.mean4."""
    spec, cs, ls, _ = ctx(xrt, name)
    osc = orc.OracleScene(spec)
    f16, f16f = px.oracle_frame(orc, osc, px.with_mode(spec, xrt.abi.MS_FIXED16))
    centers = edge_pixels(f16)
    c16 = cs.cast_rays(tp.oracle_rays(orc, spec, tp.sample_centers(centers, True)))[0]
    rgba, rgbf = cp.fold_samples(c16, 16)
    x, y = centers[:, 0].astype(int), centers[:, 1].astype(int)
    assert np.array_equal(rgba, f16[y, x]) and cp.same_bits(rgbf, f16f[y, x]), name
    assert sum(len(set(c16[16 * i:16 * i + 16].tolist())) > 1 for i in range(len(centers))) >= 4
    q, _ = cp.fold_samples(c16, 4)
    assert q.tolist() == [px.mean4(orc, c16[4 * i:4 * i + 4]) for i in range(len(q))]
    assert rgba.tolist() == [px.mean16(orc, c16[16 * i:16 * i + 16]) for i in range(len(rgba))]


def edge_pixels(frame, most=24):
    """Pixels of a frame whose right neighbour has another colour, and those neighbours -> (n, 2) float32 centres."""
    y, x = np.nonzero(frame[:, :-1] != frame[:, 1:])
    assert len(x) >= 4
    pick = np.linspace(0, len(x) - 1, min(most // 2, len(x))).astype(int)
    return np.array([(x[i] + d, y[i]) for i in pick for d in (0, 1)], dtype=np.float32)


def test_edge_table():
    """The synthetic table the GPU test feeds: every class occurs, and the checker's answers show that the classes do what they are for."""
    surface, light, reflect, refract, classes = cp.edge_table()
    n = len(surface)
    assert cp.edge_table()[0] is surface and n > 256 and not surface.flags.writeable
    f = surface["flags"][classes["flags"]]
    assert set((f & 15).tolist()) == set(range(16))
    for low in range(16):
        assert len(set(f[(f & 15) == low].tolist())) >= 4, low      # with and without bits the call ignores
    assert (surface["reserved"][classes["flags"]] != 0).any()
    s = classes["special"]

    def kinds(a):
        a = np.asarray(a, dtype=np.float32).reshape(-1)
        return (np.isnan(a).any(), (a == np.inf).any(), (a == -np.inf).any(), ((a == 0) & np.signbit(a)).any(), ((a < 0) & np.isfinite(a)).any(),
                ((a > 1) & np.isfinite(a)).any())
    for what in (surface["color"][s], light[s], surface["reflectiveness"][s], surface["alpha"][s]):
        assert all(kinds(what)), kinds(what)
    u = classes["unit"]
    assert set(zip(surface["alpha"][u].tolist(), surface["reflectiveness"][u].tolist())) == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}
    for col in (reflect, refract):
        for shift in (0, 8, 16):
            for start in (0, n - 256):
                assert len(set(((col[start:start + 256] >> shift) & 255).tolist())) == 256
        assert len(set((col >> 24).tolist())) > 100   # (the alpha byte, ignored)
    # the halves: light * colour lands below, on and above (k + 0.5) / 255 and the packed channel steps from k to k + 1 across them
    h = classes["halves"].reshape(255, 5)
    rgba, rgbf, counts = cp.compose_hits(surface, light)
    for k in range(255):
        ch = k % 3
        v = rgbf[h[k], ch]
        assert v[0] < v[1] < v[2] < v[3] < v[4] and v[2] == np.float32((k + 0.5) / 255.0)
        got = ((rgba[h[k]] >> (8 * ch)) & 255).tolist()
        assert got[0] == k and got[4] == k + 1 and got == sorted(got), (k, got)   # (4 ulp away: across the half; between them whatever the roundings give)
    assert counts["nan_vector"] > 0 and counts["miss"] > 0 and counts["hit"] > 0
    # every branch answers differently on this table, an ignored bit changes nothing, and entries do not depend on their neighbours
    a = cp.compose_hits(surface, light, reflect)
    b = cp.compose_hits(surface, light, reflect, refract)
    assert b[2]["refracted"] > 0
    assert not np.array_equal(rgba, a[0]) and not np.array_equal(a[0], b[0])
    t = (surface["flags"] & (cp.SURF_HIT | cp.SURF_TRANSPARENT)) == (cp.SURF_HIT | cp.SURF_TRANSPARENT)
    assert np.array_equal(a[0][~t], b[0][~t]) and cp.same_floats(a[1][~t], b[1][~t])
    masked = surface.copy()
    masked["flags"] &= 3
    masked["reserved"] = 0
    m = cp.compose_hits(masked, light, reflect, refract)
    assert np.array_equal(m[0], b[0]) and cp.same_floats(m[1], b[1])
    black = (surface["flags"] & cp.SURF_HIT) == 0
    assert (b[0][black] == 0xFF000000).all() and (cp.bits(b[1][black]) == 0).all()
    perm = np.random.default_rng(3).permutation(n)
    p = cp.compose_hits(surface[perm], light[perm], reflect[perm], refract[perm])
    assert np.array_equal(p[0], b[0][perm]) and cp.same_floats(p[1], b[1][perm])
    # alpha bytes are ignored
    c = cp.compose_hits(surface, light, reflect ^ np.uint32(0xFF000000), refract | np.uint32(0xFF000000))
    assert np.array_equal(c[0], b[0]) and cp.same_floats(c[1], b[1])


def test_host_program_under_the_sanitizers():
    """tests/compose/host_compose.cpp on a host-only scene, host code under ASan and UBSan, a program of its own (nothing is preloaded, no
    GPU): every XRT_E_INVALID_ARG case of both entry-point pairs in the header's order with its message, n == 0, then XRT_E_NO_DEVICE,
    nothing written on failure."""
    exe = cp.build_checked()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and "host_compose: ok" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]


def test_python_binding_checks_its_arguments(xrt):
    spec = xrt.configs.crate_scene(8, 8, max_reflections=1)
    scene, tracer = xrt.configs.build_product(spec, device=-1)
    surf = np.zeros(4, dtype=xrt.SURFACE_DTYPE)
    light = np.zeros((4, 3), dtype=np.float32)
    col = np.zeros(4, dtype=np.uint32)
    bad = [lambda: tracer.ComposeHits(surf, light, None, col),                                 # refract without reflect
           lambda: tracer.ComposeHits(surf, light[:3]), lambda: tracer.ComposeHits(surf, light.astype(np.float64)),
           lambda: tracer.ComposeHits(surf.view(np.float32).reshape(4, 16), light), lambda: tracer.ComposeHits(surf, light.reshape(-1)),
           lambda: tracer.ComposeHits(surf, light, col[:3]), lambda: tracer.ComposeHits(surf, light, col.astype(np.int64)),
           lambda: tracer.ComposeHits(surf, light, col, col.reshape(2, 2)),
           lambda: tracer.FoldSamples(col, samples=8), lambda: tracer.FoldSamples(np.zeros(17, dtype=np.uint32)),
           lambda: tracer.FoldSamples(np.zeros(16, dtype=np.float32)), lambda: tracer.FoldSamples(np.zeros(6, dtype=np.uint32), samples=4)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError) as e:
            call()
        assert "libxrt" not in str(e.value), k       # (raised before the library is called)
    out = tracer.ComposeHits(surf[:0], light[:0])
    assert out.dtype == np.uint32 and out.shape == (0,)
    rgba, rgbf = tracer.ComposeHits(surf[:0], light[:0], col[:0], col[:0], want_float=True)
    assert rgba.shape == (0,) and rgbf.shape == (0, 3) and rgbf.dtype == np.float32
    rgba, rgbf = tracer.FoldSamples(col[:0], want_float=True)
    assert rgba.shape == (0,) and rgbf.shape == (0, 3)
    # arrays in order: the library is asked, and the scene has no device
    for call in (lambda: tracer.ComposeHits(surf, light), lambda: tracer.ComposeHits(surf, light, col, col, want_float=True),
                 lambda: tracer.FoldSamples(np.zeros(32, dtype=np.uint32)), lambda: tracer.FoldSamples(np.zeros(8, dtype=np.uint32), samples=4)):
        with pytest.raises(xrt.abi.XrtError) as e:
            call()
        assert e.value.code == xrt.abi.XRT_E_NO_DEVICE


def test_no_contracted_multiply_add_in_the_kernel(tmp_path):
    """The rule of test_numerics_contract.py (check_no_contracted_fma) on the ISA of compose.hip, compiled with the Makefile's flags, and what
    this kernel adds to it: every f32 fma is a division's (ToVector3's / 255), there is no double and no square root.  And the kernel's
    resources: no scratch, 16 bytes of LDS (the count cells)."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bcompose\.hip\b", mk, flags=re.M) and re.search(r"^HDRS\s*:=.*\bcompose\.h\b", mk, flags=re.M)
    assert re.search(r"^asm:\n(?:\t.*\n)*\t.*\bcompose\.hip\b.*-o compose\.s\b", mk, flags=re.M) and re.search(r"rm -f .*\bcompose\.s\b", mk)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    flags = [f for f in flags if not f.startswith("$(") and not f.startswith("--offload-arch")] + ["--offload-arch=gfx950"]
    assert "-ffp-contract=off" in flags
    out = str(tmp_path / "compose.s")
    p = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-x", "hip", os.path.join(CSRC, "compose.hip"), "--cuda-device-only", "-S", "-o", out,
                        "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    ks = kernels(open(out).read())
    assert [k for k in ks if "k_compose_hits" in k] and len(ks) == 1
    for name, lines in ks.items():
        text = "\n".join(lines)
        got = check_no_contracted_fma(name, text)
        assert got["div"] > 0 and got["sqrt"] == 0 and got["idiv"] == 0 and got["f64"] == (0, 0, 0), (name, got)
        assert not re.search(r"\bv_\w+_f64\b|\bv_sqrt_|\bv_rsq_", text), name
    usage = p.stderr
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", usage) and re.search(r"LDS Size \[bytes/block\]: 16\b", usage), usage[-2000:]


def test_the_return_path_is_stated_once():
    """compose_last, compose_step, compose_refraction (RT:726 / 584 / 699) and mean4 (RT:309) are defined in shade_math.h alone -- a definition
    under a prefixed name is a copy too -- and their statements stand nowhere else in csrc, whatever they are called (the pattern of
    test_host_logic.py test_shared_device_statements_are_defined_once)."""
    names = ("compose_last", "compose_step", "compose_refraction", "mean4")
    statements = {"compose_step": r"mul\(\s*lerp\(\s*unpack_color\(", "compose_refraction": r"=\s*lerp\(\s*unpack_color\(|return lerp\(\s*unpack_color\(",
                  "mean4": r"add\(add\(add\(unpack_color\("}
    found = {n: [] for n in names}
    users = {n: set() for n in names}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".cpp", ".h", ".hip")):
            continue
        src = open(os.path.join(CSRC, f)).read()
        for d in re.findall(r"^\s*(?:static\s+)?(?:__host__\s+)?(?:__device__\s+)?(?:__forceinline__\s+|inline\s+)?[\w:]+ [*&]?(\w+)\([^;{]*\)\s*\{", src, re.M):
            for n in names:
                if d == n or d.endswith("_" + n):
                    found[n].append((f, d))
        for n, text in statements.items():
            if re.search(text, src) and not any(g == f for g, _ in found[n]):
                found[n].append((f, "<unnamed>"))
        code = re.sub(r"//[^\n]*", "", src)
        for n in names:
            if re.search(r"\b%s\(" % n, code) and f != "shade_math.h":
                users[n].add(f)
    for n in names:
        assert found[n] == [("shade_math.h", n)], (n, found[n])
    assert users["compose_last"] >= {"kernels.hip", "compose.hip"} and users["compose_step"] >= {"kernels.hip", "compose.hip"}
    assert users["compose_refraction"] >= {"kernels.hip", "compose.hip"} and users["mean4"] >= {"kernels.hip", "pixels.hip"}
