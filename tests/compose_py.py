"""TEST INFRASTRUCTURE -- ctypes binding of tests/compose/libcompose.so, the checker of xrt_compose_hits and xrt_fold_samples.

compose_ref.cpp: the CPU oracle (oracle/oracle.cpp, included unmodified through tests/castray/castray_ref.cpp) plus orc_compose_hits -- one
level of the return path of its CastRay (RT:584, 699, 705, 726, 732) -- and orc_fold_samples (RT:309), written with the oracle's own Lerp,
ColorFromVector3 and ColorToVector3.  tests/test_compose_cpu.py pins both against the oracle's CastRay and its XRT_MS_FIXED16 frames.

Also here: edge_table(), the synthetic inputs the GPU test feeds, and cast_by_hand(), CastRay's recursion driven from outside through a set of
calls -- the checkers' on the CPU, the product's on the GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import castray_py
import lights_py as lp
import surface_py as sp

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
LIB = os.path.join(_HERE, "compose", "libcompose.so")
SRC = os.path.join(_HERE, "compose", "compose_ref.cpp")
DEPS = [SRC, os.path.join(_HERE, "castray", "castray_ref.cpp"), os.path.join(_ROOT, "oracle", "oracle.cpp"), os.path.join(_ROOT, "oracle", "xna_math.h"),
        os.path.join(_ROOT, "include", "xrt.h")]
COUNTS = ("hit", "refracted", "nan_vector", "miss")
SURFACE_DTYPE = sp.SURFACE_DTYPE
SURF_HIT, SURF_TRANSPARENT = sp.SURF_HIT, sp.SURF_TRANSPARENT
_lib = None

bits, same_bits, same_floats = sp.bits, sp.same_bits, sp.same_floats


def build():
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in DEPS):
        return
    subprocess.check_call(["g++"] + castray_py.FLAGS + ["-shared", "-o", LIB, SRC])


def build_checked():
    """The host program of xrt_compose_hits / xrt_fold_samples on a host-only scene under ASan + UBSan (csrc/Makefile `hostcheck_compose`)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_compose"])
    return os.path.join(CSRC, "hostcheck_compose")


def lib():
    global _lib
    if _lib is None:
        build()
        l = C.CDLL(LIB)
        l.orc_compose_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        l.orc_fold_samples.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        _lib = l
    return _lib


def compose_hits(surface, light, reflect=None, refract=None):
    """orc_compose_hits -> (rgba uint32[n], colour vectors float32[n, 3], counts dict of COUNTS)."""
    surface = np.ascontiguousarray(surface, dtype=SURFACE_DTYPE)
    n = surface.shape[0]
    light = np.ascontiguousarray(light, dtype=np.float32)
    assert light.shape == (n, 3)
    cols = []
    for a in (reflect, refract):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.uint32)
            assert a.shape == (n,)
        cols.append(a)
    rgba, rgbf = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=np.float32)
    counts = np.zeros(len(COUNTS), dtype=np.uint64)
    rc = lib().orc_compose_hits(surface.ctypes.data, light.ctypes.data, cols[0].ctypes.data if cols[0] is not None else None,
                                cols[1].ctypes.data if cols[1] is not None else None, n, rgba.ctypes.data, rgbf.ctypes.data, counts.ctypes.data)
    if rc != 0:
        raise RuntimeError("orc_compose_hits failed: %d" % rc)
    return rgba, rgbf, dict(zip(COUNTS, (int(v) for v in counts)))


def fold_samples(colors, samples):
    """orc_fold_samples -> (rgba uint32[n], ToVector3() of it float32[n, 3])."""
    colors = np.ascontiguousarray(colors, dtype=np.uint32).reshape(-1)
    assert colors.size % samples == 0
    n = colors.size // samples
    rgba, rgbf = np.zeros(n, dtype=np.uint32), np.zeros((n, 3), dtype=np.float32)
    rc = lib().orc_fold_samples(colors.ctypes.data, n, int(samples), rgba.ctypes.data, rgbf.ctypes.data)
    if rc != 0:
        raise RuntimeError("orc_fold_samples failed: %d" % rc)
    return rgba, rgbf


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, -0.5, 1.5)   # NaN, +-inf, -0.0, < 0, > 1
_TABLE = None


def edge_table():
    """A deterministic table of entries for xrt_compose_hits -> (surface SURFACE_DTYPE[n], light float32[n, 3], reflect uint32[n],
    refract uint32[n], classes), classes naming the rows of every class (index arrays):
      "flags"    every combination of the four XRT_SURF_* bits, with and without bits the call ignores, non-zero reserved words;
      "special"  colour, light, reflectiveness and alpha channels at NaN, +-inf, -0.0, < 0 and > 1, one at a time, on Transparent hits;
      "halves"   light * colour 4 ulp and 1 ulp below, on, and 1 ulp and 4 ulp above the RGBA8 halves (k + 0.5) / 255, k = 0 .. 254 (five rows
                 per k), Reflectiveness 0;
      "unit"     alpha and reflectiveness at 0 and 1 in every combination;
    and, over any 256 consecutive rows, all 256 byte values in every colour channel of reflect and refract (their alpha bytes vary too).
    The fields the call does not read (normal, uv, the refraction indices) hold arbitrary values, NaN among them.  Made once; do not write
    to it."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    rng = np.random.default_rng(7)
    rows, classes = [], {"flags": [], "special": [], "halves": [], "unit": []}

    def row(flags, color=None, light=None, refl=None, alpha=None, reserved=(0, 0, 0)):
        r = np.zeros((), dtype=SURFACE_DTYPE)
        r["normal"] = rng.normal(size=3).astype(np.float32)
        r["uv"] = rng.uniform(-1, 2, size=2).astype(np.float32)
        r["refraction_index"], r["next_ref_index"] = np.float32(rng.uniform(1, 2)), np.float32(1.0)
        if len(rows) % 5 == 0:
            r["normal"][len(rows) % 3] = np.nan   # (not read)
            r["uv"][0] = np.inf
        r["color"] = rng.uniform(0, 1, size=3).astype(np.float32) if color is None else np.asarray(color, dtype=np.float32)
        r["reflectiveness"] = np.float32(rng.uniform(0, 1)) if refl is None else np.float32(refl)
        r["alpha"] = np.float32(rng.uniform(0, 1)) if alpha is None else np.float32(alpha)
        r["flags"] = np.array(flags, dtype=np.uint32).view(np.int32)
        r["reserved"] = reserved
        l = rng.uniform(0, 1.2, size=3).astype(np.float32) if light is None else np.asarray(light, dtype=np.float32)
        rows.append((r, l))
        return len(rows) - 1

    for low in range(16):
        for high, reserved in ((0, (0, 0, 0)), (0x10, (1, 0, 0)), (0x7ffffff0, (-1, 7, 0x5a5a5a5a)), (0x80000000, (0, 0, -2))):
            for _ in range(2):
                classes["flags"].append(row(low | high, reserved=reserved))
    both = SURF_HIT | SURF_TRANSPARENT
    for value in SPECIALS:
        for ch in range(3):
            c = rng.uniform(0.1, 0.9, size=3).astype(np.float32); c[ch] = value
            classes["special"].append(row(both, color=c))
            l = rng.uniform(0.1, 0.9, size=3).astype(np.float32); l[ch] = value
            classes["special"].append(row(both, light=l))
        classes["special"].append(row(both, refl=value))
        classes["special"].append(row(both, alpha=value))
        classes["special"].append(row(SURF_HIT, refl=value, alpha=value))
    for k in range(255):
        h = np.float32((k + 0.5) / 255.0)
        far = np.float32(4) * np.spacing(h)   # (4 ulp of h move h * 255 by almost 4 of its own: across the half whatever the roundings do)
        for v in (np.float32(h - far), np.nextafter(h, np.float32(0)), h, np.nextafter(h, np.float32(1)), np.float32(h + far)):
            l = np.ones(3, dtype=np.float32); l[k % 3] = v
            classes["halves"].append(row(SURF_HIT | (SURF_TRANSPARENT if k & 1 else 0), color=(1.0, 1.0, 1.0), light=l, refl=0.0, alpha=1.0))
    for a in (0.0, 1.0):
        for r in (0.0, 1.0):
            for f in (SURF_HIT, both):
                classes["unit"].append(row(f, refl=r, alpha=a))
    surface = np.array([r for r, _ in rows], dtype=SURFACE_DTYPE)
    light = np.array([l for _, l in rows], dtype=np.float32)
    i = np.arange(len(rows), dtype=np.uint32)
    reflect = (i % 256) | (((i * 3 + 1) % 256) << 8) | ((255 - i % 256) << 16) | (((i * 5) % 256) << 24)
    refract = ((i * 7 + 3) % 256) | (((i + 128) % 256) << 8) | (((i * 11 + 5) % 256) << 16) | (((i * 13) % 256) << 24)
    for a in (surface, light, reflect, refract):
        a.setflags(write=False)
    _TABLE = (surface, light, reflect.astype(np.uint32), refract.astype(np.uint32), {k: np.array(v) for k, v in classes.items()})
    return _TABLE


def tiled_table(n, seed=None):
    """n entries of the edge table: all of them in turn (np.resize), shuffled when a seed is given."""
    surface, light, reflect, refract, _ = edge_table()
    pick = np.resize(np.arange(len(surface)), n)
    if seed is not None:
        pick = np.random.default_rng(seed).permutation(pick)
    return surface[pick].copy(), light[pick].copy(), reflect[pick].copy(), refract[pick].copy()


class HandOps:
    """The calls cast_by_hand drives, on numpy arrays: the query, the surface terms and next rays, the light sum, CastRay itself and the
    composition.  A subclass binds them to the checkers or to the product; the device path of the GPU test overrides the array helpers too."""
    cast_calls = 0

    def intersect(self, rays): raise NotImplementedError
    def surface(self, hits, rays, ref_index): raise NotImplementedError      # -> (surface, reflect rays, refract rays)
    def light(self, hits): raise NotImplementedError                         # -> (n, 3)
    def cast(self, rays, iteration, ref_index): raise NotImplementedError    # -> packed colours
    def compose(self, surface, light, reflect, refract): raise NotImplementedError   # -> (rgba, rgbf)
    # the array helpers
    def colors(self, n): return np.zeros(n, dtype=np.uint32)
    def flags(self, surface): return surface["flags"]
    def next_index(self, surface): return surface["next_ref_index"]
    def where(self, mask): return np.flatnonzero(mask)
    def values(self, x): return sorted(set(float(v) for v in x))


def cast_by_hand(ops, rays, iteration, max_reflections, ref_index=1.0, hand_levels=1, hits=None):
    """CastRay(rays[i], iteration, origin, currentRefIndex = ref_index) for every ray, its recursion driven from outside as RT:506-737 runs:
    the query (or the given hits), the surface terms and the two next rays, the light sum; with iteration < max_reflections the reflected
    rays of the hits and the refracted rays of the Transparent hits -- grouped by next_ref_index, each group cast with its index (RT:698) --
    at iteration + 1; then one composition.  The first `hand_levels` levels are composed this way and the level below them is ops.cast
    (with enough of them ops.cast is never called).  -> (rgba, rgbf)"""
    if hits is None:
        hits = ops.intersect(rays)
    surf, refl, refr = ops.surface(hits, rays, ref_index)
    light = ops.light(hits)
    if iteration >= max_reflections:
        return ops.compose(surf, light, None, None)   # RT:708-727

    def below(r, ref):
        if len(r) == 0:
            return ops.colors(0)
        if hand_levels > 1:
            return cast_by_hand(ops, r, iteration + 1, max_reflections, ref, hand_levels - 1)[0]
        ops.cast_calls += 1
        return ops.cast(r, iteration + 1, ref)

    n = len(rays)
    flags = ops.flags(surf)
    live = ops.where((flags & SURF_HIT) != 0)
    reflect = ops.colors(n)
    reflect[live] = below(refl[live], ref_index)   # RT:556-559: the reflection keeps currentRefIndex
    refract = ops.colors(n)
    glassy = (flags & (SURF_HIT | SURF_TRANSPARENT)) == (SURF_HIT | SURF_TRANSPARENT)
    nxt = ops.next_index(surf)
    for g in ops.values(nxt[glassy]):
        at = ops.where(glassy & (nxt == g))
        refract[at] = below(refr[at], g)   # RT:698
    return ops.compose(surf, light, reflect, refract)


class OracleOps(HandOps):
    """cast_by_hand on the checkers: SurfaceScene (query, CastRay, surface terms), LightsScene (light sum), orc_compose_hits."""

    def __init__(self, spec, max_reflections, surface_scene=None, lights_scene=None):
        self.cs = surface_scene if surface_scene is not None else sp.SurfaceScene(spec)
        self.ls = lights_scene if lights_scene is not None else lp.LightsScene(spec)
        self.max_reflections = max_reflections

    def intersect(self, rays): return self.cs.intersect(rays)[0]
    def surface(self, hits, rays, ref_index): return self.cs.surface_hits(hits, rays, ref_index=ref_index)[:3]
    def light(self, hits): return self.ls.light_hits(hits)[0]
    def cast(self, rays, iteration, ref_index): return self.cs.cast_rays(rays, iteration=iteration, ref_index=ref_index, max_reflections=self.max_reflections)[0]
    def compose(self, surface, light, reflect, refract): return compose_hits(surface, light, reflect, refract)[:2]
