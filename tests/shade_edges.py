"""TEST INFRASTRUCTURE -- the probe tables of the shading-edge sweep and what both of its modules need: tests/test_shade_edges_cpu.py (the oracle
pinned by a float64 restatement, and the population conditions on the oracle alone) and tests/test_gpu_shade_edges.py (the oracle against k_shade).

The probe construction: a triangle whose three vertices carry the same attribute value hands that value to the shading code exactly, whatever
the barycentrics are (in ix = (uv1x + ax*u) + bx*v both ax and bx are 0).  A PROBE MESH is a grid of small separate triangles in the plane
z = 0, facing +z, each with one probe value -- a UV, a colour, three vertex normals -- and one ray straight down into each.  Lit by a white
directional light (0, 0, 1) at Reflectiveness 0 and MaxReflections 0 the colour vector CastRay returns IS the surface colour.  Where the hit
position has to vary (lights, Snell) one large two-triangle plane is hit by a sweep of rays instead.

Families: T texture lookup inside its valid range, TOUT beyond it, Q quantisation, N fragment normal, L lights, S Snell refraction."""
import functools
import math

import numpy as np

f32 = np.float32
NAN, INF = float("nan"), float("inf")
CHUNK = 4096      # triangles of one probe mesh at most
COLS = 64         # probe triangles per grid row
FRAME_FLOOR = 300 # closest hits every frame of the sweep must have (at most 96 x 64 pixels; the probe triangles cover 9/32 of the plane)


def neighbours(x):
    """x as float32 with the float below and the float above it."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    return np.unique(np.concatenate([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]))


# ---- the probe mesh ------------------------------------------------------------------------------------------------------------------------------
def grid_xy(n, cols=COLS):
    """Integer grid places of n probes, centred on the origin."""
    i = np.arange(n)
    rows = (n + cols - 1) // cols
    return (i % cols - min(cols, n) // 2).astype(np.float32), (i // cols - rows // 2).astype(np.float32)


def probe_mesh(xrt, n, uv=None, color=None, normals=None, leg=0.75, z=0.0, down=False, cols=COLS):
    """n triangles (x, y, z), (x, y + leg, z), (x + leg, y, z) facing +z (down: the winding reversed, facing -z).  uv: (n, 2), color: (n, 4) or
    (n, 3), normals: (n, 3, 3) -- one value per triangle, copied to its vertices (normals: given per vertex)."""
    x, y = grid_xy(n, cols)
    v = np.zeros((n, 3, 3), dtype=np.float32)
    v[:, :, 0], v[:, :, 1], v[:, :, 2] = x[:, None], y[:, None], f32(z)
    v[:, 1, 1] += f32(leg)
    v[:, 2, 0] += f32(leg)
    if down:
        v = v[:, [0, 2, 1]]
    nrm = np.zeros((n, 3, 3), dtype=np.float32)
    nrm[:, :, 2] = -1.0 if down else 1.0
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float32).reshape(n, 3, 3)
    uvs = np.zeros((n, 3, 2), dtype=np.float32)
    if uv is not None:
        uvs[:] = np.asarray(uv, dtype=np.float32).reshape(n, 1, 2)
    col = np.ones((n, 4), dtype=np.float32)
    if color is not None:
        color = np.asarray(color, dtype=np.float32)
        col[:, :color.shape[1]] = color
    return xrt.fixtures.MeshData(v, nrm, uvs, col)


def probe_rays(xrt, n, off=(0.2, 0.2), z=5.0, cols=COLS):
    """One ray straight down into each probe triangle, `off` (one pair, or (n, 2)) from its right-angled corner."""
    x, y = grid_xy(n, cols)
    off = np.broadcast_to(np.asarray(off, dtype=np.float32), (n, 2))
    o = np.stack([x + off[:, 0], y + off[:, 1], np.full(n, f32(z))], axis=1)
    return xrt.rays_array(o, np.tile(np.array([0, 0, -1], dtype=np.float32), (n, 1)))


def plane_mesh(xrt, half, uv=None, normal=None, alpha=1.0):
    """The square [-half, half]^2 in z = 0 as two triangles facing +z; uv: the UVs of its corners (-,-), (+,-), (+,+), (-,+)."""
    h = f32(half)
    p = np.array([(-h, -h, 0), (h, -h, 0), (h, h, 0), (-h, h, 0)], dtype=np.float32)
    t = np.array([(0, 2, 1), (0, 3, 2)])
    v = p[t]
    nrm = np.tile(np.array((0, 0, 1) if normal is None else normal, dtype=np.float32), (2, 3, 1))
    uvs = np.zeros((2, 3, 2), dtype=np.float32)
    if uv is not None:
        uvs = np.asarray(uv, dtype=np.float32)[t]
    col = np.array([(0.8, 0.6, 0.4, alpha)] * 2, dtype=np.float32)
    return xrt.fixtures.MeshData(v, nrm, uvs, col)


def one_body(xrt, name, meshes, lights, max_reflections=0, size=(8, 8)):
    s = xrt.configs.SceneSpec(name)
    s.meshes = list(meshes)
    s.objects.append((list(range(len(meshes))), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.camera = xrt.configs.camera((0, 0, 5), (0, 0, 0))
    s.lights = list(lights)
    s.max_reflections = max_reflections
    return s.with_size(*size)


def overhead(xrt):
    """The light under which the colour vector is the surface colour: white, intensity 1, direction (0, 0, 1) -- surfaceDot = 1 on the plane (DIR:23-30)."""
    return xrt.configs.directional((0.0, 0.0, 1.0))


def spot_light(xrt, position, direction, angle, color=(1.0, 1.0, 1.0), intensity=1.0):
    return dict(kind=xrt.abi.LIGHT_SPOT, position=tuple(float(f32(c)) for c in position), direction=tuple(float(f32(c)) for c in direction),
                color=color, intensity=intensity, spot_angle=float(f32(angle)), decay_exponent=float(f32(1.3)))


# ---- T: texture lookup -----------------------------------------------------------------------------------------------------------------------------
TEXTURES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (100, 37), (64, 128)]   # (W, H)
ADDRESS = ("wrap", "clamp", "mirror")
FILTERS = ("point", "bilinear")
ORDINARY = 0.37    # the axis that is not probed
FAR = [2.0 ** 23, 2.0 ** 24 + 2, 2.0 ** 30]                                               # still inside the int range; fmod1 is 0 there
BEYOND = [2.0 ** 31, 2.0 ** 32 + 512, -2.0 ** 31, -2.0 ** 33, 3e38, INF, -INF, NAN]       # TOUT: where (int)(float) leaves the int range


def tex_id(t):
    return "%dx%d" % t


def address_of(xrt, name):
    return {"wrap": xrt.abi.ADDRESS_WRAP, "clamp": xrt.abi.ADDRESS_CLAMP, "mirror": xrt.abi.ADDRESS_MIRROR}[name]


def filter_of(xrt, name):
    return {"point": xrt.abi.FILTER_POINT, "bilinear": xrt.abi.FILTER_BILINEAR}[name]


@functools.lru_cache(maxsize=None)
def texture(w, h):
    """(argb, pargb) uint32 (h, w): every texel distinct, horizontal and vertical neighbours differ in every byte (alpha included), and the
    premultiplied copy RayTracerTexture makes (TEX:24-33: every channel times alpha / 255, truncated)."""
    x, y = np.meshgrid(np.arange(w, dtype=np.uint32), np.arange(h, dtype=np.uint32))
    r, g, b = (37 * x + 101 * y + 11) % 256, (59 * x + 83 * y + 7) % 256, (113 * x + 29 * y + 3) % 256
    a = 255 - (7 * x + 13 * y) % 64
    argb = (a << 24) | (r << 16) | (g << 8) | b
    pr, pg, pb = r * a // 255, g * a // 255, b * a // 255
    pargb = (a << 24) | (pr << 16) | (pg << 8) | pb
    return np.ascontiguousarray(argb, dtype=np.uint32), np.ascontiguousarray(pargb, dtype=np.uint32)


def axis_probes(n):
    """The probe values of one axis of an n-texel-wide texture: k/n and k/(n-1) with their float neighbours, over -3 .. +4 periods (every k for a
    small texture; one whole period and five k around every period boundary for a large one), the integers -3 .. 4 with theirs, +-0, the far values."""
    if n <= 8:
        ks = np.arange(-3 * n, 4 * n + 1)
    else:
        ks = np.unique(np.concatenate([np.arange(0, n + 1)] + [p * m + np.arange(-2, 3) for p in range(-3, 5) for m in (n, n - 1)]))
    vals = [ks.astype(np.float32) / f32(n)]
    if n > 1:
        vals.append(ks.astype(np.float32) / f32(n - 1))
    vals.append(np.arange(-3, 5).astype(np.float32))
    out = neighbours(np.concatenate(vals))
    far = np.array(FAR + [-v for v in FAR], dtype=np.float32)
    return np.concatenate([out, np.array([0.0, -0.0], dtype=np.float32), far])


def texel_centres(n):
    """One UV per texel of an axis under the point filter, x = (int)(u * (n - 1)) (MAT:147): the last texel is reached at u = 1 alone -- under Mirror,
    which flips the first period (MAT:115: (int)0 % 2 == 0), at u = 0 alone."""
    if n == 1:
        return np.array([0.5], dtype=np.float32)
    return np.concatenate([(np.arange(n - 1) + 0.5) / (n - 1), [1.0, 0.0]]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def uv_table(w, h):
    """(n, 2) float32: each axis probed with the other at ORDINARY, both axes probed together, and one probe at the centre of every texel."""
    xs, ys = axis_probes(w), axis_probes(h)
    m = max(len(xs), len(ys))
    i = np.arange(m)
    both = np.stack([xs[i % len(xs)], ys[(5 * i + 1) % len(ys)]], axis=1)
    cx, cy = np.meshgrid(texel_centres(w), texel_centres(h))
    parts = [np.stack([xs, np.full(len(xs), f32(ORDINARY))], axis=1), np.stack([np.full(len(ys), f32(ORDINARY)), ys], axis=1), both,
             np.stack([cx.reshape(-1), cy.reshape(-1)], axis=1)]
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


@functools.lru_cache(maxsize=None)
def uv_table_beyond():
    """TOUT: every BEYOND value in x with y ordinary, in y with x ordinary, and in both; then every pair with one in-range partner value."""
    b = np.array(BEYOND, dtype=np.float32)
    out = [(v, f32(ORDINARY)) for v in b] + [(f32(ORDINARY), v) for v in b] + [(v, v) for v in b]
    out += [(v, f32(2.75)) for v in b] + [(f32(-1.25), v) for v in b] + [(b[i], b[(i + 3) % len(b)]) for i in range(len(b))]
    return np.array(out, dtype=np.float32)


def texture_material(xrt, w, h):
    argb, pargb = texture(w, h)
    return xrt.configs.material(0.0, texture=argb, texture_pargb=pargb)


def texture_specs(xrt, w, h, table):
    """The probe scenes of a UV table, CHUNK triangles each: [(spec, rays, slice of the table)]."""
    out = []
    for at in range(0, len(table), CHUNK):
        uv = table[at:at + CHUNK]
        spec = one_body(xrt, "T_%dx%d_%d" % (w, h, at), [(probe_mesh(xrt, len(uv), uv=uv), texture_material(xrt, w, h))], [overhead(xrt)])
        out.append((spec, probe_rays(xrt, len(uv)), slice(at, at + len(uv))))
    return out


def set_sampling(xrt, spec, address, filtering):
    spec.address_mode, spec.filtering = address_of(xrt, address), filter_of(xrt, filtering)
    return spec


QUAD_UV = [(-3.5, -2.25), (4.5, -2.25), (4.5, 3.75), (-3.5, 3.75)]
QUAD_TEXTURES = [(7, 5), (100, 37)]


def quad_spec(xrt, w, h, size=(96, 64)):
    """The interpolated probe: a quad whose UVs run from (-3.5, -2.25) to (4.5, 3.75), with an oblique camera for its frame."""
    spec = one_body(xrt, "Tquad_%dx%d" % (w, h), [(plane_mesh(xrt, 4.0, uv=QUAD_UV), texture_material(xrt, w, h))], [overhead(xrt)], size=size)
    spec.camera = xrt.configs.camera((1.5, -7.0, 6.0), (0.2, 0.0, 0.0))
    return spec


def quad_rays(xrt, n=3000, seed=41):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-3.99, 3.99, size=(n, 2)), np.full((n, 1), 5.0)], axis=1)
    return xrt.rays_array(o, np.tile(np.array([0, 0, -1], dtype=np.float32), (n, 1)))


# ---- the float64 restatement of Material.cs (LookupUV, point filter) --------------------------------------------------------------------------------
def lookup_point_f64(uv, w, h, address):
    """Material.LookupUV with the point filter, restated in float64 from the text of Material.cs: the address mode (Wrap: a value above 1 becomes
    its fractional part, one below 0 becomes 1 + its (negative) fractional part; Mirror: the same, then the value is flipped to 1 - value when
    the whole number taken off is even; Clamp: to [0, 1]), then texel (trunc(u * (W - 1)), trunc(v * (H - 1))).
    -> (x, y, sure): `sure` where the answer does not depend on rounding: every value that is compared or truncated is at least 1e-3 of a
    texel away from the value at which the result changes, and the UV is small enough for float32 to hold that distance."""
    uv = np.asarray(uv, dtype=np.float64)
    out, sure = [], np.ones(len(uv), dtype=bool)
    for c, n in ((0, w), (1, h)):
        u = uv[:, c]
        tol = 1e-3 / n
        with np.errstate(all="ignore"):
            ok = np.isfinite(u) & (np.abs(u) < 16.0)
            u = np.where(ok, u, 0.5)
            inside = np.ones(len(u), dtype=bool)
            if address == "clamp":
                m = np.clip(u, 0.0, 1.0)
                ok &= (np.abs(u) > tol) | (u == 0)
                ok &= (np.abs(u - 1) > tol) | (u == 1)
                inside = (u > 0) & (u < 1)                   # (clamped values are exactly 0 or 1: texel 0 or n - 1)
            else:
                whole = np.where(u > 1, np.trunc(u), np.where(u < 0, np.trunc(u) - 1, 0.0))
                m = u - whole
                ok &= np.abs(u - np.round(u)) > tol          # away from every period boundary
                if address == "mirror":
                    m = np.where(whole % 2 == 0, 1.0 - m, m)
            t = m * (n - 1)
            if n > 1:
                ok &= ~inside | (np.abs(t - np.round(t)) > 1e-3)         # away from every texel boundary
            out.append(np.trunc(t).astype(np.int64))
            sure &= ok
    return out[0], out[1], sure


def texel_rgb_f64(argb, x, y):
    """The colour GetColorPoint returns for a texel: its R, G, B bytes times 1/255 (float32 BYTE_RECIPROCAL), as float32."""
    t = argb[y, x]
    rec = f32(1.0) / f32(255.0)
    return np.stack([((t >> 16) & 255).astype(np.float32) * rec, ((t >> 8) & 255).astype(np.float32) * rec, (t & 255).astype(np.float32) * rec], axis=1)


def texel_of_colour(argb, rgbf):
    """Which texel a point-filtered colour vector names (every texel is distinct): (n,) flat index, -1 where it is none."""
    key = np.rint(np.asarray(rgbf, dtype=np.float64) * 255.0)
    with np.errstate(invalid="ignore"):
        good = np.isfinite(key).all(axis=1) & (np.abs(key / 255.0 - rgbf) < 1e-6).all(axis=1)
    key = np.where(np.isfinite(key), key, 0).astype(np.int64)
    code = (key[:, 0] << 16) | (key[:, 1] << 8) | key[:, 2]
    flat = (argb.reshape(-1) & 0xFFFFFF).astype(np.int64)
    assert len(np.unique(flat)) == flat.size
    order = np.argsort(flat)
    pos = np.searchsorted(flat[order], code)
    pos = np.clip(pos, 0, flat.size - 1)
    hit = good & (flat[order][pos] == code)
    return np.where(hit, order[pos], -1)


# ---- Q: quantisation -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def colour_values():
    """(k + 0.5)/255 with both float neighbours for every k, k/255 and (k + 0.25)/255, and 0, -0, 1, 1 + ulp, negatives, 2, +-inf, NaN."""
    halves = neighbours((np.arange(256, dtype=np.float64) + 0.5) / 255.0)
    plain = np.concatenate([np.arange(256) / 255.0, (np.arange(256) + 0.25) / 255.0]).astype(np.float32)   # (what the float64 restatement can answer)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0)), -1e-30, -0.5, -3.0, 2.0, 255.0, INF, -INF, NAN,
                        1e-45, 0.5 / 255.0 - 1e-9], dtype=np.float32)
    return np.concatenate([halves, plain, special])


@functools.lru_cache(maxsize=None)
def colour_table():
    """(n, 3): every value in every channel, next to two other values of the table."""
    v = colour_values()
    i = np.arange(len(v))
    return np.stack([v, v[(i + 7) % len(v)], v[(3 * i + 13) % len(v)]], axis=1).astype(np.float32)


def colour_spec(xrt, reflectiveness=0.0):
    """The colour probes on the floor z = 0, and the same table shifted by five on a ceiling z = 8 that faces down: with MaxReflections 1 the floor's
    reflection hits the ceiling, whose QUANTISED colour (RT:726) re-enters the Lerp of RT:584.  Two directional lights, one per plane."""
    t = colour_table()
    floor = probe_mesh(xrt, len(t), color=t)
    ceiling = probe_mesh(xrt, len(t), color=np.roll(t, 5, axis=0), z=8.0, down=True)
    m = xrt.configs.material(reflectiveness)
    return one_body(xrt, "Q", [(floor, m), (ceiling, dict(m))], [overhead(xrt), xrt.configs.directional((0.0, 0.0, -1.0))])


def colour_frame_spec(xrt):
    """The colour probes at MaxReflections 1 as a 64 x 48 frame: the camera looks straight down at the middle of the floor from under the ceiling."""
    spec = colour_spec(xrt, reflectiveness=0.5)
    spec.max_reflections = 1
    spec.camera = xrt.configs.camera((0.3, 0.2, 7.5), (0.3, 0.2, 0.0))
    spec.camera["up"] = (0.0, 1.0, 0.0)
    return spec.with_size(64, 48)


def pack_f64(rgbf):
    """new Color(Vector3) restated: each channel times 255, clamped to [0, 255], rounded to nearest (the half to even), NaN -> 0; R in the low byte.
    -> ((n, 3) bytes, (n, 3) sure): sure where the channel's product is not within 1e-3 of a half."""
    c = np.asarray(rgbf, dtype=np.float64) * 255.0
    with np.errstate(invalid="ignore"):
        sure = np.isnan(c) | (c < -1e-3) | (c > 255.001) | (np.abs(c - np.floor(c) - 0.5) > 1e-3)
        q = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 255.0))
    return np.rint(q).astype(np.uint32), sure


def channels(rgba):
    """(n, 3) R, G, B bytes of packed colours (R in the low byte)."""
    rgba = np.asarray(rgba, dtype=np.uint32)
    return np.stack([rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255], axis=1)


# ---- N: fragment normal ----------------------------------------------------------------------------------------------------------------------------
N_LEG = 0.5                      # powers of two: the ray at (0.125, 0.125) from the corner has u = v = 1/4 exactly
N_OFF, N_OFF_HALF = (0.15625, 0.09375), (0.125, 0.125)


@functools.lru_cache(maxsize=None)
def normal_table():
    """((n, 3, 3) vertex normals, (n, 2) ray offsets, kinds): the probes of RT:520-527."""
    a, b, c = (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8)
    rows, kinds = [], []

    def add(kind, n1, n2, n3, off=N_OFF):
        rows.append((n1, n2, n3, off)); kinds.append(kind)
    add("unit_equal", a, a, a); add("unit_equal", b, b, b); add("unit_equal", c, c, c)
    add("unit_different", a, b, c); add("unit_different", c, a, b); add("unit_different", b, c, a)
    for s in (1e-20, 1e-19, 1e-10, 1e-3, 0.5, 3.0, 1e10, 1e18, 1e19, 1e20):
        for n in (a, b):
            sn = tuple(f32(s) * f32(x) for x in n)
            add("non_unit", sn, sn, sn)
        add("non_unit", tuple(f32(s) * f32(x) for x in a), tuple(f32(s) * f32(x) for x in b), tuple(f32(s) * f32(x) for x in c))
    for n in (a, b, (1.0, 0.0, 0.0), (0.36, 0.48, 0.8)):
        m = tuple(-x for x in n)
        add("zero_blend", n, m, m, N_OFF_HALF)
    add("away", (0.0, 0.0, -1.0), (0.0, 0.0, -1.0), (0.0, 0.0, -1.0)); add("away", (0.6, 0.0, -0.8), (0.6, 0.0, -0.8), (0.6, 0.0, -0.8))
    add("away", a, (0.0, 0.0, -3.0), (0.0, 0.0, -3.0))
    for k in range(3):
        n = list(b); n[k] = NAN
        add("nan", tuple(n), tuple(n), tuple(n)); add("nan", a, tuple(n), b)
    rng = np.random.default_rng(17)
    for i in range(200):
        t = rng.normal(size=(3, 3)) + np.array([0, 0, 2.0])
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        add("random_unit", *[tuple(r) for r in t])
    for i in range(100):
        t = (rng.normal(size=(3, 3)) + np.array([0, 0, 1.0])) * 10.0 ** rng.uniform(-18, 18)
        add("random_non_unit", *[tuple(r) for r in t])
    normals = np.array([r[:3] for r in rows], dtype=np.float32)
    return normals, np.array([r[3] for r in rows], dtype=np.float32), tuple(kinds)


def normal_spec(xrt):
    normals, off, kinds = normal_table()
    m = xrt.configs.material(0.5, interpolate_normals=True)
    spec = one_body(xrt, "N", [(probe_mesh(xrt, len(normals), normals=normals, leg=N_LEG, cols=20), m)], [xrt.configs.spot((3.0, 2.0, 10.0), angle=2.5)], max_reflections=1)
    return spec, probe_rays(xrt, len(normals), off=off, cols=20)


def normal_frame_spec(xrt):
    spec = normal_spec(xrt)[0]
    spec.camera = xrt.configs.camera((0.2, -7.4, 20.0), (0.2, -7.4, 0.0))   # over the rows of the zero, opposed and not-a-number blends
    return spec.with_size(64, 64)


# ---- L: lights -------------------------------------------------------------------------------------------------------------------------------------
SWEEP = 4001
CONE_ANGLE = math.pi / 3


def sweep_x(x0, step=2e-6, n=SWEEP):
    return (x0 + (np.arange(n) - n // 2) * step).astype(np.float32)


def rays_down_at(xrt, x, y=0.0, z=5.0):
    x = np.asarray(x, dtype=np.float32)
    o = np.stack([x, np.full(len(x), f32(y)), np.full(len(x), f32(z))], axis=1)
    return xrt.rays_array(o, np.tile(np.array([0, 0, -1], dtype=np.float32), (len(x), 1)))


def cone_edge_x(position, direction, angle, y=0.0):
    """x > position's on the line (x, y, 0) at which the angle between the light's axis and the direction to the point is angle / 2 (float64, bisection)."""
    p, d = np.asarray(position, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    # the float32 angleCosine of SPOT:25
    ac = float(f32(math.cos(float(f32(angle) * f32(0.5)))))

    def f(x):
        t = np.array([x, y, 0.0]) - p
        return float(np.dot(t / np.linalg.norm(t), d)) - ac
    lo = float(p[0] - p[2] * d[0] / d[2])   # where the axis meets the plane: inside the cone
    hi = lo + 100.0
    assert f(lo) > 0 > f(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) > 0 else (lo, mid)
    return lo


def light_plane_spec(xrt, lights, normal=None, max_reflections=0):
    """One large plane z = 0 (with `normal` as the vertex normal of every corner: interpolated, so the shading normal differs from the geometric one)."""
    m = xrt.configs.material(0.0, interpolate_normals=normal is not None)
    return one_body(xrt, "L", [(plane_mesh(xrt, 64.0, normal=normal), m)], lights, max_reflections=max_reflections)


def cone_cases(xrt):
    """[(name, light, rays)]: the sweep across the cone's edge lightDot > angleCosine (SPOT:49) under a light straight above and under a tilted one."""
    out = []
    for name, pos in (("straight", (0.0, 0.0, 10.0)), ("tilted", (3.0, 2.0, 10.0))):
        light = xrt.configs.spot(pos, angle=CONE_ANGLE)
        x0 = cone_edge_x(light["position"], light["direction"], light["spot_angle"])
        out.append((name, light, rays_down_at(xrt, sweep_x(x0))))
    return out


SURFACE_NORMAL = (0.6, 0.0, 0.8)
LOW_LIGHT = (-5.0, 0.0, 0.5)


def surface_dot_case(xrt):
    """(spec, rays): a light low over the plane whose shading normal is tilted: surfaceDot = dot(dirToLight, normal) changes sign (SPOT:45) where
    (L - p).n = 0, that is at x = Lx + Lz * nz / nx, while the geometric normal still faces the light."""
    light = xrt.configs.spot(LOW_LIGHT, angle=math.pi / 2)
    x0 = LOW_LIGHT[0] + LOW_LIGHT[2] * SURFACE_NORMAL[2] / SURFACE_NORMAL[0]
    return light_plane_spec(xrt, [light], normal=SURFACE_NORMAL), rays_down_at(xrt, sweep_x(x0, step=1e-6))


def directional_cases(xrt):
    """[(name, light)]: dot(direction, normal) of 0 and of -0 on the plane's normal (0, 0, 1) (DIR:25-27), and a direction that is not of unit length."""
    d = xrt.configs.directional
    return [("dot_zero", d((1.0, 0.0, 0.0))), ("dot_minus_zero", d((-1.0, -1.0, -0.0))), ("non_unit", d((0.0, 0.0, 3.0), (0.2, 0.5, 1.0), 0.25)),
            ("non_unit_slanted", d((3.0, -2.0, 6.0), (1.0, 0.5, 0.25), 2.0))]


def many_lights(xrt):
    """32 lights, the limit of k_shade's emitMask.  The plane faces +z, so a shadow ray that climbs is answered where it is emitted (the whole mesh faces
    away from it) and one that descends is traced: 16 spots above the plane, 8 directional lights shining upwards and 8 spots below it."""
    rng = np.random.default_rng(23)
    out = []
    for i in range(16):
        out.append(xrt.configs.spot((float(rng.uniform(-6, 6)), float(rng.uniform(-6, 6)), float(rng.uniform(4, 12))), angle=float(rng.uniform(1.0, 2.5))))
    for i in range(8):
        d = rng.uniform(-1, 1, size=3); d[2] = abs(d[2]) + 0.2
        out.append(xrt.configs.directional(tuple(float(x) for x in d), tuple(float(x) for x in rng.uniform(0, 1, size=3)), float(rng.uniform(0.1, 1))))
    for i in range(8):
        out.append(xrt.configs.spot((float(rng.uniform(-6, 6)), float(rng.uniform(-6, 6)), float(rng.uniform(-12, -4))), angle=float(rng.uniform(1.0, 2.5))))
    return out


def scattered_rays(xrt, n=600, seed=29, half=8.0):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-half, half, size=(n, 2)), np.full((n, 1), 5.0)], axis=1)
    d = np.concatenate([rng.uniform(-0.3, 0.3, size=(n, 2)), np.full((n, 1), -1.0)], axis=1)
    return xrt.rays_array(o, d)


AT_HIT_XY = (1.5, 2.5)


def light_at_hit_cases(xrt, hit_w):
    """[(name, light)]: a spot exactly at the world position `hit_w` the ray at AT_HIT_XY hits (Position - position is the zero vector, its normalised
    form not a number), and one 1e-30 above it (the squared length underflows)."""
    w = np.asarray(hit_w, dtype=np.float32)
    return [("at_hit", spot_light(xrt, w, (0.0, 0.0, -1.0), math.pi / 2)),
            ("above_hit", spot_light(xrt, (w[0], w[1], w[2] + f32(1e-30)), (0.0, 0.0, -1.0), math.pi / 2))]


# ---- S: Snell refraction ----------------------------------------------------------------------------------------------------------------------------
AIM = (1.3125, 0.1875)     # where the rays meet the quad: inside one triangle, away from its edges
INDEX_GRID = (0.0, 1.0, 1.5, 1e-20, 1e20)
REF_GRID = (0.0, 1.0, 1.5)


def glass_spec(xrt, index, max_reflections=1, size=(8, 8), normal=None):
    m = xrt.configs.material(0.5, transparent=True, refraction_index=float(f32(index)), interpolate_normals=normal is not None)
    spec = one_body(xrt, "S_%g" % index, [(plane_mesh(xrt, 8.0, alpha=0.5, normal=normal), m)], [xrt.configs.spot((2.0, 1.0, 10.0))], max_reflections=max_reflections, size=size)
    return spec


def rays_at_angles(xrt, theta, dist=4.0):
    """Unit rays in the plane y = AIM's that meet the quad at AIM under the incidence angles theta (float64 radians)."""
    theta = np.asarray(theta, dtype=np.float64)
    d = np.stack([np.sin(theta), np.zeros_like(theta), -np.cos(theta)], axis=1)
    o = np.array([AIM[0], AIM[1], 0.0]) - dist * d
    return xrt.rays_array(o.astype(np.float32), d.astype(np.float32))


def critical_sweep(xrt, index, step=1e-7, n=SWEEP):
    """Incidence angles in n steps of 1e-7 rad across asin(1 / index): where the argument of the square root of RT:672 changes sign."""
    t0 = math.asin(1.0 / float(f32(index)))
    return rays_at_angles(xrt, t0 + (np.arange(n) - n // 2) * step)


def special_incidence(xrt):
    """Rays onto the quad whose SHADING normal is SURFACE_NORMAL = n (a ray that grazes the plane itself never reaches it: the slab test's parallel
    branch): normal incidence -n, grazing incidence with cos1 = 2^-24 from either side, cos1 = 0, cos1 < 0, straight down, and not of unit length."""
    c = 2.0 ** -24
    s = math.sqrt(1.0 - c * c)
    n, t, y = np.array(SURFACE_NORMAL, dtype=np.float64), np.array([-0.8, 0.0, 0.6]), np.array([0.0, 1.0, 0.0])   # (t and y span the plane normal to n)
    d = np.array([-n, -c * n - s * t, -c * n - s * (0.6 * t + 0.8 * y), (0.8, 0, -0.6), (0.96, 0, -0.28), (0, 0, -1), (0, 0, -3), (0.3, 0.2, -0.5)], dtype=np.float64)
    o = np.array([AIM[0], AIM[1], 0.0]) - 2.0 * d
    return xrt.rays_array(o.astype(np.float32), d.astype(np.float32))


def glass_frame_spec(xrt, index=1.5):
    """The quad under an oblique camera: the incidence angle runs from about 30 to 75 degrees down the 64 x 64 image, across asin(1 / 1.5) = 41.8."""
    spec = glass_spec(xrt, index, max_reflections=2, size=(64, 64))
    spec.camera = xrt.configs.camera((0.0, -8.0, 6.0), (0.0, 0.0, 0.0))
    return spec


# ---- float64 restatements of SpotLight.cs / DirectionalLight.cs and of the Snell block of RayTracer.cs ----------------------------------------------
def light_f64(light, position, normal, spot_kind=0):
    """GetLightForFragment restated in float64 from the text of SpotLight.cs / DirectionalLight.cs.  Spot: the unit vector from the fragment to the
    light; nothing if its dot with the normal is negative; nothing unless the dot of its reverse with the light's direction exceeds cos(angle / 2);
    else colour * intensity * (that excess / (1 - cos(angle / 2)) ^ decay) * surfaceDot + surfaceDot ^ 12.  Directional: colour * max(dot(direction,
    normal), 0) * intensity.  -> ((n, 3) light, (n,) margin): margin = how far the nearer of the two comparisons is from flipping (inf: directional)."""
    p, nrm = np.asarray(position, dtype=np.float64).reshape(-1, 3), np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    col, inten = np.asarray(light["color"], dtype=np.float64), float(f32(light["intensity"]))
    d = np.asarray([float(f32(c)) for c in light["direction"]])
    with np.errstate(all="ignore"):
        if light["kind"] != spot_kind:
            sd = np.maximum((nrm * d).sum(axis=1), 0.0)
            return sd[:, None] * col * inten, np.full(len(p), np.inf)
        t = np.asarray([float(f32(c)) for c in light["position"]]) - p
        t = t / np.linalg.norm(t, axis=1, keepdims=True)
        sd = (t * nrm).sum(axis=1)
        ld = (-t * d).sum(axis=1)
        ac = float(f32(math.cos(float(f32(light["spot_angle"]) * f32(0.5)))))
        denom = (1.0 - ac) ** float(f32(light["decay_exponent"]))
        lit = (sd >= 0) & (ld > ac)
        val = (col * inten)[None, :] * ((ld - ac) / denom * sd)[:, None] + (sd ** 12)[:, None]
        return np.where(lit[:, None], val, 0.0), np.minimum(np.abs(sd), np.abs(ld - ac))


def snell_f64(direction, normal, index, current):
    """The refracted direction of RT:656-694 restated in float64: n1, n2 = (1, current) if current == index else (index, 1); cos1 = -normal.dir;
    cos2 = sqrt(1 - (n1/n2)^2 (1 - cos1^2)); (n1/n2) dir +- ((n1/n2) cos1 - cos2) normal (+ for cos1 >= 0), normalised.
    -> ((n, 3) direction, NaN where the square root's argument is negative; (n,) that argument)."""
    d, nrm = np.asarray(direction, dtype=np.float64).reshape(-1, 3), np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    index, current = float(f32(index)), float(f32(current))
    n1, n2 = (1.0, current) if current == index else (index, 1.0)
    with np.errstate(all="ignore"):
        q = float(f32(n1) / f32(n2))
        cos1 = -(nrm * d).sum(axis=1)
        arg = 1 - q * q * (1 - cos1 * cos1)
        cos2 = np.sqrt(arg)
        r = q * d + np.where(cos1 >= 0, 1.0, -1.0)[:, None] * (q * cos1 - cos2)[:, None] * nrm
        return r / np.linalg.norm(r, axis=1, keepdims=True), arg


# ---- the conversion the texture lookup is defined with beyond its valid range (DESIGN.md 3 "Range of validity") ---------------------------------------
INT_MIN = -2 ** 31


def cvt_i32(x):
    """(int)(float) as the reference's platform performs it (x64 .NET, cvttss2si): truncation toward zero; 0x80000000 for NaN and outside [-2^31, 2^31)."""
    x = float(x)
    if x != x or x >= 2.0 ** 31 or x < -2.0 ** 31:
        return INT_MIN
    return int(x)


def lookup_point_guarded(u, v, w, h, address):
    """Material.LookupUV with the point filter on ANY float32 pair, in float32 steps with cvt_i32 and the index guard of the product and the oracle
    (an index outside the texture reads texel 0) -> the flat texel index."""
    out = []
    with np.errstate(all="ignore"):
        for c in (f32(u), f32(v)):
            o = c
            if address == "clamp":
                c = f32(1) if c > 1 else c
                c = f32(0) if c < 0 else c
            else:
                if c > 1:
                    c = np.fmod(c, f32(1))
                if c < 0:
                    c = f32(1) + np.fmod(c, f32(1))
                if address == "mirror":
                    k = cvt_i32(f32(o - c))
                    if (abs(k) % 2) == 0:
                        c = f32(1) - c
            out.append(c)
        x, y = cvt_i32(out[0] * f32(w - 1)), cvt_i32(out[1] * f32(h - 1))
    idx = w * y + x
    return idx if 0 <= idx < w * h else 0
