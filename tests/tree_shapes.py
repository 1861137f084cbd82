"""TEST INFRASTRUCTURE -- the generators, the ray families and the case table of the tree-shape tests: tests/test_tree_shapes_cpu.py (oracle
against the CPU single-stepper, and the stack bound) and tests/test_gpu_tree_shapes.py (oracle against the kernels).  Octrees as deep as the
builders accept, scene leaves of more than 32 bodies, and the seams between the compiled per-lane stack capacities (traverse.h
INTERSECT_STACK_CAPS) and between the packet kernel and the per-lane kernel (packet.hip packet_supported) -- DESIGN.md §3 "Tree shapes".

Every depth, leaf size and count below is a CLAIM about a tree or about the oracle's answers; tests/test_tree_shapes_cpu.py asserts each of
them from the built trees and from the oracle alone, never from the code under test."""
import functools

import numpy as np

from util import secondary_rays

S = 16.0   # edge of the staircase's mesh box
# The staircase is built in [0, S]^3 towards the corner (0, 0, 0) and then mirrored in x and z (two reflections: windings keep their sense): the mesh
# box is [-S, 0] x [0, S] x [-S, 0], its corner at the origin is the corner of child 5 at every level, and every level of the path word of
# traverse.h (three bits per level) holds 101 -- towards child 0 the word would be zero whatever became of its upper bits.
MIRROR = np.array([-1.0, 1.0, -1.0])


def _mesh(xrt, v):
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3, 3)
    n = len(v)
    rng = np.random.default_rng(n)
    md = xrt.fixtures.MeshData(v, np.zeros((n, 3, 3), dtype=np.float32), rng.uniform(0, 1, size=(n, 3, 2)).astype(np.float32),
                               rng.uniform(0.2, 1, size=(n, 4)).astype(np.float32))
    md.n = np.repeat(md.surface_normal[:, None, :], 3, axis=1).copy()
    return md


def _facing(tri, towards):
    """tri with the winding whose surface normal (TMP:199-203: cross(v3 - v1, v2 - v1)) has a positive component along `towards`."""
    nrm = np.cross(tri[2] - tri[0], tri[1] - tri[0])
    return tri if float(nrm @ towards) > 0 else tri[[0, 2, 1]]


@functools.lru_cache(maxsize=None)
def staircase(xrt, n, per=1):
    """A mesh whose octree, built with leaf threshold `per`, is exactly n levels deep: n steps of `per` small triangles each, step k sized and
    placed proportional to 2^-k towards the corner (0, 0, 0) of the mesh box (described here before MIRROR is applied: [0, S]^3) -- inside the upper octant of the cell [0, S 2^-(k+1)]^3,
    so the node [0, S 2^-L]^3 at level L >= 1 holds steps L-1 .. n-1 and is split while it holds two of them.  No two triangles share a
    vertex (MO:84-96 would not terminate).  Even steps face away from the corner, odd steps face it.  Two large backstop triangles on the
    faces x = S and y = S face the corner: what a ray leaving the corner hits after the walk has popped back up all its levels.  They
    also give the mesh box its corner at the origin.  Triangle ids: step k holds k * per .. k * per + per - 1, the backstops are the last two."""
    diag = np.ones(3) / np.sqrt(3.0)
    e1 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    e2 = np.cross(diag, e1)
    tris = []
    for k in range(n):
        h = S * 2.0 ** -(k + 1)   # the step's cell is [0, h]^3, its triangles lie in (h/2, h)^3
        for j in range(per):
            a = 2.399963 * (k * per + j) + 0.5          # golden angle: no two steps line up as seen from the corner
            r = 0.14 if per == 1 else 0.16
            c = h * (0.75 + r * (np.cos(a) * e1 + np.sin(a) * e2))
            s = h * (0.07 if per == 1 else 0.05)
            b = a * 1.7 + j
            u, w = np.cos(b) * e1 + np.sin(b) * e2, -np.sin(b) * e1 + np.cos(b) * e2
            tri = np.stack([c + s * u, c + s * (-0.5 * u + 0.87 * w) + 0.2 * s * diag, c + s * (-0.5 * u - 0.87 * w) - 0.2 * s * diag])
            tris.append(_facing(tri, diag if k % 2 == 0 else -diag))
    tris.append(_facing(np.array([[S, 0.0, 0.0], [S, S, 0.3 * S], [S, 0.3 * S, S]]), np.array([-1.0, 0.0, 0.0])))
    tris.append(_facing(np.array([[0.0, S, 0.0], [0.35 * S, S, S], [S, S, 0.45 * S]]), np.array([0.0, -1.0, 0.0])))
    return _mesh(xrt, np.array(tris) * MIRROR)


def _finish(xrt, s, lo, hi, view=((1.9, 1.5, 2.3), (0.2, 0.2, 0.2), 0.7853982), light=(2.5, 3.0, 2.0)):
    """Camera, light and image of a case whose interesting part lies in the world box lo .. hi, near its corner lo."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = float((hi - lo).max())
    s.camera = xrt.configs.camera(tuple(lo + e * np.array(view[0])), tuple(lo + e * np.array(view[1])), fov=view[2], near=0.01 * e, far=20.0 * e)
    s.lights = [xrt.configs.spot(tuple(lo + e * np.array(light)))]
    s.max_reflections = 2
    return s.with_size(32, 32)


def staircase_scene(xrt, n, per=1):
    """One body with the identity pose: the staircase of depth n."""
    s = xrt.configs.SceneSpec("staircase%d" % n)
    s.meshes.append((staircase(xrt, n, per), xrt.configs.material(0.5)))
    s.objects.append(([0], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    s.mesh_threshold, s.scene_threshold = per, 20
    return _finish(xrt, s, (0, 0, 0), (S, S, S), view=((-0.95, 0.6, -0.35), (-0.12, 0.12, -0.12), 0.5235988), light=(-2.5, 3.0, -2.0))   # (from inside the box, at the corner)


def nested_bodies(xrt, n, mesh=None, mesh_threshold=50, p=None, view=((2.2, 1.2, 0.7), (0.15, 0.15, 0.15), 0.7853982)):
    """n bodies of one mesh (default: the 12-triangle crate, whose octree is a single leaf) shrinking towards the world origin: body k scaled by
    2^-k at p 2^-k (1, 1, 1), p chosen from the mesh box (unless given) so that the world boxes are pairwise disjoint.  With scene threshold 1 the scene
    octree separates them one per level."""
    md = xrt.fixtures.crate(1) if mesh is None else mesh
    lo, hi = md.bbox[:3].astype(np.float64), md.bbox[3:].astype(np.float64)
    p = float(np.ceil(1.25 * (hi - 2.0 * lo).max())) if p is None else float(p)
    s = xrt.configs.SceneSpec("nested%d" % n)
    s.meshes.append((md, xrt.configs.material(0.5)))
    for k in range(n):
        f = 2.0 ** -k
        s.objects.append(([0], (p * f, p * f, p * f), (0.0, 0.0, 0.0), (f, f, f)))
    s.mesh_threshold, s.scene_threshold = mesh_threshold, 1
    return _finish(xrt, s, (0, 0, 0), p + hi, view=view)   # (by default from beside the diagonal the bodies line up on)


@functools.lru_cache(maxsize=None)
def _crowd_meshes(xrt):
    """Six small meshes of about the crate's size: the crate at two tessellations and four sheets of a few triangles."""
    out = [xrt.fixtures.crate(1), xrt.fixtures.crate(2)]
    for i in range(4):
        rng = np.random.default_rng(40 + i)
        c = rng.uniform(-5, 5, size=(8, 1, 3)) + np.array([0.0, 6.0, 0.0])
        out.append(_mesh(xrt, c + rng.uniform(-4, 4, size=(8, 3, 3))))
    return tuple(out)


SPACING = 0.05   # between the bodies of a crowd, along (1, 0.5, 0.25)


def crowd(xrt, counts, meshes_per_body=(1, 1, 2, 6), gap=None):
    """Clusters of overlapping bodies: cluster j holds counts[j] bodies SPACING apart, far more of them than fit apart inside one body's box, so
    one scene leaf lists them all; with scene threshold max(counts) that leaf is not split.  The first two bodies of the scene are exactly
    coincident (same meshes, same pose): every distance ties between them.  Body i carries the first meshes_per_body[i % len] of the six
    meshes.  One cluster: the root is the leaf.  More: cluster j + 1, of bodies an eighth the size, begins `gap` beyond the world box of cluster j
    along x, and the tree is split until a cell boundary falls into the gap -- a crowded leaf below some depth."""
    meshes = _crowd_meshes(xrt)
    s = xrt.configs.SceneSpec("crowd_" + "_".join(str(c) for c in counts))
    for md in meshes:
        s.meshes.append((md, xrt.configs.material(0.5)))
    lo = np.min([m.bbox[:3] for m in meshes], axis=0).astype(np.float64)
    hi = np.max([m.bbox[3:] for m in meshes], axis=0).astype(np.float64)
    x0, i = float(lo[0]), 0
    for j, cnt in enumerate(counts):
        f = 1.0 if j == 0 else 0.125   # (the later clusters are small, so that no early split of the root falls between the clusters)
        for b in range(cnt):
            t = SPACING * f * (max(b - 1, 0) if j == 0 else b)   # bodies 0 and 1 coincide
            s.objects.append((list(range(meshes_per_body[i % len(meshes_per_body)])), (x0 - lo[0] * f + t, 0.5 * t, 0.25 * t), (0.0, 0.0, 0.0), (f, f, f)))
            i += 1
        x0 += (hi[0] - lo[0] + SPACING * cnt) * f + (gap or 0.0)
    s.mesh_threshold, s.scene_threshold = 50, max(counts)
    return _finish(xrt, s, lo, hi + np.array([SPACING * counts[0], 0.0, 0.0]))


# ---- the case table --------------------------------------------------------------------------------------------------------------------
# sd, md: maxDepth of the scene octree and of the deepest mesh octree as built; leaf: the largest scene leaf; words = (sd + 1) + (md + 1), the
# per-lane stack words the scene needs.  `per`: inward rays per target (tuned until the oracle alone meets the coverage conditions of
# tests/test_tree_shapes_cpu.py).
def _case(name, kind, arg, sd, md, leaf, seam, per=40, **kw):
    return dict(name=name, kind=kind, arg=arg, sd=sd, md=md, leaf=leaf, words=sd + md + 2, seam=seam, per=per, **kw)


CASES = [_case("mesh_md%d" % d, "mesh", d, 0, d, 1, "stack words %d" % (d + 2)) for d in (6, 7, 10, 11, 14, 15, 20)]
CASES += [_case("scene_sd10", "nested", 10, 10, 0, 1, "the deepest scene tree the packet kernel takes"),
          _case("scene_sd11", "nested", 11, 11, 0, 1, "the shallowest scene tree packet_supported sends to the per-lane kernel"),
          _case("scene_sd24", "nested", 24, 24, 0, 1, "the deepest scene tree the builder accepts"),
          _case("both_sd4_md20", "both", 4, 4, 20, 1, "26 words: the first scene of the 40-word instantiation", per=12),
          _case("both_sd18_md20", "both", 18, 18, 20, 1, "40 words: the last size accepted", per=4),
          _case("crowd32", "crowd", (32,), 0, 0, 32, "one full chunk of the 32-body loop", per=12),
          _case("crowd33", "crowd", (33, 3), 3, 0, 33, "one body in the second chunk, in a leaf below the root", per=12, gap=0.5),
          _case("crowd65", "crowd", (65,), 0, 0, 65, "three chunks", per=8)]
REFUSED = _case("both_sd19_md20", "both", 19, 19, 20, 1, "41 words: refused", per=4)
CASE_IDS = [c["name"] for c in CASES]
DEEPEST = ("mesh_md20", "both_sd18_md20")   # the list calls run on these


def case(name):
    return next(c for c in CASES + [REFUSED] if c["name"] == name)


@functools.lru_cache(maxsize=None)
def case_spec(xrt, name):
    c = case(name)
    if c["kind"] == "mesh":
        return staircase_scene(xrt, c["arg"])
    if c["kind"] == "nested":
        return nested_bodies(xrt, c["arg"])
    if c["kind"] == "both":
        return nested_bodies(xrt, c["arg"], staircase(xrt, c["md"]), mesh_threshold=1, p=2.0 * S, view=((0.72, 1.02, 0.75), (0.0, 0.0, 0.0), 0.5235988))   # (p = 2 S: n bodies give scene depth n for n = 4, 18, 19 alike; the view: from inside body 0 down the line of the staircases)
    return crowd(xrt, c["arg"], gap=c.get("gap"))


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _world(xrt, spec, body):
    ids, pos, rot, scale = spec.objects[body]
    bb = np.zeros(6, dtype=np.float32)
    for i in ids:
        bb[:3] = np.minimum(bb[:3], spec.meshes[i][0].bbox[:3])
        bb[3:] = np.maximum(bb[3:], spec.meshes[i][0].bbox[3:])
    world = xrt.xna.build_world(scale, rot, pos, bb)[0]
    return xrt.xna.as_array(world).reshape(4, 4).astype(np.float64), bb.astype(np.float64)


def targets(xrt, spec, per, rng):
    """World-space points on the triangles of every body -> (points, the length scale of what each point lies on): `per` on every triangle of
    a staircase (mesh threshold below 50), else `per` for the body, on random triangles of its meshes."""
    P, L = [], []
    crowded = spec.scene_threshold > 20
    if crowded:   # the crates (mesh 0 of every body) of a crowd hide each other: what shows of one lies outside the others' boxes
        bb = spec.meshes[0][0].bbox.astype(np.float64)
        pos, scl = np.array([o[1] for o in spec.objects], dtype=np.float64), np.array([o[3] for o in spec.objects], dtype=np.float64)
        clo, chi = pos + scl * bb[:3], pos + scl * bb[3:]
    for b, (ids, pos, rot, scale) in enumerate(spec.objects):
        W, _ = _world(xrt, spec, b)
        for i in ids:
            v = spec.meshes[i][0].v.astype(np.float64)
            want = per if (spec.mesh_threshold < 50 or i == 0) else 2
            tri = np.repeat(np.arange(len(v)), per) if spec.mesh_threshold < 50 else rng.integers(0, len(v), size=want * (200 if crowded else 1))
            w = rng.dirichlet((1, 1, 1), size=len(tri))
            p = ((v[tri] * w[:, :, None]).sum(axis=1) @ W[:3, :3]) + W[3, :3]
            size = np.linalg.norm(v[tri][:, 1] - v[tri][:, 0], axis=1) * float(scale[0])
            if crowded:
                others = np.array([k != b and spec.objects[k][1] != spec.objects[b][1] for k in range(len(spec.objects))])
                shown = ~((p[:, None, :] >= clo[None, others] - 1e-9) & (p[:, None, :] <= chi[None, others] + 1e-9)).all(axis=2).any(axis=1)
                keep = np.concatenate([np.where(shown)[0], np.where(~shown)[0]])[:want]   # (nothing shows: hidden points, which is no loss)
                p, size = p[keep], np.full(len(keep), 1.0)
            P.append(p)
            L.append(size)
    return np.concatenate(P), np.concatenate(L)


def _rays(xrt, o, d):
    n = np.linalg.norm(d, axis=1, keepdims=True)
    return xrt.rays_array(o.astype(np.float32), (d / np.where(n == 0, 1, n)).astype(np.float32))


def inner_box(xrt, spec, c):
    """The world box the outward rays start in: the deepest cell of the staircase (below its last step) of the innermost body, or the middle
    of the innermost body's box."""
    W, bb = _world(xrt, spec, len(spec.objects) - 1)
    if c["md"] > 0:
        h = S * 2.0 ** -c["md"]
        lo, hi = np.sort(np.stack([0.05 * h * MIRROR, 0.45 * h * MIRROR]), axis=0)
    else:
        lo, hi = bb[:3] + 0.3 * (bb[3:] - bb[:3]), bb[:3] + 0.7 * (bb[3:] - bb[:3])
    lo, hi = np.append(lo, 1.0) @ W, np.append(hi, 1.0) @ W
    return lo[:3], hi[:3]


@functools.lru_cache(maxsize=None)
def families(xrt, name):
    """The ray families of a case -> dict of xrt_ray arrays (made once and shared: callers copy, never write)."""
    c, spec = case(name), case_spec(xrt, name)
    rng = np.random.default_rng(len(name) * 131 + c["words"])
    T, L = targets(xrt, spec, c["per"], rng)
    n = len(T)
    W0, bb0 = _world(xrt, spec, 0)
    far = 2.0 * float(np.linalg.norm((bb0[3:] - bb0[:3]) * spec.objects[0][3][0]))
    fam = {}
    # inward: from a few of the target's own sizes away (a binary32 direction cannot be aimed at a triangle of 1e-6 from 50 units), and from outside everything
    dist = np.choose(np.arange(n) % 3, [4.0 * L, 40.0 * L, np.full(n, far)])
    o = T + _unit(rng, n) * dist[:, None]
    fam["inward"] = _rays(xrt, o, T - o)
    # outward: from inside the deepest cell / the innermost body towards every target: the walk descends first and finds the hit after the pops
    lo, hi = inner_box(xrt, spec, c)
    o = lo + (hi - lo) * rng.uniform(size=(n, 3))
    fam["outward"] = _rays(xrt, o, T - o)
    # crossing: through a point within a fraction of the smallest cell of the corner everything shrinks towards, from outside, on to the large things
    big = np.argsort(-L)[: max(n // 4, 8)]
    m = len(big)
    small = float(np.linalg.norm(hi - lo))
    through = lo + (hi - lo) * rng.uniform(-1.0, 1.0, size=(m, 3))
    d = T[big] - through
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    fam["crossing"] = _rays(xrt, through - d * np.choose(np.arange(m) % 2, [far, 64.0 * small])[:, None], d)
    # axis-parallel rays at the targets, and a handful of zero and non-finite rays
    pick = rng.choice(n, size=min(n, 300), replace=False)
    ax = rng.integers(0, 3, size=len(pick))
    sign = rng.choice([-1.0, 1.0], size=len(pick))
    d = np.zeros((len(pick), 3))
    d[np.arange(len(pick)), ax] = sign
    par = xrt.rays_array((T[pick] - d * (4.0 * L[pick])[:, None]).astype(np.float32), d.astype(np.float32))
    mid = (0.5 * (lo + hi)).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    odd_o = [mid, mid, mid, mid, [nan, mid[1], mid[2]], [inf, mid[1], mid[2]], T[0], T[0], mid]
    odd_d = [[0, 0, 0], [nan, 0, 1], [inf, 0, 0], [0, -inf, 1], [1, 0, 0], [1, 1, 1], [0, 0, 0], [nan, nan, nan], [1e-7, 1e-7, 1]]
    with np.errstate(all="ignore"):
        fam["axis_and_odd"] = np.concatenate([par, xrt.rays_array(np.array(odd_o, dtype=np.float32), np.array(odd_d, dtype=np.float32))])
    return fam


@functools.lru_cache(maxsize=None)
def oracle_of(xrt, orc, name):
    return orc.OracleScene(case_spec(xrt, name))


@functools.lru_cache(maxsize=None)
def all_rays(xrt, orc, name):
    """Every family of a case in one array, with util.secondary_rays off the oracle's hits of the inward and outward rays behind them."""
    fam = families(xrt, name)
    prim = np.concatenate([fam["inward"], fam["outward"]])
    sec = secondary_rays(xrt, oracle_of(xrt, orc, name).intersect(prim), seed=5)
    return np.concatenate([fam[k] for k in FAMILIES] + [sec])


FAMILIES = ("inward", "outward", "crossing", "axis_and_odd")


def family_slice(xrt, name, family):
    """Where a family's rays stand in all_rays."""
    fam = families(xrt, name)
    at = 0
    for k in FAMILIES:
        if k == family:
            return slice(at, at + len(fam[k]))
        at += len(fam[k])
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def wanted(xrt, orc, name):
    """The oracle's answers and work counters of all_rays at the scene seam, computed once."""
    return oracle_of(xrt, orc, name).intersect(all_rays(xrt, orc, name), stats=True)


@functools.lru_cache(maxsize=None)
def wanted_mesh(xrt, orc, name):
    """... and at the mesh seam of mesh 0 (the one-body cases: world space is object space)."""
    return oracle_of(xrt, orc, name).mesh_intersect(0, all_rays(xrt, orc, name))


@functools.lru_cache(maxsize=None)
def oracle_frame(xrt, orc, name, fixed16=False):
    """(spec, rgba, rgbf, stats) of the oracle's 32 x 32 frame of a case, MaxReflections 2, at one sample or sixteen."""
    import copy
    spec = copy.copy(case_spec(xrt, name))
    if fixed16:
        spec.multisampling = xrt.abi.MS_FIXED16
    return (spec,) + orc.OracleScene(spec).render(nthreads=8)
