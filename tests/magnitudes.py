"""TEST INFRASTRUCTURE -- the tables of the magnitude sweep and what both of its modules need: tests/test_magnitudes_cpu.py (oracle against the
CPU single-stepper) and tests/test_gpu_magnitudes.py (oracle against the kernels).  Scenes scaled by 2^k and ray directions of length 2^j, at the
cells where the guards of the hot path's shortcuts flip (DESIGN.md §3 "Range of validity").  Every count below is the ORACLE's, measured with the
committed generators (util.magnitude_rays, seeds 31 / 32): the floors come from them, never from the code under test."""
import functools

from util import magnitude_fixture, magnitude_frame_spec, scaled_rays, scaled_spec, secondary_rays

# (fixture, k: scene scale 2^k, j: |D| = 2^j, origins inside the box, oracle hits of 4000 rays at the scene seam / the mesh seam, what the cell
# crosses).  None: the seam is dead there in the reference itself (fl(O + D) = O at OSM:358-364) and is not compared.
CELLS = [
    ("soup", -62, 0, False, 2815, 2815, "1/det near overflow, squares subnormal, NaN normals"),
    ("soup", -60, 0, False, 3204, 3204, "1/det near overflow, squares subnormal, NaN normals"),
    ("soup", -40, 0, False, 3207, 3207, "NaN surface normals, certainly_negative off"),
    ("soup", -31, 0, False, 2809, 2809, "|a| >= 2^-60 guard, far side"),
    ("soup", -29, 0, False, 2809, 2809, "|a| >= 2^-60 guard, near side"),
    ("soup", -20, 0, False, 2809, 2809, "control"),
    ("soup", 0, 0, False, 2809, 2809, "control"),
    ("soup", 20, 0, False, 2794, 2809, "control"),
    ("soup", 29, 19, False, 2812, 2809, "|det| <= 2^60 guard, near side (the scene seam is dead at j = 0)"),
    ("soup", 31, 19, False, 2806, 2809, "|det| <= 2^60 guard, far side"),
    ("soup", 40, 19, False, 3123, 3307, "|O| > 2^40: RayCull off"),
    ("soup", 40, 40, False, 3307, 3307, "|O| > 2^40: RayCull off"),
    ("soup", -40, -19, False, 2007, 585, "just above the 1e-6 parallel threshold, d1 near 2^-20"),
    ("soup", 0, -19, False, 1768, 458, "just above the 1e-6 parallel threshold, d1 near 2^-20"),
    ("soup", -40, 19, False, 3207, 3207, "d1 near 2^20"),
    ("soup", -40, 40, False, 3207, 3207, "d1 > 2^20: RayCull off"),
    ("soup", -40, 64, False, 603, 3207, "D.D overflows"),
    ("soup", 0, 19, False, 2809, 2809, "d1 near 2^20"),
    ("soup", 0, 40, False, 2809, 2809, "d1 > 2^20: RayCull off"),
    ("soup", 0, 64, False, 536, 2809, "D.D overflows"),
    ("soup", 0, 127, False, None, 2809, "the longest representable directions: 1/d subnormal, all_back_facing's scale_ overflows (mesh seam; the scene seam is dead)"),
    ("soup", 0, -21, True, 3153, 539, "|D| < 1e-6: every axis takes the parallel branch"),
    ("hf", -62, 0, False, 3171, 3171, "1/det near overflow, squares subnormal, NaN normals"),
    ("hf", -60, 0, False, 3171, 3171, "1/det near overflow, squares subnormal, NaN normals"),
    ("hf", -40, 0, False, 3171, 3171, "NaN surface normals, certainly_negative off"),
    ("hf", -31, 0, False, 1942, 1942, "|a| >= 2^-60 guard, far side"),
    ("hf", -29, 0, False, 1942, 1942, "|a| >= 2^-60 guard, near side"),
    ("hf", -20, 0, False, 1942, 1942, "control"),
    ("hf", 0, 0, False, 1942, 1942, "control"),
    ("hf", -40, -19, False, 967, 142, "just above the 1e-6 parallel threshold"),
    ("hf", -40, 19, False, 3171, 3171, "d1 near 2^20"),
    ("hf", -40, 40, False, 3171, 3171, "d1 > 2^20: RayCull off"),
    ("hf", -40, 64, False, 628, 3171, "D.D overflows"),
    ("hf", 0, 120, False, None, 1941, "1/d subnormal at the mesh seam (the scene seam is dead)"),
    ("hf", -40, 127, False, None, 3171, "1/d subnormal, scale_ overflows, NaN normals (mesh seam; the scene seam is dead)"),
    ("hf", 31, 19, False, 3688, 3718, "|det| > 2^60, tight boxes at 2^31"),
    ("hf", 31, 40, False, 3718, 3718, "|det| > 2^60, RayCull off"),
]
# Oracle hits of 4000 rays every cell must reach at either seam; the all-parallel cell (inside origins, j = -21).  Where the oracle's own count
# above is below twice that (short rays and overflowing D.D end most rays, above all at the mesh seam), the floor is half the oracle's count.
FLOOR, FLOOR_ALL_PARALLEL = 400, 100


def cell_id(c):
    return "%s_k%d_j%d%s" % (c[0], c[1], c[2], "_inside" if c[3] else "")


def cell_floors(c):
    """(scene seam, mesh seam) floors of a cell; None for a seam that is not compared."""
    f = FLOOR_ALL_PARALLEL if c[3] else FLOOR
    return tuple(None if n is None else min(f, n // 2) for n in c[4:6])


@functools.lru_cache(maxsize=None)
def scene_spec(xrt, name, k):
    """The fixture's one-body spec at scale 2^k."""
    return scaled_spec(magnitude_fixture(xrt, name)[1], k)


def cell_spec_and_rays(xrt, c):
    """The scene of a cell and its 4000 rays (the fixture's unit rays: origins x 2^k, directions x 2^j)."""
    name, k, j, inside = c[:4]
    md, spec, rays, rays_in = magnitude_fixture(xrt, name)
    return scene_spec(xrt, name, k), scaled_rays(rays_in if inside else rays, k, j)


@functools.lru_cache(maxsize=None)
def oracle_of(xrt, orc, name, k):
    """One oracle scene per (fixture, scale)."""
    return orc.OracleScene(scene_spec(xrt, name, k))


# Secondary rays: util.secondary_rays off the oracle's hits of a cell's rays (origins on the surface, the hit triangle ignored), directions x 2^j.
# (fixture, k, j, oracle hits at the scene seam).  The rays leave the surface upwards, so few come down on the heightfield again, and at 2^31 a
# unit direction is lost in the origin (the scene seam is all but dead at j = 0: these cases compare misses above all, and say that the kernels
# do not invent hits there); the floor is half the oracle's count where that is below FLOOR.
SECONDARY = [("soup", -40, 0, 1979), ("soup", -40, 19, 1979), ("soup", -31, 0, 1466), ("soup", -31, 19, 1466), ("soup", 31, 0, 24), ("soup", 31, 19, 1495),
             ("hf", -40, 0, 204), ("hf", -40, 19, 204), ("hf", -31, 0, 56), ("hf", -31, 19, 56), ("hf", 31, 0, 0), ("hf", 31, 19, 256)]


def secondary_id(c):
    return "%s_k%d_j%d" % c[:3]


def secondary_case(xrt, orc, c):
    """(spec, rays, floor) of a secondary-ray case: the rays leave the oracle's hits of the (k, 0) cell -- the (31, 19) cell at k = 31."""
    name, k, j, measured = c
    spec, prim = cell_spec_and_rays(xrt, (name, k, 19 if k == 31 else 0, False))
    hits = oracle_of(xrt, orc, name, k).intersect(prim)
    return spec, scaled_rays(secondary_rays(xrt, hits, seed=3), 0, j), min(FLOOR, measured // 2)


# Frames: the scales at which the oracle still shades (nothing at k >= 30 for the soup, k >= 20 for the heightfield).
FRAME_SCALES = {"soup": (-60, -40, -30, -10, 10, 20), "hf": (-60, -40, -30, -10, 10)}
FRAME_FLOOR = 500   # shaded hits of a 48 x 48 frame by the oracle (measured: 1061 .. 2011 for the soup, 1174 .. 1180 for the heightfield)
FRAMES = [(n, k, t) for n in ("soup", "hf") for t in ((False, True) if n == "soup" else (False,)) for k in FRAME_SCALES[n]]


def frame_id(c):
    return "%s_k%d%s" % (c[0], c[1], "_transparent" if c[2] else "")


@functools.lru_cache(maxsize=None)
def oracle_frame(xrt, orc, name, k, transparent=False, multisampling=None, quality=0):
    """(spec, rgba, rgbf, stats) of the oracle's frame, rendered once."""
    spec = magnitude_frame_spec(xrt, name, k, transparent, multisampling, quality)
    return (spec,) + orc.OracleScene(spec).render(nthreads=8)


# Poses (util.magnitude_pose_case): (k or None, scale triple or None, oracle hits of the 4000 rays at body 0 / body 1 with the stale scene octree,
# then after the tree is built again).  The floor is FLOOR for every uniform scale from 2^-40 to 2^20, in both phases.  Three cases cannot reach it
# and hold half the oracle's count: at scale 2^-50 the reference's own object-space ray breaks down; the world box the reference gives a rotated
# body (SO:183-199: two corners) leaves little of one flattened to a plate; a zero scale component flattens it altogether (singular inverse,
# cullOk = 0: the answers are compared, nothing is assumed).
POSES = [(-50, None, 50, 2809, 50, 2809),   # (|InverseWorld| = 2^50 > 1e15: cullOk = 0 with a finite transform)
         (-40, None, 2789, 2809, 2789, 2809), (-20, None, 2789, 2809, 2789, 2809), (-10, None, 2789, 2809, 2789, 2809),
         (10, None, 2464, 2840, 2464, 2840), (20, None, 2510, 2662, 2510, 2662),
         (None, (2.0 ** -20, 1.0, 2.0 ** 10), 269, 2811, 359, 2811), (None, (1.0, 0.0, 1.0), 63, 2809, 63, 2809)]


def pose_id(c):
    return "k%d" % c[0] if c[1] is None else "scale_%g_%g_%g" % c[1]


def pose_floors(c):
    """Floors of (body 0, body 1) with the stale tree, then with the rebuilt one."""
    return tuple(min(FLOOR, n // 2) for n in c[2:])
