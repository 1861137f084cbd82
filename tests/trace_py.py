"""TEST INFRASTRUCTURE for xrt_trace_pixels (tests/test_trace_pixels_cpu.py, tests/test_gpu_trace_pixels.py).  The oracle makes the primary rays of whole
frames only (orc_generate_primary_rays: pixel (X, Y) of the camera's viewport), so the expected ray of a listed centre is a pixel of an oracle frame
looked at through the two exact constructions of tests/pixels_py.py, composed:
  - a fractional centre x = X / k, k a power of two: Unproject divides (sx - vp.X) by vp.Width (RT:415), and scaling both by k is exact in binary32, so
    the ray at x is the ray of pixel X of the frame whose viewport is k times as wide (same matrices: the projection's aspect ratio does not change);
  - a centre outside the viewport: Unproject sees only sx - vp.X, so the ray at x = q W + r, 0 <= r < W, is the ray of pixel r of the frame whose vp.X
    is -q W.
Both at once: pixel k r of the frame with vp.Width = k W and vp.X = -k q W has sx - vp.X = k x, exactly.  The expected hit is the oracle's
GetRayIntersection (OracleScene.intersect) on that ray.  tests/test_trace_pixels_cpu.py shows on the CPU that the oracle's CastRay on these rays gives the
oracle frames' pixels, so the constructions hold for rays and hits as they do for colours."""
import ctypes as C
import os
import subprocess

import numpy as np

import pixels_py as px

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = px.CSRC
HIT_FIELDS = ("hit", "object", "mesh", "tri", "leaf", "u", "v", "d", "w")   # every field of xrt_hit but `reserved` (scheduling feedback)


def build_checked():
    """The chunk planner's host program under ASan + UBSan (csrc/Makefile `hostcheck_trace`)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_trace"])
    return os.path.join(CSRC, "hostcheck_trace")


def sample_centers(centers, fixed16):
    """The positions the call makes rays at: the centres themselves, or the sixteen level-1 positions around each, (c + (+-0.25)) + (+-0.125) in
    binary32 and in this association (pixels_py.fixed16_offsets) -> (n * samples, 2) float32."""
    c = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 2)
    if not fixed16:
        return c
    f = np.float32
    out = np.empty((c.shape[0], 16, 2), dtype=np.float32)
    for s, ((ax, bx), (ay, by)) in enumerate(px.fixed16_offsets()):
        out[:, s, 0] = (c[:, 0] + f(ax)) + f(bx)
        out[:, s, 1] = (c[:, 1] + f(ay)) + f(by)
    return out.reshape(-1, 2)


def _split(v, size):
    """v = q size + r / k exactly: (k, q, k r) with k the smallest power of two (<= 16) that makes k v an integer."""
    v = np.asarray(v, dtype=np.float64)
    k = np.ones(v.shape, dtype=np.int64)
    for _ in range(4):
        k = np.where(v * k != np.floor(v * k), k * 2, k)
    assert np.all(v * k == np.floor(v * k)), "a centre that is no multiple of 1/16"
    q = np.floor(v / size).astype(np.int64)
    return k, q, ((v - q * size) * k).astype(np.int64)


def oracle_rays(orc, spec, positions):
    """The oracle's primary ray at every screen position of `positions` (n, 2) float32, by the camera of `spec` -> RAY_DTYPE[n]."""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 2)
    W, H = spec.width, spec.height
    kx, qx, rx = _split(p[:, 0], W)
    ky, qy, ry = _split(p[:, 1], H)
    k = np.maximum(kx, ky)
    rx, ry = rx * (k // kx), ry * (k // ky)
    out = np.zeros(p.shape[0], dtype=orc.RAY_DTYPE)
    keys = np.stack([k, qx, qy], axis=1)
    for key in np.unique(keys, axis=0):
        kk, a, b = (int(v) for v in key)
        sel = np.nonzero((keys == key).all(axis=1))[0]
        cam = orc.camera_abi(spec)
        cam.vp_width, cam.vp_height, cam.vp_x, cam.vp_y = kk * W, kk * H, -kk * a * W, -kk * b * H
        frame = np.zeros(kk * W * kk * H, dtype=orc.RAY_DTYPE)
        assert orc.lib().orc_generate_primary_rays(C.byref(cam), frame.ctypes.data) == 0
        out[sel] = frame[ry[sel] * (kk * W) + rx[sel]]
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_rays(a, b):
    """Bit for bit: origin, direction, and both ignore words."""
    return (a.shape == b.shape and np.array_equal(bits(a["o"]), bits(b["o"])) and np.array_equal(bits(a["d"]), bits(b["d"]))
            and np.array_equal(a["ignore_mesh"], b["ignore_mesh"]) and np.array_equal(a["ignore_tri"], b["ignore_tri"]))


def hit_diff(a, b):
    """The fields of xrt_hit (without `reserved`) in which two arrays of hits differ, with the number of records: {} when they are the same, bit for bit."""
    assert a.shape == b.shape, (a.shape, b.shape)
    out = {}
    for f in HIT_FIELDS:
        x, y = (bits(a[f]), bits(b[f])) if a[f].dtype == np.float32 else (a[f], b[f])
        bad = x != y
        if bad.any():
            out[f] = int(bad.reshape(bad.shape[0], -1).any(axis=1).sum())
    return out


def is_miss_record(h):
    """What lane_result leaves for a miss: hit 0; object, mesh, tri, leaf -1; u, v, d, wx, wy, wz 0.0f (the bits of +0)."""
    ok = (h["hit"] == 0) & (h["object"] == -1) & (h["mesh"] == -1) & (h["tri"] == -1) & (h["leaf"] == -1)
    for f in ("u", "v", "d"):
        ok &= bits(h[f]) == 0
    return ok & (bits(h["w"]).reshape(-1, 3) == 0).all(axis=1)


def reaches_root_box(rays, box):
    """The slab test on the scene's root box (OSM:460) in double: can the ray reach the box at all?  A classification of the test's inputs (which
    rays are rejected before any traversal), not a restatement of the kernel's arithmetic: rays within 1e-6 of the boundary count as neither."""
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    lo, hi = np.asarray(box[:3], dtype=np.float64), np.asarray(box[3:], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    tmin = np.nanmax(np.minimum(t1, t2), axis=1)
    tmax = np.nanmin(np.maximum(t1, t2), axis=1)
    tmin = np.maximum(tmin, 0.0)
    return tmax - tmin > 1e-6, tmin - tmax > 1e-6   # (clearly reaches, clearly cannot)
