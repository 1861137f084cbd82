"""TEST INFRASTRUCTURE for xrt_render_pixels (tests/test_pixels_cpu.py, tests/test_gpu_pixels.py).  The oracle renders frames only, so every
expectation is an oracle frame looked at in a particular way:
  - integer centres: the frame indexed at the listed pixels;
  - CastRay at a fractional position: Unproject divides (sx - vp.X) by vp.Width (RT:415), and scaling both by a power of two is exact in
    binary32, so the XRT_MS_OFF colour at (x + a / k, y + b / k), k a power of two, is pixel (k x + a, k y + b) of the oracle's XRT_MS_OFF frame
    of k times the size (same camera: the aspect ratio W / H is the same float);
  - outside the viewport: Unproject sees only sx - vp.X, so a frame whose vp_x / vp_y are shifted by integers has the colours of the centres
    shifted the other way.
With those, GetColorForQuadrant (RT:215-311) is restated here on looked-up CastRay colours, with and without the RT:305 slip, to show on the
CPU that a listed pixel reaches the slip."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_ROOT, "xna-ray-trace_amd", "csrc")
_F = C.POINTER(C.c_float)


def build_checked():
    """The chunk planner's host program under ASan + UBSan (csrc/Makefile `hostcheck_pixels`)."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_pixels"])
    return os.path.join(CSRC, "hostcheck_pixels")


def with_mode(spec, ms, quality=0, size=None, max_reflections=None):
    s = copy.copy(spec)
    s.multisampling, s.multisample_quality = ms, quality
    if size is not None:
        s.width, s.height = size
    if max_reflections is not None:
        s.max_reflections = max_reflections
    return s


def oracle_frame(orc, osc, spec, vp=(0, 0), rows=None):
    """OracleScene.render of `spec` on the built oracle scene `osc` (meshes and bodies of spec), with the viewport's origin at vp; rows: only
    these scanlines are rendered (the others stay zero).  -> (rgba (H, W) uint32, rgbf (H, W, 3) float32)."""
    abi = orc.abi
    cam, opts = orc.camera_abi(spec), orc.opts_abi(spec)
    cam.vp_x, cam.vp_y = int(vp[0]), int(vp[1])
    lights = (abi.xrt_light * max(len(spec.lights), 1))()
    for i, l in enumerate(spec.lights):
        lights[i] = orc.light_abi(l)
    rgba = np.zeros(spec.width * spec.height, dtype=np.uint32)
    rgbf = np.zeros((spec.width * spec.height, 3), dtype=np.float32)
    st = abi.xrt_stats()
    r0, r1 = (0, spec.height) if rows is None else rows
    rc = orc.lib().orc_render(osc.h, C.byref(cam), lights, len(spec.lights), C.byref(opts), rgba.ctypes.data, rgbf.ctypes.data, C.byref(st), 1, r0, r1)
    assert rc == 0, rc
    return rgba.reshape(spec.height, spec.width), rgbf.reshape(spec.height, spec.width, 3)


def grid_centers(w, h):
    """Every pixel of a w x h frame as centres, row-major: (w h, 2) float32."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.ravel(), y.ravel()], axis=1).astype(np.float32)


def to_vector3(orc, packed):
    v = np.zeros(3, dtype=np.float32)
    orc.lib().orc_kat_unpack_color(C.c_uint32(int(packed)), v.ctypes.data_as(_F))
    return v


def mean4(orc, four):
    """RT:309: new Color((a.ToVector3() + b.ToVector3() + c.ToVector3() + d.ToVector3()) / 4.0f), in binary32, left to right."""
    v = [to_vector3(orc, c) for c in four]
    s = ((v[0] + v[1]) + v[2]) + v[3]
    s = (s * np.float32(1.0 / 4.0)).astype(np.float32)   # (Vector3 / float multiplies by the reciprocal; 1 / 4 is exact)
    return int(orc.lib().orc_kat_pack_color(np.ascontiguousarray(s, dtype=np.float32).ctypes.data_as(_F)))


def mean16(orc, sixteen):
    """The fixed 16 samples: four RT:309 means of four, each re-quantised, then their mean."""
    return mean4(orc, [mean4(orc, sixteen[4 * q:4 * q + 4]) for q in range(4)])


def fixed16_offsets():
    """The sixteen positions around a centre, as (dx, dy) the way they are added: ((+-0.25), (+-0.125)) per axis, corner q = s / 4 in UL, UR,
    LL, LR order, sub-sample s % 4 likewise."""
    out = []
    for s in range(16):
        q, r = s >> 2, s & 3
        out.append(((0.25 if q & 1 else -0.25, 0.125 if r & 1 else -0.125), (0.25 if q & 2 else -0.25, 0.125 if r & 2 else -0.125)))
    return out


def quadrant_color(orc, cast, cx, cy, size, iteration, quality, slip=True, reached=None):
    """GetColorForQuadrant(cx, cy, size, iteration) (RT:215-311) on cast(x, y) -> packed CastRay colour.  slip=False: the lower-right recursion
    writes lrColor instead of urColor (RT:305 as it was presumably meant).  reached: a list that receives the iteration of every call in
    which the lower-right corner subdivides."""
    f = np.float32
    cx, cy, size = f(cx), f(cy), f(size)
    q = f(size * f(0.25))
    pos = [(f(cx - q), f(cy - q)), (f(cx + q), f(cy - q)), (f(cx - q), f(cy + q)), (f(cx + q), f(cy + q))]
    col = [cast(x, y) for x, y in pos]   # ul, ur, ll, lr
    if iteration < quality:
        vec = [to_vector3(orc, c) for c in col]
        avg = ((((vec[0] + vec[1]) + vec[2]) + vec[3]) * f(0.25)).astype(f)

        def length(v):
            return f(np.sqrt(f(f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2]))))
        al = length(avg)
        half = f(size / f(2.0))
        for j in range(4):
            if abs(f(al - length(vec[j]))) > f(0.5):   # RT:288-303 (the vectors are those of the first pass: RT:281-284)
                c = quadrant_color(orc, cast, pos[j][0], pos[j][1], half, iteration + 1, quality, slip, reached)
                if j == 3 and reached is not None:
                    reached.append(iteration)
                col[1 if (j == 3 and slip) else j] = c
    return mean4(orc, col)
