"""xrt_render_opts.list_order (XRT_LIST_COHERENT: "this list is in screen order") without a GPU: the constants and the field in the header, which
still compiles as strict C99 with the struct's size and offsets unchanged, the field in the Python and C# bindings, the keyword of the Python
mirror, a value that is neither constant refused with the other argument errors on a host-only scene, and the host program
tests/coherent/host_coherent.cpp (csrc/Makefile `hostcheck_coherent`, the library's sources with host ASan + UBSan): chunk sizes with the packet
table included, the table's capacity, and the mask plan_frame gives hinted and unhinted batches of one-body and two-level scenes at 1, 4 and
16 samples."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xna-ray-trace_amd", "csrc")


def test_header_defines_the_hint_and_is_still_c99(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "xrt.h")).read()
    assert re.search(r"#define XRT_LIST_UNORDERED\s+0\b", hdr) and re.search(r"#define XRT_LIST_COHERENT\s+1\b", hdr)
    assert "#define XRT_VERSION 203" in hdr
    opts_c = re.search(r"typedef struct xrt_render_opts \{(.*?)\} xrt_render_opts;", hdr, re.S).group(1)
    assert re.search(r"int32_t\s+list_order;\s*int32_t\s+reserved;", opts_c)
    assert "bit for bit those of the unhinted call" in re.sub(r"\s*\n\s*\*\s*", " ", opts_c)   # the promise is in the header
    src = tmp_path / "hdr.c"
    src.write_text('#include <stddef.h>\n#include "xrt.h"\n'
                   'typedef char size_is_48[sizeof(xrt_render_opts) == 48 ? 1 : -1];\n'
                   'typedef char order_at_40[offsetof(xrt_render_opts, list_order) == 40 ? 1 : -1];\n'
                   'typedef char reserved_at_44[offsetof(xrt_render_opts, reserved) == 44 ? 1 : -1];\n'
                   'int main(void) { xrt_render_opts o; o.list_order = XRT_LIST_COHERENT; o.reserved = XRT_LIST_UNORDERED; return o.list_order + o.reserved - 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_bindings_carry_the_field(xrt):
    a = xrt.abi
    assert (a.LIST_UNORDERED, a.LIST_COHERENT) == (0, 1)
    o = a.xrt_render_opts()
    assert C.sizeof(o) == 48 and a.xrt_render_opts.list_order.offset == 40 and a.xrt_render_opts.reserved.offset == 44
    assert o.list_order == 0   # a fresh struct is the unhinted call
    cs = open(os.path.join(ROOT, "csharp", "XrtNative.cs")).read()
    opts_cs = re.search(r"public struct XrtRenderOpts\s*\{(.*?)\n    \}", cs, re.S).group(1)
    names = [n.strip() for m in re.finditer(r"public int ([^;]+);", opts_cs) for n in m.group(1).split(",")]
    assert names[-2:] == ["listOrder", "reserved"] and len(names) == 12, names
    assert re.search(r"LIST_UNORDERED = 0, LIST_COHERENT = 1", cs)
    for fn in (xrt.RayTracer.RenderPixels, xrt.RayTracer.CastRays):
        assert inspect.signature(fn).parameters["coherent"].default is False, fn


@pytest.fixture(scope="module")
def host_only(xrt):
    return xrt.configs.build_product(xrt.configs.crate_scene(8, 8, max_reflections=1), device=-1)


def test_a_value_that_is_no_constant_is_an_argument_error(xrt, host_only):
    """Said with the other argument errors, before the scene's device is looked at: xrt_render_pixels[_device] and xrt_shade_hits[_device] on a
    host-only scene.  Both constants pass the argument checks (the call then stops at the missing device)."""
    scene, tracer = host_only
    a, lib = xrt.abi, xrt.abi.lib()
    cam, lights, nl = tracer._camera_abi(), tracer._lights_abi(), len(tracer.Lights)
    c = np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32)
    rgba = np.zeros(2, dtype=np.uint32)
    rays = np.zeros(2, dtype=xrt.RAY_DTYPE)
    hits = np.zeros(2, dtype=xrt.HIT_DTYPE)
    u32 = C.POINTER(C.c_uint32)

    def pixels(o):
        return lib.xrt_render_pixels(scene.handle, C.byref(cam), lights, nl, C.byref(o), c.ctypes.data_as(C.POINTER(C.c_float)), 2, rgba.ctypes.data_as(u32), None, None)

    def pixels_device(o):   # (no device memory here: nothing reads the pointers before the scene is looked at)
        return lib.xrt_render_pixels_device(scene.handle, C.byref(cam), lights, nl, C.byref(o), C.c_void_p(4096), 2, C.c_void_p(8192), None, None, None)

    def shade(o):
        return lib.xrt_shade_hits(scene.handle, rays.ctypes.data_as(C.POINTER(a.xrt_ray)), hits.ctypes.data_as(C.POINTER(a.xrt_hit)), 2, 0, 1.0, lights, nl, C.byref(o),
                                  rgba.ctypes.data_as(u32), None, None)

    for call in (pixels, pixels_device, shade):
        for bad in (2, -1, 0x7fffffff):
            o = tracer._opts_abi(shard_count=0)
            o.n_gpus, o.list_order = 0, bad
            assert call(o) == a.XRT_E_INVALID_ARG, (call.__name__, bad)
            assert b"list_order" in lib.xrt_last_error(), lib.xrt_last_error()
        for good in (a.LIST_UNORDERED, a.LIST_COHERENT):
            o = tracer._opts_abi(shard_count=0)
            o.n_gpus, o.list_order = 0, good
            assert call(o) == a.XRT_E_NO_DEVICE, (call.__name__, good)
    # ... and the second word is still reserved: nobody reads it
    o = tracer._opts_abi(shard_count=0)
    o.n_gpus, o.reserved = 0, 77
    assert pixels(o) == a.XRT_E_NO_DEVICE


def test_host_program():
    """Chunk sizes with the table included, the table's capacity, the plan's mask (tests/coherent/host_coherent.cpp), under ASan + UBSan."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "hostcheck_coherent"])
    p = subprocess.run([os.path.join(CSRC, "hostcheck_coherent")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "host_coherent: ok" in p.stdout
    m = re.search(r"plans (\d+) masks (\d+)", p.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) == 30
    m = re.search(r"scene masks (\d+)", p.stdout)   # scene_packet_mask against plan_frame: 2 scene kinds x packetOk x 7 settings of XRT_PACKET x 3 samplings
    assert m and int(m.group(1)) == 2 * 2 * 7 * 3
