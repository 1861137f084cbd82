"""The packet walk's run test under the leaf's margin (packet.hip pk_walk) on the MI355X: a leaf of 16 references or more tests its runs of 8 against the
run's vertex box grown by the LEAF's margin when every lane of the packet has a usable one, and with the run's own full test otherwise.  A 64 x 64-quad
heightfield (840 big leaves) rendered from a grazing and from a top-down camera, and the adversarial rays of tests/run_margin/run_margin.cpp -- the
CPU test's -- cast at it through the packet kernel, answer like the oracle bit for bit."""
import numpy as np
import pytest

import run_margin_py
from util import hits_equal

pytestmark = pytest.mark.gpu


def _spec(xrt, pos, target):
    spec = xrt.configs.heightfield_scene(128, 72, m=64, max_reflections=3, multisampling=xrt.abi.MS_FIXED16)
    spec.camera = xrt.configs.camera(pos, target)
    return spec


@pytest.mark.parametrize("view", ["grazing", "top_down"])
def test_small_parity_render(xrt, orc, view):
    """128 x 72 with 16 sub-rays and depth 3 (a one-body frame with 16 sub-rays walks packets by default): RGBA8 equal to the oracle's."""
    spec = _spec(xrt, (0, 9, 70), (0, 2, 0)) if view == "grazing" else _spec(xrt, (3, 140, 12), (0, 0, 0))
    _, tracer = xrt.configs.build_product(spec)
    o_rgba, _, _ = orc.OracleScene(spec).render(nthreads=8, want_float=False)
    rgba = tracer.Render()
    assert len(np.unique(o_rgba)) > 1000   # (the terrain is in the picture)
    assert np.array_equal(rgba, o_rgba), "%d bytes differ" % int((rgba != o_rgba).sum())


def test_adversarial_rays_through_the_packet_kernel(xrt, orc, monkeypatch):
    """XRT_PACKET=31 sends caller-given batches of a one-body scene to k_packet (xrt_api.cpp: bit 3 of the mask).  Every category goes as a batch of its
    own, so the packets of the grazing and vertex / edge rays take the cheap path in the leaves they pass, those of the in-plane rays fall back in the
    leaves whose plane they lie in, and the axis-parallel, tiny-component and non-finite packets fall back everywhere."""
    monkeypatch.setenv("XRT_PACKET", "31")
    spec = xrt.configs.heightfield_scene(64, 36, m=64)
    scene, _ = xrt.configs.build_product(spec)
    o = orc.OracleScene(spec)
    sets = run_margin_py.adversarial_rays(3000)
    assert set(sets) == set(run_margin_py.CATEGORIES)
    for name, (org, d) in sets.items():
        assert len(org) >= 3000, name
        rays = xrt.rays_array(org, d)
        ho = o.intersect(rays)
        if name != "non_finite":
            assert 0.02 < (ho["hit"] != 0).mean() < 0.999, (name, (ho["hit"] != 0).mean())
        assert hits_equal(ho, scene.IntersectBatch(rays)) == {}, name
