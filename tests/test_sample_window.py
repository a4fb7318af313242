"""Sample windows of the Philox kernels (nrt_render_opts.sample_offset): a launch renders samples
[s0, s0 + spp) of every pixel.  A sample's blocks are keyed by (pixel, sample index, step) whatever launch
draws it, so the frames R(s0, m) of windows compose; offset 0 is the frame of every earlier version.  All
renders 16 x 16."""
import numpy as np
import pytest

import nrt
from helpers import in_golden

CORNELL = "scenes/cornell-box-scene.json"


def load(scene):
    with in_golden():
        return nrt.Scene.load(scene, nrt.CameraConfig(width=16, height=16))


@pytest.mark.gpu
@pytest.mark.parametrize("a,n", [(2, 2), (4, 4), (3, 5)])
@pytest.mark.parametrize("scene,precision", [(CORNELL, "f32"),              # world list, scene-specialised kernel
                                             ("scenes/spheres.toml", "f32"),  # world BVH, generic kernel, defocus on
                                             (CORNELL, "f64")])
def test_windows_compose(scene, precision, a, n):
    """(a + n) R(0, a + n) = a R(0, a) + n R(a, n) in f64.  The pixel sums are exact integers on the 2^-k grid;
    what remains is one f32 rounding per render and the grid rounding of each sample, k moving with log2(spp)
    (api.cpp) more than 20 bits below an f32 ulp of any visible radiance.  Bound 2^-22 (a + n) max(R): four f32
    ulps of the largest term, derived, not measured."""
    s = load(scene)

    def R(s0, m):  # the window [s0, s0 + m); None: a call without the keyword
        kw = {} if s0 is None else {"sample_offset": s0}
        return s.render(s.camera.with_samples(m), precision=precision, rng="philox", **kw).astype(np.float64)

    whole, head, tail = R(0, a + n), R(0, a), R(a, n)
    err = np.abs((a + n) * whole - (a * head + n * tail)).max()
    bound = 2.0 ** -22 * (a + n) * max(whole.max(), head.max(), tail.max())
    print(f"windows {scene} {precision} a={a} n={n}: max|lhs - rhs| = {err:.3e}, bound {bound:.3e}")
    assert whole.max() > 0 and err <= bound
    assert not np.array_equal(tail, R(0, n))
    assert np.array_equal(R(None, n), R(0, n))


@pytest.mark.gpu
def test_specialised_and_generic_kernels_agree_at_an_offset(monkeypatch):
    s = load(CORNELL)
    cam = s.camera.with_samples(4)
    monkeypatch.setenv("NRT_JIT", "0")
    before = nrt.jit_stats()
    generic = s.render(cam, precision="f32", rng="philox", sample_offset=12)
    assert nrt.jit_stats()["launches"] == before["launches"]
    monkeypatch.setenv("NRT_JIT", "require")
    special = s.render(cam, precision="f32", rng="philox", sample_offset=12)
    after = nrt.jit_stats()
    assert after["launches"] == before["launches"] + 1 and after["failed"] == before["failed"]
    assert generic.max() > 0
    np.testing.assert_array_equal(special.view(np.uint32), generic.view(np.uint32))
    assert not np.array_equal(special, s.render(cam, precision="f32", rng="philox"))


@pytest.mark.parametrize("kw", [dict(spp=4, precision="f64", rng="chacha8", sample_offset=1),
                                dict(spp=4, precision="f32", rng="philox", sample_offset=(1 << 24) - 3),
                                dict(spp=3, precision="f32", rng="philox", denoise="dual"),
                                dict(spp=2, precision="f32", rng="philox", denoise="dual")])
def test_argument_errors_need_no_device(kw):
    b = nrt.Builder()
    scene = b.finish(b.bvh([b.sphere((0, 0, -2), 1.0, b.lambertian(b.solid((1, 1, 1))))]))
    cam = nrt.CameraBuilder(width=4, height=4, samples_per_pixel=kw.pop("spp")).build()
    with pytest.raises(nrt.NrtError) as ei:
        scene.render(cam, **kw)
    assert ei.value.code == -1, ei.value
