"""Shading signature of the scene-specialised kernels (kernel.hpp ShadeSig, render.hip): the material
kinds a scene uses and the camera's mode (defocus on or off, spp > 1) are template arguments of its
hiprtc-built kernel, so the arms the scene cannot reach are not compiled in.  What stays is the generic
kernel's arithmetic, so every specialised frame must equal the generic kernel's (NRT_JIT=0) bit for bit;
the signature is taken from the scene and from the camera of each render, so another material set or
another camera mode gets another kernel, never a stale one.  The reference has no counterpart (its
materials are trait objects, camera.rs / material.rs); all renders 32 x 32, f32 / Philox."""
import dataclasses

import numpy as np
import pytest

import nrt
from helpers import in_golden

pytestmark = pytest.mark.gpu

CORNELL = "scenes/cornell-box-scene.json"
W = H = 32


def cornell(spp=8, **overrides):
    with in_golden():
        return nrt.Scene.load(CORNELL, nrt.CameraConfig(width=W, height=H, samples_per_pixel=spp, **overrides))


def camera(spp=8, defocus_angle=0.0):
    return nrt.CameraBuilder(width=W, height=H, look_from=(0.0, 1.2, 4.5), look_at=(0.0, 1.0, 0.0),
                             field_of_view=1.0, background_color=(0.5, 0.6, 0.8), defocus_angle=defocus_angle,
                             focus_dist=4.0, samples_per_pixel=spp, ray_max_bounces=12).build()


def mixed_scene():
    """Quads of all four kinds: a fuzzy metal wall (absorbs where the fuzzed ray points into it), a glass
    slab of two panes crossed both ways (front and back hits, reflection and refraction), a light."""
    b = nrt.Builder()
    grey, red = b.lambertian(b.solid((0.7, 0.7, 0.7))), b.lambertian(b.solid((0.7, 0.2, 0.2)))
    metal, glass = b.metal(0.4, b.solid((0.8, 0.8, 0.6))), b.dielectric(1.5)
    light = b.diffuse_light(4.0, b.solid((1.0, 1.0, 1.0)))
    quads = [b.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), grey),      # floor
             b.quad((-3, 0, -3), (6, 0, 0), (0, 4, 0), metal),     # back wall
             b.quad((-3, 0, -3), (0, 0, 6), (0, 4, 0), red),       # left wall
             b.quad((-1, 0.2, 1.0), (2, 0, 0.5), (0, 1.6, 0), glass),
             b.quad((-1, 0.2, 0.8), (2, 0, 0.5), (0, 1.6, 0), glass),
             b.quad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), light)]
    return b.finish(b.bvh(quads))


def diffuse_room():
    """Lambertian walls and a light, nothing else: the kernel carries neither metal nor dielectric arm."""
    b = nrt.Builder()
    grey, green = b.lambertian(b.solid((0.7, 0.7, 0.7))), b.lambertian(b.solid((0.2, 0.7, 0.2)))
    light = b.diffuse_light(5.0, b.solid((1.0, 0.9, 0.8)))
    quads = [b.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), grey), b.quad((-3, 0, -3), (6, 0, 0), (0, 4, 0), grey),
             b.quad((-3, 0, -3), (0, 0, 6), (0, 4, 0), green), b.quad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), light)]
    return b.finish(b.bvh(quads))


def tilted_quads(metal):
    """Five quads off the axes (one run of general quads); the last one Lambertian or metal."""
    b = nrt.Builder()
    grey = b.lambertian(b.solid((0.6, 0.6, 0.6)))
    last = b.metal(0.3, b.solid((0.6, 0.6, 0.6))) if metal else grey
    quads = [b.quad((-2 + i, 0.1 * i, -1 - 0.3 * i), (1.5, 0.2, 0.1), (0.1, 1.5, 0.3), last if i == 4 else grey)
             for i in range(5)]
    return b.finish(b.bvh(quads))


def both(monkeypatch, scene, cam):
    """(generic, specialised) frames of one camera; the specialised render must have run a hiprtc kernel."""
    monkeypatch.setenv("NRT_JIT", "0")
    before = nrt.jit_stats()
    generic = scene.render(cam, precision="f32", rng="philox")
    assert nrt.jit_stats()["launches"] == before["launches"]
    monkeypatch.setenv("NRT_JIT", "require")
    special = scene.render(cam, precision="f32", rng="philox")
    after = nrt.jit_stats()
    assert after["launches"] == before["launches"] + 1 and after["failed"] == before["failed"]
    assert np.isfinite(generic).all() and generic.max() > 0
    return generic, special


@pytest.mark.parametrize("spp", [8, 1])
def test_cornell_equals_generic(monkeypatch, spp):
    """Lambertian, a light and one slightly fuzzy metal box: no dielectric or defocus code in the kernel;
    spp 1: no pixel jitter either."""
    s = cornell(spp)
    generic, special = both(monkeypatch, s, s.camera)
    np.testing.assert_array_equal(special, generic)


def test_lambertian_and_light_only_equals_generic(monkeypatch):
    generic, special = both(monkeypatch, diffuse_room(), camera(8))
    np.testing.assert_array_equal(special, generic)


@pytest.mark.parametrize("defocus_angle", [0.0, 0.05])
def test_all_material_kinds_equal_generic(monkeypatch, defocus_angle):
    """Metal absorption (`killed`), both dielectric branches, and the defocus disk when the angle is set."""
    s = mixed_scene()
    assert s.stats()["world_list_ok"]
    cam = camera(8, defocus_angle)
    assert (any(cam.defocus_disk_u) or any(cam.defocus_disk_v)) == (defocus_angle > 0)
    generic, special = both(monkeypatch, s, cam)
    np.testing.assert_array_equal(special, generic)


def test_material_sets_build_different_kernels(monkeypatch, tmp_path):
    """The same run words with another material set is another kernel: two compiles, each frame the
    generic kernel's (a kernel built for Lambertian alone would render the metal as Lambertian)."""
    monkeypatch.setenv("NRT_JIT_CACHE", str(tmp_path))  # (an empty disk cache: both kernels are compiled here)
    cam = camera(8)
    before = nrt.jit_stats()
    frames = []
    for metal in (False, True):
        generic, special = both(monkeypatch, tilted_quads(metal), cam)
        np.testing.assert_array_equal(special, generic)
        frames.append(special)
    after = nrt.jit_stats()
    assert after["compiled"] == before["compiled"] + 2 and after["disk_hits"] == before["disk_hits"]
    assert not np.array_equal(frames[0], frames[1])


def test_camera_change_selects_its_variant(monkeypatch):
    """One loaded scene, two cameras: no defocus at spp 8, then a defocus disk at spp 1.  Each render runs
    the variant of its own camera: the frame of the generic kernel with that camera."""
    s = cornell(8)
    plain = s.camera
    blurred = dataclasses.replace(cornell(1, defocus_angle=2.0).camera)
    assert not any(plain.defocus_disk_u) and any(blurred.defocus_disk_u) and blurred.samples_per_pixel == 1
    frames = []
    for cam in (plain, blurred, plain):
        generic, special = both(monkeypatch, s, cam)
        np.testing.assert_array_equal(special, generic)
        frames.append(special)
    np.testing.assert_array_equal(frames[2], frames[0])
    assert frames[1].shape == frames[0].shape and not np.array_equal(frames[1], frames[0])
