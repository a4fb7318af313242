"""Direct light sampling in the f32 Philox kernels (nrt_render_opts.direct_light, DESIGN "Direct light").

The option changes the estimator, not the expected frame: one light sample and shadow ray at every Lambertian
hit, weighted by the density of the reference's scatter direction (not a cosine lobe), and no radiance from a
light the scattered ray then hits by chance.  The reference has no counterpart, so the checks are statistical,
against the oracle's high-spp fixtures (tests/golden/stat for the Cornell box, tests/golden/stat_direct for
scenes/direct-lights.toml: an emissive quad, triangle and sphere, a panel lit from behind, metal, glass).

Unbiasedness: A, B = the frames of two disjoint windows of S samples, m = (A + B) / 2.  (A - B) / 2 has exactly
the noise of m and is independent of it, so T = mean[((m - want)^2 - ((A - B) / 2)^2) / (var_fix / S_fix)] has
expectation 1 + bias^2 / (var_fix / S_fix) whatever the new estimator's variance is; it must lie in the project's
chi^2 window.  r = mean[((A - B) / 2)^2 / (var_fix / S_fix)] is printed with it (T's spread is about
sqrt(1 + 2 r + 2 r^2) times the plain chi^2's).
"""
import json
import os

import numpy as np
import pytest

import nrt
from helpers import GOLDEN, in_golden
from test_stat_parity import CHI2, MEAN_TOL, channel_rel, dead_tol

CORNELL, LIGHTS, EARTH = "scenes/cornell-box-scene.json", "scenes/direct-lights.toml", "scenes/earth.toml"
PHILOX = dict(precision="f32", rng="philox")


def fixture(name):
    d = os.path.join(GOLDEN, "stat" if name == "cornell_32" else "stat_direct")
    with open(os.path.join(d, "manifest.json")) as fh:
        c = json.load(fh)["cases"][name]
    shape = (c["height"], c["width"], 3)
    mean, var = (np.fromfile(os.path.join(d, c[k]), dtype="<f4").astype(np.float64).reshape(shape) for k in ("mean", "var"))
    return c, mean, np.maximum(var, 0.0)


def load(scene, w, h, spp, bounces=None):
    with in_golden():
        return nrt.Scene.load(scene, nrt.CameraConfig(width=w, height=h, samples_per_pixel=spp, ray_max_bounces=bounces))


# (fixture, trace, S per window).  S starts at 2^18 and doubles (to 2^22 at most) where T lands outside with T moving
# towards 1 as S grows (DESIGN "Direct light" has every figure): the Cornell box, whose light hangs 0.002 under the
# ceiling, so that the light samples of the ceiling around it have a very wide spread (r = 1.47 at 2^18, T = 2.66,
# 0.80, 1.00 at 2^18, 2^20, 2^22; the plain path at 2^22: 1.09).
# The scene's mirror has no fuzz: a fuzzed Metal sends its ray along reflect + fuzz p / |p|^2, whose length has no
# bound, so with two bounces its pixels are black but for events of probability ~1e-5, and 2^18 oracle samples cannot
# estimate such a pixel's variance, which T divides by (two such pixels gave the plain path T = 1.32 at 2^22).
UNBIASED = [
    ("cornell_32", "auto", 1 << 22), ("cornell_32", "world-bvh", 1 << 22), ("lights_32", "auto", 1 << 18),
    ("lights_32", "world-bvh", 1 << 18), ("lights_32_b2", "auto", 1 << 18)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,trace,S", UNBIASED, ids=[f"{u[0]}-{u[1]}" for u in UNBIASED])
def test_direct_light_is_unbiased(name, trace, S):
    c, want, var = fixture(name)
    s = load(c["scene"], c["width"], c["height"], S, c.get("ray_max_bounces"))
    a, b = (s.render(trace=trace, direct_light=True, sample_offset=k * S, **PHILOX).astype(np.float64) for k in (0, 1))
    m, half = (a + b) / 2, (a - b) / 2
    assert np.all(np.isfinite(m)) and np.all(m >= 0)
    live = var > 1e-9 * np.maximum(want * want, 1e-6)  # (test_stat_parity.chi2_per_n's constant-pixel rule)
    unit = var[live] / c["spp"]
    T = float(np.mean(((m[live] - want[live]) ** 2 - half[live] ** 2) / unit))
    r = float(np.mean(half[live] ** 2 / unit))
    dead = float(np.abs(m[~live] - want[~live]).max()) if (~live).any() else 0.0
    rel = channel_rel(m, want)
    print(f"{name} {trace} S={S}: T = {T:.4f}, r = {r:.4f}, mean rel {rel}, constant-pixel max diff {dead:.2e}")
    assert np.all(rel < MEAN_TOL), f"per-channel mean off by {rel}"
    assert CHI2[0] <= T <= CHI2[1], f"T = {T:.4f} (r = {r:.4f})"
    assert dead <= dead_tol(want, c["spp"]), dead


@pytest.mark.gpu
def test_direct_light_lowers_the_cornell_rmse():
    c, want, _ = fixture("cornell_32")
    s = load(c["scene"], c["width"], c["height"], 64)
    rmse = [float(np.sqrt(np.mean((s.render(direct_light=d, **PHILOX) - want) ** 2))) for d in (False, True)]
    print(f"cornell_32 spp 64: RMSE plain {rmse[0]:.5f}, direct {rmse[1]:.5f}, ratio {rmse[1] / rmse[0]:.3f}")
    assert rmse[1] < rmse[0]


@pytest.mark.gpu
def test_scene_without_lights_renders_the_plain_frame():
    s = load(EARTH, 48, 27, 8)
    np.testing.assert_array_equal(s.render(direct_light=True, **PHILOX), s.render(**PHILOX))


@pytest.mark.gpu
def test_specialised_and_generic_kernels_agree(monkeypatch):
    s = load(LIGHTS, 32, 32, 16)
    monkeypatch.setenv("NRT_JIT", "0")
    generic = s.render(direct_light=True, **PHILOX)
    monkeypatch.setenv("NRT_JIT", "require")
    before = nrt.jit_stats()["launches"]
    special = s.render(direct_light=True, **PHILOX)
    assert nrt.jit_stats()["launches"] == before + 1
    assert generic.max() > 0 and not np.array_equal(generic, s.render(**PHILOX))
    np.testing.assert_array_equal(special, generic)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65])
def test_pixel_list_equals_the_frame(n):
    s = load(LIGHTS, 32, 32, 16)
    frame = s.render(direct_light=True, **PHILOX).reshape(-1, 3)
    px = (np.arange(n, dtype=np.uint32) * 37 + 5) % (32 * 32)
    np.testing.assert_array_equal(s.render_pixels(px, direct_light=True), frame[px])


# ------------------------------------------------------------------ CPU: status codes and light counts

def moving_light():
    b = nrt.Builder()
    quad = b.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), b.lambertian(b.solid((0.7, 0.7, 0.7))))
    ball = b.sphere((0, 2, 0), 0.5, b.diffuse_light(4.0, b.solid((1.0, 1.0, 1.0))), speed=(0, 0.5, 0))
    return b.finish(b.bvh([quad, ball]))


STATUS = [  # (scene, camera overrides, render keywords, code): NRT_E_INVALID -1, NRT_E_UNSUPPORTED -4
    (CORNELL, {}, dict(precision="f32", rng="chacha8"), -1),
    (CORNELL, dict(ray_max_bounces=127), PHILOX, -1),
    (CORNELL, {}, dict(precision="f64", rng="philox"), -4),
    (CORNELL, {}, dict(trace="bvh", **PHILOX), -4),
    (CORNELL, {}, dict(gpus=1, **PHILOX), -4),
    (None, {}, PHILOX, -4)]


@pytest.mark.parametrize("scene,over,kw,code", STATUS, ids=["chacha8", "bounces", "f64", "instance-bvh", "gpus", "moving-light"])
def test_status_codes_arrive_without_a_device(scene, over, kw, code):
    if scene is None:
        s, cam = moving_light(), nrt.CameraBuilder(width=8, height=8, look_from=(0, 2, 6), look_at=(0, 1, 0)).build()
    else:
        with in_golden():
            s = nrt.Scene.load(scene, nrt.CameraConfig(width=8, height=8, samples_per_pixel=4, **over))
        cam = None
    with pytest.raises(nrt.NrtError) as ei:
        s.render(cam, direct_light=True, **kw)
    assert ei.value.code == code, ei.value


@pytest.mark.parametrize("scene,lights", [(CORNELL, 1), (LIGHTS, 3), (EARTH, 0)])
def test_light_count(scene, lights):
    with in_golden():
        s = nrt.Scene.load(scene, nrt.CameraConfig(width=8, height=8))
    assert s.stats()["lights"] == lights
    if scene == LIGHTS:  # the file's count
        with open(os.path.join(GOLDEN, scene)) as fh:
            text = fh.read()
        emissive = [ln.split(".")[1] for ln in text.splitlines() if ln.startswith("[materials.") and "DiffuseLight" in ln]
        assert sum(text.count(f'material = "{m}"') for m in emissive) == lights
