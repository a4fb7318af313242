"""Adaptive sampling (include/nrt.h: nrt_render_pixels, nrt_adaptive_select, nrt_render_adaptive): the list render
against the frame, the selection against its definition in numpy f64, and the refinement loop against plain window
renders.  All renders are the Cornell box, f32 / Philox unless a case says otherwise."""
import functools

import numpy as np
import pytest

import nrt
from helpers import in_golden
from test_denoise_vg import taps

CORNELL = "scenes/cornell-box-scene.json"
KW = dict(precision="f32", rng="philox")


@functools.lru_cache(maxsize=None)
def cornell(w, h):
    with in_golden():
        return nrt.Scene.load(CORNELL, nrt.CameraConfig(width=w, height=h))


@functools.lru_cache(maxsize=None)
def window(w, h, s0, m, precision="f32", trace="auto"):
    """R(s0, m): the plain frame of the window [s0, s0 + m), once per session, read-only."""
    s = cornell(w, h)
    out = s.render(s.camera.with_samples(m), precision=precision, rng="philox", trace=trace, sample_offset=s0)
    out.setflags(write=False)
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def error_f64(A, B, n, albedo, N, Z, sn=0.3, sz=0.5):
    """err(p) of nrt.h in f64."""
    A, B, n, albedo, N, Z = (x.astype(np.float64) for x in (A, B, n, albedo, N, Z))
    a = np.maximum(albedo, 1e-3)
    lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]  # noqa: E731
    v = n * (lum((A - B) / a) / 2) ** 2
    sw, s2 = np.zeros(n.shape), np.zeros(n.shape)
    for _, _, P, Q in taps(*n.shape, 3, 1):
        w = np.exp(-(((N[P] - N[Q]) ** 2).sum(-1) / sn ** 2 + (Z[P] - Z[Q]) ** 2 / sz ** 2))
        sw[P] += w
        s2[P] += w * v[Q]
    return np.sqrt(s2 / sw / n) / (lum(((A + B) / 2) / a) + 0.01)


def tile_order(mask):
    """The selected pixels' linear indices, 32 x 8 tiles row-major, pixels row-major inside a tile."""
    H, W = mask.shape
    out = []
    for ty in range(0, H, 8):
        for tx in range(0, W, 32):
            ys, xs = np.nonzero(mask[ty:ty + 8, tx:tx + 32])
            out.extend((ys + ty) * W + xs + tx)
    return np.array(out, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [1, 63, 65, 37 * 21])
@pytest.mark.parametrize("s0", [0, 6])
@pytest.mark.parametrize("precision,trace", [("f32", "world-list"), ("f32", "world-bvh"), ("f32", "bvh"), ("f64", "auto")])
def test_list_render_is_the_frame(precision, trace, s0, length):
    """37 x 21 at spp 4: list lengths that are no multiple of a group's pixels, on both sides of a wave's 64 lanes and
    the whole frame; every list holds the frame's last pixel, in a shuffled order."""
    W, H = 37, 21
    L = np.random.default_rng(length).permutation(W * H - 1)[:length - 1].astype(np.uint32)
    L = np.insert(L, length // 2, W * H - 1)
    s = cornell(W, H)
    got = s.render_pixels(L, s.camera.with_samples(4), precision=precision, trace=trace, sample_offset=s0)
    frame = window(W, H, s0, 4, precision, trace)
    assert got.shape == (length, 3) and frame.max() > 0
    np.testing.assert_array_equal(bits(got), bits(frame.reshape(-1, 3)[L]))


@pytest.mark.gpu
def test_generic_and_specialised_kernels_read_the_list(monkeypatch):
    W, H = 37, 21
    s, L = cornell(W, H), np.arange(W * H - 65, W * H, dtype=np.uint32)[::-1]
    want = window(W, H, 6, 4).reshape(-1, 3)[L]
    for jit in ("0", "require"):
        monkeypatch.setenv("NRT_JIT", jit)
        before = nrt.jit_stats()
        got = s.render_pixels(L, s.camera.with_samples(4), sample_offset=6)
        after = nrt.jit_stats()
        assert after["launches"] == before["launches"] + (jit == "require") and after["failed"] == before["failed"]
        np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.gpu
def test_selection_matches_f64_definition():
    """45 x 19: two tiles across, three down, short edge tiles both ways; two normal regions split at x = 20, a depth
    step of 1.5 at y >= 12, x >= 30; 15 % of the pixels hold 8 samples per half and are no candidates at level 4.
    The threshold is the median reference error of the candidates; pixels within a relative 1e-3 of it may fall
    either way and are left out (at most 1 % of the frame).  error_out: the ceiling 1e-4 stands for 49 non-negative
    f32 terms whose weights' exponent argument carries e 2^-23 with e up to ~100 before w vanishes; measured on the
    GPU: 2.941e-07 (relative, max), and the assertion is ten times that, 2.941e-06."""
    H, W = 19, 45
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:H, 0:W]
    N = np.where((xs < 20)[..., None], [0, 0, 1.0], [0.6, 0, 0.8]).astype(np.float32)
    Z = (2.0 + 0.01 * xs + 1.5 * ((ys >= 12) & (xs >= 30))).astype(np.float32)
    albedo = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    mean = rng.uniform(0.05, 2.0, (H, W, 1)) * albedo
    sigma = rng.uniform(0.02, 0.6, (H, W, 1))
    A, B = (np.abs(mean * (1 + sigma * rng.standard_normal((H, W, 3)))).astype(np.float32) for _ in range(2))
    n = np.where(rng.random((H, W)) < 0.15, 8, 4).astype(np.uint32)
    ref = error_f64(A, B, n, albedo, N, Z)
    threshold = float(np.float32(np.median(ref[n == 4])))
    near = np.abs(ref - threshold) <= 1e-3 * threshold
    assert near.sum() <= 0.01 * H * W
    pixels, err = nrt.adaptive_select(A, B, n, albedo, N, Z, level=4, threshold=threshold)
    want = (n == 4) & (ref >= threshold)
    got = np.zeros(H * W, bool)
    got[pixels] = True
    assert len(set(pixels.tolist())) == len(pixels) and 0 < want.sum() < (n == 4).sum()
    assert np.array_equal(got.reshape(H, W)[~near], want[~near])
    np.testing.assert_array_equal(pixels, tile_order(got.reshape(H, W)))
    rel = (np.abs(err - ref) / ref).max()
    print(f"adaptive_select {W}x{H}: {len(pixels)} selected, {near.sum()} near the threshold, max rel error {rel:.3e}")
    assert rel <= min(10 * 2.941e-7, 1e-4)


LOOP = dict(w=32, h=24, S=32, lo=8)


def run_loop(threshold):
    s = cornell(LOOP["w"], LOOP["h"])
    shape = (LOOP["h"], LOOP["w"])
    samples, halves = np.zeros(shape, np.uint32), (np.zeros(shape + (3,), np.float32), np.zeros(shape + (3,), np.float32))
    out = s.render_adaptive(s.camera.with_samples(LOOP["S"]), threshold=threshold, min_samples=LOOP["lo"],
                            samples_out=samples, halves_out=halves)
    return out, samples, halves


@pytest.mark.gpu
def test_loop_ends():
    """threshold 1e30: nothing is refined, the frame is the mean of the two first windows, bit for bit.  threshold 0:
    every pixel reaches the cap and has drawn the plain render's samples; the two frames differ by one f32 rounding
    per window frame, one per merge and one for the mean on the adaptive side against one on the plain side, all
    terms non-negative: 2^-24 (3 passes + 2) max(R) with passes = log2(S / min_samples) = 2."""
    w, h = LOOP["w"], LOOP["h"]
    out, samples, _ = run_loop(1e30)
    np.testing.assert_array_equal(bits(out), bits((window(w, h, 0, 4) + window(w, h, 16, 4)) * np.float32(0.5)))
    assert (samples == 8).all()
    out, samples, _ = run_loop(0.0)
    print("samples at threshold 0:", dict(zip(*np.unique(samples, return_counts=True))))
    assert (samples == 32).all()
    plain = window(w, h, 0, 32).astype(np.float64)
    err, bound = np.abs(out - plain).max(), 2.0 ** -24 * (3 * 2 + 2) * plain.max()
    print(f"adaptive at the cap against spp 32: max|diff| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.gpu
def test_mixed_map_merges_the_right_pixels():
    """Threshold = the median reference error at level 0: about half of the pixels stop at 8 samples.  Every pixel's
    halves are the f64 merge of the plain windows up to its level, within one f32 ulp (2^-23 relative) per merge: list
    positions map back to the right pixels, and stopped pixels are left alone (no merge: the same bits)."""
    w, h = LOOP["w"], LOOP["h"]
    aov = cornell(w, h).render_aov()
    n0 = np.full((h, w), 4, np.uint32)
    ref = error_f64(window(w, h, 0, 4), window(w, h, 16, 4), n0, aov["albedo"], aov["normal"], aov["depth"])
    _, samples, halves = run_loop(float(np.float32(np.median(ref))))
    values = set(np.unique(samples).tolist())
    assert values <= {8, 16, 32} and len(values) > 1, values
    for half, start in zip(halves, (0, 16)):
        R = [window(w, h, start + s, m).astype(np.float64) for s, m in ((0, 4), (4, 4), (8, 8))]
        merged = [R[0], (R[0] + R[1]) / 2, (R[0] + R[1] + 2 * R[2]) / 4]
        for merges, want in enumerate(merged):
            at = samples == 8 << merges
            assert (np.abs(half[at] - want[at]) <= merges * 2.0 ** -23 * want[at]).all(), (start, merges)


@pytest.mark.parametrize("call,spp,kw", [("adaptive", 32, dict(rng="chacha8", precision="f64")),
                                         ("adaptive", 31, {}),
                                         ("adaptive", 32, dict(min_samples=2)),
                                         ("adaptive", 24, dict(min_samples=8)),
                                         ("adaptive", 32, dict(row_stride=2)),
                                         ("adaptive", 32, dict(gpus=1)),
                                         ("pixels", 4, dict(rng="chacha8", precision="f64")),
                                         ("pixels", 4, dict(row_stride=2)),
                                         ("pixels", 4, dict(gpus=1)),
                                         ("pixels", 4, dict(pixels=[3, 16]))])
def test_argument_errors_need_no_device(call, spp, kw):
    b = nrt.Builder()
    scene = b.finish(b.bvh([b.sphere((0, 0, -2), 1.0, b.lambertian(b.solid((1, 1, 1))))]))
    cam = nrt.CameraBuilder(width=4, height=4, samples_per_pixel=spp).build()
    with pytest.raises(nrt.NrtError) as ei:
        if call == "adaptive":
            scene.render_adaptive(cam, threshold=0.1, **kw)
        else:
            scene.render_pixels(kw.pop("pixels", [0]), cam, **kw)
    assert ei.value.code == -1, ei.value
