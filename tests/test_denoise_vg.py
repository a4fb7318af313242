"""Variance-guided a-trous filter (nrt_denoise_vg): the filter against its definition (include/nrt.h)
restated in numpy f64, the plumbing from Scene.render(denoise="variance") down to the device entry point,
and the argument errors.

Tolerances: colour max|out - ref| <= 5e-5 max|ref|, the bound of test_denoise.py (an f32 exponent argument
on a convex weighted mean, five passes); variance <= 5e-5 max Var_0 (a sum of w^2 Var / (sum w)^2 with
w <= sum w never exceeds max Var_0).  The same formulas in numpy f32 differ from f64 by 4.6e-7 and 1.9e-7
on these scales (7.5e-7 and 2.8e-7 at 129 x 513 and 131 x 530); nothing in the derivation depends on the shape.
Shapes: as test_denoise.py (tile seams and the "tile past the end" return at every lattice pitch, degenerate frames)."""
import numpy as np
import pytest

import nrt
from helpers import PATCH, in_golden, synthetic_cases

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)


def taps(H, W, r, s):
    """(dx, dy, P, Q) of the taps q = p + s (dx, dy), |dx|, |dy| <= r: P the pixels whose tap lies in the image."""
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
            if y0 < y1 and x0 < x1:
                yield dx, dy, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))


def vg_f64(C, A, N, Z, K, sl=4.0, sn=0.3, sz=0.5):
    C, A, N, Z = (x.astype(np.float64) for x in (C, A, N, Z))
    H, W, _ = C.shape
    a = np.maximum(A, 1e-3)
    D = C / a
    lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]  # noqa: E731
    g = lambda P, Q: ((N[P] - N[Q]) ** 2).sum(-1) / sn ** 2 + (Z[P] - Z[Q]) ** 2 / sz ** 2  # noqa: E731
    l, sw, s1, s2 = lum(D), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for dx, dy, P, Q in taps(H, W, 3, 1):
        w, d = np.exp(-g(P, Q)), l[Q] - l[P]
        sw[P] += w
        s1[P] += w * d
        s2[P] += w * d * d
    var0 = var = np.maximum(0.0, s2 / sw - (s1 / sw) ** 2)
    for i in range(K):
        num, den = np.zeros((H, W)), np.zeros((H, W))
        for dx, dy, P, Q in taps(H, W, 1, 1):
            num[P] += G3[dx + 1] * G3[dy + 1] * var[Q]
            den[P] += G3[dx + 1] * G3[dy + 1]
        sigma, l = np.sqrt(num / den), lum(D)
        nD, nv, sw = np.zeros_like(D), np.zeros((H, W)), np.zeros((H, W))
        for dx, dy, P, Q in taps(H, W, 2, 1 << i):
            w = H5[dx + 2] * H5[dy + 2] * np.exp(-(np.abs(l[P] - l[Q]) / (sl * sigma[P] + 1e-6) + g(P, Q)))
            nD[P] += w[..., None] * D[Q]
            nv[P] += w * w * var[Q]
            sw[P] += w
        D, var = nD / sw[..., None], nv / sw ** 2
    return D * a, var, var0


case = synthetic_cases(vg_f64)  # (frame, f64 reference), computed once per session and read-only


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("shape", [(6, 9), (29, 37), (45, 70), (129, 513), (131, 530), (1, 1), (9, 33)])
def test_filter_matches_f64_definition(shape, K):
    """Measured on an MI355X: see DESIGN.md (the variance-guided filter's accuracy item)."""
    (C, A, N, Z), (ref, ref_var, var0) = case(shape, K)
    var = np.full(shape, np.nan, np.float32)
    out = nrt.denoise_vg(C, A, N, Z, iterations=K, variance_out=var)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    verr, vscale = np.abs(var - ref_var).max(), var0.max()
    print(f"vg a-trous {shape} K={K}: max|out - ref| = {err:.3e} = {err / scale:.3e} max|ref|; "
          f"max|var - ref| = {verr:.3e} = {verr / (vscale or 1.0):.3e} max Var_0")
    assert err <= 5e-5 * scale
    assert verr <= 5e-5 * vscale
    if shape == (1, 1):  # one sample has no spread: the relative bound has no scale, the variance is exactly 0
        assert vscale == 0 and ref_var[0, 0] == 0 and var[0, 0] == 0
    assert np.array_equal(nrt.denoise_vg(C, A, N, Z, iterations=K), out)  # run to run, and without a variance buffer
    inplace = C.copy()
    assert nrt.denoise_vg(inplace, A, N, Z, iterations=K, out=inplace) is inplace
    assert np.array_equal(inplace, out)
    if K == 5 and shape == (45, 70):
        assert not np.array_equal(out, nrt.denoise(C, A, N, Z))  # not the fixed-sigma filter


@pytest.mark.gpu
def test_tile_split_knob_gives_the_same_bits(monkeypatch):
    """NRT_ATROUS_LATTICE = first step on lattice tiles; the steps below it take image-space tiles whose taps are
    T = step points apart: 8 runs vg_atrous_kernel<2> at step 2 and <4> at step 4, 4 runs <2> at step 2, and 1, 2
    and unset no image-space tile past step 1.  Same taps in the same order per pixel: the same bits."""
    (C, A, N, Z), _ = case((129, 513), 5)
    monkeypatch.delenv("NRT_ATROUS_LATTICE", raising=False)
    want_var = np.full((129, 513), np.nan, np.float32)
    want = nrt.denoise_vg(C, A, N, Z, iterations=5, variance_out=want_var)
    for v in ("1", "2", "4", "8"):
        monkeypatch.setenv("NRT_ATROUS_LATTICE", v)
        var = np.full((129, 513), np.nan, np.float32)
        got = nrt.denoise_vg(C, A, N, Z, iterations=5, variance_out=var)
        print(f"vg a-trous (129, 513) K=5 NRT_ATROUS_LATTICE={v}: {(got != want).sum()} of {want.size} colour values "
              f"and {(var != want_var).sum()} of {var.size} variances differ from the default split")
        assert np.array_equal(got, want)
        assert np.array_equal(var, want_var)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("shape", [(29, 37), (129, 513)])
def test_albedo_floor(shape, K):
    """Albedo 0 and 5e-4 are floored to 1e-3 in the staged luminance, in the records and when remodulating alike, and
    2e-3 is left alone: D_0 stays O(1) there (so max Var_0 stays the unpatched frame's, about 0.12, and the variance
    bound is no looser), and the output is D_K a with a = max(albedo, 1e-3) (not 0, not D_K times the raw albedo, and
    no other floor).  The derivation's bound applies to D_K, so on every channel of the patch the error is within
    5e-5 max|D_K| a: 1e-3 and 2e-3 of the whole-frame bound."""
    (C, A, N, Z), (ref, ref_var, var0) = case(shape, K, floor=True)
    var = np.full(shape, np.nan, np.float32)
    out = nrt.denoise_vg(C, A, N, Z, iterations=K, variance_out=var)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    verr, vscale = np.abs(var - ref_var).max(), var0.max()
    a = np.maximum(A, 1e-3).astype(np.float64)
    dscale, perr = np.abs(ref / a).max(), (np.abs(out - ref) / a)[PATCH].max(axis=(0, 1))
    print(f"vg a-trous floor {shape} K={K}: max|out - ref| = {err:.3e} = {err / scale:.3e} max|ref|; max|var - ref| = "
          f"{verr:.3e} = {verr / vscale:.3e} max Var_0 = {vscale:.3f}; patch channels (albedo 0, 5e-4, 2e-3): "
          + ", ".join(f"{e / dscale:.3e}" for e in perr) + " of max(albedo, 1e-3) max|D_K|")
    assert np.isfinite(out).all() and np.isfinite(var).all()
    assert vscale <= 1.25 * case(shape, K)[1][2].max()  # the patch does not loosen the variance bound
    assert err <= 5e-5 * scale
    assert verr <= 5e-5 * vscale
    assert (A[PATCH] == np.float32([0.0, 5e-4, 2e-3])).all() and (ref[PATCH] > 0).all()
    assert (out[PATCH] > 0).all()
    assert (perr <= 5e-5 * dscale).all()


NON_DEFAULT = dict(sigma_luminance=1.5, sigma_normal=0.7, sigma_depth=1.3)
F64_NAMES = dict(sigma_luminance="sl", sigma_normal="sn", sigma_depth="sz")


@pytest.mark.gpu
def test_sigmas_are_honoured_and_nonpositive_selects_the_default():
    shape, K = (45, 70), 3
    (C, A, N, Z), (ref0, _, _) = case(shape, K)
    _, (ref, ref_var, var0) = case(shape, K, **{F64_NAMES[k]: v for k, v in NON_DEFAULT.items()})
    tol, vtol = 5e-5 * np.abs(ref).max(), 5e-5 * var0.max()
    assert np.abs(ref - ref0).max() > 100 * tol  # the case would not pass with the sigmas ignored,
    for k in NON_DEFAULT:  # nor with any one of them: a filter within tol of `one` is then 9 tol or more from ref
        _, (one, _, _) = case(shape, K, **{F64_NAMES[j]: v for j, v in NON_DEFAULT.items() if j != k})
        assert np.abs(ref - one).max() > 10 * tol
    var = np.full(shape, np.nan, np.float32)
    out = nrt.denoise_vg(C, A, N, Z, iterations=K, variance_out=var, **NON_DEFAULT)
    err, verr = np.abs(out - ref).max(), np.abs(var - ref_var).max()
    print(f"vg a-trous {shape} K={K} {NON_DEFAULT}: max|out - ref| = {err:.3e} = {err / np.abs(ref).max():.3e} "
          f"max|ref|; max|var - ref| = {verr:.3e} = {verr / var0.max():.3e} max Var_0")
    assert err <= tol
    assert verr <= vtol
    want_var = np.full(shape, np.nan, np.float32)
    want = nrt.denoise_vg(C, A, N, Z, iterations=K, variance_out=want_var)
    assert np.abs(want - ref0).max() <= 5e-5 * np.abs(ref0).max()
    for v in (0.0, -1.0):
        for opts in [{k: v} for k in NON_DEFAULT] + [dict.fromkeys(NON_DEFAULT, v)]:
            assert np.array_equal(nrt.denoise_vg(C, A, N, Z, iterations=K, variance_out=var, **opts), want)
            assert np.array_equal(var, want_var)


@pytest.mark.gpu
def test_plumbing_render_variance_and_device_entry_point():
    torch = pytest.importorskip("torch")  # nrt.lib() already imported it first: one HIP runtime
    W = H = 48
    with in_golden():
        s = nrt.Scene.load("scenes/cornell-box-scene.json", nrt.CameraConfig(width=W, height=H, samples_per_pixel=4))
    frame = s.render(precision="f32", rng="philox")
    aov = s.render_aov()
    var = np.empty((H, W), np.float32)
    want = nrt.denoise_vg(frame, variance_out=var, **aov)
    assert np.array_equal(s.render(precision="f32", rng="philox", denoise="variance"), want)
    assert np.array_equal(s.render(precision="f32", rng="philox", denoise=True), nrt.denoise(frame, **aov))
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in aov.items()}
    dvar = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream(0).cuda_stream
    for _ in range(2):  # scene-owned scratch, in place, twice: the host call's bits
        col = torch.from_numpy(frame).to("cuda:0")
        s.denoise_vg_device(col.data_ptr(), dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr(),
                            W, H, col.data_ptr(), dvar.data_ptr(), device=0, stream=st)
        torch.cuda.synchronize(0)
        assert np.array_equal(col.cpu().numpy(), want)
        assert np.array_equal(dvar.cpu().numpy(), var)


def test_argument_errors_and_missing_device():
    c = np.ones((4, 5, 3), np.float32)
    if nrt.device_count() == 0:
        with pytest.raises(nrt.NrtError) as ei:
            nrt.denoise_vg(c, c, c, c[..., 0])
        assert ei.value.code == -3
    for bad in (lambda: nrt.denoise_vg(c, c, c, c[..., 0], iterations=6),
                lambda: nrt.denoise_vg(c, c, c[:3], c[..., 0]),
                lambda: nrt.denoise_vg(c, c, c, c[:, :4, 0]),
                lambda: nrt.denoise_vg(c, c, c, c[..., 0], variance_out=np.empty((4, 4), np.float32)),
                lambda: nrt.denoise_vg(c, c, c, c[..., 0], variance_out=np.empty((4, 5), np.float64)),
                lambda: nrt.denoise_vg(c, c, c, c[..., 0], out=np.empty(c.shape, np.float64)),
                lambda: nrt.denoise_vg(c, c, c, c[..., 0], out=np.empty((4, 4, 3), np.float32))):
        with pytest.raises(nrt.NrtError) as ei:
            bad()
        assert ei.value.code == -1
        # (the iteration bound is the library's check, shared with nrt_denoise, and carries its prefix)
        assert ("denoise:" if "iterations" in str(ei.value) else "denoise_vg:") in str(ei.value)
    b = nrt.Builder()
    scene = b.finish(b.bvh([b.sphere((0, 0, 0), 1.0, b.lambertian(b.solid((1, 1, 1))))]))
    with pytest.raises(ValueError):
        scene.render(nrt.CameraBuilder(width=4, height=4, samples_per_pixel=1).build(), denoise="bogus")
