"""Dual-buffer variance in front of the variance-guided passes (nrt_denoise_vg_dual): the filter against its
definition (include/nrt.h) restated in numpy f64, and the plumbing from Scene.render(denoise="dual") down to the
device entry point.  Tolerances: test_denoise_vg.py's, colour 5e-5 max|ref| and variance 5e-5 max Var_0 (Var_0 is a
convex mean of delta^2 under the same f32 exponent argument; the passes are that test's)."""
import functools

import numpy as np
import pytest

import nrt
from helpers import in_golden, synthetic
from test_denoise_vg import G3, H5, taps


def dual_f64(Ca, Cb, A, N, Z, K, sl=4.0, sn=0.3, sz=0.5):
    Ca, Cb, A, N, Z = (x.astype(np.float64) for x in (Ca, Cb, A, N, Z))
    H, W, _ = Ca.shape
    a = np.maximum(A, 1e-3)
    lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]  # noqa: E731
    g = lambda P, Q: ((N[P] - N[Q]) ** 2).sum(-1) / sn ** 2 + (Z[P] - Z[Q]) ** 2 / sz ** 2  # noqa: E731
    D, d2 = ((Ca + Cb) / 2) / a, (lum((Ca - Cb) / a) / 2) ** 2
    sw, s2 = np.zeros((H, W)), np.zeros((H, W))
    for dx, dy, P, Q in taps(H, W, 3, 1):
        w = np.exp(-g(P, Q))
        sw[P] += w
        s2[P] += w * d2[Q]
    var0 = var = s2 / sw
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


@functools.lru_cache(maxsize=None)
def case(shape, K):
    """((A, B, albedo, normal, depth), f64 reference): once per session, read-only."""
    Ca, A, N, Z = synthetic(*shape)
    eta = np.random.default_rng(7).standard_normal(Ca.shape)
    Cb = (Ca * np.clip(1 + 0.3 * eta, 0.05, None)).astype(np.float32)
    ref = dual_f64(Ca, Cb, A, N, Z, K)
    for x in (Ca, Cb, A, N, Z, *ref):
        x.setflags(write=False)
    return (Ca, Cb, A, N, Z), ref


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("shape", [(1, 1), (6, 9), (9, 33), (29, 37)])
def test_filter_matches_f64_definition(shape, K):
    """(6, 9): no pixel has all 49 taps; (9, 33): a second tile of one row and one column."""
    (Ca, Cb, A, N, Z), (ref, ref_var, var0) = case(shape, K)
    var = np.full(shape, np.nan, np.float32)
    out = nrt.denoise_vg_dual(Ca, Cb, A, N, Z, iterations=K, variance_out=var)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    verr, vscale = np.abs(var - ref_var).max(), var0.max()
    print(f"dual {shape} K={K}: max|out - ref| = {err:.3e} = {err / scale:.3e} max|ref|; "
          f"max|var - ref| = {verr:.3e} = {verr / vscale:.3e} max Var_0")
    assert vscale > 0
    assert err <= 5e-5 * scale
    assert verr <= 5e-5 * vscale
    assert np.array_equal(nrt.denoise_vg_dual(Ca, Cb, A, N, Z, iterations=K), out)  # run to run
    inplace = Ca.copy()
    assert nrt.denoise_vg_dual(inplace, Cb, A, N, Z, iterations=K, out=inplace) is inplace
    assert np.array_equal(inplace, out)
    nrt.denoise_vg_dual(Ca, Ca, A, N, Z, iterations=K, variance_out=var)  # equal halves: no noise measured
    assert (var == 0).all()


@pytest.mark.gpu
def test_plumbing_render_dual_and_device_entry_point():
    torch = pytest.importorskip("torch")  # nrt.lib() already imported it first: one HIP runtime
    W = H = 32
    with in_golden():
        s = nrt.Scene.load("scenes/cornell-box-scene.json", nrt.CameraConfig(width=W, height=H, samples_per_pixel=4))
    kw = dict(precision="f32", rng="philox")
    half = s.camera.with_samples(2)
    a, b = s.render(half, sample_offset=0, **kw), s.render(half, sample_offset=2, **kw)
    aov = s.render_aov()
    var = np.empty((H, W), np.float32)
    want = nrt.denoise_vg_dual(a, b, variance_out=var, **aov)
    got_var = np.full((H, W), np.nan, np.float32)
    assert np.array_equal(s.render(denoise="dual", variance_out=got_var, **kw), want)
    assert np.array_equal(got_var, var) and var.max() > 0
    assert not np.array_equal(want, s.render(denoise="variance", **kw))
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in aov.items()}
    db, dvar = torch.from_numpy(b).to("cuda:0"), torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream(0).cuda_stream
    for _ in range(2):  # scene-owned scratch, in place, twice: the host call's bits
        da = torch.from_numpy(a).to("cuda:0")
        s.denoise_vg_dual_device(da.data_ptr(), db.data_ptr(), dev["albedo"].data_ptr(), dev["normal"].data_ptr(),
                                 dev["depth"].data_ptr(), W, H, da.data_ptr(), dvar.data_ptr(), device=0, stream=st)
        torch.cuda.synchronize(0)
        assert np.array_equal(da.cpu().numpy(), want)
        assert np.array_equal(dvar.cpu().numpy(), var)
