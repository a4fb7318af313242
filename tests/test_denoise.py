"""Feature buffers (nrt_render_aov) and the edge-avoiding a-trous filter (nrt_denoise): the filter
against its definition restated in numpy f64, the feature buffers against closed-form first hits,
and the plumbing from Scene.render(denoise=True) down to the device entry points.

Filter tolerance, max|out - ref| <= 5e-5 max|ref|: the f32 exponent argument carries ~1.7e-6
absolute error where the weight still matters (e <~ 20), i.e. ~1.2e-6 relative on a weight and
~4e-6 on a convex weighted mean per pass; passes do not amplify, five give ~2e-5; the bound is 2.5x
that.  The same formula in numpy f32 differs from f64 by 5.5e-7 on these inputs (6.5e-7 at 129 x 513 and
131 x 530).  Nothing in the derivation depends on the shape.

Shapes.  A pass of step s >= 2 runs on the s^2 lattices (x mod s, y mod s) in tiles of 32 x 8 lattice points:
129 x 513 = (8 16 + 1) x (32 16 + 1) gives lattice 0 one more tile than the others at every step (a tile seam
in both axes and the kernel's "tile past the end" return at steps 2 .. 16), 131 x 530 a partly filled last
tile in every lattice; 9 x 33 is a second image-space tile of one column, 6 x 9 a frame whose every pixel
lacks taps, 1 x 1 the centre tap alone."""
import math

import numpy as np
import pytest

import nrt
from helpers import PATCH, in_golden, synthetic_cases

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def atrous_f64(C, A, N, Z, K, sc=0.6, sn=0.3, sz=0.5):
    C, A, N, Z = (x.astype(np.float64) for x in (C, A, N, Z))
    H, W, _ = C.shape
    a = np.maximum(A, 1e-3)
    D = C / a
    for i in range(K):
        s, sci = 1 << i, sc * 2.0 ** -i
        num, den = np.zeros_like(D), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
                if y0 >= y1 or x0 >= x1:
                    continue  # every such tap lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                e = (((D[P] - D[Q]) ** 2).sum(-1) / sci ** 2 + ((N[P] - N[Q]) ** 2).sum(-1) / sn ** 2
                     + (Z[P] - Z[Q]) ** 2 / sz ** 2)
                w = H5[dy + 2] * H5[dx + 2] * np.exp(-e)
                num[P] += w[..., None] * D[Q]
                den[P] += w
        D = num / den[..., None]
    return D * a


case = synthetic_cases(atrous_f64)  # (frame, f64 reference), computed once per session and read-only


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("shape", [(29, 37), (45, 70), (129, 513), (131, 530), (1, 1), (6, 9), (9, 33)])
def test_filter_matches_f64_definition(shape, K):
    (C, A, N, Z), ref = case(shape, K)
    out = nrt.denoise(C, A, N, Z, iterations=K)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"a-trous {shape} K={K}: max|out - ref| = {err:.3e} = {err / scale:.3e} max|ref|")
    assert err <= 5e-5 * scale
    assert np.array_equal(nrt.denoise(C, A, N, Z, iterations=K), out)  # run to run
    inplace = C.copy()
    assert nrt.denoise(inplace, A, N, Z, iterations=K, out=inplace) is inplace
    assert np.array_equal(inplace, out)


@pytest.mark.gpu
def test_tile_split_knob_gives_the_same_bits(monkeypatch):
    """NRT_ATROUS_LATTICE = first step on lattice tiles; the steps below it take image-space tiles whose taps are
    T = step points apart: 8 runs atrous_kernel<2> at step 2 and <4> at step 4, 4 runs <2> at step 2, and 1, 2
    and unset no image-space tile past step 1.  Same taps in the same order per pixel: the same bits."""
    (C, A, N, Z), _ = case((129, 513), 5)
    monkeypatch.delenv("NRT_ATROUS_LATTICE", raising=False)
    want = nrt.denoise(C, A, N, Z, iterations=5)
    for v in ("1", "2", "4", "8"):
        monkeypatch.setenv("NRT_ATROUS_LATTICE", v)
        got = nrt.denoise(C, A, N, Z, iterations=5)
        print(f"a-trous (129, 513) K=5 NRT_ATROUS_LATTICE={v}: {(got != want).sum()} of {want.size} values differ "
              f"from the default split, max {np.abs(got - want).max():.3e}")
        assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("shape", [(29, 37), (129, 513)])
def test_albedo_floor(shape, K):
    """Albedo 0 and 5e-4 are floored to 1e-3 when demodulating and when remodulating alike, and 2e-3 is left alone:
    D_0 stays O(1) there, and the output is D_K a with a = max(albedo, 1e-3) (not 0, not D_K times the raw albedo,
    and no other floor).  The derivation's bound applies to D_K, so on every channel of the patch the error is within
    5e-5 max|D_K| a: 1e-3 and 2e-3 of the whole-frame bound."""
    (C, A, N, Z), ref = case(shape, K, floor=True)
    out = nrt.denoise(C, A, N, Z, iterations=K)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    a = np.maximum(A, 1e-3).astype(np.float64)
    dscale, perr = np.abs(ref / a).max(), (np.abs(out - ref) / a)[PATCH].max(axis=(0, 1))
    print(f"a-trous floor {shape} K={K}: max|out - ref| = {err:.3e} = {err / scale:.3e} max|ref|; patch channels "
          f"(albedo 0, 5e-4, 2e-3): " + ", ".join(f"{e / dscale:.3e}" for e in perr) + " of max(albedo, 1e-3) max|D_K|")
    assert np.isfinite(out).all()
    assert err <= 5e-5 * scale
    assert (A[PATCH] == np.float32([0.0, 5e-4, 2e-3])).all() and (ref[PATCH] > 0).all()
    assert (out[PATCH] > 0).all()
    assert (perr <= 5e-5 * dscale).all()


NON_DEFAULT = dict(sigma_color=0.25, sigma_normal=0.7, sigma_depth=1.3)
F64_NAMES = dict(sigma_color="sc", sigma_normal="sn", sigma_depth="sz")


@pytest.mark.gpu
def test_sigmas_are_honoured_and_nonpositive_selects_the_default():
    shape, K = (45, 70), 3
    (C, A, N, Z), ref0 = case(shape, K)
    _, ref = case(shape, K, **{F64_NAMES[k]: v for k, v in NON_DEFAULT.items()})
    tol = 5e-5 * np.abs(ref).max()
    assert np.abs(ref - ref0).max() > 100 * tol  # the case would not pass with the sigmas ignored,
    for k in NON_DEFAULT:  # nor with any one of them: a filter within tol of `one` is then 9 tol or more from ref
        _, one = case(shape, K, **{F64_NAMES[j]: v for j, v in NON_DEFAULT.items() if j != k})
        assert np.abs(ref - one).max() > 10 * tol
    out = nrt.denoise(C, A, N, Z, iterations=K, **NON_DEFAULT)
    err = np.abs(out - ref).max()
    print(f"a-trous {shape} K={K} {NON_DEFAULT}: max|out - ref| = {err:.3e} = {err / np.abs(ref).max():.3e} max|ref|")
    assert err <= tol
    want = nrt.denoise(C, A, N, Z, iterations=K)
    assert np.abs(want - ref0).max() <= 5e-5 * np.abs(ref0).max()
    for v in (0.0, -1.0):
        for k in NON_DEFAULT:
            assert np.array_equal(nrt.denoise(C, A, N, Z, iterations=K, **{k: v}), want)
        assert np.array_equal(nrt.denoise(C, A, N, Z, iterations=K, **dict.fromkeys(NON_DEFAULT, v)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("trace", ["world-list", "world-bvh", "bvh"])
def test_feature_buffers_match_closed_form(trace):
    W, H, lf, bg = 64, 48, np.array([0, 0, 3.0]), (0.2, 0.3, 0.5)
    sc, sr, scol = np.array([-0.35, 0.1, 0.0]), 0.8, (0.8, 0.4, 0.1)
    qp, qu, qv, qcol = np.array([-0.4, -1.0, -1.0]), np.array([2.2, 0, 0.5]), np.array([0, 1.9, 0.3]), (0.3, 0.6, 0.9)
    off = np.array([0.3, -0.2, 0.1])
    b = nrt.Builder()
    quad = b.translate(b.quad(qp - off, qu, qv, b.metal(0.1, b.solid(qcol))), off)
    scene = b.finish(b.bvh([b.sphere(sc, sr, b.lambertian(b.solid(scol))), quad]))
    cam = nrt.CameraBuilder(width=W, height=H, background_color=bg, look_from=tuple(lf), look_at=(0, 0, 0),
                            field_of_view=math.radians(50), samples_per_pixel=1).build()
    got = scene.render_aov(cam, trace=trace)
    # the primary rays of test_geometry_kat.py (focus distance 1, view up +y)
    vh = 2 * math.tan(math.radians(50) / 2)
    vu, vv = np.array([vh * W / H, 0, 0]), np.array([0, -vh, 0])
    du, dv = vu / W, vv / H
    tl = lf - np.array([0, 0, 1.0]) - vu / 2 - vv / 2 + (du + dv) / 2
    ys, xs = np.mgrid[0:H, 0:W]
    d = tl + xs[..., None] * du + ys[..., None] * dv - lf
    dlen = np.linalg.norm(d, axis=-1)
    oc, a = lf - sc, (d * d).sum(-1)
    hb = d @ oc
    disc = hb * hb - a * (oc @ oc - sr * sr)
    ts = (-hb - np.sqrt(np.maximum(disc, 0))) / a
    n = np.cross(qu, qv)
    nn, wq = n / np.linalg.norm(n), n / n.dot(n)
    tq = (nn @ qp - nn @ lf) / (d @ nn)
    p = lf + tq[..., None] * d - qp
    al, be = np.cross(p, qv) @ wq, np.cross(qu, p) @ wq
    sphere = disc > 0
    quad_hit = ~sphere & (tq > 0.001) & (al >= 0) & (al <= 1) & (be >= 0) & (be <= 1)
    edge = np.minimum.reduce([abs(al), abs(al - 1), abs(be), abs(be - 1)])
    keep = ~((np.abs(disc) / (a * sr * sr) < 1e-3) | (edge < 1e-3))
    assert (~keep).mean() <= 0.01 and sphere.sum() > 500 and quad_hit.sum() > 500
    albedo = np.where(sphere[..., None], scol, np.where(quad_hit[..., None], qcol, bg))
    ns = (lf + ts[..., None] * d - sc) / sr
    nq = -np.sign(d @ nn)[..., None] * nn
    normal = np.where(sphere[..., None], ns, np.where(quad_hit[..., None], nq, 0.0))
    depth = np.where(sphere, ts, np.where(quad_hit, tq, 0.0)) * dlen
    assert np.array_equal((got["depth"] > 0)[keep], (sphere | quad_hit)[keep])
    assert np.abs(got["albedo"] - albedo)[keep].max() <= 1e-6
    assert np.linalg.norm(got["normal"] - normal, axis=-1)[keep].max() <= 1e-4
    assert (np.abs(got["depth"] - depth) <= 1e-4 * depth)[keep].all()


@pytest.mark.gpu
def test_plumbing_render_denoise_shards_and_device_entry_points():
    torch = pytest.importorskip("torch")  # nrt.lib() already imported it first: one HIP runtime
    W = H = 48
    with in_golden():
        s = nrt.Scene.load("scenes/cornell-box-scene.json", nrt.CameraConfig(width=W, height=H, samples_per_pixel=4))
    frame = s.render(precision="f32", rng="philox")
    aov = s.render_aov()
    want = nrt.denoise(frame, **aov)
    assert np.array_equal(s.render(precision="f32", rng="philox", denoise=True), want)
    assert not np.array_equal(want, frame)
    shard = s.render_aov(row_offset=1, row_stride=2)
    for k in ("albedo", "normal", "depth"):
        assert np.array_equal(shard[k], aov[k][1::2])
    # the device entry points (scene-owned scratch), in place, twice: the host calls' bits
    dev = {k: torch.empty(v.shape, dtype=torch.float32, device="cuda:0") for k, v in aov.items()}
    st = torch.cuda.current_stream(0).cuda_stream
    s.render_aov_device(dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr(), W * H,
                        device=0, stream=st)
    for _ in range(2):
        col = torch.from_numpy(frame).to("cuda:0")
        s.denoise_device(col.data_ptr(), dev["albedo"].data_ptr(), dev["normal"].data_ptr(), dev["depth"].data_ptr(),
                         W, H, col.data_ptr(), device=0, stream=st)
        torch.cuda.synchronize(0)
        assert np.array_equal(col.cpu().numpy(), want)
    for k in aov:
        assert np.array_equal(dev[k].cpu().numpy(), aov[k])


@pytest.mark.gpu
def test_scene_scratch_grows_and_is_reused():
    """The scene owns one scratch per filter and device: 9 x 6, then 33 x 17 (it grows), then 9 x 6 again (it is kept),
    the two filters interleaved so that both slots live at once; every result is the host call's, bit for bit."""
    torch = pytest.importorskip("torch")  # nrt.lib() already imported it first: one HIP runtime
    b = nrt.Builder()
    scene = b.finish(b.bvh([b.sphere((0, 0, 0), 1.0, b.lambertian(b.solid((1, 1, 1))))]))
    st = torch.cuda.current_stream(0).cuda_stream
    for shape in ((6, 9), (17, 33), (6, 9)):
        frame, _ = case(shape, 5)
        C, A, N, Z = (torch.from_numpy(x.copy()).to("cuda:0") for x in frame)  # (the cases are read-only)
        var = np.empty(shape, np.float32)
        want, want_vg = nrt.denoise(*frame), nrt.denoise_vg(*frame, variance_out=var)
        out, dvar = torch.empty_like(C), torch.empty_like(Z)
        scene.denoise_device(C.data_ptr(), A.data_ptr(), N.data_ptr(), Z.data_ptr(), shape[1], shape[0], out.data_ptr(),
                             device=0, stream=st)
        torch.cuda.synchronize(0)
        assert np.array_equal(out.cpu().numpy(), want)
        scene.denoise_vg_device(C.data_ptr(), A.data_ptr(), N.data_ptr(), Z.data_ptr(), shape[1], shape[0],
                                out.data_ptr(), dvar.data_ptr(), device=0, stream=st)
        torch.cuda.synchronize(0)
        assert np.array_equal(out.cpu().numpy(), want_vg)
        assert np.array_equal(dvar.cpu().numpy(), var)


def test_argument_errors_and_missing_device():
    c = np.ones((4, 5, 3), np.float32)
    if nrt.device_count() == 0:
        with pytest.raises(nrt.NrtError) as ei:
            nrt.denoise(c, c, c, c[..., 0])
        assert ei.value.code == -3
    b = nrt.Builder()
    scene = b.finish(b.bvh([b.sphere((0, 0, 0), 1.0, b.lambertian(b.solid((1, 1, 1))))]))
    cam = nrt.CameraBuilder(width=4, height=4, samples_per_pixel=1).build()
    for bad in (lambda: nrt.denoise(c, c, c, c[..., 0], iterations=6),
                lambda: nrt.denoise(c, c, c[:3], c[..., 0]),
                lambda: nrt.denoise(c, c, c, c[:, :4, 0]),
                lambda: nrt.denoise(c, c, c, c[..., 0], out=np.empty(c.shape, np.float64)),
                lambda: nrt.denoise(c, c, c, c[..., 0], out=np.empty((4, 4, 3), np.float32)),
                lambda: scene.render_aov(cam, gpus=1)):
        with pytest.raises(nrt.NrtError) as ei:
            bad()
        assert ei.value.code == -1
        assert "denoise:" in str(ei.value) or "gpus must be 0" in str(ei.value)  # (the feature pass's own message)
