"""Temporal accumulation in front of the variance-guided filter (nrt.History, nrt_denoise_temporal): the
filter against its definition (include/nrt.h) restated in numpy f64 over analytic two-plane scenes, the
plumbing from Scene.render(denoise=<History>) down to the device entry point, and the argument errors.

Tolerances: colour max|out - ref| <= 5e-5 max|ref|, the bound of test_denoise_vg.py; variance <= 5e-5 max Var_0
and moments <= 5e-5 max m2 (every blend and pass is a convex mean of values these bound); the history length
exactly.  The reference marks as fragile every pixel where a decision of the definition sits within 1e-3
(relative) of its threshold: a tap's depth and normal tests, Cc > 0, sb >= 0.01, and u, v within 1e-3 of an
integer.  Equal cameras give u = x, v = y exactly on both sides (E = 0, t = 0 are exact zeros), so there the
last test has nothing to flip and is not applied.  Measured on an MI355X: DESIGN.md (temporal accumulation).

Cases A and B run 5 and 3 frames at the default options, where alpha = max(alpha_min, 1 / n) is 1 / n, n stays far
from its cap and the depth test decides nearly every tap the normal test would; the tests after them make the
clamp, the cap of 255, tau_n alone and non-default alpha_min, tau_z, tau_n decide, each after asserting on the
definition itself that the option changes the result."""
import dataclasses

import numpy as np
import pytest

import nrt
from helpers import in_golden

H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)
lum = lambda x: 0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]  # noqa: E731


def taps(H, W, r, s):
    """(dx, dy, P, Q) of the taps q = p + s (dx, dy), |dx|, |dy| <= r: P the pixels whose tap lies in the image."""
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
            if y0 < y1 and x0 < x1:
                yield dx, dy, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))


def cam_matrix(cam):
    return np.stack([cam.pixel_delta_u, cam.pixel_delta_v, np.subtract(cam.top_left, cam.look_from)], 1), np.array(cam.look_from)


def temporal_f64(st, cam, C, A, N, Z, K, sl=4.0, sn=0.3, sz=0.5, amin=0.2, tz=0.1, tn=0.9):
    """One frame of the definition.  st: the previous frame's state or None.  Returns out, Var_K, the new state
    (cam, N, Z, H, m1, m2, n), the fragile mask, the 4 taps' pixel indices (-1: outside) and max Var_0."""
    C, A, N, Z = (x.astype(np.float64) for x in (C, A, N, Z))
    H, W, _ = C.shape
    a = np.maximum(A, 1e-3)
    D = C / a
    g = lambda P, Q: ((N[P] - N[Q]) ** 2).sum(-1) / sn ** 2 + (Z[P] - Z[Q]) ** 2 / sz ** 2  # noqa: E731
    l, sw, s1, s2 = lum(D), np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    for dx, dy, P, Q in taps(H, W, 3, 1):
        w, d = np.exp(-g(P, Q)), l[Q] - l[P]
        sw[P] += w
        s1[P] += w * d
        s2[P] += w * d * d
    var0 = np.maximum(0.0, s2 / sw - (s1 / sw) ** 2)
    I, m1, m2, n = D.copy(), l.copy(), l * l, np.ones((H, W))
    frag, foot = np.zeros((H, W), bool), np.full((4, H, W), -1)
    if st is not None:
        (M, lf), (Mo, lfo) = cam_matrix(cam), cam_matrix(st["cam"])
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        xy1 = np.stack([xs, ys, np.ones((H, W))])
        d = np.einsum("ij,jhw->ihw", M, xy1)
        with np.errstate(divide="ignore", invalid="ignore"):
            k = Z / np.sqrt((d ** 2).sum(0))
            zr = np.sqrt((((lf - lfo)[:, None, None] + k * d) ** 2).sum(0))
            Minv = np.linalg.inv(Mo)
            e = np.einsum("ij,jhw->ihw", Minv @ (M - Mo), xy1) + (Minv @ (lf - lfo))[:, None, None] / k
            c = 1 + e[2]
            mu, mv = (e[0] - xs * e[2]) / c, (e[1] - ys * e[2]) / c
        ok = (Z > 0) & (c > 0) & np.isfinite(mu) & np.isfinite(mv)
        mu, mv, zr = np.where(ok, mu, 0), np.where(ok, mv, 0), np.where(ok, zr, 1)
        fu, fv = np.floor(mu), np.floor(mv)
        fx, fy = mu - fu, mv - fv
        near = lambda v, t: np.abs(v - t) <= 1e-3 * abs(t)  # noqa: E731
        frag |= (Z > 0) & (np.abs(c) <= 1e-3)
        if not np.array_equal(M, Mo) or not np.array_equal(lf, lfo):
            frag |= ok & ((np.minimum(fx, 1 - fx) < 1e-3) | (np.minimum(fy, 1 - fy) < 1e-3))
        sb, Hh, M1, M2, nmin = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W)), np.full((H, W), 255.0)
        for t, (i, j) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            qx, qy = (xs + fu).astype(int) + i, (ys + fv).astype(int) + j
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = np.where(inside, qx, 0), np.where(inside, qy, 0)
            foot[t] = np.where(inside, qy * W + qx, -1)
            Zq, dot = st["Z"][qy, qx], (st["N"][qy, qx] * N).sum(-1)
            hit = inside & (Zq > 0)
            frag |= hit & (near(np.abs(Zq - zr), tz * zr) | near(dot, tn))
            v = hit & (np.abs(Zq - zr) <= tz * zr) & (dot >= tn)
            b = np.where(v, (fx if i else 1 - fx) * (fy if j else 1 - fy), 0.0)
            sb += b
            Hh += b[..., None] * st["H"][qy, qx]
            M1 += b * st["m1"][qy, qx]
            M2 += b * st["m2"][qy, qx]
            nmin = np.where(v, np.minimum(nmin, st["n"][qy, qx]), nmin)
        frag |= ok & near(sb, 0.01)
        valid = ok & (sb >= 0.01)
        sbs = np.where(valid, sb, 1.0)
        n = np.where(valid, np.minimum(1 + nmin, 255), 1.0)
        al = np.maximum(amin, 1 / n)
        I = np.where(valid[..., None], Hh / sbs[..., None] + al[..., None] * (D - Hh / sbs[..., None]), D)
        m1 = np.where(valid, M1 / sbs + al * (l - M1 / sbs), l)
        m2 = np.where(valid, M2 / sbs + al * (l * l - M2 / sbs), l * l)
    var = np.where(n >= 4, np.maximum(0.0, m2 - m1 * m1), var0 / n)
    D = I
    for i in range(K):
        num, den = np.zeros((H, W)), np.zeros((H, W))
        for dx, dy, P, Q in taps(H, W, 1, 1):
            num[P] += G3[dx + 1] * G3[dy + 1] * var[Q]
            den[P] += G3[dx + 1] * G3[dy + 1]
        sigma, li = np.sqrt(num / den), lum(D)
        nD, nv, sw = np.zeros_like(D), np.zeros((H, W)), np.zeros((H, W))
        for dx, dy, P, Q in taps(H, W, 2, 1 << i):
            w = H5[dx + 2] * H5[dy + 2] * np.exp(-(np.abs(li[P] - li[Q]) / (sl * sigma[P] + 1e-6) + g(P, Q)))
            nD[P] += w[..., None] * D[Q]
            nv[P] += w * w * var[Q]
            sw[P] += w
        D, var = nD / sw[..., None], nv / sw ** 2
        hist = D if i == 0 else hist
    return D * a, var, dict(cam=cam, N=N, Z=Z, H=hist, m1=m1, m2=m2, n=n), frag, foot, var0.max()


def planes_frame(cam, planes, seed):
    """Feature buffers of the un-jittered primary rays over `planes`, a list of (point, unit normal, base colour,
    half extents or None, in-plane axes e1, e2): nearest hit wins, the normal faces the ray, depth is the distance
    from look_from (0 on a miss); a checker albedo of cell `4 pixels at distance 3` in plane coordinates;
    colour = base * albedo * (1 + 0.5 gauss).  float32."""
    M, lf = cam_matrix(cam)
    H, W = cam.height, cam.width
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.einsum("ij,jhw->hwi", M, np.stack([xs, ys, np.ones((H, W))]))
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    cell = 4 * 3 * np.linalg.norm(M[:, 0]) / np.linalg.norm(M[:, 2])
    Z, N, A, base = np.zeros((H, W)), np.zeros((H, W, 3)), np.tile([0.1, 0.2, 0.3], (H, W, 1)), np.zeros((H, W))
    for p0, nrm, b, ext, e1, e2 in planes:
        p0, nrm, e1, e2 = (np.array(v, float) for v in (p0, nrm, e1, e2))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((p0 - lf) @ nrm) / (dn @ nrm)
        hit = (t > 1e-3) & np.isfinite(t)
        a1, a2 = ((lf + t[..., None] * dn - p0) @ e1), ((lf + t[..., None] * dn - p0) @ e2)
        if ext is not None:
            hit &= (np.abs(a1) < ext[0]) & (np.abs(a2) < ext[1])
        hit &= (Z == 0) | (t < Z)
        Z = np.where(hit, t, Z)
        N = np.where(hit[..., None], -np.sign(dn @ nrm)[..., None] * nrm, N)
        chk = (np.floor(a1 / cell) + np.floor(a2 / cell)) % 2 == 0
        A = np.where(hit[..., None], np.where(chk[..., None], [0.8, 0.3, 0.2], [0.2, 0.7, 0.9]), A)
        base = np.where(hit, b, base)
    rng = np.random.default_rng(seed)
    C = np.abs(base[..., None] * A * (1 + 0.5 * rng.standard_normal((H, W, 3))))
    return tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (C, A, N, Z))


X, Y = (1, 0, 0), (0, 1, 0)
PLANES_A = [((0, 0, -3.5), (0, 0, 1), 0.7, None, X, Y), ((0.1, -0.05, -2), (0, 0, 1), 0.25, (0.9, 0.6), X, Y)]
PLANES_B = [((0, -1, 0), (0, 1, 0), 0.7, None, X, (0, 0, 1)),
            ((0.3, 0, -4.5), (0.287, 0.191, 0.939), 0.25, (1.6, 1.2), (0.956, 0, -0.292), (-0.056, 0.981, -0.183))]


def mk_cam(H, W, look_from, look_at, fov=1.0):
    return nrt.CameraBuilder(width=W, height=H, look_from=look_from, look_at=look_at, field_of_view=fov, samples_per_pixel=1).build()


def cameras_a(H, W):
    """Translations parallel to the image plane, in pixels of the background plane (depth 3.5; the foreground at
    depth 2 moves 1.75 times as far): every fractional shift of both planes lies in [0.2, 0.8]; last camera twice."""
    cams, pos = [mk_cam(H, W, (0, 0, 0), (0, 0, -1))], np.zeros(2)
    px = 3.5 * np.linalg.norm(cams[0].pixel_delta_u) / abs(cams[0].top_left[2])
    for sx, sy in ((1.5, 0.4), (-0.4, 1.5), (-1.5, -2.5)):
        pos = pos + np.array([sx, sy]) * px
        cams.append(mk_cam(H, W, (pos[0], pos[1], 0.0), (pos[0], pos[1], -1.0)))
    return cams + [cams[-1]]


def cameras_b(H, W):
    return [mk_cam(H, W, (0, 0.2, 1.0), (0, 0, -4)), mk_cam(H, W, (0.05, 0.2, 0.9), (0.22, 0, -4)),
            mk_cam(H, W, (0.1, 0.22, 0.8), (0.4, 0.02, -4), 0.96)]


def check_state(tag, hist, st, mask):
    (m, n), keep = hist.read(), ~mask
    merr = max(np.abs(m[..., 0] - st["m1"])[keep].max(), np.abs(m[..., 1] - st["m2"])[keep].max())
    print(f"{tag}: moments err {merr:.3e} = {merr / st['m2'].max():.3e} max m2; masked {mask.mean():.3%}")
    assert np.array_equal(n[keep], st["n"][keep])
    assert merr <= 5e-5 * st["m2"].max()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("shape", [(6, 9), (29, 37), (45, 70)])
def test_case_a_exact_by_construction(shape, K):
    cams = cameras_a(*shape)
    frames = [planes_frame(c, PLANES_A, 100 * shape[0] + i) for i, c in enumerate(cams)]
    hist, again, st, outs = nrt.History(shape[1], shape[0]), nrt.History(shape[1], shape[0]), None, []
    for i, (cam, (C, A, N, Z)) in enumerate(zip(cams, frames)):
        ref, ref_var, st, frag, _, v0 = temporal_f64(st, cam, C, A, N, Z, K)
        assert not frag.any()
        out = hist.denoise(C, A, N, Z, cam, iterations=K, variance_out=(var := np.empty(shape, np.float32)))
        err, verr = np.abs(out - ref).max(), np.abs(var - ref_var).max()
        print(f"temporal A {shape} K={K} frame {i}: colour err {err:.3e} = {err / np.abs(ref).max():.3e} max|ref|; "
              f"variance err {verr:.3e} = {verr / v0:.3e} max Var_0; n up to {st['n'].max():.0f}")
        assert err <= 5e-5 * np.abs(ref).max()
        assert verr <= 5e-5 * v0
        check_state(f"temporal A {shape} K={K} frame {i}", hist, st, frag)
        inplace = C.copy()  # run to run on a fresh history, in place, without a variance buffer
        assert again.denoise(inplace, A, N, Z, cam, iterations=K, out=inplace) is inplace
        assert np.array_equal(inplace, out)
        outs.append(out)
    assert st["n"].max() == 5 and st["n"].min() < 4 and hist.frames == 5
    hist.reset()
    assert np.array_equal(hist.denoise(*frames[0], cams[0], iterations=K), outs[0])
    C2 = planes_frame(cams[0], PLANES_A, 7)[0]  # a zero-motion second frame uses the history
    assert not np.array_equal(hist.denoise(C2, *frames[0][1:], cams[0], iterations=K),
                              nrt.denoise_vg(C2, *frames[0][1:], iterations=K))


@pytest.mark.gpu
def test_case_b_general_motion_temporal_state():
    shape, st, suspect = (45, 70), None, np.zeros((45, 70), bool)
    hist = nrt.History(shape[1], shape[0])
    for i, cam in enumerate(cameras_b(*shape)):
        C, A, N, Z = planes_frame(cam, PLANES_B, 500 + i)
        _, _, st, frag, foot, _ = temporal_f64(st, cam, C, A, N, Z, 2)
        suspect = frag | ((foot >= 0) & suspect.reshape(-1)[np.maximum(foot, 0)]).any(0)  # dilated through the gather
        hist.denoise(C, A, N, Z, cam, iterations=2)
        assert suspect.mean() <= 0.05
        check_state(f"temporal B frame {i}", hist, st, suspect)
    assert (st["n"] == 3).mean() >= 0.30


@pytest.mark.gpu
def test_long_zero_motion_history_alpha_min_clamp_and_length_cap():
    """258 frames of one camera: every pixel's single tap (weight 1) is valid, so n = min(i + 1, 255) at frame
    index i, alpha = max(0.2, 1 / n) is the clamp from index 5 on (1 / 6 < 0.2), and the cap of 255 binds from index
    254 on.  Every frame is compared; the blend is a contraction (alpha >= 0.2), so the f32 state's error does not
    grow with the sequence and the file's bounds apply to every frame."""
    shape, K, count = (6, 9), 2, 258
    cam = cameras_a(*shape)[0]
    frames = [planes_frame(cam, PLANES_A, 9000 + i) for i in range(count)]
    st = free = None
    for C, A, N, Z in frames[:8]:  # alpha = 1 / n alone is another filter by frame 7
        st, free = temporal_f64(st, cam, C, A, N, Z, K)[2], temporal_f64(free, cam, C, A, N, Z, K, amin=0.0)[2]
    assert np.abs(st["m1"] - free["m1"]).max() > 100 * 5e-5 * st["m2"].max()
    hist, st, worst = nrt.History(shape[1], shape[0]), None, np.zeros(3)
    for i, (C, A, N, Z) in enumerate(frames):
        ref, ref_var, st, frag, _, v0 = temporal_f64(st, cam, C, A, N, Z, K)
        assert not frag.any() and (st["n"] == min(i + 1, 255)).all()
        out = hist.denoise(C, A, N, Z, cam, iterations=K, variance_out=(var := np.full(shape, np.nan, np.float32)))
        (m, n), scale = hist.read(), np.abs(ref).max()
        err, verr = np.abs(out - ref).max(), np.abs(var - ref_var).max()
        merr = max(np.abs(m[..., 0] - st["m1"]).max(), np.abs(m[..., 1] - st["m2"]).max())
        worst = np.maximum(worst, [err / scale, verr / v0, merr / st["m2"].max()])
        if i in (5, 6, 7, 127, 128, 253, 254, 255, 257):
            print(f"temporal long {shape} K={K} frame {i}: n = {n.min():.0f} .. {n.max():.0f}; colour err "
                  f"{err / scale:.3e} max|ref|; variance err {verr / v0:.3e} max Var_0; moments err "
                  f"{merr / st['m2'].max():.3e} max m2")
        assert np.array_equal(n, st["n"]), f"frame {i}"
        assert err <= 5e-5 * scale and verr <= 5e-5 * v0 and merr <= 5e-5 * st["m2"].max(), f"frame {i}"
    print(f"temporal long {shape} K={K}: worst of {count} frames: colour {worst[0]:.3e}, variance {worst[1]:.3e}, "
          f"moments {worst[2]:.3e}")
    assert st["n"].min() == 255 and hist.frames == count


@pytest.mark.gpu
def test_case_b_non_default_alpha_min_and_tau_z():
    """Case B's three cameras with alpha_min = 0.6 (it binds at n = 2 and 3) and tau_z = 0.02 (the slanted plane's
    depth changes by more than 2 % between neighbouring taps where the default's 10 % accepts them)."""
    shape, opts, refs = (45, 70), dict(amin=0.6, tz=0.02), []
    st = dflt = lazy = None
    suspect = np.zeros(shape, bool)
    for i, cam in enumerate(cameras_b(*shape)):
        frame = planes_frame(cam, PLANES_B, 500 + i)
        dflt, lazy = temporal_f64(dflt, cam, *frame, 2)[2], temporal_f64(lazy, cam, *frame, 2, tz=0.02)[2]
        _, _, st, frag, foot, _ = temporal_f64(st, cam, *frame, 2, **opts)
        suspect = frag | ((foot >= 0) & suspect.reshape(-1)[np.maximum(foot, 0)]).any(0)  # dilated through the gather
        assert suspect.mean() <= 0.05
        refs.append((cam, frame, st, suspect))
    differ = (st["n"] != dflt["n"])[~suspect].mean()
    mdiff = np.abs(st["m1"] - lazy["m1"])[~suspect].max()
    print(f"temporal B {opts}: suspect {suspect.mean():.3%}; n differs from the default thresholds' on {differ:.1%} of "
          f"the rest; m1 differs from alpha_min 0.2's by {mdiff / st['m2'].max():.3e} max m2")
    assert differ >= 0.10                          # tau_z matters,
    assert mdiff > 100 * 5e-5 * st["m2"].max()     # and so does alpha_min
    hist = nrt.History(shape[1], shape[0])
    for i, (cam, frame, st, suspect) in enumerate(refs):
        hist.denoise(*frame, cam, iterations=2, alpha_min=0.6, tau_z=0.02)
        check_state(f"temporal B {opts} frame {i}", hist, st, suspect)


@pytest.mark.gpu
def test_normal_and_depth_thresholds_each_decide_taps():
    """Equal cameras: one tap of weight 1 per pixel, the pixel itself.  The second frame has the first one's
    feature buffers but for two rectangles: in one the normals are turned so that N' . N = 0.95, in the other the
    depth is 1.05 times the first frame's (|Z' - z'| / z' = 0.0476).  With (tau_n, tau_z) = (0.9, 0.1) every tap
    passes both tests; with (0.97, 0.02) the normal test alone rejects the first rectangle's taps and the depth test
    alone the second's.  All of 0.95, 1 and 0.0476, 0 are far from the four thresholds: no fragile pixel."""
    shape, K = (45, 70), 2
    cam = cameras_a(*shape)[0]
    C0, A, N0, Z0 = planes_frame(cam, PLANES_A, 4500)
    C1 = planes_frame(cam, PLANES_A, 4501)[0]
    assert (N0 == [0, 0, 1]).all() and (Z0 > 0).all()
    turned, scaled = (slice(10, 20), slice(8, 30)), (slice(25, 40), slice(40, 65))
    N1, Z1, rejected = N0.copy(), Z0.copy(), np.zeros(shape, bool)
    N1[turned] = [np.sqrt(1 - 0.95 ** 2), 0, 0.95]
    Z1[scaled] *= np.float32(1.05)
    rejected[turned] = rejected[scaled] = True
    for (tn, tz), want_n in (((0.9, 0.1), np.full(shape, 2.0)), ((0.97, 0.02), np.where(rejected, 1.0, 2.0))):
        _, _, st, frag0, _, _ = temporal_f64(None, cam, C0, A, N0, Z0, K, tn=tn, tz=tz)
        ref, ref_var, st, frag, _, v0 = temporal_f64(st, cam, C1, A, N1, Z1, K, tn=tn, tz=tz)
        assert not frag0.any() and not frag.any()
        assert np.array_equal(st["n"], want_n)
        hist = nrt.History(shape[1], shape[0])
        hist.denoise(C0, A, N0, Z0, cam, iterations=K, tau_n=tn, tau_z=tz)
        var = np.full(shape, np.nan, np.float32)
        out = hist.denoise(C1, A, N1, Z1, cam, iterations=K, variance_out=var, tau_n=tn, tau_z=tz)
        err, verr = np.abs(out - ref).max(), np.abs(var - ref_var).max()
        print(f"temporal thresholds tau_n={tn} tau_z={tz}: colour err {err:.3e} = {err / np.abs(ref).max():.3e} "
              f"max|ref|; variance err {verr:.3e} = {verr / v0:.3e} max Var_0; n = 1 on {(st['n'] == 1).sum()} pixels")
        check_state(f"temporal thresholds tau_n={tn} tau_z={tz}", hist, st, frag)
        assert err <= 5e-5 * np.abs(ref).max()
        assert verr <= 5e-5 * v0


def run(seq, K, **opts):
    """The sequence [(camera, frame), ...] on a fresh history: the last frame's out, variance, moments, n."""
    shape = seq[0][1][3].shape
    hist = nrt.History(shape[1], shape[0])
    for cam, frame in seq:
        var = np.full(shape, np.nan, np.float32)
        out = hist.denoise(*frame, cam, iterations=K, variance_out=var, **opts)
    return (out, var, *hist.read())


def definition(seq, K, **opts):
    """The same sequence through the definition: the last frame's out and state."""
    st = None
    with np.errstate(all="ignore"):  # (a literal sigma of -1 may overflow)
        for cam, frame in seq:
            out, _, st, _, _, _ = temporal_f64(st, cam, *frame, K, **opts)
    return out, st


def seq_a(count):
    """The first `count` frames of case A at 45 x 70 (the camera moves)."""
    return [(cam, planes_frame(cam, PLANES_A, 4500 + i)) for i, cam in enumerate(cameras_a(45, 70)[:count])]


@pytest.mark.gpu
def test_nonpositive_option_selects_the_default():
    """An option of 0 or -1 gives the default call's bits, on a sequence where the literal value would not: each
    option has a sequence on which the definition, given the literal 0 or -1, differs from the definition at the
    default, which is asserted first.
      alpha_min: 8 frames of one 6 x 9 camera, n = 8: alpha = max(0.2, 1 / 8) is the clamp, max(0, 1 / 8) is not.
      tau_n: equal cameras at 45 x 70, the first frame's normals turned to N' . N = 0.5 in a rectangle: 0.9 rejects
        those taps (n = 1), 0 and -1 accept them (n = 2).
      tau_z: two frames of case A: 0 accepts only an exactly equal depth, -1 nothing.
      sigmas: the same two frames, and for sigma_normal the turned-normal pair (case A's normals are all equal); -1 is
        another filter (or none: the luminance weight overflows); a literal 0 divides by zero on both sides, so
        only the bits are compared for it."""
    K = 2
    cam6 = cameras_a(6, 9)[0]
    clamp = [(cam6, planes_frame(cam6, PLANES_A, 9000 + i)) for i in range(8)]
    cam = cameras_a(45, 70)[0]
    C0, A, N0, Z0 = planes_frame(cam, PLANES_A, 4500)
    turned, Nt = (slice(10, 20), slice(8, 30)), N0.copy()
    Nt[turned] = [np.sqrt(1 - 0.5 ** 2), 0, 0.5]
    normals = [(cam, (C0, A, Nt, Z0)), (cam, (planes_frame(cam, PLANES_A, 4501)[0], A, N0, Z0))]
    moving = seq_a(2)
    f64 = dict(alpha_min="amin", tau_z="tz", tau_n="tn", sigma_luminance="sl", sigma_normal="sn", sigma_depth="sz")
    for seq, names in ((clamp, ["alpha_min"]), (normals, ["tau_n", "sigma_normal"]),
                       (moving, ["tau_z", "sigma_luminance", "sigma_depth"])):
        ref, st = definition(seq, K)
        tol = 5e-5 * st["m2"].max()
        want = run(seq, K)
        assert np.array_equal(want[3], st["n"])  # the default call is the definition's at the default
        for k in names:
            for v in (0.0, -1.0):
                if not (k.startswith("sigma") and v == 0.0):
                    lit, lst = definition(seq, K, **{f64[k]: v})
                    if k in ("tau_n", "tau_z"):
                        assert (lst["n"] != st["n"]).mean() >= 0.05, (k, v)
                    elif k == "alpha_min":
                        assert np.abs(lst["m1"] - st["m1"]).max() > 100 * tol, (k, v)
                    else:
                        assert not np.abs(lit - ref).max() <= 100 * 5e-5 * np.abs(ref).max(), (k, v)
                for a, b in zip(run(seq, K, **{k: v}), want):
                    assert np.array_equal(a, b), (k, v)


@pytest.mark.gpu
def test_tile_split_knob_gives_the_same_bits(monkeypatch):
    """The temporal chain's passes are the variance-guided filter's (test_denoise_vg.py has the knob's meaning): with
    NRT_ATROUS_LATTICE=8 the steps 2 and 4 of K = 5 take image-space tiles, and the bits are the default's."""
    monkeypatch.delenv("NRT_ATROUS_LATTICE", raising=False)
    want = run(seq_a(2), 5)
    monkeypatch.setenv("NRT_ATROUS_LATTICE", "8")
    for a, b in zip(run(seq_a(2), 5), want):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_plumbing_render_history_and_device_entry_point():
    torch = pytest.importorskip("torch")  # nrt.lib() already imported it first: one HIP runtime
    W = H = 48
    with in_golden():
        s = nrt.Scene.load("scenes/cornell-box-scene.json", nrt.CameraConfig(width=W, height=H, samples_per_pixel=4))
    shift = 0.8 * np.array(s.camera.pixel_delta_u)
    cams = [s.camera, dataclasses.replace(s.camera, look_from=tuple(np.array(s.camera.look_from) + shift),
                                          top_left=tuple(np.array(s.camera.top_left) + shift))]
    hist, hand, dev_hist = nrt.History(W, H), nrt.History(W, H), nrt.History(W, H, device=0)
    st = torch.cuda.current_stream(0).cuda_stream
    dvar, want = torch.empty((H, W), dtype=torch.float32, device="cuda:0"), []
    for cam in cams:
        frame, aov, var = s.render(cam, precision="f32", rng="philox"), s.render_aov(cam), np.empty((H, W), np.float32)
        want.append((frame, aov, hand.denoise(frame, camera=cam, variance_out=var, **aov), var))
        assert np.array_equal(s.render(cam, precision="f32", rng="philox", denoise=hist), want[-1][2])
    assert not np.array_equal(want[1][2], nrt.denoise_vg(want[1][0], **want[1][1]))
    for _ in range(2):  # history-owned buffers, in place, twice: the host call's bits
        dev_hist.reset()
        for cam, (frame, aov, out, var) in zip(cams, want):
            col = torch.from_numpy(frame).to("cuda:0")
            d = {k: torch.from_numpy(v).to("cuda:0") for k, v in aov.items()}
            dev_hist.denoise_device(col.data_ptr(), d["albedo"].data_ptr(), d["normal"].data_ptr(), d["depth"].data_ptr(),
                                    cam, col.data_ptr(), dvar.data_ptr(), stream=st)
            torch.cuda.synchronize(0)
            assert np.array_equal(col.cpu().numpy(), out)
            assert np.array_equal(dvar.cpu().numpy(), var)


@pytest.mark.gpu
def test_denoisers_on_second_device_keep_current_device():
    """The three host entry points run on the device asked for and leave the caller's current device unchanged (device
    guard, hip_util.hpp), as test_render_on_second_device_keeps_current_device has it for the renderer; also after a
    call that fails behind the device switch (a singular camera is rejected before it: the history's staging is
    allocated on its device first)."""
    n = nrt.device_count()
    if n < 2:
        pytest.skip(f"{n} GPU visible: needs two devices")
    torch = pytest.importorskip("torch")
    shape = (6, 9)
    cams = cameras_a(*shape)[:2]
    frames = [planes_frame(c, PLANES_A, 600 + i) for i, c in enumerate(cams)]
    torch.cuda.set_device(0)
    want = nrt.denoise(*frames[0], device=0)
    assert np.array_equal(nrt.denoise(*frames[0], device=1), want)
    assert torch.cuda.current_device() == 0
    want = nrt.denoise_vg(*frames[0], device=0)
    assert np.array_equal(nrt.denoise_vg(*frames[0], device=1), want)
    assert torch.cuda.current_device() == 0
    h0, h1 = nrt.History(shape[1], shape[0], device=0), nrt.History(shape[1], shape[0], device=1)
    for cam, frame in zip(cams, frames):
        want = h0.denoise(*frame, cam)
        assert np.array_equal(h1.denoise(*frame, cam), want)
        assert torch.cuda.current_device() == 0
    flat = dataclasses.replace(cams[0], pixel_delta_v=cams[0].pixel_delta_u)  # du = dv: a singular camera
    with pytest.raises(nrt.NrtError):
        nrt.History(shape[1], shape[0], device=1).denoise(*frames[0], flat)
    assert torch.cuda.current_device() == 0


def test_argument_errors_and_missing_device():
    c = np.ones((4, 5, 3), np.float32)
    cam = nrt.CameraBuilder(width=5, height=4, samples_per_pixel=1).build()
    hist = nrt.History(5, 4)
    if nrt.device_count() == 0:
        with pytest.raises(nrt.NrtError) as ei:
            hist.denoise(c, c, c, c[..., 0], cam)
        assert ei.value.code == -3
    for bad in (lambda: hist.denoise(c, c, c, c[..., 0], cam, iterations=1),
                lambda: hist.denoise(c, c, c, c[..., 0], cam, iterations=6),
                lambda: hist.denoise(c, c, c, c[..., 0], nrt.CameraBuilder(width=4, height=4, samples_per_pixel=1).build()),
                lambda: hist.denoise(c, c, c, c[..., 0], cam, variance_out=np.empty((4, 4), np.float32)),
                lambda: hist.denoise(c, c, c, c[..., 0], cam, variance_out=np.empty((4, 5), np.float64)),
                lambda: hist.denoise(c, c, c, c[..., 0], cam, out=np.empty(c.shape, np.float64)),
                lambda: hist.denoise(c, c, c, c[..., 0], cam, out=np.empty((4, 4, 3), np.float32)),
                lambda: hist.denoise(c[:3], c[:3], c[:3], c[:3, :, 0], cam)):
        with pytest.raises(nrt.NrtError) as ei:
            bad()
        assert ei.value.code == -1
        # (the library's own checks carry the C entry point's prefix, or nrt_denoise's for the shared upper bound)
        msg = str(ei.value)
        assert ("History.denoise:" in msg or "denoise_temporal:" in msg or "denoise: iterations" in msg), msg
