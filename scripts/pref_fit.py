"""Density of the reference's Lambertian scatter direction, and the f32 fit the kernels evaluate.

Lambertian::scatter sends the ray along n + q, q = p / |p|^2 with p uniform in the unit ball.  The density of
the direction w per solid angle depends on c = n.w alone (k = 1 - c^2, a = sqrt(k)):

    p_ref(c) = 3 / (4 pi) * (c^2 I4 + c / 2 + I2)
    I2 = (asin a - a |c| (1 - 2 k)) / (8 a^3)        = 1/3 - k/10 - k^2/56 - k^3/144 - ...
    I4 = (3 asin a - a |c| (2 k + 3)) / (8 a^5)      = 1/5 + k/14 + k^2/24 + 5 k^3/176 + ...

p_ref is analytic in |c| on each half of the range; the kernels evaluate one polynomial in c for c >= 0 and one
in 1 + c for c < 0 (Horner, f32; kernel.hpp p_ref): around c = -1, where the density is 31 times smaller than at
c = 1, the second has no cancellation.  This script fits both (Chebyshev nodes, double), prints the coefficients
for kernel.hpp, and measures the f32 evaluation against the closed form in double over the whole range:
python scripts/pref_fit.py [--check-draws]
"""
import argparse

import numpy as np

DEGREE = 12


def series(k, coef0, num):  # sum over n < num of coef0(n) k^n
    out = np.zeros_like(k)
    term = np.ones_like(k)
    for n in range(num):
        out += term * coef0(n)
        term = term * k
    return out


def i2(c):
    k = 1.0 - c * c
    a = np.sqrt(k)
    t = np.abs(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        closed = (np.arcsin(a) - a * t * (1.0 - 2.0 * k)) / (8.0 * a ** 3)
    # (1 - k r^2)^(1/2) = sum_n binom(1/2, n) (-k)^n r^(2n), integrated against r^2
    b = [1.0]
    for n in range(1, 40):
        b.append(b[-1] * (0.5 - (n - 1)) / n * -1.0)
    ser = series(k, lambda n: b[n] / (2 * n + 3), 40)
    return np.where(k < 0.05, ser, closed)


def i4(c):
    k = 1.0 - c * c
    a = np.sqrt(k)
    t = np.abs(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        closed = (3.0 * np.arcsin(a) - a * t * (2.0 * k + 3.0)) / (8.0 * a ** 5)
    b = [1.0]
    for n in range(1, 40):
        b.append(b[-1] * (-0.5 - (n - 1)) / n * -1.0)
    ser = series(k, lambda n: b[n] / (2 * n + 5), 40)
    return np.where(k < 0.05, ser, closed)


def p_ref(c):
    c = np.asarray(c, dtype=np.float64)
    return 3.0 / (4.0 * np.pi) * (c * c * i4(c) + 0.5 * c + i2(c))


def fit(f):  # polynomial in x on [0, 1] for f(x), weighted for relative error
    x = 0.5 * (np.cos(np.pi * (np.arange(200) + 0.5) / 200) + 1.0)  # Chebyshev nodes
    cheb = np.polynomial.chebyshev.Chebyshev.fit(x, f(x), DEGREE, domain=[0.0, 1.0], w=1.0 / f(x))
    return cheb.convert(kind=np.polynomial.Polynomial, domain=[0.0, 1.0], window=[0.0, 1.0]).coef


def horner_f32(coef, x):
    acc = np.full_like(x, np.float32(coef[-1]))
    for a in coef[-2::-1]:
        acc = acc * x + np.float32(a)
    return acc


def eval_f32(pos, neg, c):
    c = c.astype(np.float32)
    return np.where(c < 0, horner_f32(neg, np.float32(1.0) + c), horner_f32(pos, c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-draws", action="store_true", help="compare with 2e7 draws of n + u U^(-1/3)")
    a = ap.parse_args()
    pos, neg = fit(p_ref), fit(lambda x: p_ref(x - 1.0))
    for name, coef in (("c >= 0, in c", pos), ("c < 0, in 1 + c", neg)):
        print(f"coefficients for {name}, lowest first:")
        print(", ".join(f"{v:.9e}f" for v in coef))
    c = np.linspace(-1.0, 1.0, 2000001)
    want = p_ref(c)
    got = eval_f32(pos, neg, c).astype(np.float64)
    rel = np.abs(got / want - 1.0)
    print(f"p_ref(1) 40 pi / 31 = {p_ref(1.0) * 40 * np.pi / 31:.12f}, p_ref(-1) 40 pi = {p_ref(-1.0) * 40 * np.pi:.12f}")
    mu = np.linspace(-1.0, 1.0, 400001)
    print(f"integral over the sphere = {2 * np.pi * np.trapezoid(p_ref(mu), mu):.9f}")
    print(f"f32 fit against the closed form in double: max relative error {rel.max():.3e} at c = {c[rel.argmax()]:.6f}")
    if a.check_draws:
        rng = np.random.default_rng(1)
        n = 20_000_000
        z = rng.uniform(-1, 1, n)
        inv_r = rng.uniform(0, 1, n) ** (-1.0 / 3.0)
        s = np.sqrt(1 - z * z)
        ph = rng.uniform(0, 2 * np.pi, n)
        d = np.stack([inv_r * s * np.cos(ph), inv_r * s * np.sin(ph), 1.0 + inv_r * z])
        cc = d[2] / np.linalg.norm(d, axis=0)
        hist, edges = np.histogram(cc, bins=20, range=(-1, 1))
        for b in range(20):
            m = np.linspace(edges[b], edges[b + 1], 2001)
            print(f"  c in [{edges[b]:+.1f}, {edges[b + 1]:+.1f}): drawn {hist[b] / n:.5f}  density {2 * np.pi * np.trapezoid(p_ref(m), m):.5f}")


if __name__ == "__main__":
    main()
