"""Shared test helpers: the oracle (test infrastructure) and scene fixtures."""
import contextlib
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = os.path.join(GOLDEN, "scenes")
ORACLE_BIN = os.path.join(ROOT, "oracle", "build", "oracle")
ORACLE_STATS_BIN = os.path.join(ROOT, "oracle", "build", "oracle_stats")


@contextlib.contextmanager
def in_golden():
    """Scene files reference `scenes/...` relative to the CWD, as in the reference."""
    old = os.getcwd()
    os.chdir(GOLDEN)
    try:
        yield
    finally:
        os.chdir(old)


def ensure_oracle():
    if not os.path.exists(ORACLE_BIN) or not os.path.exists(ORACLE_STATS_BIN):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return ORACLE_BIN


def is_legacy(scene):
    """Scene files in the legacy index schema (loaded with the explicit opt-in)."""
    return scene.endswith("triangles.toml")


def oracle_tree(scene, workdir, width=None, height=None, spp=None, bounces=None):
    """Independent Python loader -> oracle tree file (path)."""
    from oracle import scene_tree

    cli = scene_tree.CameraConfig(width=width, height=height, samples_per_pixel=spp, ray_max_bounces=bounces)
    with in_golden():
        text, cam = scene_tree.build_tree(scene, cli, workdir, legacy=is_legacy(scene))
    path = os.path.join(workdir, os.path.basename(scene) + ".tree")
    with open(path, "w") as fh:
        fh.write(text)
    return path, cam


def oracle_render(tree, threads=None, rows=(0, 1), stats=False, spp=None, var=False):
    """Run the oracle; returns (image, info) or (image, info, per-sample variance) with var=True."""
    ensure_oracle()
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "img.f32")
        st = os.path.join(td, "stats.json")
        vp = os.path.join(td, "var.f32")
        cmd = [ORACLE_STATS_BIN if stats else ORACLE_BIN, "render", tree, out, "--rows", str(rows[0]), str(rows[1]),
               "--stats", st]
        if var:
            cmd += ["--var", vp]
        if threads:
            cmd += ["--threads", str(threads)]
        if spp:
            cmd += ["--spp", str(spp)]
        subprocess.run(cmd, check=True, capture_output=True)
        import json
        img = np.fromfile(out, dtype="<f4")
        with open(st) as fh:
            info = json.load(fh)
        if var:
            return img, info, np.fromfile(vp, dtype="<f4")
        return img, info


def oracle_dump(tree):
    ensure_oracle()
    return subprocess.run([ORACLE_BIN, "dump", tree], check=True, capture_output=True, text=True).stdout


# ---- the synthetic frame of the two spatial denoiser tests (test_denoise.py, test_denoise_vg.py)
PATCH = (slice(5, 12), slice(24, 35))  # 7 x 11, across the tile seams y = 8 and x = 32


def synthetic(H, W, floor=False):
    """Two regions split by a slanted line (normals, depth ramps), a 3-row miss band, a 4-pixel
    checker albedo, colour = base * albedo * (1 + 0.5 gauss); float32, as the library takes them.
    floor: the albedo of PATCH is (0, 5e-4, 2e-3), exactly zero, below the filters' floor of 1e-3 and just
    above it, and its colour base * max(albedo, 1e-3) * (1 + 0.5 gauss): the demodulated colour stays O(1)."""
    rng = np.random.default_rng(1000 * H + W)
    ys, xs = np.mgrid[0:H, 0:W]
    left = xs < W * 0.45 + ys * 0.2
    N = np.where(left[..., None], [0, 0, 1.0], [0.6, 0, 0.8])
    Z = np.where(left, 2.0 + 0.01 * xs, 3.5 + 0.02 * ys)
    N[:3], Z[:3] = 0, 0
    A = np.where(((xs // 4 + ys // 4) % 2)[..., None] == 0, [0.8, 0.3, 0.2], [0.2, 0.7, 0.9])
    A[:3] = [0.1, 0.2, 0.3]
    if floor:
        A[PATCH] = [0.0, 5e-4, 2e-3]
    C = np.abs(np.where(left[..., None], 0.7, 0.25) * (np.maximum(A, 1e-3) if floor else A)
               * (1 + 0.5 * rng.standard_normal((H, W, 3))))
    return tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (C, A, N, Z))


def synthetic_cases(reference):
    """case(shape, K, floor=False, **sigmas) -> (frame, reference(*frame, K, **sigmas)): computed once per
    session, shared by the tests that need it, and read-only."""
    @functools.lru_cache(maxsize=None)
    def case(shape, K, floor=False, **sigmas):
        frame = synthetic(*shape, floor=floor)
        ref = reference(*frame, K, **sigmas)
        for x in (*frame, *(ref if isinstance(ref, tuple) else (ref,))):
            x.setflags(write=False)
        return frame, ref
    return case
