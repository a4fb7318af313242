"""The Philox loop's group bookkeeping behind its wave-uniform guard, the folded unit-test predicates of the
world list (kernel.hpp: NRT_BOOK_GUARD, NRT_DONES_SUM, NRT_CONTRIB_BITS, NRT_QUAD_HI_FOLD)
and the scalar-pipe table of scripts/asm_stats.py.

Each of those forms decides and rounds as the form it replaced, so every frame here must equal, bit for bit, the
generic kernel's (NRT_JIT=0), the same frame rendered another way (row shards, reassembled) and the frame the
parent commit's library rendered (tests/golden/scalar_pipe, made by scripts/make_scalar_pipe_fixtures.py; the
manifest names the commit).  The reference has no counterpart (its pixels are a rayon par_iter, camera.rs);
all renders f32 / Philox.

Shapes: 37 x 5 = 185 pixels is no multiple of a group's pixels, so the last group ends in padding samples;
with 64 x 64 both hold so few groups that every wave meets the queue running dry, a fetch, a flush and the
exit test within a few iterations.  48 x 48 at spp 4 for the unit tests' edges, ties and grazing rays."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nrt
from helpers import GOLDEN, ROOT, in_golden

CORNELL = "scenes/cornell-box-scene.json"
FIX = os.path.join(GOLDEN, "scalar_pipe")
BOOK_CASES = [(37, 5, 3), (37, 5, 8), (64, 64, 3), (64, 64, 8)]
WINDOWS = {3: (1, 2), 8: (4, 4)}  # spp -> (a, n): windows [0, a) and [a, a + n)
FOLD_SCENES = ["quads", "cube_model", "cube_scene", "tilted_quads"]
FOLD_W = FOLD_H = 48
FOLD_SPP = 4


def tilted_quads():
    """Five quads off the axes: one run of general quads (PRIM_QUAD, the `inside` test), one of them a light."""
    b = nrt.Builder()
    grey = b.lambertian(b.solid((0.6, 0.6, 0.6)))
    light = b.diffuse_light(3.0, b.solid((1.0, 0.9, 0.8)))
    quads = [b.quad((-2 + i, 0.1 * i, -1 - 0.3 * i), (1.5, 0.2, 0.1), (0.1, 1.5, 0.3), light if i == 2 else grey)
             for i in range(5)]
    return b.finish(b.bvh(quads))


def fold_scene(name):
    """(scene, camera) of a predicate-fold case."""
    files = {"quads": "scenes/quads.toml", "cube_model": "scenes/cube-model.toml", "cube_scene": "scenes/cube-scene.json"}
    if name in files:
        with in_golden():
            s = nrt.Scene.load(files[name], nrt.CameraConfig(width=FOLD_W, height=FOLD_H, samples_per_pixel=FOLD_SPP))
        return s, s.camera
    cam = nrt.CameraBuilder(width=FOLD_W, height=FOLD_H, look_from=(0.0, 1.2, 4.5), look_at=(0.0, 1.0, 0.0),
                            field_of_view=1.0, background_color=(0.5, 0.6, 0.8), samples_per_pixel=FOLD_SPP,
                            ray_max_bounces=12).build()
    return tilted_quads(), cam


def cornell(w, h, spp):
    with in_golden():
        return nrt.Scene.load(CORNELL, nrt.CameraConfig(width=w, height=h, samples_per_pixel=spp))


def book_frames(w, h, spp):
    """name -> frame of one bookkeeping case, with whatever kernel the environment selects."""
    s = cornell(w, h, spp)
    a, n = WINDOWS[spp]
    kw = dict(precision="f32", rng="philox")
    return {"full": s.render(**kw),
            "shard0": s.render(row_offset=0, row_stride=2, **kw), "shard1": s.render(row_offset=1, row_stride=2, **kw),
            "head": s.render(s.camera.with_samples(a), sample_offset=0, **kw),
            "tail": s.render(s.camera.with_samples(n), sample_offset=a, **kw)}


def fold_frame(name):
    s, cam = fold_scene(name)
    return s.render(cam, precision="f32", rng="philox")


def fixture(name, shape):
    with open(os.path.join(FIX, "manifest.json")) as fh:
        entry = json.load(fh)["frames"][name]
    raw = open(os.path.join(FIX, entry["file"]), "rb").read()
    assert hashlib.sha256(raw).hexdigest() == entry["sha256"], f"{name}: fixture file does not match its manifest"
    return np.frombuffer(raw, dtype="<f4").reshape(shape)


def same(got, want, what):
    assert got.shape == want.shape, what
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def with_kernel(monkeypatch, jit, fn):
    """fn() with the generic (jit False) or the scene-specialised kernel; the launch counts say which ran."""
    monkeypatch.setenv("NRT_JIT", "require" if jit else "0")
    before = nrt.jit_stats()
    out = fn()
    after = nrt.jit_stats()
    if jit:
        assert after["launches"] > before["launches"] and after["failed"] == before["failed"]
    else:
        assert after["launches"] == before["launches"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,spp", BOOK_CASES)
def test_bookkeeping_guard(monkeypatch, w, h, spp):
    generic = with_kernel(monkeypatch, False, lambda: book_frames(w, h, spp))
    special = with_kernel(monkeypatch, True, lambda: book_frames(w, h, spp))
    tag = f"cornell_{w}x{h}_spp{spp}"
    for frames, kernel in ((generic, "generic"), (special, "specialised")):
        full = frames["full"]
        assert full.shape == (h, w, 3) and np.isfinite(full).all() and full.max() > 0
        whole = np.empty_like(full)  # two row shards, stride 2, reassembled
        whole[0::2], whole[1::2] = frames["shard0"], frames["shard1"]
        same(whole, full, f"{tag} {kernel}: row shards against the unsharded frame")
        for name, frame in frames.items():
            same(frame, fixture(f"{tag}_{name}", frame.shape), f"{tag} {kernel} {name}: against the parent's frame")
            same(frame, generic[name], f"{tag} {kernel} {name}: against the generic kernel")
        # windows compose with the unsplit frame to test_sample_window.py's derived bound (one f32 rounding per
        # render on exact pixel sums): 2^-22 (a + n) max(R).  Not at spp 3: its head window is a launch of one
        # sample, which by the camera's rule (spp 1: no pixel jitter) is not sample 0 of a three-sample pixel
        a, n = WINDOWS[spp]
        if min(a, n) < 2:
            continue
        R = {k: v.astype(np.float64) for k, v in frames.items()}
        err = np.abs((a + n) * R["full"] - (a * R["head"] + n * R["tail"])).max()
        bound = 2.0 ** -22 * (a + n) * max(R["full"].max(), R["head"].max(), R["tail"].max())
        print(f"{tag} {kernel}: windows max|lhs - rhs| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", FOLD_SCENES)
def test_predicate_folds(monkeypatch, name):
    generic = with_kernel(monkeypatch, False, lambda: fold_frame(name))
    special = with_kernel(monkeypatch, True, lambda: fold_frame(name))
    assert generic.shape == (FOLD_H, FOLD_W, 3) and np.isfinite(generic).all() and generic.max() > 0
    same(special, generic, f"{name}: specialised against generic")
    same(special, fixture(f"fold_{name}", special.shape), f"{name}: against the parent's frame")


def test_asm_stats_scalar_families_add_up():
    """scripts/asm_stats.py --asm on a trimmed sample of the headline kernel's loop: every scalar-pipe
    instruction lands in exactly one family."""
    sample = os.path.join(FIX, "loop_sample.s")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "asm_stats.py"), "--asm", sample],
                         check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    head = next(l for l in lines if l.startswith("outer loop scalar pipe:"))
    fams = next(l for l in lines if l.strip().startswith("families:"))
    total = int(head.split(":")[1].split()[0])
    words = fams.split(":")[1].split()
    counts = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert set(counts) == {"exec", "branch", "smem", "wait", "cmp_select", "bitcount", "mask", "arith_move"}
    assert sum(counts.values()) == total
    # counted by hand in the sample (its scalar instructions, in the listed order of families)
    want = {l.split("=")[0].strip("; "): int(l.split("=")[1]) for l in open(sample) if l.startswith("; want ")}
    want = {k.replace("want ", ""): v for k, v in want.items()}
    assert counts == want, (counts, want)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import asm_stats

    text = open(sample).read()
    body, head_i, tail_i = asm_stats.outer_loop(text)
    insts = asm_stats.loop_instructions(body, head_i, tail_i)
    assert sum(asm_stats.scalar_families(insts).values()) == sum(1 for l in insts if l.startswith("s_")) == total
