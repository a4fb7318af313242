"""Measurements of DESIGN.md's "Adaptive sampling" section, on one GPU: Cornell box 512^2, f32 / Philox, cap 256 spp,
min_samples 32, over a few thresholds: the mean samples per pixel render_adaptive draws, its RMSE against a plain
render of 4096 spp over a disjoint window (sample_offset 2^20) beside the RMSE of plain renders at the powers of two
around the mean, and its wall time (host clock around the synchronous call, best of three after a warm-up) beside
plain renders at the nearest spp and at the cap.  Then the device time of the select, scan and scatter chain at
1024^2 (HIP events around 200 back-to-back calls after 5 warm-ups, three rounds).

usage: python scripts/adaptive_compare.py [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-ray-tracer_amd"))
import numpy as np  # noqa: E402

import nrt  # noqa: E402

SCENE, KW = "scenes/cornell-box-scene.json", dict(precision="f32", rng="philox")
CAP, MIN, THRESHOLDS = 256, 32, (2.0, 1.0, 0.5, 0.2, 0.05)


def load(size, spp):
    os.chdir(os.path.join(ROOT, "tests", "golden"))
    return nrt.Scene.load(SCENE, nrt.CameraConfig(width=size, height=size, samples_per_pixel=spp))


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def best_ms(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(min(times), 3)


def quality_and_wall():
    s = load(512, CAP)
    ref = s.render(s.camera.with_samples(4096), sample_offset=1 << 20, **KW)
    plain = {}
    for spp in (32, 64, 128, 256):
        cam = s.camera.with_samples(spp)
        plain[spp] = {"rmse": rmse(s.render(cam, **KW), ref), "wall_ms": best_ms(lambda: s.render(cam, **KW))}
    rows = []
    for t in THRESHOLDS:
        samples = np.zeros((512, 512), np.uint32)
        out = s.render_adaptive(threshold=t, min_samples=MIN, samples_out=samples)
        rows.append({"threshold": t, "mean_spp": float(samples.mean()), "rmse": rmse(out, ref),
                     "levels": {int(k): int(v) for k, v in zip(*np.unique(samples, return_counts=True))},
                     "wall_ms": best_ms(lambda: s.render_adaptive(threshold=t, min_samples=MIN))})
    return {"plain": plain, "adaptive": rows}


def select_chain_us():
    import torch

    n, dev = 1024, "cuda:0"
    s = load(n, 8)
    half = s.camera.with_samples(4)
    t = {k: torch.from_numpy(v).to(dev) for k, v in s.render_aov().items()}
    a, b = (torch.from_numpy(s.render(half, sample_offset=o, **KW)).to(dev) for o in (0, 4))
    halves = torch.full((n, n), 4, dtype=torch.int32, device=dev)
    pixels, count = torch.empty(n * n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(0).cuda_stream

    def call():
        s.adaptive_select_device(a.data_ptr(), b.data_ptr(), halves.data_ptr(), t["albedo"].data_ptr(),
                                 t["normal"].data_ptr(), t["depth"].data_ptr(), n, n, 4, 0.1, pixels.data_ptr(), n * n,
                                 count.data_ptr(), device=0, stream=st)

    rounds = []
    for _ in range(3):
        for _ in range(5):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            call()
        e1.record()
        torch.cuda.synchronize(0)
        rounds.append(round(e0.elapsed_time(e1) * 1e3 / 200, 2))
    return {"us_per_chain": rounds, "selected": int(count.item())}


if __name__ == "__main__":
    res = {"cornell_512": quality_and_wall(), "select_chain_1024": select_chain_us()}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(os.path.join(ROOT, sys.argv[1]), "w") as fh:
            fh.write(text + "\n")
