"""Measurements of DESIGN.md's "Sample windows and the dual-buffer variance" section, on one GPU:
quality (Cornell box 256^2, spp 4, f32 / Philox, RMSE against an spp-4096 render of each pose) of
denoise="dual" against denoise="variance" on the same samples and of eight live frames through a History
with sample_offset = 4 k (still camera; orbit of 0.4 degrees per frame about look_at), and timing at 1024^2
(HIP events around back-to-back device calls after 5 warm-ups, three rounds, the arms alternating): the
variance-guided chain with the moments kernel against the one with the dual kernel at K = 1 and 5, and two
spp-2 render launches against one spp-4 launch.

usage: python scripts/measure_dual.py [out.json]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-ray-tracer_amd"))
import numpy as np  # noqa: E402

import nrt  # noqa: E402

SCENE, KW = "scenes/cornell-box-scene.json", dict(precision="f32", rng="philox")


def load(size, spp, look_from=None):
    os.chdir(os.path.join(ROOT, "tests", "golden"))
    return nrt.Scene.load(SCENE, nrt.CameraConfig(width=size, height=size, samples_per_pixel=spp, look_from=look_from))


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def quality():
    s = load(256, 4)
    ref = s.render(s.camera.with_samples(4096), **KW)
    res = {"unfiltered": rmse(s.render(**KW), ref), "variance": rmse(s.render(denoise="variance", **KW), ref),
           "dual": rmse(s.render(denoise="dual", **KW), ref)}
    for name, step in (("still", 0.0), ("orbit", 0.4)):
        hist, rows = nrt.History(256, 256), []
        for k in range(8):
            t = math.radians(step * k)  # look_from turned about look_at = (0.5, 0.5, 0.5), axis y
            pose = load(256, 4, (0.5 - 2.125 * math.sin(t), 0.5, 0.5 - 2.125 * math.cos(t)))
            pref = ref if step == 0.0 else pose.render(pose.camera.with_samples(4096), **KW)
            rows.append({"frame": k + 1, "history": rmse(pose.render(denoise=hist, sample_offset=4 * k, **KW), pref),
                         "single": rmse(pose.render(denoise="variance", sample_offset=4 * k, **KW), pref),
                         "raw": rmse(pose.render(sample_offset=4 * k, **KW), pref)})
        res[name] = rows
    return res


def timing():
    import torch

    n, dev = 1024, "cuda:0"
    s = load(n, 4)
    half = s.camera.with_samples(2)
    aov = {k: torch.from_numpy(v).to(dev) for k, v in s.render_aov().items()}
    a, b = (torch.from_numpy(s.render(half, sample_offset=o, **KW)).to(dev) for o in (0, 2))
    out, var = torch.empty_like(a), torch.empty((n, n), dtype=torch.float32, device=dev)
    ptrs = (aov["albedo"].data_ptr(), aov["normal"].data_ptr(), aov["depth"].data_ptr(), n, n, out.data_ptr(), var.data_ptr())
    st = torch.cuda.current_stream(0).cuda_stream

    def timed(fn, calls):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize(0)
        return e0.elapsed_time(e1) * 1e3 / calls  # us per call

    arms = {}
    for K in (1, 5):
        arms[f"vg K={K}"] = (lambda K=K: s.denoise_vg_device(a.data_ptr(), *ptrs, iterations=K, device=0, stream=st), 200)
        arms[f"dual K={K}"] = (lambda K=K: s.denoise_vg_dual_device(a.data_ptr(), b.data_ptr(), *ptrs, iterations=K,
                                                                    device=0, stream=st), 200)
    arms["render spp 4"] = (lambda: s.render_device(out.data_ptr(), out.numel(), device=0, stream=st), 20)
    arms["render 2 x spp 2"] = (lambda: [s.render_device(out.data_ptr(), out.numel(), half, device=0, stream=st,
                                                         sample_offset=o) for o in (0, 2)], 20)
    res = {k: [] for k in arms}
    for _ in range(3):
        for k, (fn, calls) in arms.items():
            res[k].append(round(timed(fn, calls), 2))
    return res


if __name__ == "__main__":
    res = {"quality": quality(), "timing_us": timing()}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(os.path.join(ROOT, sys.argv[1]), "w") as fh:
            fh.write(text + "\n")
