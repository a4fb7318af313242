"""Measurements of DESIGN.md's "Direct light" section, on one GPU: Cornell box 512^2, f32 / Philox, plain renders at
spp 32 / 64 / 128 / 256 with and without direct_light: RMSE against a plain render of 4096 spp over a disjoint
window (sample_offset 2^20) and wall time (host clock around the synchronous call, best of three after a warm-up).
Then one adaptive row with direct_light (cap 256, min_samples 32, threshold 0.5) beside the same row without.

usage: python scripts/direct_compare.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-ray-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import nrt  # noqa: E402
from adaptive_compare import KW, best_ms, load, rmse  # noqa: E402

CAP, MIN, THRESHOLD = 256, 32, 0.5


def main():
    s = load(512, CAP)
    ref = s.render(s.camera.with_samples(4096), sample_offset=1 << 20, **KW)
    rows = []
    for spp in (32, 64, 128, 256):
        cam = s.camera.with_samples(spp)
        row = {"spp": spp}
        for name, direct in (("plain", False), ("direct", True)):
            row[name] = {"rmse": rmse(s.render(cam, direct_light=direct, **KW), ref),
                         "wall_ms": best_ms(lambda: s.render(cam, direct_light=direct, **KW))}
        rows.append(row)
    adaptive = {}
    for name, direct in (("plain", False), ("direct", True)):
        samples = np.zeros((512, 512), np.uint32)
        out = s.render_adaptive(threshold=THRESHOLD, min_samples=MIN, samples_out=samples, direct_light=direct)
        adaptive[name] = {"threshold": THRESHOLD, "mean_spp": float(samples.mean()), "rmse": rmse(out, ref),
                          "wall_ms": best_ms(lambda: s.render_adaptive(threshold=THRESHOLD, min_samples=MIN,
                                                                       direct_light=direct))}
    return {"cornell_512": {"renders": rows, "adaptive": adaptive}}


if __name__ == "__main__":
    text = json.dumps(main(), indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(os.path.join(ROOT, sys.argv[1]), "w") as fh:
            fh.write(text + "\n")
