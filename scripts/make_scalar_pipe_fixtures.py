"""Frames of tests/test_scalar_pipe.py rendered by one library build, as fixtures (raw little-endian f32 and a
sha256 manifest).  Run it with the parent commit's library (scripts/build_prev.sh) on a GPU:

    NRT_LIB=nr-ray-tracer_amd/ab/prev/libnrt.so python scripts/make_scalar_pipe_fixtures.py OUT_DIR COMMIT

The frames are the scene-specialised kernel's; the script checks that the same library's generic kernel
(NRT_JIT=0) renders each of them bit for bit before it writes anything."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nr-ray-tracer_amd"), os.path.join(ROOT, "tests")]


def main():
    out, commit = sys.argv[1], sys.argv[2]
    import nrt
    import test_scalar_pipe as T

    def frames():
        f = {}
        for w, h, spp in T.BOOK_CASES:
            for name, frame in T.book_frames(w, h, spp).items():
                f[f"cornell_{w}x{h}_spp{spp}_{name}"] = frame
        for name in T.FOLD_SCENES:
            f[f"fold_{name}"] = T.fold_frame(name)
        return f

    os.environ["NRT_JIT"] = "require"
    special = frames()
    launched = nrt.jit_stats()["launches"]
    os.environ["NRT_JIT"] = "0"
    generic = frames()
    assert nrt.jit_stats()["launches"] == launched > 0
    os.makedirs(out, exist_ok=True)
    manifest = {"note": "f32 / Philox frames of tests/test_scalar_pipe.py as rendered by the library of the commit "
                        "below (its scene-specialised kernels; its generic kernels gave the same bits); "
                        "little-endian f32, rows x W x 3; made by scripts/make_scalar_pipe_fixtures.py",
                "commit": commit, "library_build_id": nrt.build_id(), "frames": {}}
    for name, frame in special.items():
        assert np.array_equal(frame.view(np.uint32), generic[name].view(np.uint32)), name
        assert np.isfinite(frame).all(), name  # (a one-sample window of 185 pixels may well be all black)
        raw = np.ascontiguousarray(frame, dtype="<f4").tobytes()
        with open(os.path.join(out, name + ".f32"), "wb") as fh:
            fh.write(raw)
        manifest["frames"][name] = {"file": name + ".f32", "shape": list(frame.shape),
                                    "sha256": hashlib.sha256(raw).hexdigest()}
    with open(os.path.join(out, "manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1)
        fh.write("\n")
    print(f"wrote {len(special)} frames, {sum(f.nbytes for f in special.values())} bytes, library {nrt.build_id()}")


if __name__ == "__main__":
    main()
