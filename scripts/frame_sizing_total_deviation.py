#!/usr/bin/env python3
"""Records how far optimize_frames(gradient="total") on the GPU is from the project's CPU oracle of the loop
(tests/golden/frame_sizing_total_reference.npz): the figures tests/test_gpu_frame_sizing_total.py takes its tolerances from
(at most 5 x the recorded worst; profiles/frame_sizing_total_deviation.json).

    python scripts/frame_sizing_total_deviation.py OUT.json
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpystruct_amd import _cabi  # noqa: E402
from tests import test_gpu_frame_sizing_total as t  # noqa: E402


def main():
    _cabi.set_option("frame_latency_batch", 0)       # as the test's fixture
    runs, worst = {}, {}
    for tag in ("free", "limit"):
        for frame in t.FRAMES:
            z, I, ep, hist = t.run_loop(tag, frame, 1)
            dev = t.trajectory_deviation(z, tag, frame, I, ep, hist)
            runs[f"{tag}_{frame}"] = dev
            same = [d for d, a, b in zip(dev["I_rel_to_max"], dev["epochs"], dev["epochs_fixture"]) if a == b]
            w = worst.setdefault(tag, {"loss_first20": 0.0, "I_rel_to_max": 0.0, "frames_with_another_stop_epoch": 0})
            w["loss_first20"] = max(w["loss_first20"], dev["loss_first20"])
            w["I_rel_to_max"] = max([w["I_rel_to_max"]] + same)
            w["frames_with_another_stop_epoch"] += len(dev["epochs"]) - len(same)
    out = {"what": "optimize_frames(gradient=\"total\") on the GPU (poll_every = 1, loss_history) against tests/golden/frame_sizing_total_reference.npz, "
                   "the project's own CPU oracle of the loop (tests/frame_sizing_total_ref.py::loop_oracle_frames): 2 x 3 and 4 x 2 frames, "
                   "4 start designs each, two objectives.  One run; the kernels use no atomics beyond the solve's, so a run repeats bit for bit.",
           "fields": {"loss_first20": "worst relative deviation of the per-epoch loss over the first 20 epochs, all frames",
                      "I_rel_to_max": "|I - I_fixture| over the frame's largest inertia, final float32 I, per frame",
                      "epochs": "stop epochs, HIP loop / fixture"},
           "runs": runs, "worst": worst}
    print(json.dumps(out["worst"]))
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
