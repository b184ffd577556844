#!/usr/bin/env python3
"""Deviations of one GPU run of `optimize_grouped_frame_designs` (story groups) from the CPU oracle of the grouped loop
(tests/golden/frame_groups_reference.npz), as tests/test_gpu_frame_groups.py::test_grouped_loop_against_the_cpu_oracle takes them,
beside the tolerances that test applies (TOL_LOSS_20 and TOL_I of the ungrouped loop, tests/test_gpu_frame_designs.py):

    python scripts/frame_groups_deviation.py [--json PATH]        (default profiles/frame_groups_deviation.json)

Per run (sum / weighted / max) and frame (2x3, 4x2): the worst relative deviation of the design loss over the first 20 epochs, per
design the deviation of the final inertias over the design's largest, stop epochs and governing cases of both sides; and per run
whether a deviation exceeds a fifth of its tolerance."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from openpystruct_amd import _cabi
    from tests import test_gpu_frame_groups as t
    args = sys.argv[1:]
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_groups_deviation.json")
    _cabi.set_option("frame_latency_batch", 0)      # the tuned kernels for every batch, as the test's fixture sets it
    out = {"device": torch.cuda.get_device_name(0), "tolerance_loss_first20": t.TOL_LOSS_20, "tolerance_I_rel_to_max": t.TOL_I, "runs": {}}
    for tag in t.TAGS:
        worst_loss, worst_I = 0.0, 0.0
        for frame in t.FRAMES:
            z, r, hist = t.run_group_loop(tag, frame, 10)
            dev = t.trajectory_deviation(z, tag, frame, r, hist)
            out["runs"][f"{tag}_{frame}"] = dev
            worst_loss = max(worst_loss, dev["loss_first20"])
            worst_I = max([worst_I] + [d for d, a, b in zip(dev["I_rel_to_max"], dev["epochs"], dev["epochs_fixture"]) if a == b])
        out["runs"][f"{tag}_worst"] = {"loss_first20": worst_loss, "I_rel_to_max": worst_I,
                                       "loss_over_a_fifth_of_tolerance": worst_loss > t.TOL_LOSS_20[tag] / 5,
                                       "I_over_a_fifth_of_tolerance": worst_I > t.TOL_I[tag] / 5}
        print(tag, out["runs"][f"{tag}_worst"], flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
