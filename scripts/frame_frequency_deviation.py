#!/usr/bin/env python3
"""Deviations of one GPU run of the design loops with a natural-frequency floor (`frequency=`) from the CPU oracle
that truncates its subspace iteration identically (tests/golden/frame_frequency_reference.npz), as
tests/test_gpu_frame_frequency.py takes them, beside the caps that test applies (10 x TOL_LOSS_20 / TOL_I of the plain loop,
tests/test_gpu_frame_designs.py):

    python scripts/frame_frequency_deviation.py [--json PATH]        (default profiles/frame_frequency_deviation.json)

Per run (sum / max on the three designs, grouped on design (b)): per design the worst relative deviation of the design loss over the
first 20 epochs and the deviation of the final inertias over the design's largest, stop epochs and governing cases of both sides,
the term's last penalty beside the oracle's; and per run the worst over the designs whose term is on, (b) and (c)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from openpystruct_amd import _cabi
    from tests import test_gpu_frame_frequency as t
    args = sys.argv[1:]
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_frequency_deviation.json")
    _cabi.set_option("frame_latency_batch", 0)      # the tuned kernels for every batch, as the test's fixture sets it
    out = {"device": torch.cuda.get_device_name(0), "cap_loss_first20": t.CAP_LOSS_20, "cap_I_rel_to_max": t.CAP_I, "runs": {}}
    for tag in ("sum", "max", "grouped"):
        z, r, hist, term = t.run_frequency_loop(tag)
        dev = t.loop_deviation(z, tag, r, hist, term)
        dev["penalty"], dev["penalty_fixture_last_epoch"] = term.penalty.tolist(), z[f"{tag}_penalty"].tolist()
        dev["change_last"] = term.modes.change.tolist()
        on = [0] if tag == "grouped" else [1, 2]
        dev["worst"] = {"loss_first20": max(dev["loss_first20"][g] for g in on), "I_rel_to_max": max(dev["I_rel_to_max"][g] for g in on)}
        dev["worst"]["within_cap"] = dev["worst"]["loss_first20"] <= t.CAP_LOSS_20[tag] and dev["worst"]["I_rel_to_max"] <= t.CAP_I[tag]
        out["runs"][tag] = dev
        print(tag, dev, flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
