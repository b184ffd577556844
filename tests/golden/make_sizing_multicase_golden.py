"""Generates tests/golden/sizing_multicase_reference.npz: the project's own oracle of the multi-load-case sizing loop
(tests/sizing_multicase_ref.py::loop_oracle -- per design float32 I, torch.optim.Adam + ExponentialLR + clamp on the CPU, .grad the
float64 group gradient through the dense model).  It reads nothing of the reference.

Cases: `fixture_cases()` -- make_cases(9, SizingConfig(num_nodes=41, roller_nodes=(14, 27, 41), max_e=150), seed=20250307,
device="cpu") as G = 3 designs x C = 3 load cases, design-major.  Three runs:
  sum        L = sum I + sum_c P_c
  sum_defl   the same with alpha_deflection = 100, deflection_limit = DEFL_LIMIT per load case
  max        L = sum I + max_c P_c on cases whose load case 1 has its forces scaled by MAX_SCALE, so that one case governs clearly
Per run: every epoch's design loss [3, max_e] float32 (NaN past a design's last epoch), the final float32 I [3, 40], epochs [3],
the governing case of the last epoch [3].  The drawn loads and supports are stored too.

The generator asserts, on the oracle alone, that in the "max" run the largest penalty exceeds the second largest by at least 5 % at
every epoch of every design: a governing case that changed hands within float32 round-off would make the trajectory a coin toss.

Run:  python tests/golden/make_sizing_multicase_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import sizing  # noqa: E402
from tests import sizing_multicase_ref as mr  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402

G, C, SEED = 3, 3, 20250307
DEFL_ALPHA, DEFL_LIMIT = 100.0, 0.01
MAX_SCALE = 4.0
RUNS = {"sum": (mr.SUM, 0.0, 0.0), "sum_defl": (mr.SUM, DEFL_ALPHA, DEFL_LIMIT), "max": (mr.MAX, 0.0, 0.0)}


def fixture_config():
    return sizing.SizingConfig(num_nodes=41, roller_nodes=(14, 27, 41), max_e=150)


def fixture_cases(tag):
    """The 9 cases of the fixture as 3 designs x 3 load cases; for "max", load case 1 of every design scaled by MAX_SCALE."""
    cfg = fixture_config()
    cases = sizing.make_cases(G * C, cfg, seed=SEED, device="cpu")
    if tag == "max":
        scale = np.ones((G * C, 1))
        scale[1::C] = MAX_SCALE
        s = sizing.torch.as_tensor(scale)
        cases = sizing.Cases(cases.node_positions, cases.L, cases.roller_nodes_t, cases.n_rollers, cases.force_nodes_t, cases.n_forces,
                             cases.force_values_t * s, cases.fix, cases.Fy * s)
    return cfg, cases


def main():
    out = {"G": G, "C": C, "seed": SEED, "max_scale": MAX_SCALE}
    for tag, (aggregate, alpha, limit) in RUNS.items():
        cfg, cases = fixture_cases(tag)
        r = mr.loop_oracle(cases, cfg, tr.objective(alpha, limit), C, aggregate)
        last = [int(e) - 1 for e in r.epochs]
        print(tag, "epochs", r.epochs, "final loss", [float(r.loss[g, last[g]]) for g in range(G)], "governing", r.governing)
        print("   last penalties", [r.penalties[g, last[g]].tolist() for g in range(G)])
        if tag == "max":
            for g in range(G):
                P = np.sort(r.penalties[g, :r.epochs[g]].astype(np.float64), axis=1)
                margin = float((P[:, -1] / P[:, -2]).min())
                print(f"   design {g}: largest / second largest penalty, least over the epochs: {margin:.4f}")
                assert margin >= 1.05, (g, margin)
        out.update({f"{tag}_Fy": cases.Fy.numpy(), f"{tag}_fix": cases.fix.numpy(), f"{tag}_loss": r.loss, f"{tag}_I": r.I,
                    f"{tag}_epochs": r.epochs, f"{tag}_governing": r.governing, f"{tag}_objective": np.array([alpha, limit]),
                    f"{tag}_aggregate": aggregate})
    path = os.path.join(HERE, "sizing_multicase_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
