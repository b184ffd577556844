"""Generates tests/golden/sizing_total_reference.npz: the project's own oracle of the exact-gradient ("total") sizing loop
(tests/sizing_total_ref.py::loop_oracle -- float32 I, torch.optim.Adam + ExponentialLR + clamp on the CPU, .grad from autograd
of the float64 objective through the dense model).  It reads nothing of the reference.

Cases: make_cases(4, SizingConfig(), seed=20250307, device="cpu") (the fixed bridge, 100 elements).  Two objectives:
  free   no deflection term
  defl   alpha_deflection = 100, deflection_limit = 0.01
Per objective: every epoch's loss [4, max_e] float32 (NaN past a case's last epoch), the final float32 I [4, 100], epochs_run [4],
max |v| of each case's last solve [4].  The drawn loads and supports are stored too, so a test can tell a different case draw
from a different trajectory.

The generator asserts what the constrained design has to show: the oracle's worst max|v| / v_lim stays below 1.05.

Run:  python tests/golden/make_sizing_total_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import sizing  # noqa: E402
from tests import sizing_total_ref as tr  # noqa: E402

N_CASES, SEED = 4, 20250307
OBJECTIVES = {"free": (0.0, 0.0), "defl": (100.0, 0.01)}


def main():
    cfg = sizing.SizingConfig()
    cases = sizing.make_cases(N_CASES, cfg, seed=SEED, device="cpu")
    out = {"Fy": cases.Fy.numpy(), "fix": cases.fix.numpy(), "n_cases": N_CASES, "seed": SEED}
    for tag, (alpha, limit) in OBJECTIVES.items():
        r = tr.loop_oracle(cases, cfg, tr.objective(alpha, limit))
        print(tag, "epochs", r.epochs, "final loss", [float(r.loss[b, r.epochs[b] - 1]) for b in range(N_CASES)],
              "max|v|", r.vmax, "" if not alpha else f"max|v| / v_lim {r.vmax / limit}")
        if alpha:
            assert (r.vmax / limit).max() < 1.05, r.vmax / limit
        out.update({f"{tag}_loss": r.loss, f"{tag}_I": r.I, f"{tag}_epochs": r.epochs, f"{tag}_vmax": r.vmax,
                    f"{tag}_objective": np.array([alpha, limit])})
    path = os.path.join(HERE, "sizing_total_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
