"""Generates tests/golden/frame_sizing_total_reference.npz: the project's own oracle of the exact-gradient ("total") frame sizing
loop (tests/frame_sizing_total_ref.py::loop_oracle_frames -- float32 I, torch.optim.Adam without a scheduler + clamp on the CPU,
.grad from autograd of the float64 objective through the dense model of tests/frame_dense.py).  It reads nothing of the reference.

Frames: the 2 x 3 and the 4 x 2 grid frame (bays x stories) of FrameConfig's geometry and loads, B = 4 each, I0 log-uniform in
[2e-4, 2e-3] from a fixed seed per frame.  Two runs per frame:
  free    the default FrameConfig, no displacement term, max_epochs = 60
  limit   alpha_moment = alpha_shear = 1e-4, lr = 3e-4, alpha_sway = 1 with sway_limit = 2.5e-3 (2 x 3) / 1.4e-3 (4 x 2),
          alpha_deflection = 1 with deflection_limit = 2e-4 (2 x 3) / 1e-4 (4 x 2), max_epochs = 120
Per run `<tag>_<frame>_`: loss [4, max_epochs] float32 (NaN past a frame's last epoch), I [4, Ne] float32 after the last step,
epochs [4], umax [4, 2] (max |ux|, max |uy| of the last solve), objective (alpha_sway, sway_limit, alpha_deflection,
deflection_limit), max_epochs; per frame `I0_<frame>`.

The limits are penalties: the generator prints max |u| / limit and asserts nothing about it.  It asserts that no early-stop decision of
the oracle, at any epoch of any of the sixteen runs, is marginal (a loss within MARGIN, relative, of the threshold it is compared
with): a marginal frame's stop epoch could differ on the GPU for rounding alone.

Run:  python tests/golden/make_frame_sizing_total_golden.py
"""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import frames  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_sizing_total_ref as ft  # noqa: E402

B = 4
FRAMES = {"2x3": (2, 3, 2), "4x2": (4, 2, 4)}          # bays, stories, seed of I0 (seeds 1-4 tried: these keep every decision clear)
LIMITS = {"2x3": (1.0, 2.5e-3, 1.0, 2e-4), "4x2": (1.0, 1.4e-3, 1.0, 1e-4)}
MARGIN = 2e-6      # several times the loss deviation of the recorded GPU run (3.5e-7: profiles/frame_sizing_total_deviation.json)


def runs(frame):
    """tag -> (FrameConfig, objective, max_epochs)."""
    return {"free": (frames.FrameConfig(), ft.objective(), 60),
            "limit": (dataclasses.replace(frames.FrameConfig(), alpha_moment=1e-4, alpha_shear=1e-4, lr=3e-4),
                      ft.objective(*LIMITS[frame]), 120)}


def main():
    out, marginal = {}, []
    for frame, (bays, stories, seed) in FRAMES.items():
        topo = frames.grid_frame(bays, stories, device="cpu")
        case = fd.case_of(topo)
        rng = np.random.default_rng(seed)
        I0 = np.exp(rng.uniform(np.log(2e-4), np.log(2e-3), size=(B, topo.Ne))).astype(np.float32)
        out[f"I0_{frame}"] = I0
        for tag, (cfg, obj, max_epochs) in runs(frame).items():
            r = ft.loop_oracle_frames(case, cfg, obj, I0, max_epochs)
            print(frame, tag, "epochs", r.epochs, "final loss", [float(r.loss[b, r.epochs[b] - 1]) for b in range(B)], "margin", r.margin)
            if tag == "limit":
                print("   max|ux| / sway_limit", r.umax[:, 0] / obj.sway_limit, "max|uy| / deflection_limit", r.umax[:, 1] / obj.deflection_limit)
            marginal += [(frame, tag, b) for b in range(B) if r.margin[b] < MARGIN]
            p = f"{tag}_{frame}_"
            out.update({p + "loss": r.loss, p + "I": r.I, p + "epochs": r.epochs, p + "umax": r.umax, p + "max_epochs": max_epochs,
                        p + "objective": np.array([obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])})
    assert not marginal, f"marginal stop decisions, change the seed: {marginal}"
    path = os.path.join(HERE, "frame_sizing_total_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
