"""Generates tests/golden/frame_sizing_designs_reference.npz: the project's own oracle of multi-load-case frame sizing
(tests/frame_designs_ref.py::loop_oracle_designs -- float32 I, torch.optim.Adam without a scheduler + clamp on the CPU, .grad from
autograd of the float64 per-case objectives through the dense model of tests/frame_dense_w.py, aggregated).  It reads nothing of
the reference.

Frames: the 2 x 3 and the 4 x 2 grid frame (bays x stories) of FrameConfig's geometry, G = 3 designs x C = 3 load cases each: wind from
the left with gravity, wind from the right with gravity, 1.5 x gravity alone -- `grid_load_cases` with (lateral, vertical) =
(+H, q), (-H, q), (0, 1.5 q), H uniform in [0.5e4, 2e4] and q in [-2e4, -0.5e4] per design; I0 log-uniform in [2e-4, 2e-3]; one seed
per frame.  Three runs per frame:
  sum        aggregate "sum", no displacement term, max_epochs = 60
  weighted   aggregate "sum" with weights (1, 1, 0.5) and both hinges in the "limit" configuration of
             tests/golden/make_frame_sizing_total_golden.py (alpha_moment = alpha_shear = 1e-4, lr = 3e-4, its limits), max_epochs = 120
  max        aggregate "max", no displacement term, max_epochs = 60
Per frame `<frame>_`: I0 [3,Ne] float32, loads [3,3,Nn,3], w [3,3,Ne,2]; per run `<tag>_<frame>_`: loss [3, max_epochs] float32 (NaN past
a design's last epoch), I [3,Ne] float32 after the last step, epochs [3], governing [3], case_penalty [3,3], objective, max_epochs,
aggregate, weights (empty: none).

Asserted, for the oracle alone: no early-stop decision of any design is marginal (a loss within MARGIN, relative, of the threshold it
is compared with), no governing-case choice of a "max" run at any epoch and of any run at its last epoch is marginal (the two
largest scores within MARGIN, relative), and in every "max" run at least one design is governed by a case other than case 0 at its
last epoch.  MARGIN is that of make_frame_sizing_total_golden.py, for its reason: several times the loss deviation of a recorded GPU
run, so a decision of the GPU loop can differ from the oracle's for more than rounding alone.  Change the seed until this holds.

Run:  python tests/golden/make_frame_sizing_designs_golden.py
"""
from __future__ import annotations

import dataclasses
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import frames  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_designs_ref as dr  # noqa: E402
from tests import frame_sizing_total_ref as ft  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_frame_sizing_total_golden", os.path.join(HERE, "make_frame_sizing_total_golden.py"))
single = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(single)

G, C = 3, 3
FRAMES = {"2x3": (2, 3, 3), "4x2": (4, 2, 1)}          # bays, stories, seed (2 x 3: seeds 1 and 2 each leave a marginal stop decision)
MARGIN = single.MARGIN
WEIGHTS = (1.0, 1.0, 0.5)
TAGS = ("sum", "weighted", "max")


def runs(frame):
    """tag -> (FrameConfig, objective, max_epochs, aggregate, weights)."""
    limit_cfg, limit_obj, limit_epochs = single.runs(frame)["limit"]
    return {"sum": (frames.FrameConfig(), ft.objective(), 60, "sum", None),
            "weighted": (dataclasses.replace(limit_cfg), limit_obj, limit_epochs, "sum", WEIGHTS),
            "max": (frames.FrameConfig(), ft.objective(), 60, "max", None)}


def fixture_inputs(frame):
    """(topology on the CPU, I0 [G,Ne] float32, loads [G,C,Nn,3], w [G,C,Ne,2]) of a frame, from its seed."""
    bays, stories, seed = FRAMES[frame]
    topo = frames.grid_frame(bays, stories, device="cpu")
    rng = np.random.default_rng(seed)
    I0 = np.exp(rng.uniform(np.log(2e-4), np.log(2e-3), size=(G, topo.Ne))).astype(np.float32)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    lateral = np.stack([H, -H, np.zeros(G)], axis=1).reshape(-1)
    vertical = np.stack([q, q, 1.5 * q], axis=1).reshape(-1)
    loads, w = frames.grid_load_cases(topo, lateral, vertical)
    return topo, I0, loads.numpy().reshape(G, C, topo.Nn, 3), w.numpy().reshape(G, C, topo.Ne, 2)


def main():
    out, marginal = {"C": C}, []
    for frame in FRAMES:
        topo, I0, loads, w = fixture_inputs(frame)
        case = fd.case_of(topo)
        out.update({f"{frame}_I0": I0, f"{frame}_loads": loads, f"{frame}_w": w})
        for tag, (cfg, obj, max_epochs, aggregate, weights) in runs(frame).items():
            agg = dr.MAX if aggregate == "max" else dr.SUM
            r = dr.loop_oracle_designs(case, cfg, obj, I0, loads, w, max_epochs, agg, weights)
            print(frame, tag, "epochs", r.epochs, "governing", r.governing, "margin", r.margin, "gap", r.gov_gap, "last gap", r.gov_gap_last)
            marginal += [(frame, tag, g, "stop") for g in range(G) if r.margin[g] < MARGIN]
            marginal += [(frame, tag, g, "governing") for g in range(G) if (r.gov_gap if tag == "max" else r.gov_gap_last)[g] < MARGIN]
            if tag == "max":
                assert (r.governing != 0).any(), f"{frame}: every design of the max run is governed by case 0, change the seed"
            p = f"{tag}_{frame}_"
            out.update({p + "loss": r.loss, p + "I": r.I, p + "epochs": r.epochs, p + "governing": r.governing,
                        p + "case_penalty": r.case_penalty, p + "max_epochs": max_epochs, p + "aggregate": agg,
                        p + "weights": np.asarray([] if weights is None else weights, dtype=np.float64),
                        p + "objective": np.array([obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])})
    assert not marginal, f"marginal decisions, change the seed: {marginal}"
    path = os.path.join(HERE, "frame_sizing_designs_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
