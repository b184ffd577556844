"""Generates tests/golden/frame_groups_reference.npz: the project's own oracle of frame sizing with linked member groups
(tests/frame_groups_ref.py::loop_oracle_groups -- one float32 leaf per group, torch.optim.Adam without a scheduler + clamp on the
CPU, .grad the left-to-right float64 segment sum of the aggregated per-element gradient through the dense model of
tests/frame_dense_w.py).  It reads nothing of the reference.

Frames, load cases, runs (sum / weighted / max) and configurations are those of make_frame_sizing_designs_golden.py: the 2 x 3 and
the 4 x 2 grid frame, G = 3 designs x C = 3 load cases, the same draws from this file's seeds; the groups are `story_groups` (2 x 3:
6 groups, 4 x 2: 4) and X0 is log-uniform in [2e-4, 2e-3] per group.
Per frame `<frame>_`: groups [Ne] int32, X0 [3,Ng] float32, loads [3,3,Nn,3], w [3,3,Ne,2]; per run `<tag>_<frame>_`: loss
[3, max_epochs] float32 (NaN past a design's last epoch), X [3,Ng] and I [3,Ne] float32 after the last step, epochs [3], governing [3],
case_penalty [3,3], objective, max_epochs, aggregate, weights (empty: none).

Asserted, for the oracle alone, by the MARGIN rule of make_frame_sizing_designs_golden.py: no early-stop decision of any design is
marginal, no governing-case choice of a "max" run at any epoch and of any run at its last epoch is marginal.  Change the seed until
this holds.

Run:  python tests/golden/make_frame_groups_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import frame_groups, frames  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_groups_ref as gr  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_frame_sizing_designs_golden", os.path.join(HERE, "make_frame_sizing_designs_golden.py"))
designs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(designs)

G, C = designs.G, designs.C
SEEDS = {"2x3": 11, "4x2": 12}
MARGIN = designs.MARGIN
TAGS = designs.TAGS
runs = designs.runs


def fixture_inputs(frame):
    """(topology on the CPU, groups [Ne], X0 [G,Ng] float32, loads [G,C,Nn,3], w [G,C,Ne,2]) of a frame, from its seed."""
    bays, stories, _ = designs.FRAMES[frame]
    topo = frames.grid_frame(bays, stories, device="cpu")
    groups = frame_groups.story_groups(topo)
    rng = np.random.default_rng(SEEDS[frame])
    X0 = np.exp(rng.uniform(np.log(2e-4), np.log(2e-3), size=(G, int(groups.max()) + 1))).astype(np.float32)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    lateral = np.stack([H, -H, np.zeros(G)], axis=1).reshape(-1)
    vertical = np.stack([q, q, 1.5 * q], axis=1).reshape(-1)
    loads, w = frames.grid_load_cases(topo, lateral, vertical)
    return topo, groups, X0, loads.numpy().reshape(G, C, topo.Nn, 3), w.numpy().reshape(G, C, topo.Ne, 2)


def main():
    out, marginal = {"C": C}, []
    for frame in designs.FRAMES:
        topo, groups, X0, loads, w = fixture_inputs(frame)
        case = fd.case_of(topo)
        out.update({f"{frame}_groups": groups, f"{frame}_X0": X0, f"{frame}_loads": loads, f"{frame}_w": w})
        for tag, (cfg, obj, max_epochs, aggregate, weights) in runs(frame).items():
            agg = gr.MAX if aggregate == "max" else gr.SUM
            r = gr.loop_oracle_groups(case, cfg, obj, X0, groups, loads, w, max_epochs, agg, weights)
            print(frame, tag, "epochs", r.epochs, "governing", r.governing, "margin", r.margin, "gap", r.gov_gap, "last gap", r.gov_gap_last, flush=True)
            marginal += [(frame, tag, g, "stop") for g in range(G) if r.margin[g] < MARGIN]
            marginal += [(frame, tag, g, "governing") for g in range(G) if (r.gov_gap if tag == "max" else r.gov_gap_last)[g] < MARGIN]
            p = f"{tag}_{frame}_"
            out.update({p + "loss": r.loss, p + "X": r.X, p + "I": r.I, p + "epochs": r.epochs, p + "governing": r.governing,
                        p + "case_penalty": r.case_penalty, p + "max_epochs": max_epochs, p + "aggregate": agg,
                        p + "weights": np.asarray([] if weights is None else weights, dtype=np.float64),
                        p + "objective": np.array([obj.alpha_sway, obj.sway_limit, obj.alpha_deflection, obj.deflection_limit])})
    assert not marginal, f"marginal decisions, change the seed: {marginal}"
    path = os.path.join(HERE, "frame_groups_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
