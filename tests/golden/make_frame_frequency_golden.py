"""Generates tests/golden/frame_frequency_reference.npz: the project's own oracle of multi-load-case frame sizing with a
natural-frequency floor (tests/frame_frequency_ref.py::loop_oracle_frequency -- `loop_oracle_designs` / `loop_oracle_groups` with the
term added, the eigenpairs from the NumPy restatement of the subspace iteration, continued across the epochs).  It reads nothing of
the reference.

Frame: the 2-bay x 3-story grid frame of FrameConfig's geometry, G = 3 designs x C = 2 load cases each -- wind with gravity, and
1.5 x gravity alone: `grid_load_cases` with (lateral, vertical) = (H, q), (0, 1.5 q), H uniform in [0.5e4, 2e4] and q in
[-2e4, -0.5e4] per design --, every design starting from cfg.I0, 40 epochs, FrameConfig's objective with lr = 3e-3 (with FrameConfig's
5e-3 the losses of the last epochs come within 1.7e-3 of the early-stop threshold: the condition below asks for 2e-3).  Mass: consistent, 157 kg/m
(tests/frame_modes_ref.py MBAR), 2000 kg (NODAL) on the translations and 50 kg m^2 on the rotation of every node.  Term: m = 2 tracked
modes on p = 6 vectors, start_iters = 12, iters = 2, alpha = 25, and per design a floor relative to lambda_1(I0):
  (a) x 1e-3   far below lambda_1: the term is never on
  (b) x 60     the hinge of mode 1 is on throughout (lambda_1 ends at 0.6 floor); the hinge of mode 2 is on for the first two epochs
               only -- lambda_2(I0) is 11 lambda_1(I0) and passes 60 lambda_1(I0) once I has grown about sevenfold, whatever the mass
  (c) x C_FLOOR (about 4): lambda_1 crosses the floor while the static penalties drive I up
Runs: "sum" and "max" on the three designs; "grouped": design (b) alone with `story_groups`, "sum".
Stored: min_frequency [3] (Hz), loads [3,2,Nn,3], w [3,2,Ne,2]; per run `<tag>_`: loss [G,40] float32, I [G,Ne] float32, X (grouped),
epochs, governing, case_penalty, penalty (P_f at the last epoch), lam (the tracked eigenvalues at the last epoch), hinges_on [G,40],
and the least hinge margin, mode gap, early-stop margin and governing gap over the epochs.

Asserted, for the oracle alone: hinge margin >= 1e-3, mode gap >= 0.05, early-stop margin >= 2e-3, governing gap >= 2e-3 in every
run.  Move C_FLOOR or the seed until this holds.

Run:  python tests/golden/make_frame_frequency_golden.py
"""
from __future__ import annotations

import dataclasses
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from openpystruct_amd import frames  # noqa: E402
from openpystruct_amd.frame_groups import story_groups  # noqa: E402
from tests import frame_dense as fd  # noqa: E402
from tests import frame_designs_ref as dr  # noqa: E402
from tests import frame_frequency_ref as qr  # noqa: E402
from tests import frame_modes_ref as fr  # noqa: E402
from tests import frame_sizing_total_ref as ft  # noqa: E402

BAYS, STORIES, G, C, SEED, EPOCHS = 2, 3, 3, 2, 4, 40
M_MODES, P_VECTORS, ITERS, START_ITERS, ALPHA = 2, 6, 2, 12, 25.0
C_FLOOR = 4.0
FACTORS = (1e-3, 60.0, C_FLOOR)
TAGS = ("sum", "max", "grouped")
LIMITS = dict(hinge_margin=1e-3, mode_gap=0.05, margin=2e-3, gov_gap=2e-3)


def config():
    return dataclasses.replace(frames.FrameConfig(), lr=3e-3)


def nodal_mass(topo):
    return np.tile(np.array([fr.NODAL, fr.NODAL, 50.0]), (topo.Nn, 1))


def fixture_inputs():
    """(topology on the CPU, case, I0 [G,Ne] float32, loads [G,C,Nn,3], w [G,C,Ne,2], dense M, min_frequency [G] in Hz)."""
    cfg = config()
    topo = frames.grid_frame(BAYS, STORIES, device="cpu")
    case = fd.case_of(topo)
    rng = np.random.default_rng(SEED)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    loads, w = frames.grid_load_cases(topo, np.stack([H, np.zeros(G)], axis=1).reshape(-1), np.stack([q, 1.5 * q], axis=1).reshape(-1))
    I0 = np.full((G, topo.Ne), cfg.I0, dtype=np.float32)
    M = fr.dense_M(case, fr.MBAR, "consistent", nodal_mass(topo))
    lam1 = fr.dense_modes(case, I0[0].astype(np.float64), M, 1)[0][0]
    min_frequency = np.sqrt(np.array(FACTORS) * lam1) / (2.0 * math.pi)
    return topo, case, I0, loads.numpy().reshape(G, C, topo.Nn, 3), w.numpy().reshape(G, C, topo.Ne, 2), M, min_frequency


def oracle(tag, designs=None, max_epochs=None, exact=False, iters=ITERS):
    topo, case, I0, loads, w, M, fmin = fixture_inputs()
    sel = list(designs) if designs is not None else ([1] if tag == "grouped" else list(range(G)))
    term = types.SimpleNamespace(M=M, floor=qr.floor_of(fmin)[sel], alpha=ALPHA, m=M_MODES, p=P_VECTORS, iters=iters, start_iters=START_ITERS)
    labels = story_groups(topo) if tag == "grouped" else None
    V0 = I0[sel] if labels is None else np.full((len(sel), int(labels.max()) + 1), config().I0, dtype=np.float32)
    return qr.loop_oracle_frequency(case, config(), ft.objective(), V0, loads[sel], w[sel], max_epochs or EPOCHS,
                                    dr.MAX if tag == "max" else dr.SUM, None, term, labels=labels, exact=exact)


def main():
    topo, case, I0, loads, w, M, fmin = fixture_inputs()
    out, short = {"tags": np.array(TAGS), "min_frequency": fmin, "loads": loads, "w": w}, []
    for tag in TAGS:
        r = oracle(tag)
        print(tag, "epochs", r.epochs, "governing", r.governing, {k: getattr(r, k) for k in LIMITS}, "penalty", r.penalty)
        print("   hinges on:", [r.hinges_on[g][r.hinges_on[g] >= 0].tolist() for g in range(len(r.epochs))])
        short += [(tag, k, getattr(r, k).tolist()) for k, v in LIMITS.items() if getattr(r, k).min() < v]
        for k in ("loss", "I", "epochs", "governing", "case_penalty", "penalty", "lam", "hinges_on") + tuple(LIMITS) + (("X",) if tag == "grouped" else ()):
            out[f"{tag}_{k}"] = getattr(r, k)
    assert not short, f"conditions not met, move C_FLOOR or the seed: {short}"
    path = os.path.join(HERE, "frame_frequency_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
