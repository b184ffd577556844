#!/usr/bin/env python3
"""The design-objective term as a training loss, recorded on one GPU:

    python scripts/design_loss_train.py [--designs 2048] [--cases 6] [--epochs 40] [--weight 0.5] [--out PATH]

Trains the Transformer-Diffusion surrogate on one `generate_multicase_dataset` set (designs optimised under all their load cases
together: the label IS the optimiser's design) twice from the same seed -- `train.DesignTerm(weight=0)` (the data loss alone; the
term's launches run and add nothing) and `train.DesignTerm(weight=w)` -- and writes both runs' `design_gap_val`
(L(I_pred) / L(I_label) - 1 over the validation split), R² on I and losses to profiles/design_loss_notes.md.
A record of one run, not a target."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    from openpystruct_amd import dataprep, multicase, runtime, sizing, train
    runtime.configure()
    if not torch.cuda.is_available():
        raise SystemExit("design_loss_train.py trains on a GPU: none is visible")
    dev = torch.device("cuda", 0)
    designs, C, epochs, weight = arg("--designs", 2048), arg("--cases", 6), arg("--epochs", 40), arg("--weight", 0.5)
    path = arg("--out", os.path.join(ROOT, "profiles", "design_loss_notes.md"))
    cfg = sizing.SizingConfig(max_e=300)
    t0 = time.perf_counter()
    rec = multicase.generate_multicase_dataset(designs, C, cfg, dev, seed=7)
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    assert int(rec["status"].abs().sum()) == 0
    fix = sizing.make_cases(1, cfg, seed=7, device="cpu").fix[0]
    data = dataprep.prepare(rec, kind="tfd", n_cases=C, seed=0, device=dev)
    tcfg = train.TfdConfig(n_cases=C, batch_size=128)
    runs = {}
    for w in (0.0, weight):
        term = train.DesignTerm(weight=w, x=rec["node_positions"][0].double().cpu(), E=cfg.E, fix=fix, wy=cfg.uniform_udl, hp=cfg)
        t0 = time.perf_counter()
        r = train.train_surrogate("tfd", data, tcfg, device=dev, max_epochs=epochs, seed=1, physics=term)
        runs[w] = {"design_gap_val": r["design_gap_val"], "r2_val_I": r["r2_val_I"], "best_val": r["best_val"], "epochs": r["epochs"],
                   "train_loss_last": r["history"]["train"][-1], "wall_s": round(time.perf_counter() - t0, 1)}
        print(json.dumps({"weight": w, **runs[w]}), flush=True)
    pct = lambda v: f"{100.0 * v:.2f} %"      # noqa: E731
    lines = ["# The design-objective term as a training loss: one recorded run", "",
             f"`python scripts/design_loss_train.py` on {torch.cuda.get_device_name(0)}: {designs} designs x {C} load cases of the reference",
             f"bridge from `generate_multicase_dataset` (max_e {cfg.max_e}, aggregate \"sum\"; {gen_s:.1f} s), `dataprep.prepare(kind=\"tfd\",",
             f"n_cases={C})` ({data.X_train.shape[0]} training / {data.X_val.shape[0]} validation designs), `TfdConfig(batch_size=128)`, {epochs} epochs, seed 1,",
             "the same seed for both runs.  `design_gap_val` = L(I_pred) / L(I_label) - 1 over the validation designs, both objectives by",
             "`design_objective` under the design's own load cases.  A measurement of one run; no threshold is set on any figure.", "",
             "| run | gap mean | gap median | gap max | failed | R² on I | best val loss | last train loss (data + term) | epochs | wall s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for w, r in runs.items():
        g = r["design_gap_val"]
        lines.append(f"| `DesignTerm(weight={w})` | {pct(g['mean'])} | {pct(g['median'])} | {pct(g['max'])} | {g['failed']} of {g['samples']} | "
                     f"{r['r2_val_I']:.4f} | {r['best_val']:.5f} | {r['train_loss_last']:.5f} | {r['epochs']} | {r['wall_s']} |")
    lines += ["", "With weight 0 the term's four launches run and its gradient is zero: the run is the data loss alone, scored by the same metric.",
              "The training loss of the weighted run includes the term's value (weight x the mean optimality ratio, about the weight itself",
              "near the labels), so the two columns of losses are not comparable; the gap and R² columns are.", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
