#!/usr/bin/env python3
"""Time per epoch of `optimize_frame_designs` with and without a natural-frequency floor (`frequency=`) on one GPU:

    python scripts/frame_frequency_time.py [bays x stories x G ...] [--json PATH]

Per shape, C = 4 load cases per design (per-case nodal and element loads from `grid_load_cases`), consistent mass (157 kg/m members,
2000 kg nodal masses shared by the batch), m = 2 tracked modes on p = 6 vectors, a floor at 60 x lambda_1(I0), alpha 25:
    plain     optimize_frame_designs(topo, loads, w)                                            six launches per epoch
    iters_k   the same call with frequency=FrequencyFloor(..., iters=k, start_iters=k), k = 1, 2, 4:    6 + 3 k + 1 launches per epoch
All run a fixed number of epochs with the early stop disabled through tolerance and patience, one poll at the end; the time is that of
the whole call -- buffers, epochs, the last solve -- over the number of epochs.  A warm-up, a short run to size the timed window to
about a second, then three rounds alternating the forms; the median and the rounds are printed.  Host clock around a call that ends
in a device synchronise.  There is no target and no pass/fail number.  Every shape runs in a process of its own under a time limit;
after a shape that fails or runs out of time nothing more is started.  Default: 5x5x4096 and 5x5x1, written to
profiles/frame_frequency_timing.json."""
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL_LIMIT_S = 200
C, M_MODES, P_VECTORS, ITERS = 4, 2, 6, (1, 2, 4)


def cell(bays, stories, G):
    import numpy as np
    import torch
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    topo = frames.grid_frame(bays, stories)
    f64 = dict(dtype=torch.float64, device=topo.device)
    R = G * C
    lateral, vertical = torch.linspace(-2e4, 2e4, R, **f64), torch.linspace(-2e4, -0.5e4, R, **f64)
    loads_rows, w_rows = frames.grid_load_cases(topo, lateral, vertical)
    loads, w = loads_rows.view(G, C, topo.Nn, 3), w_rows.view(G, C, topo.Ne, 2)
    cfg = dataclasses.replace(frames.FrameConfig(), tolerance=-1e30, patience=2 ** 30)      # every epoch improves: nothing stops
    mass = oa.FrameMass(topo, 157.0, np.full((topo.Nn, 3), 2000.0) * np.array([1.0, 1.0, 0.0]))
    I0 = torch.full((1, topo.Ne), cfg.I0, **f64)
    lam1 = float(oa.frame_solve_modes(topo, I0, mass, n_modes=1, iters=24).eigenvalues[0, 0])
    fmin = (60.0 * lam1) ** 0.5 / (2.0 * np.pi)
    terms = {f"iters_{k}": oa.FrequencyFloor(mass, fmin, alpha=25.0, n_modes=M_MODES, n_vectors=P_VECTORS, iters=k, start_iters=k) for k in ITERS}

    def form(term):
        def run(n):
            r = oa.optimize_frame_designs(topo, loads, w, n_designs=G, cfg=cfg, max_epochs=n, poll_every=n, frequency=term)
            assert int(r.epochs.min()) == n and int(r.solution.status.abs().sum()) == 0
        return run

    forms, epochs = {"plain": form(None), **{k: form(t) for k, t in terms.items()}}, {}
    for name, run in forms.items():
        run(3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(10)
        torch.cuda.synchronize()
        epochs[name] = max(10, min(5000, int(10 / (time.perf_counter() - t0))))
    times = {name: [] for name in forms}
    for _ in range(3):
        for name, run in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(epochs[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / epochs[name] * 1e6)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"frame": f"{bays}x{stories}", "G": G, "C": C, "Nn": topo.Nn, "Ne": topo.Ne, "n_eq": topo.n_eq, "kd": topo.kd,
            "n_modes": M_MODES, "n_vectors": P_VECTORS, "epochs_per_window": epochs, "us_per_epoch": {k: round(v, 1) for k, v in med.items()},
            "us_per_epoch_rounds": {k: [round(t, 1) for t in v] for k, v in times.items()},
            "over_plain": {k: round(med[k] / med["plain"], 3) for k in terms},
            "us_per_iteration_added": {f"iters_{k}": round((med[f"iters_{k}"] - med["plain"]) / k, 1) for k in ITERS},
            "change_last_max": {k: float(t.modes.change.max()) for k, t in terms.items()},
            "designs_with_a_mode_status": {k: int((t.modes.status != 0).sum()) for k, t in terms.items()}, "device": torch.cuda.get_device_name(0)}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--cell"]:
        print("CELL " + json.dumps(cell(*(int(v) for v in args[1:4]))), flush=True)
        return 0
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_frequency_timing.json")
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if a.count("x") == 2 and a[0].isdigit()] or [(5, 5, 4096), (5, 5, 1)]
    rows, device, rc = [], None, 0
    for bays, stories, G in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(bays), str(stories), str(G)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=CELL_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{bays}x{stories}x{G}: no result within {CELL_LIMIT_S} s; nothing more is started", flush=True)
            rc = 124
            break
        line = [ln for ln in done.stdout.splitlines() if ln.startswith("CELL ")]
        if done.returncode != 0 or not line:
            print(f"{bays}x{stories}x{G}: ended with {done.returncode}; nothing more is started\n{done.stderr[-2000:]}", flush=True)
            rc = done.returncode or 1
            break
        row = json.loads(line[-1][5:])
        device = row.pop("device")
        rows.append(row)
        print(json.dumps(row), flush=True)
    if rows:
        with open(path, "w") as f:
            json.dump({"device": device, "rows": rows}, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
