#!/usr/bin/env python3
"""Time per epoch of sizing G frame designs under C load cases each on one kept factorisation (`optimize_frame_designs`, DESIGN.md
§9l) against what served the same rows before it, on one GPU:

    python scripts/frame_designs_time.py [bays x stories x G ...] [--cases 1,2,4,8] [--json PATH]

Per shape and C, two forms on the same loads (per-case nodal and element loads from `grid_load_cases`):
    designs   optimize_frame_designs(topo, loads [G,C,..], w [G,C,..])                     one factorisation per design and epoch
    rows      optimize_frames(topo, G * C, gradient="total", loads=, element_loads=)       two factorisations per ROW and epoch
(the rows form sizes every row on its own: it answers another question, and is what there was.)  Both run a fixed number of epochs
with the early stop disabled through tolerance and patience, one poll at the end; the time is that of the whole call -- buffers,
epochs, the last solve -- over the number of epochs.  A warm-up, a short run to size the timed window to about a second, then three
rounds alternating the two forms; the median and the rounds are printed.  Host clock around a call that ends in a device
synchronise.  Every (shape, C) cell runs in a process of its own under a time limit; after a cell that fails or runs out of time
nothing more is started.  Default: 5x5x4096, 10x10x2048 and 15x16x1024 designs at C = 1, 2, 4, 8, written to
profiles/frame_designs_timing.json."""
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL_LIMIT_S = 150


def cell(bays, stories, G, C):
    import torch
    from openpystruct_amd import frames
    from openpystruct_amd.frame_designs import optimize_frame_designs
    topo = frames.grid_frame(bays, stories)
    f64 = dict(dtype=torch.float64, device=topo.device)
    R = G * C
    lateral, vertical = torch.linspace(-2e4, 2e4, R, **f64), torch.linspace(-2e4, -0.5e4, R, **f64)
    loads_rows, w_rows = frames.grid_load_cases(topo, lateral, vertical)
    loads, w = loads_rows.view(G, C, topo.Nn, 3), w_rows.view(G, C, topo.Ne, 2)
    cfg = dataclasses.replace(frames.FrameConfig(), tolerance=-1e30, patience=2 ** 30)      # every epoch improves: nothing stops

    def designs(n):
        r = optimize_frame_designs(topo, loads, w, cfg=cfg, max_epochs=n, poll_every=n)
        assert int(r.epochs.min()) == n and int(r.solution.status.abs().sum()) == 0

    def rows(n):
        _, sol, ep = frames.optimize_frames(topo, R, cfg, max_epochs=n, poll_every=n, gradient="total", loads=loads_rows, element_loads=w_rows)
        assert int(ep.min()) == n and int(sol.status.abs().sum()) == 0

    forms, epochs = {"designs": designs, "rows": rows}, {}
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
            "epochs_per_window": epochs, "us_per_epoch": {k: round(v, 1) for k, v in med.items()},
            "us_per_epoch_rounds": {k: [round(t, 1) for t in v] for k, v in times.items()},
            "rows_over_designs": round(med["rows"] / med["designs"], 3),
            "designs_faster_in_every_round": all(a < b for a, b in zip(times["designs"], times["rows"])),
            "device": torch.cuda.get_device_name(0)}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--cell"]:
        print("CELL " + json.dumps(cell(*(int(v) for v in args[1:5]))), flush=True)
        return 0
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_designs_timing.json")
    cases = [int(v) for v in args[args.index("--cases") + 1].split(",")] if "--cases" in args else [1, 2, 4, 8]
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if a.count("x") == 2 and a[0].isdigit()] \
        or [(5, 5, 4096), (10, 10, 2048), (15, 16, 1024)]
    rows, device, rc = [], None, 0
    for bays, stories, G in shapes:
        for C in cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(bays), str(stories), str(G), str(C)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=CELL_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"{bays}x{stories}x{G} C = {C}: no result within {CELL_LIMIT_S} s; nothing more is started", flush=True)
                rc = 124
                break
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("CELL ")]
            if done.returncode != 0 or not line:
                print(f"{bays}x{stories}x{G} C = {C}: ended with {done.returncode}; nothing more is started\n{done.stderr[-2000:]}", flush=True)
                rc = done.returncode or 1
                break
            row = json.loads(line[-1][5:])
            device = row.pop("device")
            rows.append(row)
            print(json.dumps(row), flush=True)
        if rc:
            break
    if rows:
        with open(path, "w") as f:
            json.dump({"device": device, "rows": rows}, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
