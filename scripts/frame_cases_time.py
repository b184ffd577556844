#!/usr/bin/env python3
"""Time of B designs under C load cases each on one kept factorisation against what serves the same request without
it, on one GPU:

    python scripts/frame_cases_time.py [bays x stories x B ...] [--cases 1,2,4,8] [--json PATH]

Per shape and C, four forms on the same inputs (per-case nodal and element loads from `grid_load_cases`, cotangents of disp and M):
    a  cases        frame_solve_cases(topo, I, loads, w)                                   one factorisation per design
    b  rows         frame_solve(topo, I_rows, loads_rows, element_loads=w_rows)            I repeated per case: C factorisations per design
    c  cases_vjp    frame_solve_cases_vjp(factor, sol, g_disp, gM=gM)                      no factorisation
    d  rows_vjp     frame_solve_vjp + frame_element_load_vjp on the rows                   one factorisation per row
A warm-up, a short run to size the timed window to about a second, then three rounds alternating the four forms; the median and the
rounds are printed.  Host clock around a loop that ends in a device synchronise.  Default: 5x5x8192, 10x10x4096 and 15x16x3072 at
C = 1, 2, 4, 8, written to profiles/frame_cases_timing.json."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openpystruct_amd import frames  # noqa: E402


def main():
    args = sys.argv[1:]
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_cases_timing.json")
    cases = [int(v) for v in args[args.index("--cases") + 1].split(",")] if "--cases" in args else [1, 2, 4, 8]
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if a.count("x") == 2 and a[0].isdigit()] \
        or [(5, 5, 8192), (10, 10, 4096), (15, 16, 3072)]
    rows = []
    for bays, stories, B in shapes:
        topo = frames.grid_frame(bays, stories)
        f64 = dict(dtype=torch.float64, device=topo.device)
        I = torch.full((B, topo.Ne), frames.FrameConfig().I0, **f64) * torch.linspace(0.5, 2.0, B, **f64)[:, None]
        for C in cases:
            R = B * C
            lateral, vertical = torch.linspace(-2e4, 2e4, R, **f64), torch.linspace(-2e4, -0.5e4, R, **f64)
            loads_rows, w_rows = frames.grid_load_cases(topo, lateral, vertical)
            loads, w = loads_rows.view(B, C, topo.Nn, 3), w_rows.view(B, C, topo.Ne, 2)
            I_rows = I.repeat_interleave(C, 0)
            factor = frames.frame_factor(topo, I)
            sol = frames.frame_resolve(factor, loads, w)
            sol_rows = frames.frame_solve(topo, I_rows, loads_rows, element_loads=w_rows)
            assert int(sol.status.abs().sum()) == 0 and int(sol_rows.status.abs().sum()) == 0
            g_disp, gM = sol.disp.clone() * 1e6, sol.M.clone() * 1e-4
            g_disp_rows, gM_rows = g_disp.view(R, topo.Nn, 3), gM.view(R, topo.Ne)

            def cases_(n):
                for _ in range(n):
                    frames.frame_solve_cases(topo, I, loads, w)

            def rows_(n):
                for _ in range(n):
                    frames.frame_solve(topo, I_rows, loads_rows, element_loads=w_rows)

            def cases_vjp(n):
                for _ in range(n):
                    frames.frame_solve_cases_vjp(factor, sol, g_disp, gM=gM)

            def rows_vjp(n):
                for _ in range(n):
                    _, lam, st = frames.frame_solve_vjp(topo, I_rows, sol_rows.disp, g_disp_rows, gM=gM_rows, status=sol_rows.status)
                    frames.frame_element_load_vjp(topo, lam, gM=gM_rows, status=sol_rows.status, status_adj=st)

            forms, calls = {"cases": cases_, "rows": rows_, "cases_vjp": cases_vjp, "rows_vjp": rows_vjp}, {}
            for name, run in forms.items():
                run(3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(5)
                torch.cuda.synchronize()
                calls[name] = max(5, min(20000, int(5 / (time.perf_counter() - t0))))
            times = {name: [] for name in forms}
            for _ in range(3):
                for name, run in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(calls[name])
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / calls[name] * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            row = {"frame": f"{bays}x{stories}", "B": B, "C": C, "Nn": topo.Nn, "Ne": topo.Ne, "n_eq": topo.n_eq, "kd": topo.kd,
                   "calls_per_window": calls, "us_per_call": {k: round(v, 1) for k, v in med.items()},
                   "us_per_call_rounds": {k: [round(t, 1) for t in v] for k, v in times.items()},
                   "rows_over_cases": round(med["rows"] / med["cases"], 3), "rows_vjp_over_cases_vjp": round(med["rows_vjp"] / med["cases_vjp"], 3),
                   "cases_faster_in_every_round": all(a < b for a, b in zip(times["cases"], times["rows"])),
                   "cases_vjp_faster_in_every_round": all(a < b for a, b in zip(times["cases_vjp"], times["rows_vjp"]))}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del factor, sol, sol_rows
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if os.path.exists(path):            # keep what else the file records (the frames benchmark of this commit and of its parent)
        with open(path) as f:
            out = {**{k: v for k, v in json.load(f).items() if k not in out}, **out}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
