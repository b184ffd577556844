#!/usr/bin/env python3
"""Time of the frame solve under per-frame element loads (three launches) and of the element-load VJP (one launch), on
one GPU:

    python scripts/frame_loads_time.py [bays x stories x B ...] [--json PATH]

Per shape: a warm-up, a short run to size the timed window to about a second, then three rounds alternating the two forms; the median and
the rounds are printed.  Host clock around a loop that ends in a device synchronise."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpystruct_amd import frames  # noqa: E402


def main():
    args = sys.argv[1:]
    path = args[args.index("--json") + 1] if "--json" in args else None
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a and not a.startswith("-") and a != path] or [(5, 5, 32768)]
    rows = []
    for bays, stories, B in shapes:
        topo = frames.grid_frame(bays, stories)
        f64 = dict(dtype=torch.float64, device=topo.device)
        I = torch.full((B, topo.Ne), frames.FrameConfig().I0, **f64)
        w = torch.linspace(-2e4, -0.5e4, B, **f64)[:, None, None].expand(B, topo.Ne, 2).contiguous()
        sol = frames.frame_solve(topo, I, element_loads=w)
        lam, gM = sol.disp.clone(), sol.M.clone()

        def solve_loads(n):
            for _ in range(n):
                frames.frame_solve(topo, I, out=sol, element_loads=w)

        def load_vjp(n):
            for _ in range(n):
                frames.frame_element_load_vjp(topo, lam, gM=gM, status=sol.status)

        forms, calls = {"solve_loads": solve_loads, "load_vjp": load_vjp}, {}
        for name, run in forms.items():
            run(5)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(10)
            torch.cuda.synchronize()
            calls[name] = max(20, min(20000, int(10 / (time.perf_counter() - t0))))
        times = {name: [] for name in forms}
        for _ in range(3):
            for name, run in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(calls[name])
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / calls[name] * 1e6)
        row = {"frame": f"{bays}x{stories}", "B": B, "Nn": topo.Nn, "Ne": topo.Ne, "kd": topo.kd, "calls_per_window": calls,
               "us_per_call": {k: round(statistics.median(v), 1) for k, v in times.items()},
               "us_per_call_rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
