#!/usr/bin/env python3
"""Time of the natural-frequency iteration on the kept factorisation (`frame_modes`) on one GPU:

    python scripts/frame_modes_time.py [bays x stories x B ...] [--json PATH]

Per shape (consistent mass, 157 kg/m members, 2000 kg nodal masses shared by the batch, log-uniform inertias):
    iteration   the three launches of one iteration alone -- the re-solve of the B * p rows, the mass apply, the Ritz step -- each 20
                times back to back between two device events, on the buffers of a run that has converged (p = 8 vectors)
    to_tol      `frame_modes(factor, mass, n_modes=m, tol=1e-10)` for m = 1 and m = 4 on a kept factor: the host clock around the
                call and a device synchronise, with the iterations it ran; the factorisation is not in it (`factor_ms` beside it)
A warm-up, then five rounds; the medians and the rounds are written.  There is no target and no pass/fail number.  Every shape runs
in a process of its own under a time limit; after a shape that fails or runs out of time nothing more is started.  Default: 5x5x8192,
10x10x4096 and 15x16x3072 frames, written to profiles/frame_modes_timing.json."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELL_LIMIT_S = 150
LAUNCHES = 20
ROUNDS = 5


def cell(bays, stories, B):
    import numpy as np
    import torch
    import openpystruct_amd as oa
    from openpystruct_amd import _cabi, frames
    from openpystruct_amd.frame_modes import _mass_apply, default_vectors
    topo = frames.grid_frame(bays, stories)
    dev = topo.device
    rng = np.random.default_rng(0)
    I = torch.tensor(np.exp(rng.uniform(np.log(5e-5), np.log(5e-3), size=(B, topo.Ne))), dtype=torch.float64, device=dev)
    mass = oa.FrameMass(topo, 157.0, np.full((topo.Nn, 3), 2000.0) * np.array([1.0, 1.0, 0.0]))

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    factor_ms, fac = [], None
    for _ in range(ROUNDS + 1):
        ms, fac = timed(lambda: oa.frame_factor(topo, I))
        factor_ms.append(ms)
    to_tol = {}
    for m in (1, 4):
        rounds, its = [], None
        for _ in range(ROUNDS + 1):
            ms, r = timed(lambda: oa.frame_modes(fac, mass, n_modes=m, tol=1e-10))
            rounds.append(ms)
            its = r.iterations
        assert int(r.status.abs().sum()) == 0
        to_tol[f"m{m}"] = {"n_vectors": default_vectors(topo, m), "iterations": its,
                           "converged": bool((r.change <= 1e-10).all()), "ms": round(statistics.median(rounds[1:]), 3),
                           "ms_rounds": [round(t, 3) for t in rounds[1:]]}
    # the three launches alone, on the buffers of a converged run on eight vectors
    p = min(8, topo.n_eq)
    oa.frame_modes(fac, mass, n_modes=1, n_vectors=p, iters=8)
    shape = (B, p, topo.Nn, 3)
    out = frames.FrameCaseSolution(fac._buffer("modes_X", shape), fac._buffer("modes_forces", (B, p, topo.Ne, 6)), fac._buffer("modes_V", (B, p, topo.Ne)),
                                   fac._buffer("modes_M", (B, p, topo.Ne)), fac._buffer("modes_row_status", (B, p), torch.int32))
    X, MX, R, Q = out.disp, fac._buffer("modes_MX", shape), fac._buffer("modes_R", shape), fac._buffer("modes_Q", shape)
    lam, change, status = fac._buffer("modes_lambda", (B, p)), fac._buffer("modes_change", (B, p)), fac._buffer("modes_status", (B,), torch.int32)
    lib, stream = _cabi.load(), torch.cuda.current_stream(dev).cuda_stream
    R0 = R.clone()

    def ritz():
        R.copy_(R0)                      # (the step rewrites its right-hand sides: every launch starts from the same ones)
        _cabi.check(lib.ops_frame_modes_ritz_f64(B, p, topo.Nn, X.data_ptr(), MX.data_ptr(), R.data_ptr(), Q.data_ptr(), lam.data_ptr(),
                                                 change.data_ptr(), out.status.data_ptr(), status.data_ptr(), stream), "ops_frame_modes_ritz_f64")

    parts = {"resolve": lambda: frames._resolve_launch(fac, p, R0, p * topo.Nn * 3, out), "mass_apply": lambda: _mass_apply(mass, B * p, p, X, MX),
             "ritz_with_copy": ritz, "copy": lambda: R.copy_(R0)}
    us = {k: [] for k in parts}
    for rnd in range(ROUNDS + 1):                     # the first round is the warm-up
        for name, launch in parts.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                launch()
            b.record()
            b.synchronize()
            if rnd:
                us[name].append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    med = {k: statistics.median(v) for k, v in us.items()}
    med["ritz"] = med.pop("ritz_with_copy") - med.pop("copy")
    assert int(status.abs().sum()) == 0
    return {"frame": f"{bays}x{stories}", "B": B, "Nn": topo.Nn, "Ne": topo.Ne, "n_eq": topo.n_eq, "kd": topo.kd, "n_vectors": p,
            "us_per_iteration": {k: round(v, 1) for k, v in med.items()}, "us_per_iteration_total": round(sum(med.values()), 1),
            "us_rounds": {k: [round(t, 1) for t in v] for k, v in us.items()},
            "factor_ms": round(statistics.median(factor_ms[1:]), 3), "to_tol": to_tol, "device": torch.cuda.get_device_name(0)}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--cell"]:
        print("CELL " + json.dumps(cell(*(int(v) for v in args[1:4]))), flush=True)
        return 0
    path = args[args.index("--json") + 1] if "--json" in args else os.path.join(ROOT, "profiles", "frame_modes_timing.json")
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if a.count("x") == 2 and a[0].isdigit()] \
        or [(5, 5, 8192), (10, 10, 4096), (15, 16, 3072)]
    rows, device, rc = [], None, 0
    for bays, stories, B in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(bays), str(stories), str(B)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=CELL_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{bays}x{stories}x{B}: no result within {CELL_LIMIT_S} s; nothing more is started", flush=True)
            rc = 124
            break
        line = [ln for ln in done.stdout.splitlines() if ln.startswith("CELL ")]
        if done.returncode != 0 or not line:
            print(f"{bays}x{stories}x{B}: ended with {done.returncode}; nothing more is started\n{done.stderr[-2000:]}", flush=True)
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
