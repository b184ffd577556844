#!/usr/bin/env python3
"""Time per epoch of the frame sizing loop in its three forms, on one GPU, at sizes a user would run:

  explicit   frames.optimize_frames(gradient="explicit"): the reference's loop (one solve + the step), unchanged by the "total" mode
  total      frames.optimize_frames(gradient="total"): solve, adjoint right-hand side, adjoint solve, gradient, step
  unfused    the same mathematics glued from public pieces: torch elementwise operations form gV, gM, g_disp, the explicit part and
             the hinge sum, frames.frame_solve_vjp does the adjoint (its two streaming kernels read the cotangents from memory)

    python scripts/frame_sizing_total_epoch_time.py [bays x stories x B ...] [--json PATH]

Every form runs with both displacement penalties on (except explicit, which cannot see them) and with early stopping disabled
(patience beyond the epoch count), so every epoch does the same work.  Per shape: one warm-up run of each form, a short run to size
the timed window to about a second, then three rounds alternating the forms; the median and the spread of the rounds are printed.
Host clock around a loop that ends in a device synchronise."""
import ctypes
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openpystruct_amd import _cabi, frames  # noqa: E402

PENALTY = dict(alpha_sway=1.0, sway_limit=1e-3, alpha_deflection=1.0, deflection_limit=1e-4)


def unfused_epochs(topo, B, cfg, n):
    """n epochs of the "total" loop without csrc/frame_sizing_grad.hip: what a user could write before it existed."""
    lib, dev, Ne = _cabi.load(), topo.device, topo.Ne
    f32 = dict(dtype=torch.float32, device=dev)
    I = torch.full((B, Ne), cfg.I0, **f32)
    I64 = I.double()
    ea, es = torch.zeros((B, Ne), **f32), torch.zeros((B, Ne), **f32)
    best, last = torch.full((B,), float("inf"), **f32), torch.zeros((B,), **f32)
    cnt, ep = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(2))
    active = torch.ones((B,), dtype=torch.uint8, device=dev)
    hp = frames._sizing_params(cfg, n)
    aS, sl, aD, dl = PENALTY["alpha_sway"], PENALTY["sway_limit"], PENALTY["alpha_deflection"], PENALTY["deflection_limit"]
    sol = None
    for _ in range(n):
        sol = frames.frame_solve(topo, I64, out=sol)
        den = 2.0 * cfg.E * I64 + 1e-8
        qV = sol.V / (cfg.G * cfg.k * torch.sqrt(I64))
        gM, gV = 2.0 * cfg.alpha_moment * sol.M / den, 2.0 * cfg.alpha_shear * qV
        explicit = 1.0 - cfg.alpha_moment * 2.0 * cfg.E * (sol.M / den) ** 2 - cfg.alpha_shear * 0.5 * sol.V * qV / I64
        ux, uy = sol.disp[..., 0], sol.disp[..., 1]
        ex, ey = torch.clamp(ux.abs() - sl, min=0.0), torch.clamp(uy.abs() - dl, min=0.0)
        g_disp = torch.zeros_like(sol.disp)
        g_disp[..., 0] = 2.0 * aS * ex * torch.sign(ux) / sl ** 2
        g_disp[..., 1] = 2.0 * aD * ey * torch.sign(uy) / dl ** 2
        extra = aS * ((ex / sl) ** 2).sum(-1) + aD * ((ey / dl) ** 2).sum(-1)
        gI, _, _ = frames.frame_solve_vjp(topo, I64, sol.disp, g_disp=g_disp, gV=gV, gM=gM, status=sol.status)
        grad = explicit + gI
        with torch.cuda.device(dev):
            rc = lib.ops_beam_sizing_step_grad_f32(B, Ne, I.data_ptr(), I64.data_ptr(), sol.V.data_ptr(), sol.M.data_ptr(), grad.data_ptr(),
                                                   extra.data_ptr(), ea.data_ptr(), es.data_ptr(), best.data_ptr(), cnt.data_ptr(),
                                                   ep.data_ptr(), active.data_ptr(), last.data_ptr(), None, None, ctypes.byref(hp), None,
                                                   torch.cuda.current_stream(dev).cuda_stream)
        _cabi.check(rc, "ops_beam_sizing_step_grad_f32")
    torch.cuda.synchronize(dev)
    return I


def main():
    args = sys.argv[1:]
    path = args[args.index("--json") + 1] if "--json" in args else None
    shapes = [tuple(int(v) for v in a.split("x")) for a in args if "x" in a and not a.startswith("-") and a != path] or [(3, 3, 65536), (10, 10, 16384)]
    cfg = dataclasses.replace(frames.FrameConfig(), patience=10 ** 6)
    forms = {"explicit": lambda topo, B, n: frames.optimize_frames(topo, B, cfg, max_epochs=n, poll_every=10 ** 9),
             "total": lambda topo, B, n: frames.optimize_frames(topo, B, cfg, max_epochs=n, poll_every=10 ** 9, gradient="total", **PENALTY),
             "unfused": lambda topo, B, n: unfused_epochs(topo, B, cfg, n)}
    rows = []
    for bays, stories, B in shapes:
        topo = frames.grid_frame(bays, stories)
        epochs = {}
        for name, run in forms.items():
            run(topo, B, 5)                              # warm: library, plans, workspaces, the allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(topo, B, 10)
            epochs[name] = max(20, min(4000, int(10 / (time.perf_counter() - t0))))      # about a second per timed window
        times = {name: [] for name in forms}
        for _ in range(3):
            for name, run in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(topo, B, epochs[name])
                times[name].append((time.perf_counter() - t0) / epochs[name] * 1e6)
        row = {"frame": f"{bays}x{stories}", "B": B, "Nn": topo.Nn, "Ne": topo.Ne, "kd": topo.kd, "epochs_per_window": epochs,
               "us_per_epoch": {k: round(statistics.median(v), 1) for k, v in times.items()},
               "us_per_epoch_rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
        m = row["us_per_epoch"]
        row["total_over_explicit"] = round(m["total"] / m["explicit"], 3)
        row["unfused_over_total"] = round(m["unfused"] / m["total"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
