#!/usr/bin/env python3
"""What the design-objective term costs, on one GPU:

    python scripts/design_loss_time.py [--designs 5120] [--epochs 6] [--json PATH]

  term    the term alone at 512 samples x 6 load cases x 100 elements (the reference bridge): its four launches eagerly, and as one
          replayed graph; per launch, the device time between events around each of the four
  step    a Transformer-Diffusion training step at batch 512 with the term (`train.DesignTerm`) and without it -- the step without
          it is existing code -- on the same `generate_multicase_dataset` set, both in this run, three rounds alternating the two;
          the epoch time (training steps and the validation pass, the first epoch of a run excluded) over the steps per epoch

Host clock around work that ends in a device synchronise; a measurement, not a target.  Writes profiles/design_loss_timing.json."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, C = 512, 6


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def term_alone(torch, cfg, rec, fix, data):
    from openpystruct_amd import _cabi, design_loss, runtime
    dev = torch.device("cuda", 0)
    Ne = cfg.num_elements
    Fy = data.Fy_cases_train[:B].contiguous()
    sI = data.scalers_Y["I"]
    preds = data.Y_train[:B, :Ne].contiguous() + 0.05 * torch.randn((B, Ne), device=dev)     # standardised labels, perturbed
    spec = design_loss._term_spec(dev, Ne, sI, None, Fy, rec["node_positions"][0].double(), torch.tensor(cfg.E, dtype=torch.float64, device=dev),
                                  fix, torch.tensor(cfg.uniform_udl, dtype=torch.float64, device=dev), cfg, 1.0, "sum", None, 0.0, None,
                                  None, None)
    run = lambda: design_loss._term_launches(preds, spec)      # noqa: E731
    for _ in range(10):
        o = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.value))

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    n = max(50, min(20000, int(0.5e6 / window(run, 50))))
    eager = [window(run, n) for _ in range(3)]
    graph, _ = runtime.capture_graph(torch.cuda.Stream(device=dev), dev, run, 2)
    graph.replay()
    n = max(50, min(50000, int(0.5e6 / window(graph.replay, 50))))
    replay = [window(graph.replay, n) for _ in range(3)]
    # the four launches, one by one, between device events (their order is the term's; each on the buffers of the last eager call)
    lib, hp = _cabi.load(), cfg.c_params()
    from openpystruct_amd.beam import beam_solve
    from openpystruct_amd.sizing import _beam_sizing_grad_launch, sizing_tiling
    import ctypes
    sol, grad, _, gstatus = o.keep[:4]
    x, E, fx, wy = spec[4], spec[5], spec[6], spec[7]
    obj = _cabi.SizingObjective(alpha_deflection=0.0, deflection_limit=0.0)
    a = _cabi.DesignLossArgs(B=B, C=C, Ne=Ne, G=B, ldp=Ne, preds=preds.data_ptr(), I_scale=o.keep[4].data_ptr(), I_mean=o.keep[5].data_ptr(),
                             I_min=1e-8, weight=1.0, Fy_src=Fy.data_ptr(), I_rows=o.I_rows.data_ptr(), Fy_rows=o.Fy_rows.data_ptr(),
                             V=sol.V.data_ptr(), M=sol.M.data_ptr(), grad=grad.data_ptr(), status_solve=sol.status.data_ptr(),
                             status_grad=gstatus.data_ptr(), sample_loss=o.sample_loss.data_ptr(), gI=o.gI.data_ptr(),
                             dpreds=o.dpreds.data_ptr(), part=o.part.data_ptr(), value=o.value.data_ptr())
    s = lambda: torch.cuda.current_stream(dev).cuda_stream      # noqa: E731
    launches = {
        "prep": lambda: _cabi.check(lib.ops_design_loss_prep(ctypes.byref(a), s()), "prep"),
        "solve": lambda: beam_solve(x, E, o.I_rows, fx, o.Fy_rows, wy, tiling=sizing_tiling(Ne + 1), out=sol),
        "grad": lambda: _beam_sizing_grad_launch(x, E, o.I_rows, fx, wy, sol, hp, obj, None, grad, None, gstatus),
        "finish": lambda: _cabi.check(lib.ops_design_loss_finish(ctypes.byref(a), ctypes.byref(hp), s()), "finish"),
    }
    per = {}
    for name, fn in launches.items():
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(200):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        per[name] = round(ev[0].elapsed_time(ev[1]) / 200 * 1e3, 2)
    return {"samples": B, "cases": C, "elements": Ne, "beam_rows": B * C, "eager_us": [round(t, 1) for t in eager],
            "graph_replay_us": [round(t, 1) for t in replay], "back_to_back_us_per_launch": per,
            "note": "back_to_back: 200 enqueues of one launch between two device events (host enqueue time included where it is the longer)"}


def main():
    import torch
    from openpystruct_amd import dataprep, multicase, runtime, sizing, train
    runtime.configure()
    if not torch.cuda.is_available():
        raise SystemExit("design_loss_time.py measures on a GPU: none is visible")
    dev = torch.device("cuda", 0)
    cfg = sizing.SizingConfig(max_e=40)
    designs, epochs = arg("--designs", 5120), arg("--epochs", 6)
    path = arg("--json", os.path.join(ROOT, "profiles", "design_loss_timing.json"))
    t0 = time.perf_counter()
    rec = multicase.generate_multicase_dataset(designs, C, cfg, dev, seed=5)
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    fix = sizing.make_cases(1, cfg, seed=5, device="cpu").fix[0]
    data = dataprep.prepare(rec, kind="tfd", n_cases=C, seed=0, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "designs": designs, "dataset_s": round(gen_s, 2),
           "term": term_alone(torch, cfg, rec, fix, data)}
    print(json.dumps(out["term"]), flush=True)
    term = train.DesignTerm(weight=0.1, x=rec["node_positions"][0].double().cpu(), E=cfg.E, fix=fix, wy=cfg.uniform_udl, hp=cfg)
    tcfg = train.TfdConfig(n_cases=C, batch_size=B)
    legs = {"without": None, "with_term": term}
    per_step = {k: [] for k in legs}
    steps = None
    for _ in range(3):
        for name, phys in legs.items():
            r = train.train_surrogate("tfd", data, tcfg, device=dev, max_epochs=epochs, seed=1, physics=phys)
            ep, steps = r["history"]["epoch_s"][1:], r["steps_per_epoch"]
            per_step[name].append(statistics.median(ep) / steps * 1e6)
            assert all(v == v for v in r["history"]["train"])
    med = {k: statistics.median(v) for k, v in per_step.items()}
    out["step"] = {"batch": B, "cases": C, "steps_per_epoch": steps, "epochs_per_run": epochs,
                   "epoch_us_per_step_rounds": {k: [round(t, 1) for t in v] for k, v in per_step.items()},
                   "epoch_us_per_step": {k: round(v, 1) for k, v in med.items()},
                   "term_adds_us_per_step": round(med["with_term"] - med["without"], 1),
                   "note": "epoch time (training steps + the validation pass) over the steps per epoch, median over the epochs after the first"}
    print(json.dumps(out["step"]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
