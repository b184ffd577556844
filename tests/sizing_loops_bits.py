"""The cases behind tests/golden/sizing_loops_parent_bits.npz (test code only): seeded inputs and one function, `run_all`, that goes
through the public entry points of the five sizing loops, their dataset generators and the gradient entries beside them on the GPU
and returns every output as raw bits.  tests/golden/make_sizing_loops_parent_bits.py records them, tests/test_gpu_sizing_loops_bits.py
compares a later build with the record: restating the host side of the loops (optimiser state, step-size table, loop driver, checks)
changes no launch, so no output may move by a bit.

Every array is keyed "<name>.<dtype>" ("I.f4", "epochs.i4"), so the reader knows which bits are floats (NaNs compare as NaN-ness).
Every loop case holds "epochs" (or a generator's "epochs_run"), and `loop_condition` states what the recorder asserts of them: rows
stop at different epochs, one of them before a poll the loop went past -- the freeze of finished rows and the poll are then part of
what is compared.  Small on purpose: 6 beams of 20 elements, 3 designs x 2 load cases, 4 frames of a 2 x 2 grid, POLL = 5 epochs per
poll and a number of epochs that is no multiple of it."""
import dataclasses

import numpy as np

SEED = 20261021
POLL = 5
DEV = "cuda"
# beams: 21 nodes, rollers inside 2..21; the loss starts near sum(I_0) = 10 and falls by about lr * Ne * gamma^t per epoch, so an early
# stop on "improved by less than `tolerance`" inside a few tens of epochs takes a tolerance of that size
BEAM = dict(num_nodes=21, roller_nodes=(5, 11, 17), max_e=32, tolerance=0.17, patience=2)
BEAM_TOTAL = dict(alpha_deflection=100.0, deflection_limit=0.01)
N_BEAMS, G, C = 6, 3, 2
WEIGHTS = (0.75, 1.5)
# frames: grid_frame(2, 2); every row starts from its own inertias, a factor 2 apart from row to row, and the tolerance of a case is
# of the size of its loss's improvement per epoch somewhere inside the run
FRAME = dict(patience=2)
FRAME_TOLERANCE = {"frames_explicit": 1.0, "frames_total_sway": 0.1, "frames_total_loads": 0.1, "frame_designs_shared_sum": 0.1,
                   "frame_designs_own_max": 0.1, "frame_groups": 0.1}
FRAME_EPOCHS, N_FRAMES = 32, 4
SWAY = dict(alpha_sway=1.0, sway_limit=1e-4)
CATALOGUE = (1e-4, 3e-4, 6e-4, 1.2e-3)
BEAM_STATE = ("I", "exp_avg", "exp_avg_sq", "best_loss", "last_loss", "patience_cnt", "epochs_run", "active", "V32", "M32", "I64")
DESIGN_STATE = BEAM_STATE[:-1] + ("case_penalty", "governing", "I64_rows", "active_rows")
CODES = {"float32": "f4", "float64": "f8", "int32": "i4", "int64": "i8", "uint8": "u1", "bool": "b1"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def put(out, name, v):
    """`v` (a tensor, an array or a number) into `out` as raw bits under "<name>.<dtype>"."""
    a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    out[f"{name}.{CODES[a.dtype.name]}"] = bits(a.reshape(-1) if a.ndim == 0 else a)


def floats(key, z):
    """The array of key "<name>.<dtype>" as floats, or None for an integer array."""
    code = key.rsplit(".", 1)[1]
    return z.view({"f4": np.float32, "f8": np.float64}[code]) if code[0] == "f" else None


def epochs_of(arrays):
    key = "epochs.i4" if "epochs.i4" in arrays else "epochs_run.i4"
    return arrays[key].view(np.int32)


def loop_condition(arrays):
    """(rows stop at >= 2 distinct epochs, one row stopped at or before a poll that found another row still active)."""
    ep = epochs_of(arrays)
    poll = (int(ep.max()) - 1) // POLL * POLL          # the last poll before the last row stopped
    return len(np.unique(ep)) >= 2, poll >= POLL and int(ep.min()) <= poll


def _solution(out, sol, prefix="sol_"):
    for k, t in zip(type(sol)._fields, sol):
        put(out, prefix + k, t)


# ---------------------------------------------------------------------------------------------------------------------
# beams
# ---------------------------------------------------------------------------------------------------------------------
def beam_cfg(**kw):
    from openpystruct_amd import sizing
    return sizing.SizingConfig(**{**BEAM, **kw})


def _beam_state(st, names):
    out = {}
    for k in names:
        put(out, "epochs" if k == "epochs_run" else k, getattr(st, k))
    _solution(out, st.sol)
    if hasattr(st, "loss_history"):
        put(out, "loss_history", st.loss_history)
    return out


def _beam_runs(torch):
    from openpystruct_amd import multicase, sizing
    cfg = beam_cfg()
    cases = [sizing.make_cases(N_BEAMS, cfg, SEED + s, device=DEV) for s in (0, 1)]
    got = {}
    fused_was = sizing._FUSED_EPOCH
    try:
        for mode, fused, kw in (("fused", True, {}), ("separate", False, {}), ("total", True, dict(gradient="total", **BEAM_TOTAL))):
            sizing._FUSED_EPOCH = fused
            sizing._EPOCH_GRAPHS.clear()
            got[f"beam_{mode}_graph"] = _beam_state(sizing.optimize_cases(cases[0], cfg, DEV, poll_every=POLL, use_graph=True, **kw), BEAM_STATE)
            got[f"beam_{mode}_record"] = _beam_state(sizing.optimize_cases(cases[0], cfg, DEV, poll_every=POLL, record_loss=True, **kw), BEAM_STATE)
            for s in (0, 1):          # the second shard runs on the first one's state, re-armed in place
                got[f"beam_{mode}_reuse{s}"] = _beam_state(sizing.optimize_cases(cases[s], cfg, DEV, poll_every=POLL, reuse=True, **kw), BEAM_STATE)
            sizing._EPOCH_GRAPHS.clear()
    finally:
        sizing._FUSED_EPOCH = fused_was
    designs = multicase.make_design_cases(G, C, cfg, SEED + 2, device=DEV)
    for mode, kw in (("sum", dict(aggregate="sum", weights=WEIGHTS, **BEAM_TOTAL)), ("max", dict(aggregate="max"))):
        got[f"designs_{mode}_graph"] = _beam_state(multicase.optimize_designs(designs, cfg, DEV, C, poll_every=POLL, **kw), DESIGN_STATE)
        got[f"designs_{mode}_record"] = _beam_state(multicase.optimize_designs(designs, cfg, DEV, C, poll_every=POLL, record_loss=True, **kw), DESIGN_STATE)
    for name, zero in (("dataset", False), ("dataset_zero_last", True)):
        rec = sizing.generate_dataset(N_BEAMS, beam_cfg(zero_last_node=zero), DEV, seed=SEED + 3, poll_every=POLL)
        got[name] = {}
        for k, v in rec.items():
            put(got[name], k, v)
    sizing._EPOCH_GRAPHS.clear()
    rec = multicase.generate_multicase_dataset(G, C, beam_cfg(zero_last_node=True), DEV, seed=SEED + 4, aggregate="sum", weights=WEIGHTS, poll_every=POLL)
    got["dataset_multicase"] = {}
    for k, v in rec.items():
        put(got["dataset_multicase"], k, v)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
def frame_inputs(topo, torch):
    """Seeded starts and loads of the frame cases, on the topology's device."""
    from openpystruct_amd import frame_groups, frames
    rng = np.random.default_rng(SEED)
    dev = topo.device
    u = lambda *shape: torch.as_tensor(rng.uniform(0.5, 2.0, size=shape), device=dev)      # noqa: E731
    start = lambda rows, cols: (2.5e-4 * u(rows, cols) * 2.0 ** torch.arange(rows, device=dev)[:, None]).float()      # noqa: E731
    x = dict(I0=start(N_FRAMES, topo.Ne), I0_designs=start(G, topo.Ne))
    x["loads_frames"], x["w_frames"] = frames.grid_load_cases(topo, 1e4 * u(N_FRAMES), -1e4 * u(N_FRAMES))
    loads, w = frames.grid_load_cases(topo, 1e4 * u(G * C), -1e4 * u(G * C))
    x["loads"], x["w"] = loads.reshape(G, C, topo.Nn, 3), w.reshape(G, C, topo.Ne, 2)
    x["groups"] = frame_groups.story_groups(topo)
    x["X0"] = start(G, int(x["groups"].max()) + 1)
    return x


def _frame_loop(I, sol, epochs, hist, torch):
    out = {}
    put(out, "I", I)
    put(out, "epochs", epochs)
    _solution(out, sol)
    put(out, "loss_history", torch.stack(hist))
    return out


def _designs(r, hist, torch):
    out = {}
    for k in type(r)._fields:
        v = getattr(r, k)
        if k == "solution":
            _solution(out, v)
        elif k == "discrete":
            for kk, vv in v._asdict().items():
                put(out, "discrete_" + kk, vv)
        else:
            put(out, k, v)
    put(out, "loss_history", torch.stack(hist))
    return out


def _frame_runs(torch):
    import openpystruct_amd as oa
    from openpystruct_amd import frame_groups, frames
    cfg = dataclasses.replace(frames.FrameConfig(), **FRAME)
    topo = frames.grid_frame(2, 2, cfg, device=DEV)
    x = frame_inputs(topo, torch)
    loop = lambda case: dict(cfg=dataclasses.replace(cfg, tolerance=FRAME_TOLERANCE[case]), max_epochs=FRAME_EPOCHS, poll_every=POLL)      # noqa: E731
    got = {}
    for name, kw in (("explicit", {}), ("total_sway", dict(gradient="total", **SWAY)),
                     ("total_loads", dict(gradient="total", loads=x["loads_frames"], element_loads=x["w_frames"]))):
        hist = []
        I, sol, ep = frames.optimize_frames(topo, N_FRAMES, I0=x["I0"], loss_history=hist, **loop("frames_" + name), **kw)
        got["frames_" + name] = _frame_loop(I, sol, ep, hist, torch)
    for name, args, kw in (("shared_sum", (x["loads"][0],), dict(n_designs=G, aggregate="sum", weights=WEIGHTS, **SWAY)),
                           ("own_max", (x["loads"], x["w"]), dict(aggregate="max"))):
        hist = []
        r = oa.optimize_frame_designs(topo, *args, I0=x["I0_designs"], loss_history=hist, **loop("frame_designs_" + name), **kw)
        got["frame_designs_" + name] = _designs(r, hist, torch)
    hist = []
    r = oa.optimize_grouped_frame_designs(topo, x["groups"], x["loads"], x["w"], X0=x["X0"], catalogue=CATALOGUE, aggregate="sum",
                                          weights=WEIGHTS, loss_history=hist, **loop("frame_groups"), **SWAY)
    got["frame_groups"] = _designs(r, hist, torch)
    # the gradient entries and the evaluation on one factor / re-solve each (the grouped one on I = X[:, groups])
    mg = frame_groups.member_groups(topo, x["groups"])
    objective = dict(aggregate="sum", weights=WEIGHTS, **SWAY)
    for name, I64 in (("design", x["I0_designs"].double()), ("group", mg.expand(x["X0"]).double())):
        factor = frames.frame_factor(topo, I64)
        sol = frames.frame_resolve(factor, x["loads"], x["w"])
        if name == "design":
            grad, extra, gov = oa.frame_design_gradient(factor, sol, cfg, **objective)
        else:
            grad, extra, gov = oa.frame_group_gradient(factor, sol, x["groups"], cfg, **objective)
        out = got[f"frame_{name}_gradient"] = {}
        put(out, "grad", grad)
        put(out, "loss_extra", extra)
        put(out, "governing", gov)
    for name, kw in (("sum", objective), ("max", dict(aggregate="max"))):
        ev = oa.evaluate_frame_designs(topo, x["I0_designs"], x["loads"], x["w"], cfg=cfg, **kw)
        out = got["frame_evaluate_" + name] = {}
        for k in ("value", "case_penalty", "governing", "status"):
            put(out, k, getattr(ev, k))
        _solution(out, ev.solution)
    torch.cuda.synchronize()
    return got


NOT_LOOPS = ("frame_design_gradient", "frame_group_gradient", "frame_evaluate_sum", "frame_evaluate_max")


def run_all():
    """Every case on the GPU: {case: {"<array>.<dtype>": raw bits}}."""
    import torch
    return {**_beam_runs(torch), **_frame_runs(torch)}
