"""Host-side logic that needs no GPU: the OpenSees-command shim's model recording and result assembly,
the seeded case generator, sharding (including a 2-process gloo run), the reference JSON wire format."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import beam_oracle as bo
from openpystruct_amd import ops, sizing


def setup_model(I_values, node_positions, roller_nodes, force_nodes, force_values, A, E, uniform_udl):
    """Re-typed command sequence of the reference's setup_model (SingleCore.py:89-124), driving the shim."""
    ops.model('basic', '-ndm', 2, '-ndf', 3)
    for i, x in enumerate(node_positions):
        ops.node(i + 1, x, 0.0)
    ops.fix(1, 1, 1, 0)
    for n in roller_nodes:
        ops.fix(n, 0, 1, 0)
    ops.geomTransf('Linear', 1)
    for i in range(len(node_positions) - 1):
        ops.element('elasticBeamColumn', i + 1, i + 1, i + 2, A, E, float(I_values[i]), 1)
    ops.timeSeries('Linear', 1)
    ops.pattern('Plain', 1, 1)
    for n, f in zip(force_nodes, force_values):
        ops.load(n, 0.0, f, 0.0)
    for e in range(1, len(node_positions)):
        ops.eleLoad('-ele', e, '-type', '-beamUniform', uniform_udl, uniform_udl)
    ops.system('BandSPD'); ops.numberer('RCM'); ops.constraints('Plain')
    ops.integrator('LoadControl', 1.0); ops.algorithm('Linear')


def test_shim_records_the_reference_model():
    ops.wipe()
    x = np.linspace(0, 200, 101)
    setup_model(np.full(100, 0.5), x, bo.ROLLERS_REF, [50, 20], [-355857.0, -1e5], bo.A_REF, bo.E_REF, -1000.0)
    a = ops._arrays(ops._dom)
    assert (a["fix"] == bo.reference_fix_mask()).all() and a["fix_x"].sum() == 1 and a["fix_x"][0]
    assert a["Fy"][49] == -355857.0 and a["Fy"][19] == -1e5 and a["Fy"].sum() == -455857.0
    assert (a["wy"] == -1000.0).all() and (a["wx"] == -1000.0).all()     # Wx = Wy quirk, SingleCore.py:117
    assert a["I"].shape == (100,) and (a["E"] == bo.E_REF).all()


def test_shim_result_assembly_matches_3dof_oracle():
    """eleResponse 6-vectors and nodeDisp(n, 1|2|3) assembled from (v, theta, V, M) == OpenSees-like 3-DOF oracle."""
    ops.wipe()
    rng = np.random.default_rng(3)
    x = np.linspace(0, 200, 101)
    I = np.exp(rng.uniform(np.log(3e-3), np.log(0.75), size=100))
    setup_model(I, x, bo.ROLLERS_REF, [50, 20, 77], [-355857.0, -1e5, -5e4], bo.A_REF, bo.E_REF, -1000.0)
    a = ops._arrays(ops._dom)
    v, th, V, M, st = bo.solve_beam_dense(x, bo.E_REF, I, a["fix"], a["Fy"], -1000.0)
    assert ops._finish(ops._dom, a, v, th, V, M, 0) == 0
    d, f, st3, neq, kd = bo.solve_reference_beam_3dof(x, bo.A_REF, bo.E_REF, I, bo.ROLLERS_REF, [50, 20, 77],
                                                      [-355857.0, -1e5, -5e4], -1000.0)
    for e in (1, 2, 37, 100):
        got = np.array(ops.eleResponse(e, 'forces'))
        np.testing.assert_allclose(got, f[e - 1], rtol=2e-7, atol=1e-3)
    for n in (1, 2, 50, 101):
        assert ops.nodeDisp(n, 2) == pytest.approx(d[n - 1, 1], rel=1e-8, abs=1e-15)
        assert ops.nodeDisp(n, 3) == pytest.approx(d[n - 1, 2], rel=1e-8, abs=1e-15)
        assert ops.nodeDisp(n, 1) == pytest.approx(d[n - 1, 0], rel=1e-8, abs=1e-15)
    assert isinstance(ops.eleResponse(1, 'forces'), list) and ops.eleResponse(1, 'forces') is not ops.eleResponse(1, 'forces')


def test_shim_failed_analyze_is_a_code_not_an_exception():
    ops.wipe()
    x = np.linspace(0, 10, 11)
    setup_model(np.full(10, 0.1), x, [11], [5], [-1.0], 0.01, 2e11, 0.0)
    a = ops._arrays(ops._dom)
    rc = ops._finish(ops._dom, a, None, None, None, None, 1)
    assert rc != 0
    with pytest.raises(RuntimeError):
        ops.nodeDisp(1, 2)


def test_shim_rejects_what_is_not_on_the_path():
    ops.wipe()
    with pytest.raises(NotImplementedError):
        ops.model('basic', '-ndm', 3, '-ndf', 6)
    with pytest.raises(NotImplementedError):
        ops.element('truss', 1, 1, 2, 1.0, 1.0)
    with pytest.raises(NotImplementedError):
        ops.eleResponse(1, 'stress')


def test_make_cases_distribution_and_determinism():
    cfg = sizing.SizingConfig()
    a = sizing.make_cases(500, cfg, seed=1)
    b = sizing.make_cases(500, cfg, seed=1)
    assert torch.equal(a.Fy, b.Fy) and a.force_nodes == b.force_nodes
    k = np.array([len(f) for f in a.force_nodes])
    assert k.min() >= 1 and k.max() <= 4 and set(k) == {1, 2, 3, 4}
    vals = np.concatenate([np.array(f) for f in a.force_values])
    assert vals.min() >= cfg.max_force and vals.max() <= cfg.min_force
    forbidden = set(cfg.roller_nodes) | {1, 101}                    # SingleCore.py:63-66: range(2, num_nodes) minus rollers
    assert all(not (set(f) & forbidden) and len(set(f)) == len(f) for f in a.force_nodes)
    assert (a.fix[0].numpy() == bo.reference_fix_mask()).all()
    # Fy is the scatter of the ragged lists
    b0 = np.zeros(101); b0[np.array(a.force_nodes[0]) - 1] = a.force_values[0]
    np.testing.assert_array_equal(a.Fy[0].numpy(), b0)
    # random_bridge = 1 (SingleCore.py:133-151)
    c = sizing.make_cases(200, sizing.SizingConfig(random_bridge=1), seed=2)
    assert float(c.L.min()) >= 15 and float(c.L.max()) <= 215
    nr = np.array([len(r) for r in c.roller_nodes])
    assert all(int(c.fix[b].sum()) == 1 + len(c.roller_nodes[b]) for b in range(200))
    assert nr.min() >= 1 and nr.max() <= 4
    assert all(not (set(f) & set(r)) for f, r in zip(c.force_nodes, c.roller_nodes))


def test_shard_ranges_partition_the_cases():
    for n, w in [(10, 3), (50000, 8), (7, 8), (32, 1)]:
        rs = [sizing.shard_range(n, r, w) for r in range(w)]
        assert rs[0][0] == 0 and rs[-1][1] == n and all(rs[i][1] == rs[i + 1][0] for i in range(w - 1))
    full = sizing.make_cases(64, sizing.SizingConfig(), seed=5)
    lo, hi = sizing.shard_range(64, 1, 4)
    part = full.slice(lo, hi)
    assert torch.equal(part.Fy, full.Fy[lo:hi]) and part.force_nodes == full.force_nodes[lo:hi]


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=120))
    n = 37
    lo, hi = sizing.shard_range(n, rank, world)
    cases = sizing.make_cases(n, sizing.SizingConfig(), seed=9).slice(lo, hi)
    mine = torch.zeros(n, dtype=torch.float64)
    mine[lo:hi] = cases.Fy.sum(dim=1)
    dist.all_reduce(mine)                                  # test-only gather; the data path itself has no collective
    q.put((rank, mine.numpy()))
    dist.destroy_process_group()


def test_two_rank_shards_reassemble_the_global_case_list():
    from tests.helpers import run_ranks
    outs = run_ranks(_gloo_worker, 2, timeout=180)
    ref = sizing.make_cases(37, sizing.SizingConfig(), seed=9).Fy.sum(dim=1).numpy()
    for _, got in outs:
        np.testing.assert_array_equal(got, ref)


def test_reference_json_wire_format(tmp_path):
    cfg = sizing.SizingConfig()
    cases = sizing.make_cases(5, cfg, seed=4)
    B, N = cases.Fy.shape
    xs = cases.node_positions.numpy()
    rec = {
        "roller_x_locations": [[float(xs[b, n - 1]) for n in cases.roller_nodes[b]] for b in range(B)],
        "force_x_locations": [[float(xs[b, n - 1]) for n in cases.force_nodes[b]] for b in range(B)],
        "force_values": cases.force_values,
        "I_values": torch.rand(B, N - 1), "shear_forces": torch.rand(B, N - 1), "bending_moments": torch.rand(B, N - 1),
        "node_positions": cases.node_positions, "roller_nodes": cases.roller_nodes,
        "force_nodes": cases.force_nodes, "num_nodes": N, "L": cases.L,
        "rotations": torch.rand(B, N, dtype=torch.float64), "deflections": torch.rand(B, N, dtype=torch.float64),
        "status": torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32),
    }
    path = str(tmp_path / "training_data_PINN_mini.json")
    kept = sizing.records_to_reference_json(rec, path)
    assert kept == 4                                                     # failed sample dropped (MultiCore.py:265)
    d = json.load(open(path))
    assert tuple(d.keys()) == sizing.RECORD_KEYS                         # SingleCore.py:73-87
    assert all(len(d[k]) == 4 for k in d)
    assert d["roller_x_locations"][0] == [18.0, 58.0, 138.0, 168.0, 198.0]
    assert len(d["I_values"][0]) == 100 and len(d["deflections"][0]) == 101 and d["num_nodes"][0] == 101
    # ... and back: the reader returns the tensor form generate_dataset produces, prepare() accepts both forms alike
    back = sizing.records_from_reference_json(path)
    keep = [0, 1, 3, 4]
    assert torch.equal(back["I_values"], rec["I_values"][keep]) and torch.equal(back["deflections"], rec["deflections"][keep])
    assert back["roller_nodes"].tolist() == [cases.roller_nodes[b] for b in keep] and back["n_forces"].tolist() == [len(cases.force_nodes[b]) for b in keep]
    assert back["force_values"][0, : len(cases.force_values[0])].tolist() == list(cases.force_values[0]) and back["num_nodes"] == N
    binp = str(tmp_path / "records.pt")
    sizing.save_records(back, binp)
    again = sizing.load_records(binp)
    assert all(torch.equal(again[k], back[k]) if torch.is_tensor(back[k]) else again[k] == back[k] for k in back)
    json.dump({"I_values": []}, open(path, "w"))
    with pytest.raises(KeyError):
        sizing.records_from_reference_json(path)


def test_prepare_accepts_json_lists_and_reader_tensors_alike(tmp_path):
    from openpystruct_amd import dataprep
    cfg = sizing.SizingConfig()
    cases = sizing.make_cases(36, cfg, seed=6)
    B, N = cases.Fy.shape
    xs = cases.node_positions.numpy()
    g = torch.Generator().manual_seed(0)
    rec = {
        "roller_x_locations": [[float(xs[b, n - 1]) for n in cases.roller_nodes[b]] for b in range(B)],
        "force_x_locations": [[float(xs[b, n - 1]) for n in cases.force_nodes[b]] for b in range(B)],
        "force_values": cases.force_values, "I_values": torch.rand(B, N - 1, generator=g),
        "shear_forces": torch.rand(B, N - 1, generator=g), "bending_moments": torch.rand(B, N - 1, generator=g),
        "node_positions": cases.node_positions, "roller_nodes": cases.roller_nodes, "force_nodes": cases.force_nodes,
        "num_nodes": N, "L": cases.L, "rotations": torch.rand(B, N, dtype=torch.float64, generator=g),
        "deflections": torch.rand(B, N, dtype=torch.float64, generator=g),
    }
    path = str(tmp_path / "d.json")
    sizing.records_to_reference_json(rec, path)
    as_lists = json.load(open(path))                     # what the reference's scripts hold after json.load
    as_tensors = sizing.records_from_reference_json(path)
    a = dataprep.prepare(as_lists, kind="pinn", seed=3)
    b = dataprep.prepare(as_tensors, kind="pinn", seed=3)
    assert torch.allclose(a.X_train, b.X_train, atol=1e-6) and torch.allclose(a.Y_val, b.Y_val, atol=1e-6)


def test_analysis_object_commands_reject_what_they_cannot_honour():
    """the analysis-object commands are accepted only in the forms that mean 'one linear static solve'."""
    from openpystruct_amd import ops
    ops.numberer('RCM'); ops.constraints('Plain'); ops.integrator('LoadControl', 1.0); ops.algorithm('Linear'); ops.algorithm('Newton')
    ops.system('BandSPD'); ops.system('BandGeneral')
    for bad in (lambda: ops.constraints('Penalty', 1e12, 1e12), lambda: ops.integrator('LoadControl', 0.1),
                lambda: ops.integrator('DisplacementControl', 1, 2, 0.1), lambda: ops.algorithm('BFGS'), lambda: ops.analysis('Transient')):
        with pytest.raises(NotImplementedError):
            bad()
    with pytest.raises(ValueError):
        ops.system('Mumps')


def test_runtime_helpers_on_the_cpu(monkeypatch):
    """openpystruct_amd/runtime.py: importing the package leaves the environment alone (r05); `configure()` -- what entry points call --
    sets the HIP graph environment default without overriding a user's choice and reports what it did; the usable core count honours
    affinity and quota; the throttle counters are a dict (empty where cgroup v2 is not mounted)."""
    import os
    import subprocess
    import sys
    from openpystruct_amd import runtime
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != runtime.PACKET_CAPTURE_ENV}
    code = ("import os, openpystruct_amd; from openpystruct_amd import runtime; a = os.environ.get(runtime.PACKET_CAPTURE_ENV); "
            "r = runtime.configure(cpu_threads=False); print(a, os.environ.get(runtime.PACKET_CAPTURE_ENV), r['graph_env_too_late'], r['hip_runtime'])")
    out = subprocess.check_output([sys.executable, "-c", code], env=env, cwd=root, text=True).split()
    assert out[:3] == ["None", "0", "False"] and out[3] != ""          # the import set nothing; configure() did
    monkeypatch.setenv(runtime.PACKET_CAPTURE_ENV, "1")
    rec = runtime.configure(cpu_threads=False)
    assert os.environ[runtime.PACKET_CAPTURE_ENV] == "1" and rec["packet_capture_env"] == "1"      # setdefault: a user's value stays
    n = runtime.usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)
    c = runtime.cpu_throttle_counters()
    assert isinstance(c, dict) and all(isinstance(v, int) for v in c.values())
    import torch
    old = torch.get_num_threads()
    try:
        assert 1 <= runtime.fit_cpu_threads() <= max(1, n)
    finally:
        torch.set_num_threads(old)


def test_frame_equation_numbering_candidates_on_the_host():
    """frames.FrameTopology(numbering=...): every numbering is a permutation of the free DOFs that keeps a node's DOFs together; "auto"
    takes the narrowest of node order / reverse Cuthill-McKee / the two coordinate sweeps (node order on a tie) -- the reference asks
    OpenSees for numberer('RCM') (FR:135).  No GPU involved: the kernels take whatever elem_eq / node_eq they are given."""
    from openpystruct_amd import frames
    for bays, stories, kd_node, kd_auto in [(10, 10, 35, 32), (15, 16, 50, 50), (10, 2, 35, 8), (21, 3, 68, 11), (3, 10, 14, 14), (1, 1, 5, 5)]:
        auto = frames.grid_frame(bays, stories, device="cpu")
        node = frames.grid_frame(bays, stories, device="cpu", numbering="node")
        rcm = frames.grid_frame(bays, stories, device="cpu", numbering="rcm")
        assert (node.kd, auto.kd) == (kd_node, kd_auto) and rcm.kd <= kd_node + 3 and node.numbering == "node"
        assert (auto.numbering == "node") == (kd_auto == kd_node)
        for t in (auto, node, rcm):
            eq = t.d_node_eq.numpy()
            free = eq[eq >= 0]
            assert sorted(free.tolist()) == list(range(t.n_eq)) and t.n_eq == 3 * (bays + 1) * stories
            assert (eq[t.fix3] == -1).all()
            live = eq[(eq >= 0).all(axis=1)]
            assert (np.diff(live, axis=1) == 1).all()                     # a node's three equations are consecutive
            span = max(int(q[q >= 0].max() - q[q >= 0].min()) for q in t.d_elem_eq.numpy() if (q >= 0).any())
            assert span == t.kd
    # a frame in two disconnected pieces + a fully fixed node: every free node is numbered exactly once
    coords = np.array([(0, 0), (0, 3), (6, 3), (20, 0), (20, 3), (26, 3), (40, 0)], dtype=float)
    conn = np.array([(0, 1), (1, 2), (3, 4), (4, 5)])
    fix3 = np.zeros((7, 3), dtype=bool); fix3[0] = fix3[3] = fix3[6] = True
    order = frames.rcm_node_order(7, conn, ~fix3.all(axis=1))
    assert sorted(order.tolist()) == list(range(7)) and set(order[-3:].tolist()) == {0, 3, 6}
    with pytest.raises(ValueError):
        frames.grid_frame(2, 2, device="cpu", numbering="minimum-degree")


def test_marginal_stop_decisions_helper():
    """tests/helpers.py: the rule that replaced "+- 3 epochs" -- a stop may move by up to `patience` epochs only where the reference's own
    loss history holds a decision within float32 round-off of its threshold."""
    from tests.helpers import assert_stop_epochs_agree, marginal_stop_decisions
    tol = 5e-3
    clear = [10.0 - 0.1 * k for k in range(30)] + [7.1] * 6            # every decision far from the threshold
    assert marginal_stop_decisions(clear, tol) == []
    assert assert_stop_epochs_agree(36, 36, clear, tol, 5) is True
    with pytest.raises(AssertionError):
        assert_stop_epochs_agree(34, 36, clear, tol, 5)                 # two epochs off without a marginal decision: a real difference
    hug = [100.0, 99.0, 99.0 - tol - 1e-5, 98.9, 98.9, 98.9, 98.9, 98.9]   # epoch 3 improves on 99.0 by tol + 1e-5: inside 2e-6 * |loss|
    assert marginal_stop_decisions(hug, tol) == [3]
    assert assert_stop_epochs_agree(6, 8, hug, tol, 5) is False          # allowed: within patience of a run with a marginal decision
    with pytest.raises(AssertionError):
        assert_stop_epochs_agree(1, 8, hug, tol, 5)                     # ... but not further than `patience`


def test_bench_protocol_is_frozen():
    """the untimed prelude in front of the 0.23 ms headline region (40 ms of a copy kernel + 60 ms of the region's own launches)
    is a steady-state protocol that must not grow again, `roofline.frac` is the HBM-resident figure, and the metric's epoch time is the mean."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    src = open(spec.origin).read()
    ns = {}
    for name in ("CHIP_WARM_MS", "OWN_LOAD_WARM_MS"):
        line = [ln for ln in src.splitlines() if ln.startswith(name + " = ")][0]
        ns[name] = float(line.split("=")[1].split("#")[0])
    assert ns["CHIP_WARM_MS"] <= 40.0 and ns["OWN_LOAD_WARM_MS"] <= 60.0
    assert 'rl["achieved"], rl["frac"], rl["kernel_us"] = extras["cold"]["achieved"], extras["cold"]["frac"], extras["cold"]["kernel_us"]' in src
    assert '"epoch_stat": "mean of the epochs after the first"' in src


def test_configure_makes_no_hip_call():
    """runtime.configure() is the call an entry point makes BEFORE its first HIP call (and before bench.py forks its CPU pool): it may
    not initialise the runtime itself."""
    from openpystruct_amd import runtime
    import inspect
    body = "\n".join(ln.split("#")[0] for ln in inspect.getsource(runtime.configure).split('"""')[2].splitlines())     # code: no docstring, no comments
    assert "is_available(" not in body and "device_count(" not in body and "hip_runtime_version(query_runtime=False)" in body
    assert runtime.hip_runtime_version(query_runtime=False) == str(torch.version.hip)


def test_switch_registry():
    """r06: the A/B switches of the fused training pieces are entries of ONE registry (openpystruct_amd/switches.py), not ~50 environment variables:
    unknown names raise, `set` returns the previous value, OPS_AMD_SWITCHES is parsed at import (checked in a child process)."""
    import subprocess
    import sys
    from openpystruct_amd import switches
    assert switches.get("fused_prep") == "1" and switches.on("tfd_front") and switches.get("split_wgrad_rows") == "16"
    old = switches.set("fused_prep", 0)
    try:
        assert old == "1" and switches.get("fused_prep") == "0" and switches.snapshot() == {"fused_prep": "0"}
    finally:
        switches.set("fused_prep", old)
    assert switches.snapshot() == {}
    with pytest.raises(KeyError):
        switches.get("fused_perp")
    with pytest.raises(KeyError):
        switches.set("no_such_switch", 1)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from openpystruct_amd import switches; print(sorted(switches.snapshot().items()))"
    p = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, OPS_AMD_SWITCHES="pinn_norm_fold=0, tfd_head=0;val_whole"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[('pinn_norm_fold', '0'), ('tfd_head', '0')]", p.stdout + p.stderr
    p = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, OPS_AMD_SWITCHES="tpyo=0"), capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "unknown switch" in p.stderr


def test_flat_grads_makes_every_grad_a_view_of_one_zeroed_buffer():
    """flat_adam.flat_grads: every `.grad` a view at the running offset, in parameter order; autograd accumulates into the views in place."""
    from openpystruct_amd import flat_adam
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    params = list(model.parameters())
    flat = flat_adam.flat_grads(model.parameters(), "cpu")          # (a generator is as good as a list)
    assert flat.dtype == torch.float32 and flat.shape == (sum(q.numel() for q in params),) == (3 * 4 + 4 + 4 * 2 + 2,) and not flat.any()
    for q, off in zip(params, np.cumsum([0] + [q.numel() for q in params])):
        assert q.grad.shape == q.shape and q.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        assert q.grad.data_ptr() == flat.data_ptr() + 4 * int(off)
    ptrs = [q.grad.data_ptr() for q in params]
    model(torch.randn(5, 3)).square().sum().backward()
    assert [q.grad.data_ptr() for q in params] == ptrs and all(q.grad.any() for q in params) and flat.any()
