"""What `dataprep.prepare` hands the design-objective term: the dense nodal loads of every load case of a group,
for any n_cases, next to the unchanged per-case fields; and what `train._check_shared_bridge` refuses."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def records(G, C, N, rng, as_lists=False, random_bridge=False):
    R, F = G * C, 4
    n_f = rng.integers(1, F + 1, size=R)
    nodes = np.zeros((R, F), dtype=np.int64)
    vals = np.zeros((R, F))
    for r in range(R):
        nodes[r, :n_f[r]] = rng.choice(np.arange(2, N), size=n_f[r], replace=False)
        vals[r, :n_f[r]] = rng.uniform(-3e5, -3e4, size=n_f[r])
    xs = np.tile(np.linspace(0, 200, N), (R, 1))
    if random_bridge:
        xs = xs * rng.uniform(0.5, 1.0, size=(R, 1))
    rec = {"roller_x_locations": torch.as_tensor(np.tile([20.0, 90.0, 200.0], (R, 1))),
           "force_x_locations": torch.as_tensor(np.where(nodes > 0, xs[np.arange(R)[:, None], np.maximum(nodes - 1, 0)], 0.0)),
           "force_values": torch.as_tensor(vals), "node_positions": torch.as_tensor(xs),
           "I_values": torch.as_tensor(np.repeat(rng.uniform(0.1, 0.5, size=(G, N - 1)), C, axis=0).astype(np.float32)),
           "deflections": torch.as_tensor(rng.standard_normal((R, N))), "rotations": torch.as_tensor(rng.standard_normal((R, N))),
           "force_nodes": torch.as_tensor(nodes), "num_nodes": N}
    if as_lists:
        rec["force_nodes"] = [nodes[r, :n_f[r]].tolist() for r in range(R)]
        rec["force_values"] = [vals[r, :n_f[r]].tolist() for r in range(R)]
    dense = np.zeros((R, N))
    for r in range(R):
        for n, f in zip(nodes[r, :n_f[r]], vals[r, :n_f[r]]):
            dense[r, n - 1] += f
    return rec, dense.reshape(G, C, N)


@pytest.mark.parametrize("as_lists", [False, True])
@pytest.mark.parametrize("kind", ["tfd", "fnn"])
def test_the_grouped_loads_are_the_scatter_of_the_grouped_records(kind, as_lists):
    from openpystruct_amd import dataprep
    G, C, N = 10, 3, 13
    rec, dense = records(G, C, N, np.random.default_rng(7), as_lists)
    perm = torch.as_tensor(np.random.default_rng(1).permutation(G))
    d = dataprep.prepare(rec, kind=kind, n_cases=C, perm=perm, train_split=0.8)
    assert d.Fy_cases_train.dtype == torch.float64 and d.Fy_cases_train.is_contiguous() and tuple(d.Fy_cases_train.shape) == (8, C, N)
    assert np.array_equal(d.Fy_cases_train.numpy(), dense[perm[:8].numpy()])
    assert np.array_equal(d.Fy_cases_val.numpy(), dense[perm[8:].numpy()])
    assert d.Fy_train is None and d.Fy_val is None and d.v_train is None      # the per-case fields: n_cases == 1 only, as before


def test_one_case_per_group_keeps_the_per_case_loads():
    from openpystruct_amd import dataprep
    G, N = 9, 13
    rec, dense = records(G, 1, N, np.random.default_rng(8))
    d = dataprep.prepare(rec, kind="fnn", n_cases=1, seed=3)
    assert d.Fy_train is not None and tuple(d.Fy_train.shape) == (7, N) and d.Fy_train.is_contiguous()
    assert torch.equal(d.Fy_cases_train, d.Fy_train[:, None]) and torch.equal(d.Fy_cases_val, d.Fy_val[:, None])
    assert np.array_equal(np.sort(torch.cat([d.Fy_train, d.Fy_val]).numpy().sum(1)), np.sort(dense[:, 0].sum(1)))
    names = list(dataprep.SurrogateData.__dataclass_fields__)
    assert names[-2:] == ["Fy_cases_train", "Fy_cases_val"]
    assert all(dataprep.SurrogateData.__dataclass_fields__[n].default is None for n in names[-2:])
    rec.pop("force_nodes")
    d = dataprep.prepare(rec, kind="fnn", n_cases=1, seed=3)
    assert d.Fy_cases_train is None and d.Fy_train is None


@pytest.mark.parametrize("kind", ["tfd", "fnn"])
def test_only_one_geometry_and_one_support_set_pass(kind):
    from openpystruct_amd import dataprep, sizing, train
    G, C, N = 10, 3, 13
    rng = np.random.default_rng(9)
    rec, _ = records(G, C, N, rng)
    term = train.DesignTerm(weight=1.0, x=torch.linspace(0, 200, N, dtype=torch.float64), E=200e9, fix=torch.zeros(N, dtype=torch.uint8),
                            wy=-1000.0, hp=sizing.SizingConfig(num_nodes=N))
    d = dataprep.prepare(rec, kind=kind, n_cases=C, seed=0)
    train._check_shared_bridge(term, d, d.X_train, C, "training")
    train._check_shared_bridge(term, d, d.X_val, C, "validation")
    other = train.DesignTerm(**{**term.__dict__, "x": term.x * 0.5})
    with pytest.raises(ValueError, match="not the geometry"):
        train._check_shared_bridge(other, d, d.X_train, C, "training")
    rec2, _ = records(G, C, N, rng, random_bridge=True)
    d2 = dataprep.prepare(rec2, kind=kind, n_cases=C, seed=0)
    with pytest.raises(ValueError, match="ONE geometry"):
        train._check_shared_bridge(term, d2, d2.X_train, C, "training")
    rec["roller_x_locations"][4, 1] = 95.0
    d3 = dataprep.prepare(rec, kind=kind, n_cases=C, seed=0)
    with pytest.raises(ValueError, match="ONE support set"):
        train._check_shared_bridge(term, d3, d3.X_train if (d3.X_train.reshape(8, C, -1)[..., 1] != d3.X_train.reshape(8, C, -1)[0, 0, 1]).any()
                                   else d3.X_val, C, "split")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        train._DesignInputs(term, kind, None, d, "cpu", None, None)
