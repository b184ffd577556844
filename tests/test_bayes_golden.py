"""BTFD / BTFDM against fixtures produced by the REFERENCE'S OWN scripts (tests/golden/make_bayes_golden.py executed
OpenPyStruct_Bayesian_TFDModule_MultiCase_Beta.py and its _Meta_ sibling, torchbnn replaced by a stand-in with its public semantics):
data prep (24-head padding; n_cases 8, c = 1 for BTFDM), state-dict layout, the eval- and train-mode forward with gradients, three
epochs of the script's loop and its evaluation block.  The Bayesian draws and the diffusion draws are the generator's counter-based
`DeterministicNoise` streams on both sides.  Tolerances as in tests/test_surrogate_golden.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from openpystruct_amd import dataprep, train

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLD, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


mbg = _load("make_bayes_golden")      # fill_bayes_state / records_for; no reference access
msg = mbg.msg
KINDS = ("btfd", "btfdm")


def gold(kind):
    return np.load(os.path.join(GOLD, f"surrogate_{kind}.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def records():
    return msg.unpack_records(np.load(os.path.join(GOLD, "surrogate_records.npz")))


def cfg_for(kind):
    c = (train.BtfdConfig if kind == "btfd" else train.BtfdmConfig)()
    c.dropout_rate, c.sigma_0, c.batch_size = 0.0, 0.0, 8        # the generator's overrides
    return c


def prep(kind, records, g, device=None):
    c = cfg_for(kind)
    return dataprep.prepare(mbg.records_for(kind, records), kind="tfd", n_cases=c.n_cases, c=c.c, train_split=c.train_split,
                            nheads=c.num_heads, refit_val_scalers=False, perm=torch.as_tensor(g["perm"]), device=device)


def close(got, want, tol, what=""):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-30)
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol:.1e}"


def _dataprep_check(kind, records, device):
    g = gold(kind)
    d = prep(kind, records, g, device=device)
    assert d.feat_dim % 24 == 0 and d.X_train.shape[1] == cfg_for(kind).n_cases
    for got, key in ((d.X_train, "X_train_tensor"), (d.Y_train, "Y_train_tensor"), (d.X_val, "X_val_tensor"), (d.Y_val, "Y_val_tensor")):
        assert tuple(got.shape) == g[key].shape, key
        close(got, g[key], 1e-5, key)
    close(d.min_constraint, g["min_constraint"], 1e-6, "min"); close(d.max_constraint, g["max_constraint"], 1e-6, "max")
    close(d.scalers_Y["I"].scale_, g["scaler_Y/I/scale"], 1e-5, "scaler_Y scale")


@pytest.mark.parametrize("kind", KINDS)
def test_dataprep_matches_reference(kind, records):
    _dataprep_check(kind, records, None)


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_layout_matches_reference(kind, records):
    g = gold(kind)
    d = prep(kind, records, g)
    model, crit = train.build_model_and_loss(kind, cfg_for(kind), d, torch.device("cpu"))
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [",".join(str(v) for v in t.shape) for t in sd.values()] == [str(s) for s in g["sd_shapes"]]
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"])
    assert list(crit.state_dict().keys()) == [str(k) for k in g["crit_sd_keys"]]


def _forward_check(kind, records, device, tol, tol_grad):
    g = gold(kind)
    d = prep(kind, records, g, device=device)
    model, crit = train.build_model_and_loss(kind, cfg_for(kind), d, torch.device(device))
    mbg.fill_bayes_state(model)
    Xe, Ye = d.X_val[:6], d.Y_val[:6]
    Xt, Yt = d.X_train[:8].clone().requires_grad_(True), d.Y_train[:8]
    with msg.DeterministicNoise() as noise:
        noise.calls = 1000
        model.eval()
        with torch.no_grad():
            pe = model(Xe)
        close(pe, g["eval_preds"], tol, "eval preds")
        close(crit(pe, Ye), g["eval_loss"], tol, "eval loss")
        noise.calls = 2000
        model.train()
        pt = model(Xt)
        loss = crit(pt, Yt)
    close(pt, g["train_preds"], tol, "train preds")
    close(loss, g["train_loss"], tol, "train loss")
    loss.backward()
    close(Xt.grad, g["train_input_grad"], tol_grad, "input grad")
    got = msg.projections((n, p.grad) for n, p in model.named_parameters())
    for n, p in model.named_parameters():
        want = g["grad/" + n]
        ref = max(float(want[1]), 1e-12)
        assert abs(got[n][1] - want[1]) <= tol_grad * ref, n
        assert abs(got[n][0] - want[0]) <= tol_grad * ref * 10, n


@pytest.mark.parametrize("kind", KINDS)
def test_modules_match_reference_cpu(kind, records):
    _forward_check(kind, records, "cpu", 2e-5, 2e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_loop_and_evaluation_match_reference_cpu(kind, records):
    """Three epochs of the script's loop (its DataLoader order replayed, the same draws) vs train_surrogate on the CPU, then the
    script's evaluation block: best checkpoint, un-standardised validation predictions, R^2."""
    g = gold(kind)
    d = prep(kind, records, g)
    batches = g["loop_batches"]
    with msg.DeterministicNoise() as noise:
        noise.calls = 0
        res = train.train_surrogate(kind, d, cfg_for(kind), device="cpu", autocast_dtype=None, max_epochs=batches.shape[0],
                                    init_fn=mbg.fill_bayes_state, batch_order=lambda ep: batches[ep - 1])
    close(np.array(res["history"]["train"]), g["loop_train_losses"], 5e-4, "train-loss history")
    close(np.array(res["history"]["val"]), g["loop_val_losses"], 5e-4, "val-loss history")
    assert int(np.argmin(res["history"]["val"])) + 1 == int(g["eval_best_epoch"])
    close(res["val_true_I"].cpu().numpy(), g["eval_labels_unstd"], 1e-5, "un-standardised validation labels")
    close(res["val_pred_I"].cpu().numpy(), g["eval_preds_unstd"], 5e-3, "un-standardised validation predictions")
    assert abs(res["r2_val_I"] - float(g["eval_r2_val"])) <= 2e-2 * max(1.0, abs(float(g["eval_r2_val"])))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_dataprep_matches_reference_on_the_gpu(kind, records):
    _dataprep_check(kind, records, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_modules_match_reference_gpu_fp32(kind, records):
    """The framework modules on the MI355X in fp32 (the draws replayed: the HIP sampler is the training loop's, pinned against these
    modules in tests/test_gpu_bayes.py)."""
    _forward_check(kind, records, "cuda", 1e-4, 1e-3)
