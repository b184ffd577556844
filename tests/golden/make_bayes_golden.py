"""Generates tests/golden/surrogate_btfd.npz and surrogate_btfdm.npz by EXECUTING the reference's two Bayesian model scripts (build
container only): OpenPyStruct_Bayesian_TFDModule_MultiCase_Beta.py (BTFD) and OpenPyStruct_Bayesian_TFDModule_Meta_MultiCase_Beta.py
(BTFDM).

The runner, the overrides (num_epochs 3, batch_size 8, dropout 0, sigma_0 0), the synthetic dataset, the weight fill and the
deterministic noise are those of make_surrogate_golden.py, imported from it (that file is not changed).  The scripts are run through
its Transformer-Diffusion path, so `torch.randint` / `torch.randn_like` are the counter-based `DeterministicNoise` streams while they
run, with the same call counters for the evaluation forward (1000), the training forward (2000) and the loop (0).

torchbnn is not installed here.  The scripts `import torchbnn as bnn` and use `bnn.BayesLinear` only, so a small stand-in module is
put into `sys.modules` first (`_torchbnn_stand_in`).  It follows torchbnn 1.2's public semantics: parameters weight_mu,
weight_log_sigma, bias_mu, bias_log_sigma; mu ~ U(+-1/sqrt(in_features)), log_sigma = log(prior_sigma); every forward draws
W = mu + exp(log_sigma) * randn_like(log_sigma), then the bias likewise; no `kl_loss` method.  The fixtures therefore pin what belongs to
the SCRIPTS -- data prep (24-head padding, n_cases 8 and c = 1 for BTFDM), the module structure and its state-dict key names and
shapes, the forward arithmetic given the draws, the training loop's loss history and the evaluation block -- and NOT torchbnn itself.

Weights: `fill_state` of make_surrogate_golden.py, then every `*_log_sigma` is shifted by log(0.01) (`fill_bayes_state`): the
generic fill would give sigma ~ 1, a weight noise ten times the weights.

Run (in the build container):  python tests/golden/make_bayes_golden.py
"""
from __future__ import annotations

import importlib.util
import math
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_surrogate_golden", os.path.join(HERE, "make_surrogate_golden.py"))
msg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(msg)

SCRIPTS = {"btfd": "OpenPyStruct_Bayesian_TFDModule_MultiCase_Beta.py", "btfdm": "OpenPyStruct_Bayesian_TFDModule_Meta_MultiCase_Beta.py"}
LOG_SIGMA_SHIFT = math.log(0.01)
_FILL = msg.fill_state
# samples of surrogate_records.npz each script runs on: with n_cases 8, 160 samples give 20 groups, 16 of them training = two whole
# batches of 8 (the fixture's batch schedule is rectangular)
N_RECORDS = {"btfd": 180, "btfdm": 160}


def records_for(kind, rec):
    n = N_RECORDS[kind]
    return {k: v[:n] for k, v in rec.items()}


def fill_bayes_state(module, seed=msg.FILL_SEED):
    """msg.fill_state, then log_sigma += log(0.01) (shared with tests/test_bayes_golden.py)."""
    import torch
    _FILL(module, seed)
    with torch.no_grad():
        for k, t in module.state_dict().items():
            if k.endswith("_log_sigma"):
                t.add_(LOG_SIGMA_SHIFT)
    return module


def _torchbnn_stand_in():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class BayesLinear(nn.Module):
        def __init__(self, prior_mu, prior_sigma, in_features, out_features, bias=True):
            super().__init__()
            self.prior_mu, self.prior_sigma = prior_mu, prior_sigma
            self.in_features, self.out_features = in_features, out_features
            self.weight_mu = nn.Parameter(torch.empty(out_features, in_features))
            self.weight_log_sigma = nn.Parameter(torch.empty(out_features, in_features))
            self.bias_mu = nn.Parameter(torch.empty(out_features))
            self.bias_log_sigma = nn.Parameter(torch.empty(out_features))
            bound = 1.0 / math.sqrt(in_features)
            with torch.no_grad():
                self.weight_mu.uniform_(-bound, bound)
                self.bias_mu.uniform_(-bound, bound)
                self.weight_log_sigma.fill_(math.log(prior_sigma))
                self.bias_log_sigma.fill_(math.log(prior_sigma))

        def forward(self, x):
            w = self.weight_mu + torch.exp(self.weight_log_sigma) * torch.randn_like(self.weight_log_sigma)
            b = self.bias_mu + torch.exp(self.bias_log_sigma) * torch.randn_like(self.bias_log_sigma)
            return F.linear(x, w, b)

    mod = types.ModuleType("torchbnn")
    mod.BayesLinear = BayesLinear
    return mod


def generate(kind, records, out_path):
    sys.modules["torchbnn"] = _torchbnn_stand_in()
    saved = (msg.SCRIPTS["tfd"], msg.fill_state, msg.run_script)
    run_script = msg.run_script

    def run_with_heavy(k, workdir, *a, **kw):       # the _Meta_ script reads StructDataHeavy.json
        shutil.copy(os.path.join(workdir, "StructDataMedium.json"), os.path.join(workdir, "StructDataHeavy.json"))
        return run_script(k, workdir, *a, **kw)

    try:
        msg.SCRIPTS["tfd"] = SCRIPTS[kind]
        msg.fill_state = fill_bayes_state
        msg.run_script = run_with_heavy
        return msg.generate("tfd", records, out_path)
    finally:
        msg.SCRIPTS["tfd"], msg.fill_state, msg.run_script = saved


def main():
    assert os.path.isdir(msg.REF), "the reference is only present in the build container"
    rec = msg.unpack_records(np.load(os.path.join(HERE, "surrogate_records.npz")))
    for kind in (sys.argv[1:] or SCRIPTS):
        o = generate(kind, records_for(kind, rec), os.path.join(HERE, f"surrogate_{kind}.npz"))
        print(kind, "params", int(o["n_params"]), "train_loss", float(o["train_loss"]), "loop", o["loop_train_losses"], o["loop_val_losses"])


if __name__ == "__main__":
    main()
