"""Per-case CPU restatement of the reference's sizing loop -- TEST INFRASTRUCTURE ONLY.

Follows /root/reference/OpenPyStruct_BeamOpt_training_SingleCore.py:163-249 line by line
(torch CPU autograd, torch.optim.Adam, ExponentialLR, clamp, early stopping, one-step lag of
the recorded responses), with the OpenSees model build + analyze + response queries
(:176-190, :224-232) replaced by the oracle FE solve (oracle/c_oracle.py).
PARITY UNPINNED for the FE part (see oracle/beam_oracle.py: openseespy is unavailable).
The LOOP is no longer "re-typed and trusted": it is checked against fixtures the reference's OWN code produced
(r05, tests/golden/sizing_reference_{sc,mc,gpu,sc_rb,mc_rb,bo}.npz: SingleCore / MultiCore / GPU `main()` + `generate_sample`
and the BeamOpt script executed in the build container with openseespy replaced by a recorder backed by the oracle's 3-DOF
solve, tests/golden/make_sizing_golden.py) -- epoch counts equal in all 60 runs, every epoch's loss equal to 1e-6, final
float32 inertias bit-equal in >= 80 % of the cases and within 2e-5 in the rest (tests/test_sizing_golden.py).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.optim.lr_scheduler import ExponentialLR

from . import beam_oracle as bo
from . import c_oracle as co


def generate_sample(node_positions, roller_nodes, force_nodes, force_values, *, E=bo.E_REF, udl=bo.UDL_REF,
                    I_0=bo.I0_REF, max_e=600, lr=0.01, gamma=0.98, alpha_moment=1e-2, alpha_shear=1e-2,
                    tolerance=5e-3, patience=5, zero_last_node=False):
    """One sample.  `zero_last_node` reproduces MultiCore.py:222-223 (last node forced to 0.0)."""
    x = np.asarray(node_positions, dtype=np.float64)
    N = x.shape[0]
    Ne = N - 1
    G = E / (2 * (1 + bo.NU_REF))
    fix = np.zeros(N, dtype=np.uint8)
    fix[0] = 1
    for r in roller_nodes:
        fix[r - 1] = 1
    Fy = np.zeros((1, N))
    for n, F in zip(force_nodes, force_values):
        Fy[0, n - 1] += F

    I_tensor = torch.tensor([I_0] * Ne, dtype=torch.float32, requires_grad=True)     # :163
    optimizer = torch.optim.Adam([I_tensor], lr=lr)                                   # :166
    scheduler = ExponentialLR(optimizer, gamma=gamma)                                 # :167
    best_loss = float("inf")
    patience_counter = 0
    epochs = 0
    loss_history = []
    for epoch in range(max_e):                                                        # :174
        optimizer.zero_grad()
        I64 = I_tensor.detach().numpy().astype(np.float64)[None, :]                   # .item() widening, :107
        v, th, V, M, st = co.solve_beam_batched(x, E, I64, fix, Fy, udl)              # :176-182
        if st[0] != 0:
            break
        bending_moments = torch.tensor(M[0], dtype=torch.float32)                     # :189
        shear_forces = torch.tensor(V[0], dtype=torch.float32)                        # :190
        bending_energy = torch.sum((bending_moments ** 2) / (2 * E * I_tensor + 1e-6))  # :195
        A_approx = 0.03 * I_tensor ** 0.5                                             # :196
        shear_energy = torch.sum(shear_forces ** 2 / (G * A_approx))                  # :197
        primary_loss = torch.sum(I_tensor)                                            # :198
        total_loss = primary_loss + alpha_moment * bending_energy + alpha_shear * shear_energy
        total_loss.backward()                                                         # :202
        loss_history.append(float(total_loss.item()))
        optimizer.step()
        scheduler.step()
        with torch.no_grad():
            I_tensor.clamp_(min=1e-8)                                                 # :208
        epochs = epoch + 1
        if total_loss.item() < best_loss - tolerance:                                 # :211
            best_loss = total_loss.item()
            patience_counter = 0
        else:
            patience_counter += 1
        if patience_counter >= patience:
            break
    rotations = th[0].copy()
    deflections = v[0].copy()
    if zero_last_node:
        rotations[-1] = 0.0
        deflections[-1] = 0.0
    return {
        "roller_x_locations": [float(x[n - 1]) for n in roller_nodes],
        "force_x_locations": [float(x[n - 1]) for n in force_nodes],
        "force_values": [float(f) for f in force_values],
        "I_values": I_tensor.detach().numpy().tolist(),
        "shear_forces": shear_forces.detach().tolist(),
        "bending_moments": bending_moments.detach().tolist(),
        "node_positions": x.tolist(),
        "roller_nodes": list(roller_nodes),
        "force_nodes": [int(n) for n in force_nodes],
        "num_nodes": N,
        "L": float(x[-1]),
        "rotations": rotations.tolist(),
        "deflections": deflections.tolist(),
        "epochs_run": epochs,
        "final_loss": float(total_loss.item()),
        "loss_history": loss_history,
    }


def _schedule_f64(t, hp):
    """Adam step size with ExponentialLR, lr gamma^t / (1 - beta1^(t+1)), and sqrt(1 - beta2^(t+1)); all in double."""
    t = np.asarray(t, dtype=np.float64)
    return hp.lr * hp.gamma ** t / (1.0 - hp.beta1 ** (t + 1.0)), np.sqrt(1.0 - hp.beta2 ** (t + 1.0))


def sizing_step_reference(I32, exp_avg32, exp_avg_sq32, V, M, t, best, cnt, hp):
    """ONE optimiser epoch of B cases in numpy float64: the formulas of SingleCore.py:195-219 and torch's Adam evaluated on the
    float32 state widened to double.  I32, exp_avg32, exp_avg_sq32 [B, Ne] float32; V, M [B, Ne] (rounded to float32 first like
    :189-190, then widened); t [B] 0-based epoch = Adam steps taken so far; best [B] float32 best loss, cnt [B] patience counter;
    hp: anything with the fields of `ops_sizing_params`.  Every hyper-parameter stays a double and so do 1 - beta1, 1 - beta2,
    the step size and the bias correction.  Returns a dict of
        I (clamped at clamp_min), exp_avg, exp_avg_sq [B, Ne]; loss, best [B] float64; cnt [B] int; stop [B] bool;
        I_free: I before the clamp;  upd: the Adam update I - I_free
        tM, tV: the moment / shear terms of the gradient g = 1 - tM - tV;  mag = 1 + |tM| + |tV|: what errors of g scale with."""
    f64 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    I, m, v, Vf, Mf = f64(I32), f64(exp_avg32), f64(exp_avg_sq32), f64(V), f64(M)
    t, cnt = np.asarray(t, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    best = f64(best)
    den_b = 2.0 * hp.E * I + hp.bend_eps                                   # :195
    sq = np.sqrt(I)
    den_s = hp.G * (hp.area_coef * sq)                                     # :196-197
    loss = I.sum(-1) + hp.alpha_moment * (Mf ** 2 / den_b).sum(-1) + hp.alpha_shear * (Vf ** 2 / den_s).sum(-1)
    tM = hp.alpha_moment * Mf ** 2 * (2.0 * hp.E) / den_b ** 2
    tV = hp.alpha_shear * Vf ** 2 / den_s ** 2 * (hp.G * hp.area_coef * 0.5 / sq)
    g = 1.0 - tM - tV
    ea = hp.beta1 * m + (1.0 - hp.beta1) * g
    es = hp.beta2 * v + (1.0 - hp.beta2) * g * g
    step_size, bc2s = _schedule_f64(t, hp)
    upd = step_size[..., None] * (ea / (np.sqrt(es) / bc2s[..., None] + hp.adam_eps))
    I_free = I - upd
    improved = loss < best - hp.tolerance                                  # :211
    new_cnt = np.where(improved, 0, cnt + 1)
    return {"I": np.maximum(I_free, hp.clamp_min), "I_free": I_free, "exp_avg": ea, "exp_avg_sq": es, "loss": loss,
            "best": np.where(improved, loss, best), "cnt": new_cnt,
            "stop": (new_cnt >= hp.patience) | (t + 1 >= hp.max_epochs),
            "tM": tM, "tV": tV, "mag": 1.0 + np.abs(tM) + np.abs(tV), "upd": upd}


def sizing_step_float32(I32, exp_avg32, exp_avg_sq32, V, M, t, hp, f32_one_minus_beta=False):
    """The same epoch with every operation rounded to float32 (numpy float32 arithmetic, operation order of a plain elementwise
    implementation; hyper-parameters and the schedule formed in double and rounded once, as torch does).  It measures what float32
    round-off ALONE does to the step: the error bounds of tests/test_gpu_sizing_step.py are multiples of its distance from
    `sizing_step_reference`.  `f32_one_minus_beta`: form 1 - beta as float32(1) - float32(beta) instead -- 4.7e-5 off for 0.999.
    Returns I, exp_avg, exp_avg_sq [B, Ne] float32 and loss [B] float32."""
    f = np.float32
    I, m, v = (np.asarray(a, dtype=f) for a in (I32, exp_avg32, exp_avg_sq32))
    Vf, Mf = np.asarray(V, dtype=np.float64).astype(f), np.asarray(M, dtype=np.float64).astype(f)
    twoE, G, ac = f(2.0 * hp.E), f(hp.G), f(hp.area_coef)
    aM, aV = f(hp.alpha_moment), f(hp.alpha_shear)
    b1, b2 = f(hp.beta1), f(hp.beta2)
    omb1, omb2 = (f(1) - b1, f(1) - b2) if f32_one_minus_beta else (f(1.0 - hp.beta1), f(1.0 - hp.beta2))
    t64 = np.asarray(t, dtype=np.float64)
    step_size = (hp.lr * hp.gamma ** t64).astype(f) / (1.0 - hp.beta1 ** (t64 + 1.0)).astype(f)
    bc2s = np.sqrt(1.0 - hp.beta2 ** (t64 + 1.0)).astype(f)
    den_b = twoE * I + f(hp.bend_eps)
    sq = np.sqrt(I)
    den_s = G * (ac * sq)
    loss = I.sum(-1, dtype=f) + aM * ((Mf * Mf) / den_b).sum(-1, dtype=f) + aV * ((Vf * Vf) / den_s).sum(-1, dtype=f)
    g = f(1) - aM * ((Mf * Mf) / (den_b * den_b)) * twoE - aV * ((Vf * Vf) / (den_s * den_s)) * (G * ac * (f(0.5) / sq))
    ea = b1 * m + omb1 * g
    es = b2 * v + omb2 * g * g
    In = np.maximum(I - step_size[..., None] * (ea / (np.sqrt(es) / bc2s[..., None] + f(hp.adam_eps))), f(hp.clamp_min))
    assert all(a.dtype == f for a in (In, ea, es, loss))
    return In, ea, es, loss


def sizing_step_errors(ref, I_in, exp_avg_in, exp_avg_sq_in, I, exp_avg, exp_avg_sq, loss, hp):
    """Elementwise errors of one epoch's outputs against `sizing_step_reference`'s dict, each over the magnitude its float32
    round-off scales with, in units of eps32 = 2^-23: the largest of exp_avg, exp_avg_sq, I [B, Ne] and loss [B]."""
    eps32 = 2.0 ** -23
    d = lambda a: np.asarray(a).astype(np.float64)      # noqa: E731
    m_in, v_in, mag = np.abs(d(exp_avg_in)), d(exp_avg_sq_in), ref["mag"]
    s_ea = hp.beta1 * m_in + (1.0 - hp.beta1) * mag
    s_es = hp.beta2 * v_in + (1.0 - hp.beta2) * mag ** 2
    ea_ref = np.abs(ref["exp_avg"])                     # (a zero first moment has a zero update: its term drops out)
    s_I = np.abs(d(I_in)) + np.abs(ref["upd"]) * s_ea / np.where(ea_ref > 0, ea_ref, 1.0)
    return {"exp_avg": float((np.abs(d(exp_avg) - ref["exp_avg"]) / s_ea).max() / eps32),
            "exp_avg_sq": float((np.abs(d(exp_avg_sq) - ref["exp_avg_sq"]) / s_es).max() / eps32),
            "I": float((np.abs(d(I) - ref["I"]) / s_I).max() / eps32),
            "loss": float((np.abs(d(loss) - ref["loss"]) / np.abs(ref["loss"])).max() / eps32)}
