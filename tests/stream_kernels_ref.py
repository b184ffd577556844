"""Float64 references, error units and the case tables of the five streaming kernels every surrogate training step runs (test code,
NumPy): csrc/stencil_bn.hip, fused_bn.hip, fused_loss.hip, flat_adam.hip and input_prep.hip (+ input_noise.hpp).

One function per entry point, in the style of tests/seq_block_ref.py.  Inputs are what the device receives: float32 arrays, bf16 bit
patterns (uint16) and hyper-parameters ROUNDED TO float32 as the C ABI receives them.  With dt = float64 a function is the reference,
with dt = float32 it is the kernel's documented formula (the header comment of its .hip file) evaluated in float32:

    stencil_bn   variance as E[y^2] - m^2
    fused_bn     per row group (count, mean, M2), the sixteen groups combined pairwise (Chan)
    flat_adam    float32 beta as received, 1 - beta formed from it

Every function returns {output: (value, unit)}.  The unit is the output's formula with every sum replaced by the sum of the absolute
values of its terms (a first-order running error bound), in units of EPS32 = 2^-24:

    float32 outputs   |got - ref| <= C unit EPS32
    bf16 outputs      |got - ref| <= 1/2 ulp_bf16(ref) + C unit EPS32
    ref == 0          got == 0 where the formula gives an exact zero (EXACT_ZERO: a dropped element, p == t, a zeroed gradient)

C = 4 x CPU_CONST[output]: CPU_CONST is the largest constant the float32 evaluation shows over the case tables (measured and asserted
by tests/test_stream_kernels_reference.py).  The factor four covers the device's rsqrtf, reciprocals and butterfly orders, and
1 / (1 - p) and 1 / (B n) formed in float32.  No constant comes from a GPU's output.

A value a later stage consumes is TAKEN AS GIVEN by that stage's reference: the statistics of fused_bn are those of the stored sum
z (the float32 or bf16 array the forward wrote, itself held to the exact sum), the backward passes get the float64 forward's saved
statistics rounded to float32, and the second optimiser step starts from the stored state of the first.  So every bound is a
one-stage bound and no error is carried from one comparison into the next.

Streams: dropout masks from tests/bayes_stream.py (drop_key / drop_uniform, bit for bit the device's) at element r F + c, kept when
u >= float32(p); the input noise from `input_noise` here: ip_mix of input_noise.hpp in exact 64-bit integer arithmetic, Box-Muller in
float64 -- an ABSOLUTE bound (NOISE_BOUND), derived at its definition.

`bug=`: deliberately wrong variants of the float32 evaluation (the teeth check of test_stream_kernels_reference.py).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import bayes_stream as bs
# bf16 helpers, the error measure, the seed and the counters are seq_block_ref's (imported, not copied; the test files use them from here)
from tests.seq_block_ref import COUNTERS, EPS32, SEED, SENT_BF16, SENT_F32, bf16_bits, bf16_f32, bf16_f64, error_ratio, exact_zeros, ulp_bf16  # noqa: F401

f32, f64 = np.float32, np.float64
MASK64 = (1 << 64) - 1

# Largest constant of the float32 evaluation per output over the tables below (test_stream_kernels_reference.py asserts that none is
# exceeded and prints the measured values; an entry is the measurement plus about 12 %, rounded up to a twentieth); the bound of the GPU
# test is four times this.
CPU_CONST = {
    "sb.z32": 2.2, "sb.mean": 1.05, "sb.invstd": 2.2, "sb.rmean": 2.3, "sb.rvar": 2.2,
    "sb.dx": 3.5, "sb.dw0": 1.5, "sb.dw1": 1.3, "sb.dw2": 1.45, "sb.db": 1.0, "sb.dgamma": 0.9, "sb.dbeta": 0.35,
    "fb.zsave": 2.2, "fb.y": 2.8, "fb.mean": 2.95, "fb.rstd": 1.15, "fb.rmean": 1.8, "fb.rvar": 1.45,
    "fb.dz": 4.4, "fb.dgamma": 3.45, "fb.dbeta": 4.55,
    "fl.loss": 2.9, "fl.loss_sum": 2.85, "fl.grad": 4.2,
    "fa.p": 2.6, "fa.m": 3.25, "fa.v": 6.1,
}
# An output that is only ever stored as bf16 shows its float32 error at the few elements next to a rounding tie alone: it is held to the
# constant of its float32 twin (the same value before it is rounded)
BF16_TWINS = {"sb.z16": "sb.z32", "fa.shadow": "fa.p"}
CPU_CONST.update({k: CPU_CONST[v] for k, v in BF16_TWINS.items()})
# outputs whose formula gives exact zeros (a dropped element, p == t, a zeroed gradient): there got == 0 is demanded
EXACT_ZERO = {"fb.y", "fb.dz", "fl.grad"}


def bound_constant(name: str) -> float:
    return 4.0 * CPU_CONST[name]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _r32(rng, shape, scale=1.0, shift=0.0):
    return (shift + scale * rng.standard_normal(shape)).astype(f32)


def _h(v, dt):
    """A hyper-parameter as the device has it (rounded to float32 by the C ABI), in the evaluation's type."""
    return dt(f32(v))


def _wide(a, bf16, dt):
    return (bf16_f32(a) if bf16 else np.asarray(a, dtype=f32)).astype(dt)


def _store(v, bf16):
    """A float32 evaluation's value as the kernel leaves it in memory, widened to float64."""
    v = np.asarray(v, dtype=f32)
    return bf16_f64(bf16_bits(v)) if bf16 else v.astype(f64)


def keep_mask(seed, call, idx, p, bug=()):
    p32 = float(f32(p))
    idx = np.asarray(idx, dtype=np.uint64)
    if not p32 > 0.0:
        return np.ones(idx.shape, dtype=bool)
    u = bs.drop_uniform(bs.drop_key(seed, call), idx)
    return u > p32 if "keep_gt" in bug else u >= p32


def _ks(p, dt):
    return dt(1.0) / (dt(1.0) - dt(f32(p))) if f32(p) > 0 else dt(1.0)


# =================================================================================================================================
# input_prep.hip: out[b, :] = X[idx[b], :] + sigma N(0, 1)
# =================================================================================================================================
IP_GOLDEN, IP_SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
# Absolute bound on the noise term: |out - (X[idx] + sigma n_ref)| <= sigma NOISE_BOUND + 1 ulp_f32 (+ 1/2 ulp_bf16).  ip_noisy uses
# __logf and __cosf.  An absolute error of 1e-6 in the logarithm moves the radius sqrt(-2 log u1) by at most sqrt(2e-6) = 1.4e-3 (near
# u1 = 1, where the radius itself is 0); the same error in the cosine times the largest radius sqrt(2 * 24 log 2) = 5.8 gives 6e-6.
NOISE_BOUND = 2e-3

# (B, F, out offset in floats): (5, 7) scalar path; (3, 8) VEC4; (130, 1024) VEC4 with the grid at its 128-workgroup cap and several
# trips; (9, 4) once aligned and once with `out` one float off, which falls to the scalar path and must draw the SAME noise
IP_SHAPES = [(1, 1, 0), (5, 7, 0), (3, 8, 0), (37, 684, 0), (130, 1024, 0), (9, 4, 0), (9, 4, 1)]
IP_SIGMAS = (None, 0.0, 0.5)           # NULL pointer, 0 and 0.5
# (B, F, off, out bf16, targets columns or 0, counter (None: NULL pointer = call 0), sigma)
IP_COUNTERS = (None,) + tuple(COUNTERS)
IP_CASES = [(B, F, off, (n + k) % 2 == 1, 302 if (B, F) == (37, 684) else (0, 3, 0)[(n + k) % 3], IP_COUNTERS[(n + 2 * k) % 4], IP_SIGMAS[k])
            for n, (B, F, off) in enumerate(IP_SHAPES) for k in range(3)]
IP_CASES += [(9, 4, off, False, 0, COUNTERS[2], 0.5) for off in (0, 1)] + [(5, 7, 0, True, 2, COUNTERS[1], 0.5), (3, 8, 0, True, 0, COUNTERS[2], 0.5)]


def ip_mix(z):
    """splitmix64's finaliser on uint64 arrays (exact: the products wrap modulo 2^64 as the device's do)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def input_noise(seed, call, idx):
    """The standard normal that element `idx` of call `call` draws (input_noise.hpp ip_noisy): the hash in exact integer arithmetic,
    u1 in (0, 1] and u2 in [0, 1) on the 2^-24 grid (exact in float32), Box-Muller in float64."""
    base = (int(seed) + IP_GOLDEN * ((int(call) + 1) & MASK64)) & MASK64
    with np.errstate(over="ignore"):
        h = ip_mix(np.uint64(base) + np.asarray(idx, dtype=np.uint64) * np.uint64(IP_SALT))
    u1 = ((h >> np.uint64(40)).astype(f64) + 1.0) * 2.0 ** -24
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(f64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def ip_inputs(case):
    B, F, off, bf, C, counter, sigma = case
    rng = _rng(B, F, 11)
    rows = max(B // 2, 1) + 3
    idx = rng.integers(0, rows, B).astype(np.int64)
    if B > 1:
        idx[-1] = idx[0]                                 # a repeated row
    return dict(X=_r32(rng, (rows, F)), idx=idx, Y=_r32(rng, (rows, max(C, 1))) if C else None)


def gather_rows_noise(X, idx, sigma, seed, call, bug=()):
    """{"out": (value, noise term)}: X[idx] + sigma n in float64; the second entry is sigma n, for the teeth check."""
    B, F = idx.shape[0], X.shape[1]
    sg = 0.0 if sigma is None else float(f32(sigma))
    e = np.arange(B * F, dtype=np.uint64).reshape(B, F)
    if "row_index" in bug:
        e = np.broadcast_to(np.arange(F, dtype=np.uint64), (B, F))
    noise = sg * input_noise(seed, (call - 1) if "call_not_plus_1" in bug else call, e) if sg != 0.0 else np.zeros((B, F))
    return {"out": (X[idx].astype(f64) + noise, noise)}


def ip_bound(ref, sigma, bf16):
    """The absolute bound of a gather output (array)."""
    sg = 0.0 if sigma is None else float(f32(sigma))
    if sg == 0.0:
        return 0.5 * ulp_bf16(ref) if bf16 else np.zeros_like(ref)
    ulp32 = np.spacing(np.abs(ref).astype(f32)).astype(f64)
    return sg * NOISE_BOUND + ulp32 + (0.5 * ulp_bf16(ref) if bf16 else 0.0)


# =================================================================================================================================
# fused_loss.hip
# =================================================================================================================================
FL_SHAPES = [(1, 1, 1, 0), (1, 3, 1, 1), (3, 5, 5, 0), (5, 7, 2, 0), (5, 7, 2, 5), (7, 302, 100, 101), (128, 302, 100, 101),
             (300, 302, 100, 101)]                                       # (B, C, nI, nD); nR = C - nI - nD
FL_ALPHAS = (-0.5, 1e-6, 0.3, 1.0, 1.7)
FL_BOXES = ("none", "min", "max", "both")
FL_LO, FL_HI = -0.75, 0.875                                              # exact in bf16: a prediction can sit ON a bound in both types
FL_BOX_W, FL_PENALTY, FL_SUM0 = 0.1, 1.5e-6, 3.25
# every shape with every alpha; box, alpha0 and the predictions' type cycle so that each value meets each shape and each alpha
FL_CASES = [(B, C, nI, nD, FL_BOXES[(s + k) % 4], FL_ALPHAS[k], (float("nan"), 0.5)[(s + k // 2) % 2], (s + k + k // 4) % 2 == 1)
            for s, (B, C, nI, nD) in enumerate(FL_SHAPES) for k in range(5)]


def fl_inputs(case):
    """Predictions and targets with, per column group and as far as its elements go, planted in this order: p == t, p == lo, p == hi
    (first group), t == 0 (relative groups), p == t again."""
    B, C, nI, nD, box, alpha, alpha0, bf = case
    rng = _rng(B, C, nI, nD, 12)
    p, t = _r32(rng, (B, C)), _r32(rng, (B, C))
    if bf:
        p = bf16_f32(bf16_bits(p))
    groups = [("I", 0, nI), ("D", nI, nI + nD), ("R", nI + nD, C)]
    for name, c0, c1 in groups:
        cells = [(r, c) for r in range(B) for c in range(c0, c1)]
        if not cells:
            continue
        order = rng.permutation(len(cells))[:7]
        plan = ["eq", "lo", "hi", "eq", "eq", "lo", "hi"] if name == "I" else ["eq", "t0", "eq", "t0", "eq", "t0", "eq"]
        for what, j in zip(plan, order):
            r, c = cells[j]
            if what == "eq":
                t[r, c] = p[r, c]
            elif what == "t0":
                t[r, c] = 0.0
            else:
                p[r, c] = FL_LO if what == "lo" else FL_HI
    return dict(p=bf16_bits(p) if bf else p, t=t)


def surrogate_loss_grad(preds, bf, targets, nI, nD, alpha, alpha0, lo, hi, w, penalty, loss_sum0=0.0, calls=1, dt=f64, bug=()):
    """loss, loss_sum after `calls` calls from loss_sum0, and d loss / d preds (already divided by the means' counts)."""
    p, t = _wide(preds, bf, dt), np.asarray(targets, dtype=f32).astype(dt)
    B, C = p.shape
    nR = C - nI - nD
    a_raw = _h(alpha, dt)
    a = a_raw if "no_clamp" in bug else np.minimum(np.maximum(a_raw, dt(1e-6)), dt(1.0))
    w_, pen, eps = _h(w, dt), _h(penalty, dt), dt(1e-8)
    d = p - t
    sg = np.sign(d)
    if "sign0_is_1" in bug:
        sg = np.where(d == 0, dt(1.0), sg)
    one = dt(1.0)
    inv = [one / (dt(B) * dt(n)) if n > 0 else dt(0.0) for n in (nI, nD, nR)]
    if "swap_inv" in bug:
        inv[1], inv[2] = inv[2], inv[1]
    g, ug = np.zeros((B, C), dtype=dt), np.zeros((B, C), dtype=dt)
    dI, sI = d[:, :nI], sg[:, :nI]
    g[:, :nI] = (a * sI + (one - a) * dt(2.0) * dI) * inv[0]
    ug[:, :nI] = (np.abs(a * sI) + np.abs((one - a) * dt(2.0) * dI)) * inv[0]
    box = np.zeros((), dtype=dt)
    pI = p[:, :nI]
    if lo is not None:
        below = pI <= _h(lo, dt) if "box_ge" in bug else pI < _h(lo, dt)
        g[:, :nI] -= np.where(below, w_, dt(0.0))
        ug[:, :nI] += np.where(below, np.abs(w_), dt(0.0))
        box = box + np.where(below, _h(lo, dt) - pI, dt(0.0)).sum(dtype=dt)
    if hi is not None:
        above = pI >= _h(hi, dt) if "box_ge" in bug else pI > _h(hi, dt)
        g[:, :nI] += np.where(above, w_, dt(0.0))
        ug[:, :nI] += np.where(above, np.abs(w_), dt(0.0))
        box = box + np.where(above, pI - _h(hi, dt), dt(0.0)).sum(dtype=dt)
    l1, l2 = np.abs(dI).sum(dtype=dt) * inv[0], (dI * dI).sum(dtype=dt) * inv[0]
    v = a * l1 + (one - a) * l2 + w_ * box
    uv = np.abs(a) * l1 + np.abs(one - a) * l2 + np.abs(w_) * box
    for k, (c0, c1) in enumerate(((nI, nI + nD), (nI + nD, C)), start=1):
        if c1 > c0:
            den = np.abs(t[:, c0:c1]) + eps
            g[:, c0:c1] = pen * sg[:, c0:c1] / den * inv[k]
            ug[:, c0:c1] = np.abs(g[:, c0:c1])
            term = pen * (np.abs(d[:, c0:c1]) / den).sum(dtype=dt) / (dt(B) * dt(c1 - c0))
            v, uv = v + term, uv + np.abs(term)
    a0 = f32(alpha0)
    if a0 == a0:                                                         # NaN alpha0: no such term
        da = dt(a0) - a_raw
        v, uv = v + da * da, uv + (np.abs(dt(a0)) + np.abs(a_raw)) ** 2
    once = dt(f32(v))                                                    # loss[0] as stored: what the running sum adds
    tot, utot = dt(f32(loss_sum0)), np.abs(dt(f32(loss_sum0)))
    for _ in range(calls):
        tot, utot = once + (dt(0.0) if "sum_overwrite" in bug else tot), utot + uv
    return {"loss": (np.asarray(v), np.asarray(uv)), "loss_sum": (np.asarray(tot), np.asarray(utot)), "grad": (g, ug)}


# =================================================================================================================================
# flat_adam.hip
# =================================================================================================================================
DECOUPLED, ZERO_GRADS, NORM_READY, MAX_PARTS = 1, 2, 4, 1024
FA_DEFAULT = dict(wd=0.0, flags=0, shadow=False, max_norm=1.0, norm=50.0, grad_scale=1.0, step0=0, offset="none", parts=0)
FA_VARIANTS = {
    "plain": {}, "l2": dict(wd=1e-2), "adamw": dict(wd=1e-2, flags=DECOUPLED), "zero": dict(flags=ZERO_GRADS), "shadow": dict(shadow=True),
    "noclip": dict(max_norm=0.0), "tiny": dict(norm=1e-3), "gscale": dict(grad_scale=1.0 / 1024), "step9": dict(step0=9, shadow=True),
    "step9999": dict(step0=9999), "off1": dict(offset="all", shadow=True, flags=ZERO_GRADS), "shoff": dict(offset="shadow", shadow=True),
    "ready1": dict(parts=1), "ready300": dict(parts=300, wd=1e-2, flags=DECOUPLED | ZERO_GRADS, shadow=True), "ready1024": dict(parts=1024),
}
FA_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 131072 + 7, 4194304 + 3075)      # the last two: the norm kernel strides / the update strides
FA_CASES = [(n, "plain") for n in FA_SIZES] + [(n, v) for v in FA_VARIANTS if v != "plain" for n in (3, 5, 1025)]
FA_LRS, FA_B1, FA_B2, FA_EPS = (1e-3, 7e-4), 0.9, 0.999, 1e-8              # lr is changed on the device between the two steps


def fa_config(case):
    return {**FA_DEFAULT, **FA_VARIANTS[case[1]]}


def fa_inputs(case):
    """p, g, m, v of the first step; g is scaled so that ||g * grad_scale|| is the case's `norm`; elements 1, 6, 11, ... (every
    fifth) have g = m = v = 0."""
    n, cfg = case[0], fa_config(case)
    rng = _rng(n, len(case[1]), 13)
    p, g, m, v = _r32(rng, n), rng.standard_normal(n), _r32(rng, n, 0.3), (0.1 * rng.standard_normal(n) ** 2).astype(f32)
    if n >= 3:
        g[1::5], m[1::5], v[1::5] = 0.0, 0.0, 0.0
    g = (g * (cfg["norm"] / max(np.sqrt((g * g).sum()), 1e-30)) / float(f32(cfg["grad_scale"]))).astype(f32)
    return dict(p=p, g=g, m=m, v=v)


def fa_partials(g, grad_scale, parts):
    """What a gradient producer leaves in the workspace for OPS_ADAM_NORM_READY: `parts` partial sums of (g grad_scale)^2 in float64."""
    sq = (g.astype(f64) * float(f32(grad_scale))) ** 2
    out = np.zeros(parts)
    for k, chunk in enumerate(np.array_split(sq, min(parts, sq.size))):
        out[k] = chunk.sum()
    return out


def fa_corrections(step, b1=FA_B1, b2=FA_B2):
    """(1 - b1^t, sqrt(1 - b2^t)) in float64 from the float32 betas, as the norm pass tabulates them."""
    return 1.0 - float(f32(b1)) ** step, np.sqrt(1.0 - float(f32(b2)) ** step)


def flat_clip_adam_step(p, g, m, v, lr, step, max_norm, grad_scale, b1, b2, eps, wd, flags, normsq=None, dt=f64, bug=()):
    """One step; `step` is the ADVANCED count t.  normsq: the sum of the partial sums a producer left (OPS_ADAM_NORM_READY)."""
    p_, g_, m_, v_ = (np.asarray(a).astype(dt) for a in (p, g, m, v))           # float32 arrays (float64: the autograd check)
    one = dt(1.0)
    gsc, b1_, b2_, eps_, wd_, lr_, mx = (_h(x, dt) for x in (grad_scale, b1, b2, eps, wd, lr, max_norm))
    if normsq is None:
        sc = g_ if "clip_no_scale" in bug else g_ * gsc
        normsq = (sc * sc).sum(dtype=dt)
    norm = np.sqrt(dt(normsq))
    clip = np.minimum(mx / (norm + dt(f32(1e-6))), one) if mx > 0 else one
    t = step - 1 if "late_correction" in bug else step
    c1, c2s = fa_corrections(t, b1, b2)
    bc1, bc2s = dt(c1), dt(c2s)
    gs = clip * gsc
    decoupled = bool(flags & DECOUPLED) and "l2_for_decoupled" not in bug
    gi, ugi = g_ * gs, np.abs(g_ * gs)
    pw = p_
    if decoupled:
        pw = p_ * (one - lr_ * wd_)
    else:
        gi, ugi = gi + wd_ * p_, ugi + np.abs(wd_ * p_)
    mn = b1_ * m_ + (one - b1_) * gi
    um = np.abs(b1_ * m_) + (one - b1_) * ugi
    vn = b2_ * v_ + (one - b2_) * gi * gi
    uv = b2_ * v_ + (one - b2_) * ugi * ugi
    root = np.sqrt(vn)
    den = (np.sqrt(vn + eps_) / bc2s) if "eps_in_sqrt" in bug else root / bc2s + eps_
    with np.errstate(divide="ignore", invalid="ignore"):
        uden = den + np.where(vn > 0, dt(0.5) * uv / np.where(vn > 0, root, one) / bc2s, dt(0.0))
        step_size = lr_ / bc1
        pn = pw - step_size * (mn / den)
        up = np.abs(p_) + np.abs(step_size) * (um / den + np.abs(mn) * uden / (den * den))
    if "tail_unchanged" in bug and p_.size % 4:
        k = p_.size - p_.size % 4
        pn[k:], mn[k:], vn[k:] = p_[k:], m_[k:], v_[k:]
    return {"p": (pn, up), "m": (mn, um), "v": (vn, uv), "shadow": (pn, up)}


# =================================================================================================================================
# stencil_bn.hip: z = gamma (y - mean) invstd + beta, y the 3-tap stencil of x with zero padding, one channel over all B F values
# =================================================================================================================================
SB_SHAPES = [(1, 2), (3, 1), (4, 64), (5, 65), (7, 5), (128, 350), (257, 129), (1030, 3)]
SB_CASES = [(B, F, ratio) for B, F in SB_SHAPES for ratio in (0, 30)]            # |mean(y)| / std(y)
SB_EPS, SB_MOM = 1e-5, 0.1
SB_MODES = [(zb, gb, tr) for tr in (1, 0) for zb in (False, True) for gb in (False, True)]     # z bf16, grad_z bf16, training


def _taps(x, dt, bug=()):
    """x[i - 1] and x[i + 1] with zero padding at the row ends."""
    xm, xp = np.zeros_like(x), np.zeros_like(x)
    xm[:, 1:], xp[:, :-1] = x[:, :-1], x[:, 1:]
    if "pad_from_neighbour_row" in bug:
        flat = x.reshape(-1)
        xm.reshape(-1)[1:], xp.reshape(-1)[:-1] = flat[:-1], flat[1:]
    return xm, xp


def sb_inputs(case):
    """x has mean 3 when the ratio is not 0 (an input far from zero); the convolution's bias then completes |mean(y)| / std(y) to the
    case's ratio exactly -- at F < 64 the padded columns bound what the input's offset alone can reach."""
    B, F, ratio = case
    rng = _rng(B, F, 14)
    cw, gamma, beta = np.array([0.3, 0.55, -0.2], dtype=f32), np.array([-1.3 if B % 2 else 0.8], dtype=f32), np.array([0.1], dtype=f32)
    x = _r32(rng, (B, F), 1.0, 3.0 if ratio else 0.0)
    xm, xp = _taps(x.astype(f64), f64)
    y0 = cw[0] * xm + cw[1] * x + cw[2] * xp
    sd = y0.std() if y0.size > 1 and y0.std() > 0 else 1.0
    cb = np.array([ratio * sd - y0.mean() if ratio else 0.05], dtype=f32)
    return dict(x=x, cw=cw, cb=cb, gamma=gamma, beta=beta, rmean=np.array([0.4 + float(cb[0])], dtype=f32), rvar=np.array([0.6], dtype=f32),
                g32=_r32(rng, (B, F)), g16=bf16_bits(_r32(rng, (B, F))))


def _sb_y(x, cw, cb, dt, bug=()):
    w0, w1, w2 = (cw.astype(dt)[k] for k in ((2, 1, 0) if "taps_reversed" in bug else (0, 1, 2)))
    xm, xp = _taps(x, dt, bug)
    y = w0 * xm + w1 * x + w2 * xp + cb.astype(dt)[0]
    uy = np.abs(w0 * xm) + np.abs(w1 * x) + np.abs(w2 * xp) + np.abs(cb.astype(dt)[0])
    return y, uy, (xm, xp)


def stencil_bn_fwd(x, cw, cb, gamma, beta, eps, mom, training, rmean, rvar, calls=2, dt=f64, bug=()):
    """z, save = (mean, invstd) and the running statistics after `calls` training calls (eval: the running statistics normalise)."""
    x = x.astype(dt)
    n = x.size
    one = dt(1.0)
    y, uy, _ = _sb_y(x, cw, cb, dt, bug)
    g, b, mo = gamma.astype(dt)[0], beta.astype(dt)[0], _h(mom, dt)
    rm, rv = rmean.astype(dt)[0], rvar.astype(dt)[0]
    urm, urv = np.abs(rm), np.abs(rv)
    if training:
        mean, umean = y.mean(dtype=dt), uy.mean(dtype=dt)
        var = np.maximum((y * y).mean(dtype=dt) - mean * mean, dt(0.0))
        uvar = (uy * uy).mean(dtype=dt) + umean * umean
        invstd = one / np.sqrt(var + _h(eps, dt))
        uinv = invstd * (one + dt(0.5) * invstd * invstd * uvar)
        unb = var if "biased_running_var" in bug else var * dt(n) / dt(max(n - 1, 1))
        for _ in range(calls):
            if "momentum_on_old" in bug:
                rm, rv = mo * rm + (one - mo) * mean, mo * rv + (one - mo) * unb
            else:
                rm, rv = (one - mo) * rm + mo * mean, (one - mo) * rv + mo * unb
            urm, urv = (one - mo) * urm + mo * umean, (one - mo) * urv + mo * uvar * dt(n) / dt(max(n - 1, 1))
    else:
        mean, umean = rm, dt(0.0)
        invstd = one / np.sqrt(rv + _h(eps, dt))
        uinv = invstd
    z = g * (y - mean) * invstd + b
    uz = np.abs(g) * ((uy + np.abs(mean) + umean) * invstd + np.abs(y - mean) * uinv) + np.abs(b)
    A = np.asarray
    return {"z32": (z, uz), "z16": (z, uz), "mean": (A(mean), A(umean + np.abs(mean))), "invstd": (A(invstd), A(uinv)),
            "rmean": (A(rm), A(urm)), "rvar": (A(rv), A(urv))}


def stencil_bn_bwd(x, grad, gbf, cw, cb, gamma, save, training, dt=f64, bug=()):
    """dx and the six parameter gradients; save = (mean, invstd), the forward's float32 values taken as given."""
    x, gz = x.astype(dt), _wide(grad, gbf, dt)
    n = dt(x.size)
    y, uy, (xm, xp) = _sb_y(x, cw, cb, dt, bug)
    w0, w1, w2 = (cw.astype(dt)[k] for k in ((2, 1, 0) if "taps_reversed" in bug else (0, 1, 2)))
    mean, invstd = dt(save[0]), dt(save[1])                   # float32 values as the device reads them (float64: the autograd check)
    k = gamma.astype(dt)[0] * invstd
    yh, uyh = (y - mean) * invstd, (uy + np.abs(y - mean)) * invstd
    sg, sgy = gz.sum(dtype=dt), (gz * yh).sum(dtype=dt)
    usg, usgy = np.abs(gz).sum(dtype=dt), (np.abs(gz) * uyh).sum(dtype=dt)
    live = training or "frozen_as_training" in bug
    mg, mgy = (sg / n, sgy / n) if live else (dt(0.0), dt(0.0))
    umg, umgy = (usg / n, usgy / n) if live else (dt(0.0), dt(0.0))
    dy = k * (gz - mg - yh * mgy)
    udy = np.abs(k) * (np.abs(gz) + umg + uyh * umgy + np.abs(yh) * umgy)
    sh = lambda a, s: _taps(a, dt)[s]                     # noqa: E731   (0: a[i - 1], 1: a[i + 1])
    dx = w0 * sh(dy, 1) + w1 * dy + w2 * sh(dy, 0)
    udx = np.abs(w0) * sh(udy, 1) + np.abs(w1) * udy + np.abs(w2) * sh(udy, 0)
    out = {"dx": (dx, udx)}
    for name, a in (("dw0", xm), ("dw1", x), ("dw2", xp)):
        out[name] = (np.asarray((dy * a).sum(dtype=dt)), np.asarray((udy * np.abs(a)).sum(dtype=dt)))
    out["db"] = (np.asarray(dy.sum(dtype=dt)), np.asarray(udy.sum(dtype=dt)))
    out["dgamma"], out["dbeta"] = (np.asarray(sgy), np.asarray(usgy)), (np.asarray(sg), np.asarray(usg))
    return out


@functools.lru_cache(maxsize=None)
def sb_saved(case, training):
    """(mean, invstd) the backward of a case is given: the float64 forward's, rounded to float32."""
    i = sb_inputs(case)
    f = stencil_bn_fwd(i["x"], i["cw"], i["cb"], i["gamma"], i["beta"], SB_EPS, SB_MOM, training, i["rmean"], i["rvar"])
    return np.array([f["mean"][0], f["invstd"][0]], dtype=f32)


# =================================================================================================================================
# fused_bn.hip: [sum of up to three addends] -> BatchNorm1d over the rows -> LeakyReLU -> dropout
# =================================================================================================================================
FB_SHAPES = [(2, 1), (15, 17), (16, 16), (17, 15), (128, 33), (129, 33), (300, 350)]
FB_EPS, FB_MOM = 1e-5, 0.1
FB_SLOPES = (None, 0.01, 0.0)          # no activation, LeakyReLU(0.01), slope 0
FB_PS = (0.0, 0.1, 0.5)


def _fb_cases():
    """A covering set: every shape six times; the addends, the type, normalisation off (k = 5), the activation, p and eval mode (k = 4)
    cycle so that each value meets each shape (and each other option at some shape).
    (B, F, addends, bf16, norm, slope, p, training, running buffers, z_save given)"""
    out = []
    for s, (B, F) in enumerate(FB_SHAPES):
        for k in range(6):
            training = 0 if k == 4 else 1
            out.append((B, F, 1 + (s + k) % 3, (s + k // 2) % 2 == 1, k != 5, FB_SLOPES[(s + k) % 3 if k != 5 else 1 + s % 2],
                        FB_PS[(s // 3 + k) % 3], training, training == 0 or (s + k) % 2 == 0, (s + k) % 3 != 0 or k % 2 == 1))
    return out


# A seed (bit 62 set) under which, at call counter 5, element FB_TIE_INDEX of a (300, 350) launch draws u == 0.5 EXACTLY: with p = 0.5
# that element is kept by u >= p and dropped by u > p (found by inverting the two-round hash; asserted by the reference test)
FB_TIE_SEED, FB_TIE_CALL, FB_TIE_INDEX = 0x400000002545F4D6, 5, 48513
FB_TIE_CASE = (300, 350, 1, False, True, 0.01, 0.5, 1, True, True)
FB_CASES = _fb_cases() + [FB_TIE_CASE]


@functools.lru_cache(maxsize=None)
def fb_seed_call(case):
    """(seed, call counter) of a case.  The counter takes COUNTERS' values in turn down the table; the seed is the first of SEED,
    SEED + 1, ... under which every column has both kept and dropped elements (asserted by the reference test)."""
    if case == FB_TIE_CASE:
        return FB_TIE_SEED, FB_TIE_CALL
    B, F, p, call = case[0], case[1], case[6], COUNTERS[FB_CASES.index(case) % 3]
    if not (case[7] and p > 0):
        return SEED, call
    idx = np.arange(B * F, dtype=np.uint64).reshape(B, F)
    for seed in range(SEED, SEED + 4096):
        keep = keep_mask(seed, call, idx, p)
        if keep.any(0).all() and (~keep).any(0).all():
            return seed, call
    raise AssertionError(("no seed with kept and dropped elements in every column", case))


def fb_keep(case, bug=()):
    B, F, p = case[0], case[1], case[6]
    seed, call = fb_seed_call(case)
    r, c = np.arange(B, dtype=np.uint64)[:, None], np.arange(F, dtype=np.uint64)[None, :]
    idx = c * np.uint64(B) + r if "mask_transposed" in bug else r * np.uint64(F) + c
    return keep_mask(seed, call, idx, p if case[7] else 0.0, bug)


def _fb_raw_inputs(case, salt):
    B, F, na, bf = case[:4]
    rng = _rng(B, F, na, int(bf), salt, 15)
    shift = 15.0 * ((np.arange(F) % 5) - 2)                              # column means up to 30 standard deviations
    xs = [_r32(rng, (B, F), 1.0 if k == 0 else 0.5, shift if k == 0 else 0.0) for k in range(na)]
    if bf:
        xs = [bf16_bits(a) for a in xs]
    sign = np.where(np.arange(F) % 2 == 0, 1.0, -1.0)
    return dict(xs=xs, gamma=(sign * rng.uniform(0.5, 1.5, F)).astype(f32), beta=_r32(rng, F, 0.3), dy=bf16_bits(_r32(rng, (B, F))) if bf else
                _r32(rng, (B, F)), rmean=(shift + 0.2 * rng.standard_normal(F)).astype(f32), rvar=rng.uniform(0.5, 1.5, F).astype(f32))


def fb_sum(xs, bf, dt=f64, bug=()):
    """The summed input and its unit.  bf16 with more than one addend: the sum ROUNDED to bf16 is what is normalised and saved."""
    ws = [_wide(a, bf, dt) for a in xs]
    if "drop_second" in bug and len(ws) > 1:
        ws = ws[:1] + ws[2:]
    z, uz = ws[0], np.abs(ws[0])
    for a in ws[1:]:
        z, uz = z + a, uz + np.abs(a)
    return z, (uz if len(xs) > 1 else np.zeros_like(uz))


def fb_stored_sum(xs, bf, bug=()):
    """The float32 evaluation's z as it is stored (and, for bf16, normalised): float32 array holding float32 or bf16 values."""
    z, _ = fb_sum(xs, bf, f32, bug)
    if bf and len(xs) > 1 and "no_bf16_round" not in bug:
        z = bf16_f32(bf16_bits(z))
    return z


def _fb_stats32(z, B):
    """float32 (mean, M2) of every column the kernel's way: row r belongs to group r % 16; each group runs Welford over its rows, then
    the sixteen (count, mean, M2) are combined in order (Chan); groups that own no row are skipped."""
    F = z.shape[1]
    N, M, Q = np.zeros(F, dtype=f32), np.zeros(F, dtype=f32), np.zeros(F, dtype=f32)
    for rg in range(16):
        rows = z[rg::16]
        if rows.shape[0] == 0:
            continue
        cnt, mu, m2 = f32(0.0), np.zeros(F, dtype=f32), np.zeros(F, dtype=f32)
        for zz in rows:
            cnt = f32(cnt + f32(1.0))
            d = zz - mu
            mu = mu + d / cnt
            m2 = m2 + d * (zz - mu)
        nt, d = N + cnt, mu - M
        Q = Q + (m2 + d * d * (N * cnt / nt))
        M = M + d * (cnt / nt)
        N = nt
    return M, Q


def fused_bn_fwd(z, bf, gamma, beta, eps, mom, training, rmean, rvar, slope, p, keep, dt=f64, bug=()):
    """Everything after the sum, from the STORED z (taken as given): y, mean, rstd, running statistics after one call, and `pre`, the
    pre-activation with its unit (for the LeakyReLU-side condition)."""
    z = np.asarray(z, dtype=f32).astype(dt)
    B = z.shape[0]
    one = dt(1.0)
    out = {}
    if gamma is not None:
        g, b = gamma.astype(dt), beta.astype(dt)
        mabs = np.abs(z).mean(0, dtype=dt)
        if training:
            if dt is f32:
                mean, Q = _fb_stats32(z, B)
            else:
                mean = z.mean(0, dtype=dt)
                Q = ((z - mean) ** 2).sum(0, dtype=dt)
            var = Q / dt(B - 1 if "var_bm1" in bug and B > 1 else B)
            c = z - mean
            uc = np.abs(c) + mabs
            uvar = (c * c + dt(2.0) * np.abs(c) * uc).mean(0, dtype=dt)
            rstd = one / np.sqrt(var + _h(eps, dt))
            urstd = rstd * (one + dt(0.5) * rstd * rstd * uvar)
            out["mean"], out["rstd"] = (mean, mabs), (rstd, urstd)
            if rmean is not None:
                mo, fac = _h(mom, dt), dt(B) / dt(max(B - 1, 1))
                out["rmean"] = ((one - mo) * rmean.astype(dt) + mo * mean, (one - mo) * np.abs(rmean.astype(dt)) + mo * mabs)
                out["rvar"] = ((one - mo) * rvar.astype(dt) + mo * var * fac, (one - mo) * rvar.astype(dt) + mo * uvar * fac)
        else:
            mean, rstd = rmean.astype(dt), one / np.sqrt(rvar.astype(dt) + _h(eps, dt))
            c = z - mean
            uc, urstd = np.abs(c), rstd
        pre = c * rstd * g + b
        upre = np.abs(g) * (uc * rstd + np.abs(c) * urstd) + np.abs(pre)
        side = z if "side_from_z" in bug else pre
    else:
        pre, upre, side = z, np.zeros_like(z), z
    y, uy = pre, (upre if gamma is not None else np.abs(pre))
    if slope is not None:
        sl = _h(slope, dt)
        y, uy = np.where(side > 0, y, y * sl), np.where(side > 0, uy, uy * np.abs(sl))
    ks = _ks(p, dt) if training else one
    out["y"] = (np.where(keep, y * ks, dt(0.0)), np.where(keep, uy * ks, dt(0.0)))
    out["pre"] = (pre, upre)
    return out


def fused_bn_bwd(dy, bf, z, mean, rstd, gamma, beta, slope, p, keep, dt=f64, bug=()):
    """dz, dgamma, dbeta from the stored z, mean, rstd (float32, taken as given) and the stored mask."""
    gy, z = _wide(dy, bf, dt), np.asarray(z, dtype=f32).astype(dt)
    B = dt(z.shape[0])
    ks = dt(1.0) if "no_ks_bwd" in bug else _ks(p, dt)
    gy = np.where(keep, gy * ks, dt(0.0))
    if gamma is None:
        if slope is not None:
            gy = np.where(z > 0, gy, gy * _h(slope, dt))
        return {"dz": (gy, np.abs(gy)), "pre": (z, np.zeros_like(z))}
    g, b, mu, rs = gamma.astype(dt), beta.astype(dt), mean.astype(dt), rstd.astype(dt)
    xh = (z - mu) * rs
    pre = xh * g + b
    if slope is not None:
        gy = np.where((z if "side_from_z" in bug else pre) > 0, gy, gy * _h(slope, dt))
    sg, sgx = gy.sum(0, dtype=dt), (gy * xh).sum(0, dtype=dt)
    usg, usgx = np.abs(gy).sum(0, dtype=dt), np.abs(gy * xh).sum(0, dtype=dt)
    k2 = g * rs
    dz = k2 * (gy - sg / B - xh * (sgx / B))
    udz = np.abs(k2) * (np.abs(gy) + usg / B + np.abs(xh) * usgx / B)
    return {"dz": (dz, udz), "dgamma": (sgx, usgx), "dbeta": (sg, usg), "pre": (pre, np.abs(xh * g) + np.abs(b))}


# Margin of the LeakyReLU-side condition in units of unit x EPS32: a fixed number (the inputs are drawn against it, so it must not move
# with the table) that is at least the GPU bound of fb.y and fb.dz (asserted by the reference test)
SIDE_MARGIN = 32.0


def side_margin_ok(pre_unit, slope):
    """No pre-activation lies within the float32 bound of zero: the LeakyReLU side is unambiguous in float32."""
    if slope is None:
        return True
    pre, unit = pre_unit
    return bool((np.abs(pre) > SIDE_MARGIN * unit * EPS32).all())


@functools.lru_cache(maxsize=None)
def fb_inputs_cached(case):
    return fb_inputs(case)


def fb_inputs(case):
    """Inputs of a case; with an activation, redrawn (salt 0, 1, ...) until no pre-activation of the forward or of the backward (which is
    given the float64 statistics rounded to float32) lies within the float32 bound of zero."""
    B, F, na, bf, norm, slope, p, training, running, zs = case
    for salt in range(64):
        i = _fb_raw_inputs(case, salt)
        z = fb_stored_sum(i["xs"], bf)
        gm, be = (i["gamma"], i["beta"]) if norm else (None, None)
        fwd = fused_bn_fwd(z, bf, gm, be, FB_EPS, FB_MOM, training, i["rmean"], i["rvar"], slope, p, fb_keep(case))
        ok = side_margin_ok(fwd["pre"], slope) if norm else bool(slope is None or (z != 0).all())
        if ok and training and norm:
            i["mean"], i["rstd"] = fwd["mean"][0].astype(f32), fwd["rstd"][0].astype(f32)
            bwd = fused_bn_bwd(i["dy"], bf, z, i["mean"], i["rstd"], gm, be, slope, p, fb_keep(case))
            ok = side_margin_ok(bwd["pre"], slope)
        if ok:
            return i
    raise AssertionError(("no draw with every pre-activation clear of zero", case))


# =================================================================================================================================
# The protocols: what is run and compared per case, stage by stage.  `impl` runs the stages -- tests/test_gpu_stream_kernels.py through
# the C ABI on the device, tests/test_stream_kernels_reference.py with the float32 evaluation (CpuImpl) -- and both are held to the
# same records: ("cmp", name, got, ref, unit, bf16), ("abs", name, got, ref, bound) and ("exact", label, holds).
# =================================================================================================================================
def sb_protocol(case, impl):
    i = sb_inputs(case)
    B, F, _ = case
    recs = []
    for zb, tr in ((zb, tr) for tr in (1, 0) for zb in (False, True)):
        got = impl.sb_fwd(case, i, zb, tr, 2)             # two calls: z, save, running statistics, num_batches_tracked (started at 7)
        ref = stencil_bn_fwd(i["x"], i["cw"], i["cb"], i["gamma"], i["beta"], SB_EPS, SB_MOM, tr, i["rmean"], i["rvar"], 2)
        zn = "z16" if zb else "z32"
        recs.append(("cmp", "sb." + zn, got["z"], *ref[zn], zb))
        for k in ("mean", "invstd", "rmean", "rvar"):
            recs.append(("cmp", "sb." + k, got[k], *ref[k], False))
        recs.append(("exact", f"num_batches_tracked training={tr}", got["nbt"] == 7 + 2 * tr))
        if not tr:
            recs.append(("exact", "eval leaves the running statistics alone", got["rmean"] == float(i["rmean"][0]) and got["rvar"] == float(i["rvar"][0])))
    for gb, tr in ((gb, tr) for tr in (1, 0) for gb in (False, True)):
        save = sb_saved(case, tr)
        grad = i["g16"] if gb else i["g32"]
        got = impl.sb_bwd(case, i, grad, gb, tr, save)
        ref = stencil_bn_bwd(i["x"], grad, gb, i["cw"], i["cb"], i["gamma"], save, tr)
        for k in ("dx", "dw0", "dw1", "dw2", "db", "dgamma", "dbeta"):
            recs.append(("cmp", "sb." + k, got[k], *ref[k], False))
    return recs


def fb_protocol(case, impl):
    B, F, na, bf, norm, slope, p, training, running, zs = case
    i = fb_inputs_cached(case)
    keep = fb_keep(case)
    seed, call = fb_seed_call(case)
    drop = bool(training and p > 0)
    gm, be = (i["gamma"], i["beta"]) if norm else (None, None)
    recs = []
    got = impl.fb_fwd(case, i, zs or na > 1, seed, call)
    if got["zsave"] is not None:
        recs.append(("cmp", "fb.zsave", got["zsave"], *_fb_zsave_ref(i["xs"], bf), bf))
        z = got["zsave"].astype(f32)
    else:
        z = _wide(i["xs"][0], bf, f32)
    rm, rv = (i["rmean"], i["rvar"]) if running else (None, None)
    ref = fused_bn_fwd(z, bf, gm, be, FB_EPS, FB_MOM, training, rm, rv, slope, p, keep)
    recs.append(("exact", "every pre-activation is clear of zero", (not norm) or side_margin_ok(ref["pre"], slope)))
    recs.append(("cmp", "fb.y", got["y"], *ref["y"], bf))
    for k in ("mean", "rstd", "rmean", "rvar"):
        if k in ref:
            recs.append(("cmp", "fb." + k, got[k], *ref[k], False))
    if drop:
        recs.append(("exact", "mask is the mirror's at r F + c", np.array_equal(got["mask"].astype(bool), keep) and (got["mask"] <= 1).all()))
        recs.append(("exact", "kept and dropped elements in every column", bool(keep.any(0).all() and (~keep).any(0).all())))
    recs.append(("exact", "call counter after the launch", got["counter"] == ((call + 1) if drop else call)))
    if norm and running:
        recs.append(("exact", "num_batches_tracked", got["nbt"] == 7 + (1 if training else 0)))
    if not training:
        return recs
    zg = fb_stored_sum(i["xs"], bf)
    mean, rstd = (i["mean"], i["rstd"]) if norm else (None, None)
    got = impl.fb_bwd(case, i, zg, mean, rstd, keep)
    ref = fused_bn_bwd(i["dy"], bf, zg, mean, rstd, gm, be, slope, p if drop else 0.0, keep)
    recs.append(("exact", "every pre-activation of the backward is clear of zero", (not norm) or side_margin_ok(ref["pre"], slope)))
    recs.append(("cmp", "fb.dz", got["dz"], *ref["dz"], bf))
    if norm:
        recs.append(("cmp", "fb.dgamma", got["dgamma"], *ref["dgamma"], False))
        recs.append(("cmp", "fb.dbeta", got["dbeta"], *ref["dbeta"], False))
    return recs


def _fb_zsave_ref(xs, bf):
    z, uz = fb_sum(xs, bf)
    return z, (uz if len(xs) > 1 else np.abs(z) * 0.0)


def fl_box(case):
    box = case[4]
    return (FL_LO if box in ("min", "both") else None), (FL_HI if box in ("max", "both") else None)


def fl_protocol(case, impl):
    B, C, nI, nD, box, alpha, alpha0, bf = case
    i = fl_inputs(case)
    lo, hi = fl_box(case)
    got = impl.fl(case, i, lo, hi)                        # two calls, loss_sum started at FL_SUM0
    ref = surrogate_loss_grad(i["p"], bf, i["t"], nI, nD, alpha, alpha0, lo, hi, FL_BOX_W, FL_PENALTY, FL_SUM0, 2)
    return [("cmp", "fl.loss", got["loss"], *ref["loss"], False), ("cmp", "fl.loss_sum", got["loss_sum"], *ref["loss_sum"], False),
            ("cmp", "fl.grad", got["grad"], *ref["grad"], bf)]


def fa_second_gradient(case, g):
    """The gradient of the second step: the first one reversed and scaled by 0.7."""
    return (g[::-1] * f32(0.7)).astype(f32)


def fa_protocol(case, impl):
    n, cfg = case[0], fa_config(case)
    i = fa_inputs(case)
    state = dict(p=i["p"], m=i["m"], v=i["v"])
    recs = []
    impl.fa_begin(case, i)
    for k in range(2):
        g = i["g"] if k == 0 else fa_second_gradient(case, i["g"])
        t = cfg["step0"] + k + 1
        normsq = fa_partials(g, cfg["grad_scale"], cfg["parts"]).sum() if cfg["parts"] else None
        got = impl.fa_step(case, state, g, FA_LRS[k], t)          # -> p, m, v (float32 arrays), shadow (uint16 or None), g, step
        ref = flat_clip_adam_step(state["p"], g, state["m"], state["v"], FA_LRS[k], t, cfg["max_norm"], cfg["grad_scale"], FA_B1, FA_B2, FA_EPS,
                                  cfg["wd"], cfg["flags"], normsq)
        for name in ("p", "m", "v"):
            recs.append(("cmp", "fa." + name, got[name].astype(f64), *ref[name], False))
        if cfg["shadow"]:
            recs.append(("cmp", "fa.shadow", bf16_f64(got["shadow"]), *ref["shadow"], True))
            recs.append(("exact", "shadow is the new parameter rounded to nearest even", np.array_equal(got["shadow"], bf16_bits(got["p"]))))
        recs.append(("exact", f"step counter after step {k + 1}", got["step"] == t))
        recs.append(("exact", "gradient zeroed" if cfg["flags"] & ZERO_GRADS else "gradient untouched",
                     np.array_equal(got["g"], np.zeros_like(g) if cfg["flags"] & ZERO_GRADS else g)))
        if n >= 3 and cfg["wd"] == 0:
            recs.append(("exact", "g = m = v = 0 leaves the parameter alone", np.array_equal(got["p"][1::5], state["p"][1::5])
                         and not got["m"][1::5].any() and not got["v"][1::5].any()) if k == 0 else ("exact", "-", True))
        state = dict(p=got["p"], m=got["m"], v=got["v"])
    impl.fa_end()
    return recs


def ip_protocol(case, impl):
    B, F, off, bf, C, counter, sigma = case
    i = ip_inputs(case)
    call = 0 if counter is None else counter
    got = impl.ip(case, i)                                # -> out (float64), yout (float32 or None), counter after (or None)
    ref = gather_rows_noise(i["X"], i["idx"], sigma, SEED, call)["out"][0]
    recs = [("abs", "ip.out16" if bf else "ip.out32", got["out"], ref, ip_bound(ref, sigma, bf))]
    if sigma is None or f32(sigma) == 0:
        want = bf16_f64(bf16_bits(i["X"][i["idx"]])) if bf else i["X"][i["idx"]].astype(f64)
        recs.append(("exact", "sigma = 0: the gather bit for bit", np.array_equal(got["out"], want)))
    if C:
        recs.append(("exact", "targets gathered bit for bit", np.array_equal(got["yout"], i["Y"][i["idx"]])))
    if counter is not None:
        recs.append(("exact", "call counter advanced by one", got["counter"] == counter + 1))
    return recs


PROTOCOLS = {"sb": (sb_protocol, SB_CASES), "fb": (fb_protocol, FB_CASES), "fl": (fl_protocol, FL_CASES), "fa": (fa_protocol, FA_CASES),
             "ip": (ip_protocol, IP_CASES)}


def measure(recs):
    """({name: largest error in units of unit x EPS32 (inf for a non-zero against an exact zero)}, {name: largest |got - ref| / bound of
    the absolute records}, [labels of the exact records that do not hold])."""
    ratios, absr, failed = {}, {}, []
    for rec in recs:
        if rec[0] == "cmp":
            _, name, got, ref, unit, bf = rec
            got, ref, unit = (np.asarray(a, dtype=f64) for a in (got, ref, unit))
            got = got.reshape(ref.shape)
            e = error_ratio(got, ref, unit, bf)
            if not np.isfinite(got).all() or (name in EXACT_ZERO and not exact_zeros(got, ref)):
                e = np.inf
            ratios[name] = max(ratios.get(name, 0.0), e)
        elif rec[0] == "abs":
            _, name, got, ref, bound = rec
            err = np.abs(np.asarray(got, dtype=f64).reshape(ref.shape) - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(err == 0, 0.0, err / bound)
            absr[name] = max(absr.get(name, 0.0), float(np.nan_to_num(r, nan=np.inf).max()))
        elif not rec[2]:
            failed.append(rec[1])
    return ratios, absr, failed


class CpuImpl:
    """The stages in float32 NumPy (with `bug`, a deliberately wrong variant): what CPU_CONST is measured on."""

    def __init__(self, bug=()):
        self.bug = frozenset([bug] if isinstance(bug, str) else bug)

    def sb_fwd(self, case, i, zb, tr, calls):
        o = stencil_bn_fwd(i["x"], i["cw"], i["cb"], i["gamma"], i["beta"], SB_EPS, SB_MOM, tr, i["rmean"], i["rvar"], calls, f32, self.bug)
        out = {k: float(f32(o[k][0])) for k in ("mean", "invstd", "rmean", "rvar")}
        out.update(z=_store(o["z32"][0], zb), nbt=7 + calls * tr)
        return out

    def sb_bwd(self, case, i, grad, gb, tr, save):
        o = stencil_bn_bwd(i["x"], grad, gb, i["cw"], i["cb"], i["gamma"], save, tr, f32, self.bug)
        return {k: _store(v[0], False) for k, v in o.items()}

    def fb_fwd(self, case, i, zs, seed, call):
        B, F, na, bf, norm, slope, p, training, running, _ = case
        z = fb_sum(i["xs"], bf, f32, self.bug)[0]
        zst = bf16_f32(bf16_bits(z)) if bf and na > 1 else z
        gm, be = (i["gamma"], i["beta"]) if norm else (None, None)
        rm, rv = (i["rmean"], i["rvar"]) if running else (None, None)
        keep = fb_keep(case, self.bug)
        o = fused_bn_fwd(z if "no_bf16_round" in self.bug else zst, bf, gm, be, FB_EPS, FB_MOM, training, rm, rv, slope, p, keep, f32, self.bug)
        out = {k: _store(o[k][0], False) for k in ("mean", "rstd", "rmean", "rvar") if k in o}
        drop = bool(training and p > 0)
        out.update(y=_store(o["y"][0], bf), zsave=_store(zst, bf) if zs else None, mask=keep.astype(np.uint8), counter=call + int(drop),
                   nbt=7 + (1 if training and norm else 0))
        return out

    def fb_bwd(self, case, i, z, mean, rstd, keep):
        B, F, na, bf, norm, slope, p, training, running, _ = case
        gm, be = (i["gamma"], i["beta"]) if norm else (None, None)
        o = fused_bn_bwd(i["dy"], bf, z, mean, rstd, gm, be, slope, p, keep, f32, self.bug)
        return {k: _store(v[0], bf and k == "dz") for k, v in o.items() if k != "pre"}

    def fl(self, case, i, lo, hi):
        B, C, nI, nD, box, alpha, alpha0, bf = case
        o = surrogate_loss_grad(i["p"], bf, i["t"], nI, nD, alpha, alpha0, lo, hi, FL_BOX_W, FL_PENALTY, FL_SUM0, 2, f32, self.bug)
        return dict(loss=_store(o["loss"][0], False), loss_sum=_store(o["loss_sum"][0], False), grad=_store(o["grad"][0], bf))

    def fa_begin(self, case, i):
        pass

    def fa_end(self):
        pass

    def fa_step(self, case, state, g, lr, t):
        cfg = fa_config(case)
        normsq = fa_partials(g, cfg["grad_scale"], cfg["parts"]).sum() if cfg["parts"] else None
        with np.errstate(all="ignore"):
            o = flat_clip_adam_step(state["p"], g, state["m"], state["v"], lr, t, cfg["max_norm"], cfg["grad_scale"], FA_B1, FA_B2, FA_EPS, cfg["wd"],
                                    cfg["flags"], normsq, f32, self.bug)
        p = o["p"][0].astype(f32)
        return dict(p=p, m=o["m"][0].astype(f32), v=o["v"][0].astype(f32), step=t, g=np.zeros_like(g) if cfg["flags"] & ZERO_GRADS else g,
                    shadow=bf16_bits(p, truncate="shadow_truncated" in self.bug) if cfg["shadow"] else None)

    def ip(self, case, i):
        B, F, off, bf, C, counter, sigma = case
        call = 0 if counter is None else counter
        v, _ = gather_rows_noise(i["X"], i["idx"], sigma, SEED, call, self.bug)["out"]
        return dict(out=_store(v, bf), yout=i["Y"][i["idx"]] if C else None, counter=None if counter is None else counter + 1)
