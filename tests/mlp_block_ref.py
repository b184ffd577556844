"""Float64 references, error units and the case tables of the PINN layer-block launches of csrc/mlp_block.hip (test code, NumPy):
`ops_mlp_strip_launch` -- the product with every tail, addition and side job -- and `ops_mlp_wgrad_group[_norm]`, ONE LAUNCH per
comparison, in the style of tests/stream_kernels_ref.py (whose helpers are imported, not copied).

Inputs are what the device receives: bf16 bit patterns (uint16), float32 arrays and hyper-parameters rounded to float32.  A launch is
a dict (`launch(...)` below builds one with its inputs); `strip(a, dt, bug, stored)` evaluates it -- dt = float64: the reference,
dt = float32: the documented formula in float32 with the product accumulated in the kernel's order (32-wide steps added to a running
float32 accumulator) and every bf16 rounding the kernel makes.  It returns {output: (value, unit, slack)}:

    unit    the output's formula with every sum replaced by the sum of the absolute values of its terms, in units of EPS32 = 2^-24
    slack   the half ulps of the bf16 roundings that lie between the launch's inputs and this output (an absolute allowance):
            |got - ref| <= slack + C unit EPS32,     C = 4 x CPU_CONST[output]

The roundings and how they enter (the reference itself rounds NOTHING but the bias):
    bias             rounded to bf16 on entry (an input transformation, exact in both evaluations)
    Linear output    bf16: 1/2 ulp; continuous tails carry it on: TAIL_ACT_DROP  keep_scale L (1/2 ulp_lin + C unit EPS32) + 1/2 ulp_Y
                     (L: the LeakyReLU's slope on that side, max(1, |slope|) where the pre-activation is within its bound of zero)
    stencil term     bf16: 1/2 ulp;   block sum  bf16: 1/2 ulp  -> the block sum carries three half ulps
    backward         bf16(product), bf16(product + dZ + stencil gradient): carried through the activation factor and the BatchNorm
                     backward by the same absolute-value formula as the unit
A value a later stage consumes is TAKEN AS GIVEN (`stored`): BatchNorm statistics, normalisation and the running buffers are those of
the STORED Zt; the loss gradient, the box penalty, sign(p - t) and the partial sums those of the STORED P; dbias is the column sum of
the STORED bf16 gradient; `spart` (the side job's partial sums) is an input of the launch that consumes it; the loss value is formed
from the stored partial sums; the norm partials of the weight gradients from the stored gradients.  So every bound is a one-stage
bound.  Exact zeros: a dropped element, a dead row or column and p == t must be 0; Y and Yt must hold identical bit patterns.

Constants.  A bf16 output, and whatever lies behind an intermediate rounding, shows its float32 error next to a rounding tie alone, so
CpuImpl also evaluates every launch WITHOUT the bf16 roundings (from the same stored Zt / P) and that twin is held to the reference
with no slack: CPU_CONST is the larger of the two measurements.  Where the slack would hide a float32 output -- dgamma, dbeta behind
bf16(product) -- the tables also run the tail behind an EXACT product (`exact`: small-integer operands, every partial sum an integer
below 2^8, so the product and its rounding are exact in any order): no slack there, on the device either.

Product ceiling: bf16 x bf16 is exact in float32, so only the additions round; ANY order of the K' = K r.u. 32 additions stays within
(K' - 1) unit 2^-24 to first order, 2 K' is the a-priori bound used here (`product_ceiling`), and 4 x CPU_CONST["prod.y"] must stay
below it for every K of the table (asserted by tests/test_mlp_block_reference.py).

`bug=`: deliberately wrong variants of the float32 evaluation (the teeth check):
    skip_last_step   the last 32-wide reduction step is not added          fa1_reuse       steps 24..31 multiply the operands of 8..15
    left_tap_col0    column 0 is not seen as a left neighbour (y[1] misses w0 x[0]; the transposed stencil likewise)
    right_tap_last   column No - 1 keeps a right tap: it reads the next row's column 0 (the transposed stencil: dy of that element)
    biased_running_var, count_padded (stencil count B (N r.u. 16)), invB_128 (1 / B over 128 rows), keep_gt, dbias_unrounded,
    dgamma_no_mean, yt_tile_transposed, loss_mean_N (data term of the first group divided by B N), wgrad_past_edge (a tile written past
    N or K), range_half (a range's partial sum misses elements i + 64)
"""
import numpy as np

from tests.stream_kernels_ref import (COUNTERS, EPS32, SEED, SENT_BF16, SENT_F32, bf16_bits, bf16_f32, bf16_f64, error_ratio,  # noqa: F401
                                      exact_zeros, keep_mask, surrogate_loss_grad, ulp_bf16, FB_TIE_CALL, FB_TIE_INDEX, FB_TIE_SEED)

f32, f64 = np.float32, np.float64
ROWS = 128
NONE, ACT_DROP, BN_ACT_DROP, BN, BWD_ACT_DROP, BWD_BN, BWD_BN_ACT_DROP, LOSS = range(8)      # OPS_MLP_TAIL_*
ADD_NONE, ADD_FWD, ADD_BWD = range(3)                                                         # OPS_MLP_ADD_*
SIDE_NONE, SIDE_FWD, SIDE_BWD = range(3)                                                      # OPS_MLP_SIDE_*
TAIL_NAMES = ("none", "act_drop", "bn_act_drop", "bn", "bwd_act_drop", "bwd_bn", "bwd_bn_act_drop", "loss")
FWD_TAILS, BN_TAILS, ACT_BWD = (NONE, ACT_DROP, BN_ACT_DROP, BN, LOSS), (BN, BN_ACT_DROP, BWD_BN, BWD_BN_ACT_DROP), (BWD_ACT_DROP, BWD_BN_ACT_DROP)
# the twelve combinations ops_mlp_strip_launch compiles with their mode folded in: (tail, add_mode, eval_stats)
COMPILED = [(BN_ACT_DROP, 0, 0), (ACT_DROP, 0, 0), (BN, ADD_FWD, 0), (LOSS, 0, 0), (BWD_BN, 0, 0), (BWD_ACT_DROP, 0, 0), (BWD_BN, ADD_BWD, 0),
            (BWD_BN_ACT_DROP, ADD_BWD, 0), (BN_ACT_DROP, 0, 1), (ACT_DROP, 0, 1), (BN, ADD_FWD, 1), (LOSS, 0, 1)]
# valid combinations that fall through to the generic kernel
GENERIC_ONLY = [(BN, 0, 0), (NONE, ADD_FWD, 0), (BWD_ACT_DROP, ADD_BWD, 0), (BN, 0, 1), (NONE, 0, 0), (BWD_BN_ACT_DROP, 0, 0), (ACT_DROP, ADD_FWD, 0)]
EPS, MOM, SEPS, SMOM = 1e-5, 0.1, 1e-5, 0.1
NBT0, SUM0 = 7, 3.25
LO, HI, BOX_W, PENALTY = -0.75, 0.875, 0.1, 1.5e-6

# Largest constant of the float32 evaluation per output over the tables below (tests/test_mlp_block_reference.py asserts that none is
# exceeded and prints the measured values; an entry is the measurement plus about 12 %); the GPU bound is four times the entry.
CPU_CONST = {
    "prod.y": 1.05, "fwd.z": 1.20, "fwd.y": 1.55, "fwd.mean": 1.00, "fwd.rstd": 2.50, "fwd.rmean": 1.65, "fwd.rvar": 1.95,
    "st.part": 2.15, "st.save": 0.90, "st.rmean": 1.80, "st.rvar": 1.05, "st.bsums": 1.05, "st.dparams": 1.05,
    "bwd.y": 0.90, "bwd.dgamma": 0.30, "bwd.dbeta": 0.35, "bwd.dbias": 0.50,
    "loss.p": 1.15, "loss.grad": 4.55, "loss.dbias": 3.25, "loss.parts": 1.50, "loss.value": 2.25, "loss.sum": 1.70,
    "wg.out": 1.25, "wg.part": 1.35, "wg.range": 0.60,
}
EXACT_ZERO = {"fwd.y", "bwd.y", "loss.grad"}


def bound_constant(name: str) -> float:
    return 4.0 * CPU_CONST[name]


def product_ceiling(K: int) -> float:
    return 2.0 * ru(K, 32)


def ru(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _h(v, dt):
    return dt(f32(v))


# =================================================================================================================================
# the fragment-tiled storage (include/openpystruct_amd.h; checked against pinn_fused.to_tiled / from_tiled)
# =================================================================================================================================
def to_tiled(x):
    """[rows, K] (rows % 16 == 0, K % 32 == 0) -> tile (row >> 4, k >> 5) of 512 elements, element ((k >> 3) & 3) * 128 + (row & 15) * 8 + (k & 7)."""
    R, K = x.shape
    return np.ascontiguousarray(x.reshape(R // 16, 16, K // 32, 4, 8).transpose(0, 2, 3, 1, 4)).reshape(R, K)


def from_tiled(t):
    R, K = t.shape
    return np.ascontiguousarray(t.reshape(R // 16, K // 32, 4, 16, 8).transpose(0, 3, 1, 2, 4)).reshape(R, K)


def tiled_offset(row, k, KS):
    """mb_toff of mlp_block.hip: the element offset of (row, k) in a tiled matrix of KS steps."""
    return ((row >> 4) * KS + (k >> 5)) * 512 + ((k >> 3) & 3) * 128 + (row & 15) * 8 + (k & 7)


def pack(bits, rows, ld, live_k=None):
    """A [r, k] matrix of bf16 bit patterns in tiled storage [rows, ld]: zero outside the live corner up to k r.u. 32, and the SENTINEL in
    the columns from there to ld (a larger leading dimension: columns the kernel must never read)."""
    r, k = bits.shape
    out = np.full((rows, ld), SENT_BF16, dtype=np.uint16)
    out[:, :ru(k if live_k is None else live_k, 32)] = 0
    out[:r, :k] = bits
    return to_tiled(out)


def pack_t(bits, rows_t=None):
    """The transposed copy [cols r.u. 32, 128] of a [B, cols] matrix."""
    return pack(np.ascontiguousarray(bits.T), rows_t or ru(bits.shape[1], 32), ROWS, ROWS)


# =================================================================================================================================
# pieces
# =================================================================================================================================
def _product(Ab, Wb, dt, bug=()):
    """A W^T over K r.u. 32 in 32-wide steps added to a running accumulator of type dt (a step's 32 exact products are summed in float64:
    the MFMA's internal order is part of the factor four); unit: |A| |W|^T."""
    a, w = bf16_f64(Ab), bf16_f64(Wb)
    (B, K), N = a.shape, w.shape[0]
    Kp = ru(K, 32)
    ap, wp = np.zeros((B, Kp)), np.zeros((N, Kp))
    ap[:, :K], wp[:, :K] = a, w
    steps = list(range(Kp // 32))
    if "skip_last_step" in bug and len(steps) > 1:
        steps = steps[:-1]
    if "fa1_reuse" in bug:
        steps = [s - 16 if 24 <= s < 32 else s for s in steps]
    acc = np.zeros((B, N), dtype=dt)
    for s in steps:
        acc = (acc + (ap[:, 32 * s:32 * s + 32] @ wp[:, 32 * s:32 * s + 32].T).astype(dt)).astype(dt)
    return acc, np.abs(a) @ np.abs(w).T


def _shift(x, s, bug=()):
    """x[:, c + s] with zeros outside (s = -1: the left neighbour, +1: the right one)."""
    out = np.zeros_like(x)
    if x.shape[1] > 1:
        if s < 0:
            out[:, 1:] = x[:, :-1]
            if "left_tap_col0" in bug:
                out[:, 1] = 0
        else:
            out[:, :-1] = x[:, 1:]
    if s > 0 and "right_tap_last" in bug:
        flat = x.reshape(-1)
        out[:-1, -1] = x[1:, 0]
        out[-1, -1] = flat[0]
    return out


def _conv(O, cw, cb, dt, bug=()):
    w0, w1, w2, b = (dt(v) for v in (*cw, cb[0]))
    xm, xp = _shift(O, -1, bug), _shift(O, 1, bug)
    y = w0 * xm + w1 * O + w2 * xp + b
    return y, np.abs(w0 * xm) + np.abs(w1 * O) + np.abs(w2 * xp) + np.abs(b), (xm, xp)


def side_rows(No):
    return (No + 7) // 8


def _rb(x, dt, bug=()):
    """An intermediate bf16 rounding: made by the float32 evaluation (but for its twin without them), carried as slack by the reference."""
    return x if dt is f64 or "_unrounded" in bug else bf16_f32(bf16_bits(x))


def _hu(x):
    return 0.5 * ulp_bf16(x)


def _wide(bits, dt):
    """bf16 bit patterns widened (a float array passes as it is: the autograd check feeds unrounded activations)."""
    bits = np.asarray(bits)
    return bf16_f32(bits).astype(dt) if bits.dtype == np.uint16 else bits.astype(dt)


def side_job(a, dt=f64, bug=()):
    """The partial sums a SIDE_* launch leaves in spart, row by row (8 columns of the block input each): (value [rows, 2 or 12], unit)."""
    B, No = a["B"], a["No"]
    O = _wide(a["O"], dt)
    y, uy, (xm, xp) = _conv(O, a["cw"], a["cb"], dt, bug)
    if a["side"] == SIDE_FWD:
        terms = [(y, uy), (y * y, 2 * np.abs(y) * uy + y * y)]
    else:
        g = _wide(a["dZ"], dt)
        mean_s, inv_s = dt(a["ssave"][0]), dt(a["ssave"][1])
        yh = (y - mean_s) * inv_s
        uyh = (uy + np.abs(y) + np.abs(mean_s)) * np.abs(inv_s) + np.abs(yh)
        xs = (xm, O, xp)
        terms = [(g, np.abs(g)), (g * yh, np.abs(g) * uyh), (yh, uyh)] + [(g * x, np.abs(g * x)) for x in xs] + [(x, np.abs(x)) for x in xs] + \
                [(yh * x, uyh * np.abs(x)) for x in xs]
    rows = side_rows(No)
    val, unit = np.zeros((rows, len(terms))), np.zeros((rows, len(terms)))
    for j in range(rows):
        for k, (t, u) in enumerate(terms):
            val[j, k] = t[:, 8 * j:8 * j + 8].sum(dtype=dt)
            unit[j, k] = u[:, 8 * j:8 * j + 8].sum(dtype=f64)
    return val, unit


def _bn_stats(z, B, eps, dt, bug):
    Bd = dt(ROWS if "invB_128" in bug else B)
    mean = z.sum(0, dtype=dt) / Bd
    c = z - mean
    var = (c * c).sum(0, dtype=dt) / Bd
    mabs = np.abs(z).sum(0, dtype=dt) / dt(B)
    uc = np.abs(c) + mabs
    uvar = (c * c + dt(2) * np.abs(c) * uc).sum(0, dtype=dt) / dt(B)
    rstd = dt(1) / np.sqrt(var + _h(eps, dt))
    return mean, mabs, var, uvar, rstd, rstd * (dt(1) + dt(0.5) * rstd * rstd * uvar)


# =================================================================================================================================
# ops_mlp_strip_launch
# =================================================================================================================================
def strip(a, dt=f64, bug=(), stored=None):
    """{output: (value, unit, slack)} of one strip launch (see the module docstring).  `stored`: what the launch left in memory and
    later stages of the same launch consume -- "Z" (Zt as [B, N] bit patterns), "P", "Y" -- taken as given where present; without it
    the evaluation goes on with its own value (float64: unrounded, the plain composition autograd can be compared with)."""
    st = stored or {}
    B, N, tail, add = a["B"], a["N"], a["tail"], a["add"]
    fwd, has_bn = tail in FWD_TAILS, tail in BN_TAILS
    one = dt(1)
    out = {}
    zero = np.zeros((B, N))
    acc, uacc = _product(a["A"], a["W"], dt, bug)
    ks = one / (one - _h(a["p"], dt)) if f32(a["p"]) > 0 else one
    sl = _h(a["slope"], dt)
    if a["side"] != SIDE_NONE:
        v, u = side_job(a, dt, bug)
        out["spart"] = (v, u, np.zeros_like(u))
    if add != ADD_NONE:
        No = a["No"]
        O = _wide(a["O"], dt)
        conv, uconv, _ = _conv(O, a["cw"], a["cb"], dt, bug)
        NS = 2 if fwd else 12
        tot = np.asarray(a["spart"], dtype=f64).reshape(-1, NS)[:side_rows(No)].sum(0)
        n = float(B) * (ru(N, 16) if "count_padded" in bug else No)
        sg_, sb_ = dt(a["sgamma"][0]), dt(a["sbeta"][0])
    if fwd:
        bias_b = _wide(bf16_bits(a["bias"]), dt) if a["bias"] is not None else np.zeros(N, dtype=dt)
        x = (acc + bias_b).astype(dt)
        ux = uacc + np.abs(bias_b)
        sx, rounded = _hu(x), True
        x = _rb(x, dt, bug)
        if add == ADD_FWD:
            m = tot[0] / n
            var = max(tot[1] / n - m * m, 0.0)
            if a["eval_stats"]:
                mean_s, inv_s = dt(a["srm"][0]), 1.0 / np.sqrt(f64(a["srv"][0]) + f64(f32(a["seps"])))
            else:
                mean_s, inv_s = m, 1.0 / np.sqrt(var + f64(f32(a["seps"])))
                mo = _h(a["smom"], dt)
                unb = var if "biased_running_var" in bug else var * n / (n - 1.0 if n > 1 else 1.0)
                out["ssave"] = (np.array([mean_s, inv_s]), np.abs(np.array([mean_s, inv_s])), np.zeros(2))
                rm, rv = dt(a["srm"][0]), dt(a["srv"][0])
                m_, unb_ = (dt(f32(m)), dt(f32(unb))) if dt is f32 else (m, unb)
                out["srm"] = (np.asarray((one - mo) * rm + mo * m_), np.asarray((one - mo) * np.abs(rm) + mo * abs(m)), np.zeros(()))
                out["srv"] = (np.asarray((one - mo) * rv + mo * unb_), np.asarray((one - mo) * np.abs(rv) + mo * abs(unb)), np.zeros(()))
            if dt is f32:
                mean_s, inv_s = f32(mean_s), f32(inv_s)
            mean_s, inv_s = dt(mean_s), dt(inv_s)
            scale = sg_ * inv_s
            shift = sb_ - mean_s * scale
            s = conv * scale + shift
            us = np.abs(scale) * uconv + np.abs(conv * scale) + 2 * np.abs(mean_s * scale) + np.abs(sb_) + np.abs(s)
            ss = _hu(s)
            s = _rb(s, dt, bug)
            z = (x + s + O).astype(dt)
            ux = ux + us + np.abs(x) + np.abs(s) + np.abs(O)
            sx = sx + ss + _hu(z)
            x = _rb(z, dt, bug)
        if has_bn:
            out["z"], rounded = (x, ux, sx), False
            z = _wide(st["Z"], dt) if "Z" in st else x
            g, be = a["gamma"].astype(dt), a["beta"].astype(dt)
            if a["eval_stats"]:
                mean, rstd = a["rmean"].astype(dt), one / np.sqrt(a["rvar"].astype(dt) + _h(a["eps"], dt))
                c = z - mean
                uc, urstd = np.abs(z) + np.abs(mean), rstd
            else:
                mean, mabs, var, uvar, rstd, urstd = _bn_stats(z, B, a["eps"], dt, bug)
                c = z - mean
                uc = np.abs(c) + mabs
                zz = np.zeros(N)
                out["mean"], out["rstd"] = (mean, mabs, zz), (rstd, urstd, zz)
                if a["rmean"] is not None:
                    mo, fac = _h(a["momentum"], dt), (one if "biased_running_var" in bug else dt(B) / dt(max(B - 1, 1)))
                    rm, rv = a["rmean"].astype(dt), a["rvar"].astype(dt)
                    out["rmean"] = ((one - mo) * rm + mo * mean, (one - mo) * np.abs(rm) + mo * mabs, zz)
                    out["rvar"] = ((one - mo) * rv + mo * var * fac, (one - mo) * np.abs(rv) + mo * (uvar + var) * fac, zz)
            x = c * rstd * g + be
            ux, sx = np.abs(g) * (uc * rstd + np.abs(c) * urstd) + np.abs(x) + np.abs(be), zero
        if tail in (ACT_DROP, BN_ACT_DROP):
            r, c_ = np.arange(B, dtype=np.uint64)[:, None], np.arange(N, dtype=np.uint64)[None, :]
            keep = keep_mask(a["seed"], a["call"] or 0, r * np.uint64(N) + c_, a["p"], bug)
            near0 = np.abs(x) <= 2 * sx + 4096 * ux * EPS32
            L = np.where(near0, max(1.0, abs(float(sl))), np.where(x > 0, 1.0, abs(float(sl))))
            y = np.where(x > 0, x, x * sl)
            y = np.where(keep, y * ks, dt(0))
            ux, sx = np.where(keep, float(ks) * L * ux + np.abs(y), 0.0), np.where(keep, float(ks) * L * sx, 0.0)
            x, rounded = y.astype(dt), False
            out["keep"] = keep
        if tail == LOSS:
            out["p"], rounded = (x, ux, sx), False
            pb = st["P"] if "P" in st else bf16_bits(x.astype(f32))
            lo, hi = a["lo"], a["hi"]
            ref = surrogate_loss_grad(pb, True, a["targets"], a["nI"], a["nD"], a["alpha"], a["alpha0"], lo, hi, a["box_w"], a["pen"], a["sum0"], 2, dt)
            g, ug = ref["grad"]
            if "loss_mean_N" in bug:
                nI = a["nI"]
                p_ = bf16_f64(pb)[:, :nI]
                gbox = np.zeros_like(p_)
                if lo is not None:
                    gbox -= np.where(p_ < f64(f32(lo)), f64(f32(a["box_w"])), 0.0)
                if hi is not None:
                    gbox += np.where(p_ > f64(f32(hi)), f64(f32(a["box_w"])), 0.0)
                g = g.copy()
                g[:, :nI] = ((g[:, :nI] - gbox) * nI / N + gbox).astype(dt)
            out["value"] = (*ref["loss"], np.zeros(()))
            out["parts"] = (*_loss_parts(pb, a, dt), 0.0)
            x, ux, sx = g, ug, zero
        out["y"] = (x, ux, sx if rounded else sx + _hu(x))
    else:
        # (small-integer operands, `exact`: the product and its bf16 rounding are exact in any order -- no slack, so the tail behind it
        # is held at float32 level)
        x, ux, sx = _rb(acc, dt, bug), uacc, (zero if a.get("exact") else _hu(acc))
        if add == ADD_BWD:
            gz = _wide(a["dZ"], dt)
            mean_s, inv_s = dt(a["ssave"][0]), dt(a["ssave"][1])
            yh = (conv - mean_s) * inv_s
            uyh = (uconv + np.abs(conv) + np.abs(mean_s)) * np.abs(inv_s) + np.abs(yh)
            mg, mgy = dt(f32(tot[0] / n)) if dt is f32 else tot[0] / n, dt(f32(tot[1] / n)) if dt is f32 else tot[1] / n
            kk = sg_ * inv_s
            dy = kk * (gz - mg - yh * mgy)
            udy = np.abs(kk) * (np.abs(gz) + np.abs(mg) + uyh * np.abs(mgy)) + np.abs(dy)
            w0, w1, w2 = (dt(v) for v in a["cw"])
            sdx = w0 * _shift(dy, 1, bug) + w1 * dy + w2 * _shift(dy, -1, bug)
            usdx = np.abs(w0) * _shift(udy, 1) + np.abs(w1) * udy + np.abs(w2) * _shift(udy, -1) + np.abs(sdx)
            x2 = (x + gz + sdx).astype(dt)
            ux, sx = ux + np.abs(x) + np.abs(gz) + usdx, sx + _hu(x2)
            x = _rb(x2, dt, bug)
            kd = f64(kk)
            dp = np.array([kd * (tot[3 + s] - f64(mg) * tot[6 + s] - f64(mgy) * tot[9 + s]) for s in range(3)] +
                          [kd * (tot[0] - f64(mg) * n - f64(mgy) * tot[2]), tot[1], tot[0]])
            udp = np.array([abs(kd) * (abs(tot[3 + s]) + abs(f64(mg) * tot[6 + s]) + abs(f64(mgy) * tot[9 + s])) for s in range(3)] +
                           [abs(kd) * (abs(tot[0]) + abs(f64(mg) * n) + abs(f64(mgy) * tot[2])), abs(tot[1]), abs(tot[0])])
            out["sdparams"] = (dp, udp, np.zeros(6))
        if tail in ACT_BWD:
            yr = _wide(a["Yref"], f64)
            fac = np.where(yr == 0, dt(0), np.where(yr > 0, ks, dt(sl * ks))).astype(dt)
            x = (x * fac).astype(dt)
            ux, sx = ux * np.abs(fac) + np.abs(x), sx * np.abs(fac)
        if has_bn:
            z, mean, rstd, g = _wide(a["Z"], dt), a["mean"].astype(dt), a["rstd"].astype(dt), a["gamma"].astype(dt)
            xh = ((z if "dgamma_no_mean" in bug else z - mean) * rstd).astype(dt)
            uxh = (np.abs(z) + np.abs(mean)) * np.abs(rstd) + np.abs(xh)
            sgm, sgx = x.sum(0, dtype=dt), (x * xh).sum(0, dtype=dt)
            usg, ssg = ux.sum(0), sx.sum(0)
            usgx, ssgx = (ux * np.abs(xh) + np.abs(x) * uxh).sum(0), (sx * np.abs(xh)).sum(0)
            out["dbeta"], out["dgamma"] = (sgm, usg, ssg), (sgx, usgx, ssgx)
            k2, Bd = g * rstd, dt(ROWS if "invB_128" in bug else B)
            dz = k2 * (x - sgm / Bd - xh * (sgx / Bd))
            ux = np.abs(k2) * (ux + usg / B + uxh * np.abs(sgx) / B + np.abs(xh) * usgx / B) + np.abs(dz)
            sx = np.abs(k2) * (sx + ssg / B + np.abs(xh) * ssgx / B)
            x = dz.astype(dt)
        out["y"] = (x, ux, sx + _hu(x))
    if a["dbias"] and (not fwd or tail == LOSS):
        if "dbias_unrounded" in bug:
            yb = out["y"][0].astype(f64)
        else:
            yb = bf16_f64(st["Y"]) if "Y" in st else bf16_f64(bf16_bits(out["y"][0].astype(f32)))
        out["dbias"] = (yb.astype(dt).sum(0, dtype=dt), np.abs(yb).sum(0), np.zeros(N))
    return out


def _loss_parts(pb, a, dt):
    """The five partial sums per strip of 16 columns TAIL_LOSS leaves in loss_ws, from the stored predictions: (value, unit) [strips, 5]."""
    p, t = _wide(pb, dt), a["targets"].astype(dt)
    B, N = p.shape
    nI, nD = a["nI"], a["nD"]
    d, ud = p - t, np.abs(p) + np.abs(t)
    cols = np.arange(N)
    I, D, R_ = cols < nI, (cols >= nI) & (cols < nI + nD), cols >= nI + nD
    den = np.abs(t) + dt(1e-8)
    box, ubox = np.zeros_like(p), np.zeros_like(p, dtype=f64)
    if a["lo"] is not None:
        lo = _h(a["lo"], dt)
        box, ubox = box + np.where(p < lo, lo - p, dt(0)), ubox + np.where(p < lo, np.abs(lo) + np.abs(p), 0)
    if a["hi"] is not None:
        hi = _h(a["hi"], dt)
        box, ubox = box + np.where(p > hi, p - hi, dt(0)), ubox + np.where(p > hi, np.abs(hi) + np.abs(p), 0)
    rel, urel = np.abs(d) / den, ud / den + np.abs(d) / den
    terms = [(np.abs(d) * I, ud * I), (d * d * I, (2 * np.abs(d) * ud + d * d) * I), (box * I, ubox * I), (rel * D, urel * D), (rel * R_, urel * R_)]
    ns = (N + 15) // 16
    val, unit = np.zeros((ns, 5)), np.zeros((ns, 5))
    for s in range(ns):
        for k, (v, u) in enumerate(terms):
            val[s, k], unit[s, k] = v[:, 16 * s:16 * s + 16].sum(dtype=dt), u[:, 16 * s:16 * s + 16].sum(dtype=f64)
    return val, unit


def loss_finish(parts, a, B):
    """loss[0] as the launch with loss_finish_rows forms it from the stored partial sums (float64 on the device): (value, unit)."""
    lp = np.asarray(parts, dtype=f64).reshape(-1, 5).sum(0)
    al_raw = f64(f32(a["alpha"]))
    al = min(max(al_raw, 1e-6), 1.0)
    nI, nD, nR = a["nI"], a["nD"], a["N"] - a["nI"] - a["nD"]
    terms = [al * lp[0] / (B * nI), (1 - al) * lp[1] / (B * nI), f64(f32(a["box_w"])) * lp[2]]
    if nD > 0:
        terms.append(f64(f32(a["pen"])) * lp[3] / (B * nD))
    if nR > 0:
        terms.append(f64(f32(a["pen"])) * lp[4] / (B * nR))
    a0 = f32(a["alpha0"])
    if a0 == a0:
        terms.append((f64(a0) - al_raw) ** 2)
    return sum(terms), sum(abs(t) for t in terms)


# =================================================================================================================================
# ops_mlp_wgrad_group[_norm]
# =================================================================================================================================
def wgrad_group(problems, dt=f64, bug=(), norm=None, stored=None):
    """problems: [(At bits [N, B], Bt bits [K, B])]; out_i = At_i Bt_i^T over the 128 (zero-padded) batch rows, four 32-wide steps.
    norm = dict(scale, ranges=[float32 arrays], step, beta1, beta2): also "parts" (one partial sum of (g scale)^2 per 32 x 32 tile, tile
    by tile, from the STORED gradients when given), "ranges", "step" and "corr" = (1 - beta1^t, sqrt(1 - beta2^t))."""
    out = {"out": []}
    for i, (At, Bt) in enumerate(problems):
        acc, unit = _product(At, Bt, dt)
        out["out"].append((acc, unit))
    if norm is not None:
        sc = _h(norm["scale"], dt)
        parts, uparts = [], []
        for i, (At, Bt) in enumerate(problems):
            g = (np.asarray(stored[i], dtype=f32) if stored is not None else out["out"][i][0]).astype(dt)
            N, K = g.shape
            for tn in range((N + 31) // 32):
                for tk in range((K + 31) // 32):
                    v = g[32 * tn:32 * tn + 32, 32 * tk:32 * tk + 32] * sc
                    parts.append((v * v).sum(dtype=dt))
                    uparts.append(2.0 * (v.astype(f64) ** 2).sum())
        rng_, urng = [], []
        for r in norm["ranges"]:
            v = r.astype(dt) * sc
            sq = v * v
            if "range_half" in bug:
                sq = sq * ((np.arange(r.size) % 128) < 64)
            rng_.append(sq.sum(dtype=dt))
            urng.append(2.0 * (v.astype(f64) ** 2).sum())
        t = norm["step"] + 1
        c1, c2 = 1.0 - f64(f32(norm["beta1"])) ** t, np.sqrt(1.0 - f64(f32(norm["beta2"])) ** t)
        out.update(parts=(np.array(parts), np.array(uparts)), ranges=(np.array(rng_), np.array(urng)), step=t, corr=(c1, c2))
    return out


# =================================================================================================================================
# launches and their inputs
# =================================================================================================================================
def launch(B, N, K, tail=NONE, add=ADD_NONE, side=SIDE_NONE, ev=0, p=0.0, slope=0.01, call=None, pad=(0, 0, 0), ratio=30, key=0, No=None,
           loss=None, exact=False, bias=True):
    """A launch with its inputs.  pad: extra columns of lda, ldw, ldy.  ratio: |mean| / std of the stencil's conv1(O) (stream_kernels_ref's
    SB_CASES).  exact: small-integer operands -- every partial sum an integer below 2^8, so float32 accumulation in ANY order and the bf16
    rounding are exact (`exact_twin_ok` checks the limit).  loss: (nI, nD, box, alpha, alpha0)."""
    rng = _rng(B, N, K, tail, add, side, ev, key, 21)
    a = dict(B=B, N=N, K=K, tail=tail, add=add, side=side, eval_stats=ev, p=p, slope=slope, seed=SEED, call=call, eps=EPS, momentum=MOM, seps=SEPS,
             smom=SMOM, lda=ru(K, 32) + pad[0], ldw=ru(K, 32) + pad[1], ldy=ru(N, 32) + pad[2], dbias=False, finish=None, exact=exact)
    if exact:
        # at most forty non-zero products of magnitude <= 2 x 3 per output: |partial sums| <= 40 * 6 + |bias| <= 248 < 2^8; one of the
        # forty columns in every 32-wide step (33 steps at most), so that no step can go missing unseen
        steps = ru(K, 32) // 32
        first = np.array([min(32 * s + int(rng.integers(0, 32)), K - 1) for s in range(steps)])
        rest = np.setdiff1d(np.arange(K), first)
        colsA = np.concatenate([first, rng.permutation(rest)[:max(0, min(K, 40) - first.size)]])
        Aq, Wq = np.zeros((B, K)), np.zeros((N, K))
        Aq[:, colsA] = rng.choice([-2, -1, 1, 2], (B, colsA.size))
        Wq[:, :] = rng.choice([-3, -2, -1, 1, 2, 3], (N, K))
        a["A"], a["W"] = bf16_bits(Aq.astype(f32)), bf16_bits(Wq.astype(f32))
        a["bias"] = rng.integers(-8, 9, N).astype(f32) if bias and tail in FWD_TAILS else None
    else:
        a["A"] = bf16_bits(rng.standard_normal((B, K)).astype(f32))
        a["W"] = bf16_bits((rng.standard_normal((N, K)) / np.sqrt(K)).astype(f32))
        a["bias"] = (0.3 * rng.standard_normal(N)).astype(f32) if bias and tail in FWD_TAILS else None
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    a["gamma"], a["beta"] = (sign * rng.uniform(0.5, 1.5, N)).astype(f32), (0.3 * rng.standard_normal(N)).astype(f32)
    a["rmean"], a["rvar"] = (0.2 * rng.standard_normal(N)).astype(f32), rng.uniform(0.5, 1.5, N).astype(f32)
    if tail in (BWD_BN, BWD_BN_ACT_DROP):
        Z = bf16_bits((rng.standard_normal((B, N)) + 2.0 * (np.arange(N) % 3 - 1)).astype(f32))
        zz = bf16_f64(Z)
        a["Z"], a["mean"] = Z, zz.mean(0).astype(f32)
        a["rstd"] = (1.0 / np.sqrt(zz.var(0) + f64(f32(EPS)))).astype(f32)
        a["dbias"] = True
    if tail in ACT_BWD:
        r, c = np.arange(B, dtype=np.uint64)[:, None], np.arange(N, dtype=np.uint64)[None, :]
        keep = keep_mask(SEED, 3, r * np.uint64(N) + c, p)
        yr = rng.standard_normal((B, N)).astype(f32)
        a["Yref"] = bf16_bits(np.where(keep, yr, f32(0)))
        a["dbias"] = True
    if add != ADD_NONE or side != SIDE_NONE:
        No = N if add != ADD_NONE else (No or N)
        a["No"] = No
        O = (rng.standard_normal((B, No)) + (3.0 if ratio else 0.0)).astype(f32)
        a["O"] = bf16_bits(O)
        a["cw"] = np.array([0.3, 0.55, -0.2], dtype=f32)
        y0 = _conv(bf16_f64(a["O"]), a["cw"], np.zeros(1), f64)[0]
        sd = y0.std() if y0.size > 1 and y0.std() > 0 else 1.0
        a["cb"] = np.array([ratio * sd - y0.mean() if ratio else 0.05], dtype=f32)
        a["sgamma"], a["sbeta"] = np.array([-1.3 if B % 2 else 0.8], dtype=f32), np.array([0.1], dtype=f32)
        a["srm"], a["srv"] = np.array([0.4 + float(a["cb"][0])], dtype=f32), np.array([0.6], dtype=f32)
        a["dZ"] = bf16_bits(rng.standard_normal((B, No)).astype(f32))
        y = _conv(bf16_f64(a["O"]), a["cw"], a["cb"], f64)[0]
        a["ssave"] = np.array([y.mean(), 1.0 / np.sqrt(y.var() + f64(f32(SEPS)))], dtype=f32)
    if tail == LOSS:
        nI, nD, box, alpha, alpha0 = loss
        t = rng.standard_normal((B, N)).astype(f32)
        a.update(nI=nI, nD=nD, alpha=alpha, alpha0=alpha0, lo=LO if box in ("min", "both") else None, hi=HI if box in ("max", "both") else None,
                 box_w=BOX_W, pen=PENALTY, sum0=SUM0, targets=t, dbias=True, ldp=ru(N, 16) + 8 * (pad[2] > 0))
        # planted: p == t (an exact zero), t == 0 in the relative groups, p on a box bound -- through the bias of a row of zeros in A
        pl = strip(dict(a, tail=NONE), f32)["y"][0]
        pb = bf16_f32(bf16_bits(pl))
        for k, (r, c) in enumerate(zip(rng.integers(0, B, 6), rng.integers(0, N, 6))):
            t[r, c] = pb[r, c] if k % 2 == 0 or c < nI else 0.0
    return a


def exact_twin_ok(a):
    """Every partial sum of the twin's product, in the order of the columns and hence in ANY order, is an integer below 2^8."""
    A, W = np.abs(bf16_f64(a["A"])), np.abs(bf16_f64(a["W"]))
    tot = A @ W.T + (np.abs(a["bias"].astype(f64)) if a["bias"] is not None else 0.0)
    vals = np.concatenate([bf16_f64(a["A"]).ravel(), bf16_f64(a["W"]).ravel()])
    return bool((vals == np.round(vals)).all() and tot.max() < 256)


# (B, N, K, pad): every K, N, B of the issue's sets appears; the K edges meet N = 17, B = 33; lda / ldw / ldy minimal and 32 larger
PRODUCT_CASES = [(33, 17, 1, 0), (33, 17, 31, 1), (33, 17, 32, 0), (33, 17, 33, 1), (33, 17, 256, 0), (33, 17, 257, 1), (33, 17, 512, 0),
                 (33, 17, 513, 1), (33, 17, 768, 0), (33, 17, 769, 1), (33, 17, 1025, 0), (33, 17, 1056, 1), (1, 1, 33, 0), (31, 15, 257, 1),
                 (32, 16, 769, 0), (127, 175, 513, 1), (128, 175, 1056, 0), (128, 1, 1, 1), (1, 16, 1025, 1), (127, 15, 32, 0)]
SHAPES = [(1, 16, 32), (33, 17, 33), (127, 40, 70), (128, 175, 350)]
SIDE_NO = (1, 2, 7, 8, 9, 17, 40)
PS, SLOPES = (0.0, 0.1, 0.5), (0.0, 0.01, 1.0)
COMBO_CASES = [(t, ad, ev, s) for (t, ad, ev) in COMPILED + GENERIC_ONLY if t != LOSS for s in range(len(SHAPES))]
# backward tails behind an EXACT product (small-integer operands): dgamma, dbeta and the normalisation's gradient at float32 level
EXACT_BWD_CASES = [(t, s) for t in (BWD_ACT_DROP, BWD_BN, BWD_BN_ACT_DROP) for s in range(len(SHAPES))]
BLOCK_CASES = [(t, ad, No, (33, 128, 1, 127)[k % 4]) for k, No in enumerate(SIDE_NO) for (t, ad) in ((BN, ADD_FWD), (BWD_BN_ACT_DROP, ADD_BWD))]
LOSS_SHAPES = [(1, 1, 1, 0), (5, 7, 2, 5), (33, 17, 5, 6), (128, 302, 100, 101)]
LOSS_ALPHAS = (-0.5, 0.3, 1.7)
LOSS_CASES = [(B, C, nI, nD, ("none", "min", "max", "both")[(s + k) % 4], LOSS_ALPHAS[k % 3], (float("nan"), 0.5)[(s + k) % 2], k % 2)
              for s, (B, C, nI, nD) in enumerate(LOSS_SHAPES) for k in range(4)]      # ..., eval_stats
WG_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (175, 350)]
# (problems [(N, K, ldo - K)], B, grad_scale, range lengths)
WG_CASES = [([(1, 1, 0)], 1, 1.0, (1,)), ([(31, 33, 3), (32, 32, 0), (33, 31, 3)], 33, 1.0 / 128, (63, 64, 65)),
            ([(175, 350, 0)], 128, 1.0, (129, 1000)), ([(175, 350, 3)], 33, 1.0 / 128, ()),
            ([(1, 1, 3), (31, 33, 0), (32, 32, 3), (33, 31, 0), (1, 1, 0), (33, 31, 3), (31, 33, 3), (32, 32, 0)], 128, 1.0, (1, 63, 64, 65, 129, 1000))]
WG_B1, WG_B2, WG_STEP0 = 0.9, 0.999, 4


def combo_launches(case):
    """[launches] of a combination case: a side-job launch first where the combination consumes `spart`."""
    t, ad, ev, s = case
    B, N, K = SHAPES[s]
    k = COMBO_CASES.index(case)
    p, slope = PS[(k + s) % 3] if not ev and t in (ACT_DROP, BN_ACT_DROP) else (PS[(k + s) % 3] if t in ACT_BWD else 0.0), SLOPES[(k // 2 + s) % 3]
    main = launch(B, N, K, t, ad, SIDE_NONE, ev, p, slope, COUNTERS[k % 3], (32 * (k % 2), 32 * ((k // 2) % 2), 32 * ((k // 3) % 2)), key=k)
    return _with_side(main, k)


def exact_bwd_launches(case):
    t, s = case
    B, N, K = SHAPES[s]
    k = EXACT_BWD_CASES.index(case)
    return [launch(B, N, K, t, p=PS[(k + 1) % 3] if t in ACT_BWD else 0.0, slope=SLOPES[(k + 1) % 3], call=COUNTERS[k % 3], key=700 + k, exact=True)]


def block_launches(case):
    t, ad, No, B = case
    k = BLOCK_CASES.index(case)
    main = launch(B, No, (33, 70)[k % 2], t, ad, SIDE_NONE, 0, PS[k % 3] if t in ACT_BWD else 0.0, SLOPES[k % 3], COUNTERS[k % 3], key=100 + k)
    return _with_side(main, k)


def _with_side(main, k):
    if main["add"] == ADD_NONE:
        return [main]
    fwd = main["add"] == ADD_FWD
    # the launch before: any product (here 16 x 32 columns through the generic kernel) with the side job over the SAME block input
    side = launch(main["B"], 16, 32, NONE, ADD_NONE, SIDE_FWD if fwd else SIDE_BWD, 0, key=200 + k, No=main["No"])
    for name in ("O", "cw", "cb", "sgamma", "sbeta", "srm", "srv", "dZ", "ssave"):
        side[name] = main[name]
    return [side, main]


# stream_kernels_ref's planted tie: under FB_TIE_SEED at call 5 element 48513 draws u == 0.5 exactly -- here row 127, column 253 of a
# (128, 380) launch with p = 0.5, kept by u >= p and dropped by u > p
TIE_CASES = [(128, 380, 32)]


def tie_launches(case):
    B, N, K = case
    assert FB_TIE_INDEX < B * N
    a = launch(B, N, K, ACT_DROP, p=0.5, slope=0.01, call=FB_TIE_CALL, key=500)
    a["seed"] = FB_TIE_SEED
    return [a]


def loss_launches(case):
    B, C, nI, nD, box, alpha, alpha0, ev = case
    k = LOSS_CASES.index(case)
    a = launch(B, C, (33, 70, 175, 175)[LOSS_SHAPES.index((B, C, nI, nD))], LOSS, ADD_NONE, SIDE_NONE, ev, pad=(0, 0, 32 * (k % 2)), key=300 + k,
               loss=(nI, nD, box, alpha, alpha0))
    fin = launch(B, 16, 32, NONE, key=400 + k)
    fin["finish"] = a
    return [a, fin]


def wgrad_inputs(case):
    probs, B, scale, rl = case
    rng = _rng(len(probs), B, 31)
    ps = [(bf16_bits(rng.standard_normal((N, B)).astype(f32)), bf16_bits(rng.standard_normal((K, B)).astype(f32))) for N, K, _ in probs]
    return ps, [(0.1 * rng.standard_normal(n)).astype(f32) for n in rl]


# =================================================================================================================================
# what a launch leaves in memory: raw buffers (as the device holds them) and their decoding
# =================================================================================================================================
def decode_tiled(raw, rows, ld, B, N, transposed, label):
    """The live [B, N] corner of a tiled output and the exact records of what surrounds it: rows 0..127 x columns 0..(N r.u. 16) - 1
    hold zeros outside the live corner, everything else the sentinel."""
    m = from_tiled(np.asarray(raw, dtype=np.uint16).reshape(rows, ld))
    if transposed:
        m = m.T                                           # [128, rows]: rows of the storage are columns of the matrix
    n16 = ru(N, 16)
    live = m[:B, :N].copy()
    dead = m[:ROWS, :n16].copy()
    dead[:B, :N] = 0
    recs = [("exact", f"{label}: zeros outside the live corner", not dead.any()),
            ("exact", f"{label}: columns past N r.u. 16 untouched", bool((m[:, n16:] == SENT_BF16).all()))]
    return live, recs


class CpuImpl:
    """The launches in float32 NumPy (with `bug`, a deliberately wrong variant): what CPU_CONST is measured on.  It builds the RAW
    buffers a launch leaves, so the layout checks run on it too."""

    def __init__(self, bug=()):
        self.bug = frozenset([bug] if isinstance(bug, str) else bug)

    def strip(self, a):
        B, N = a["B"], a["N"]
        o = strip(a, f32, self.bug)
        raw = {"intact": True}
        # the twin: the same float32 evaluation WITHOUT the bf16 roundings (from the same stored Zt / P), held to the reference with no slack --
        # a bf16 output, and whatever lies behind an intermediate rounding, shows its float32 error next to a rounding tie alone
        given = {k: bf16_bits(o[n][0].astype(f32)) for k, n in (("Z", "z"), ("P", "p")) if n in o}
        o2 = strip(a, f32, self.bug | {"_unrounded"}, given)
        raw["twin"] = {k: o2[k][0] for k in ("y", "z", "p", "dgamma", "dbeta") if k in o2}
        yb = np.zeros((ROWS, a["ldy"]), dtype=np.uint16)
        yb[:, ru(N, 16):] = SENT_BF16
        yb[:B, :N] = bf16_bits(o["y"][0].astype(f32))
        raw["Y"] = to_tiled(yb).ravel()

        def tr(bits):
            t = np.full((ru(N, 32), ROWS), SENT_BF16, dtype=np.uint16)
            t[:ru(N, 16)] = 0
            t[:N, :B] = bits.T
            if "yt_tile_transposed" in self.bug:          # (column, row) <-> (row, column) inside every 16 x 16 block
                t = np.ascontiguousarray(t.reshape(-1, 16, ROWS // 16, 16).transpose(0, 3, 2, 1)).reshape(ru(N, 32), ROWS)
            return to_tiled(t).ravel()
        raw["Yt"] = tr(yb[:B, :N])
        if "z" in o:
            raw["Zt"] = tr(bf16_bits(o["z"][0].astype(f32)))
        if "p" in o:
            pb = np.full((ROWS, a["ldp"]), SENT_BF16, dtype=np.uint16)
            pb[:, :ru(N, 16)] = 0
            pb[:B, :N] = bf16_bits(o["p"][0].astype(f32))
            raw["P"] = pb.ravel()
        for k in ("mean", "rstd", "rmean", "rvar", "dgamma", "dbeta", "dbias", "ssave", "srm", "srv", "sdparams"):
            if k in o:
                raw[k] = np.asarray(o[k][0], dtype=f32).reshape(-1)
        if a["eval_stats"] and a["tail"] in BN_TAILS:
            raw["rmean"], raw["rvar"] = a["rmean"], a["rvar"]
        if "spart" in o:
            raw["spart"] = o["spart"][0].astype(f64).ravel()
        if "parts" in o:
            raw["loss_ws"] = o["parts"][0].astype(f64).ravel()
        if a["finish"] is not None:
            v = f32(loss_finish(a["loss_ws_in"], a["finish"], a["finish"]["B"])[0])
            raw["loss"], raw["loss_sum"] = np.array([v]), np.array([f32(f32(a["loss_sum_in"]) + v)])
        training_bn = a["tail"] in (BN, BN_ACT_DROP) and not a["eval_stats"]
        raw["nbt"] = NBT0 + int(training_bn)
        raw["snbt"] = NBT0 + int(a["add"] == ADD_FWD and not a["eval_stats"])
        draws = a["tail"] in (ACT_DROP, BN_ACT_DROP) and a["p"] > 0
        raw["counter"] = None if a["call"] is None else a["call"] + int(draws)
        return raw

    def wgrad(self, case, problems, ranges, norm):
        probs, B, scale, rl = case
        o = wgrad_group(problems, f32, self.bug, dict(scale=scale, ranges=ranges, step=WG_STEP0, beta1=WG_B1, beta2=WG_B2) if norm else None)
        outs = []
        for (N, K, extra), (v, _) in zip(probs, o["out"]):
            buf = np.full((N, K + extra), SENT_F32, dtype=f32)
            buf[:, :K] = v
            if "wgrad_past_edge" in self.bug and extra:
                buf[:, K] = v[:, 0]
            outs.append(buf)
        got = dict(out=outs, intact=True)
        if norm:
            got.update(parts=np.concatenate([o["parts"][0], o["ranges"][0]]).astype(f64), step=o["step"], corr=o["corr"],
                       nparts=len(o["parts"][0]) + len(rl))
        return got


# =================================================================================================================================
# the protocols: what is run and compared per case.  `impl` is CpuImpl here and the C ABI in tests/test_gpu_mlp_block.py; both are held
# to the same records: ("cmp", name, got, ref, unit, slack) and ("exact", label, holds).
# =================================================================================================================================
def strip_records(a, raw):
    """The records of one strip launch from the raw buffers it left."""
    B, N, tail = a["B"], a["N"], a["tail"]
    fwd, has_bn = tail in FWD_TAILS, tail in BN_TAILS
    recs = [("exact", "inputs unchanged, guards and workspace ends untouched", bool(raw["intact"]))]
    if a.get("exact"):
        recs.append(("exact", "small-integer operands stay below 2^8", exact_twin_ok(a)))
    Y, r1 = decode_tiled(raw["Y"], ROWS, a["ldy"], B, N, False, "Y")
    Yt, r2 = decode_tiled(raw["Yt"], ru(N, 32), ROWS, B, N, True, "Yt")
    recs += r1 + r2 + [("exact", "Y and Yt hold identical bit patterns", np.array_equal(Y, Yt))]
    st = {"Y": Y}
    if fwd and has_bn:
        Z, r3 = decode_tiled(raw["Zt"], ru(N, 32), ROWS, B, N, True, "Zt")
        recs += r3
        st["Z"] = Z
    if tail == LOSS:
        Pm = np.asarray(raw["P"], dtype=np.uint16).reshape(ROWS, a["ldp"])
        n16 = ru(N, 16)
        dead = Pm[:, :n16].copy()
        dead[:B, :N] = 0
        recs += [("exact", "P: zeros outside the live corner", not dead.any()),
                 ("exact", "P: columns past N r.u. 16 untouched", bool((Pm[:, n16:] == SENT_BF16).all()))]
        st["P"] = Pm[:B, :N].copy()
    ref = strip(a, f64, (), st)
    yname = {True: "fwd.y", False: "bwd.y"}[fwd]
    if tail == NONE and a["add"] == ADD_NONE:
        yname = "prod.y"
    if tail == LOSS:
        yname = "loss.grad"
        recs.append(("cmp", "loss.p", bf16_f64(st["P"]), *ref["p"]))
        recs.append(("cmp", "loss.parts", np.asarray(raw["loss_ws"])[:ref["parts"][0].size].reshape(-1, 5), *ref["parts"]))
    recs.append(("cmp", yname, bf16_f64(Y), *ref["y"]))
    if "z" in ref:
        recs.append(("cmp", "fwd.z", bf16_f64(st["Z"]), *ref["z"]))
    # the float32 evaluation's twin without bf16 roundings (CpuImpl): no slack -- what the constants of these outputs are measured on
    for k, name in (("y", yname), ("z", "fwd.z"), ("p", "loss.p"), ("dgamma", "bwd.dgamma"), ("dbeta", "bwd.dbeta")):
        if k in raw.get("twin", {}):
            recs.append(("cmp", name, np.asarray(raw["twin"][k], dtype=f64), ref[k][0], ref[k][1], 0.0))
    if tail in (ACT_DROP, BN_ACT_DROP) and a["p"] > 0:
        recs.append(("exact", "dropped elements are zero", not bf16_f64(Y)[~ref["keep"]].any()))
    names = dict(mean="fwd.mean", rstd="fwd.rstd", rmean="fwd.rmean", rvar="fwd.rvar", dgamma="bwd.dgamma", dbeta="bwd.dbeta",
                 dbias="loss.dbias" if tail == LOSS else "bwd.dbias", ssave="st.save", srm="st.rmean", srv="st.rvar", sdparams="st.dparams",
                 spart="st.part" if a["side"] == SIDE_FWD else "st.bsums")
    for k, name in names.items():
        if k in ref:
            got = np.asarray(raw[k], dtype=f64)
            recs.append(("cmp", name, got[:ref[k][0].size].reshape(np.shape(ref[k][0])), *ref[k]))
    if has_bn and fwd and a["eval_stats"]:
        same = np.array_equal(raw["rmean"], a["rmean"]) and np.array_equal(raw["rvar"], a["rvar"])
        recs.append(("exact", "eval leaves the running statistics alone", same))
    training_bn = tail in (BN, BN_ACT_DROP) and not a["eval_stats"]
    recs.append(("exact", "num_batches_tracked", raw["nbt"] == NBT0 + int(training_bn)))
    recs.append(("exact", "stencil num_batches_tracked", raw["snbt"] == NBT0 + int(a["add"] == ADD_FWD and not a["eval_stats"])))
    if a["call"] is not None:
        draws = tail in (ACT_DROP, BN_ACT_DROP) and a["p"] > 0
        recs.append(("exact", "call counter after the launch", raw["counter"] == a["call"] + int(draws)))
    return recs, st


def run_launches(launches, impl):
    """A case's launches in order; a launch that consumes `spart` or finishes a loss is given what the launch before it LEFT."""
    recs, prev_raw = [], None
    for a in launches:
        if a["add"] != ADD_NONE:
            a = dict(a, spart=np.asarray(prev_raw["spart"], dtype=f64))
        if a["finish"] is not None:
            a = dict(a, loss_ws_in=np.asarray(prev_raw["loss_ws"], dtype=f64), loss_sum_in=SUM0)
            L = a["finish"]
            vals = []
            for _ in range(2):                            # two steps: the value, and the running total over both
                raw = impl.strip(a)
                vals.append(raw)
                a = dict(a, loss_sum_in=float(raw["loss_sum"][0]))
            r, _ = strip_records(a, raw)
            recs += r
            ns = (L["N"] + 15) // 16
            v, uv = loss_finish(a["loss_ws_in"][:5 * ns], L, L["B"])
            recs.append(("cmp", "loss.value", f64(vals[1]["loss"][0]), v, uv, 0.0))
            recs.append(("exact", "the value is the same in both steps", vals[0]["loss"][0] == vals[1]["loss"][0]))
            once = f64(f32(vals[0]["loss"][0]))
            recs.append(("cmp", "loss.sum", f64(vals[1]["loss_sum"][0]), f64(f32(SUM0)) + 2 * once, abs(f64(f32(SUM0))) + 2 * abs(once), 0.0))
            # and against the loss of the stored predictions end to end (stream_kernels_ref.surrogate_loss_grad: clamp, alpha0, the means)
            full = strip(L, f64, (), {"P": prev_st["P"]})
            recs.append(("cmp", "loss.value", f64(vals[1]["loss"][0]), *full["value"]))
            continue
        raw = impl.strip(a)
        r, prev_st = strip_records(a, raw)
        recs += r
        prev_raw = raw
    return recs


def product_protocol(case, impl):
    B, N, K, pd = case
    k = PRODUCT_CASES.index(case)
    pad = (32 * pd, 32 * ((pd + k // 2) % 2), 32 * ((pd + k // 4) % 2))
    recs = run_launches([launch(B, N, K, pad=pad, key=k)], impl)
    a = launch(B, N, K, pad=pad, key=k, exact=True)
    raw = impl.strip(a)
    r, st = strip_records(a, raw)
    want = bf16_bits(strip(a, f64)["y"][0].astype(f32))
    return recs + r + [("exact", "twin: bit for bit", np.array_equal(st["Y"], want))]


def wgrad_protocol(case, impl, norm=True):
    probs, B, scale, rl = case
    problems, ranges = wgrad_inputs(case)
    got = impl.wgrad(case, problems, ranges, norm)
    ref = wgrad_group(problems, f64, (), dict(scale=scale, ranges=ranges, step=WG_STEP0, beta1=WG_B1, beta2=WG_B2) if norm else None,
                      [g[:, :K] for g, (N, K, _) in zip(got["out"], probs)])
    recs = [("exact", "inputs unchanged, guards untouched", bool(got["intact"]))]
    for (N, K, extra), g, (v, u) in zip(probs, got["out"], ref["out"]):
        recs.append(("cmp", "wg.out", g[:, :K].astype(f64), v, u, 0.0))
        recs.append(("exact", "columns K .. ldo - 1 untouched", bool((g[:, K:] == SENT_F32).all())))
    if norm:
        nt = ref["parts"][0].size
        recs.append(("exact", "*nparts = tiles + ranges", got["nparts"] == nt + len(rl)))
        recs.append(("cmp", "wg.part", got["parts"][:nt], *ref["parts"], 0.0))
        if rl:
            recs.append(("cmp", "wg.range", got["parts"][nt:nt + len(rl)], *ref["ranges"], 0.0))
        recs.append(("exact", "step advanced by one", got["step"] == WG_STEP0 + 1))
        # double pow / sqrt on the device: a few ulps of float64 on 1 - beta^t (terms 1 and beta^t), carried through the square root
        c1, c2 = ref["corr"]
        u53 = 16 * 2.0 ** -53
        recs.append(("exact", "bias corrections", abs(got["corr"][0] - c1) <= u53 * 2 and abs(got["corr"][1] - c2) <= u53 * (1 / c2 + c2)))
    return recs


PROTOCOLS = {"product": (product_protocol, PRODUCT_CASES),
             "combo": (lambda c, impl: run_launches(combo_launches(c), impl), COMBO_CASES),
             "bwdx": (lambda c, impl: run_launches(exact_bwd_launches(c), impl), EXACT_BWD_CASES),
             "block": (lambda c, impl: run_launches(block_launches(c), impl), BLOCK_CASES),
             "loss": (lambda c, impl: run_launches(loss_launches(c), impl), LOSS_CASES),
             "tie": (lambda c, impl: run_launches(tie_launches(c), impl), TIE_CASES),
             "wgrad": (wgrad_protocol, WG_CASES)}


def measure(recs):
    """({name: largest (|got - ref| - slack) / (unit EPS32) (inf for a non-zero against an exact zero)}, [labels of the exact records
    that do not hold])."""
    ratios, failed = {}, []
    for rec in recs:
        if rec[0] == "cmp":
            _, name, got, ref, unit, slack = rec
            got, ref, unit, slack = (np.asarray(v, dtype=f64) for v in (got, ref, unit, slack))
            got = got.reshape(ref.shape)
            err = np.abs(got - ref) - slack
            e = error_ratio(np.where(err > 0, err, 0.0), np.zeros_like(ref), unit, False)
            if not np.isfinite(got).all() or (name in EXACT_ZERO and not exact_zeros(got, ref)):
                e = np.inf
            ratios[name] = max(ratios.get(name, 0.0), e)
        elif not rec[2]:
            failed.append(rec[1])
    return ratios, failed
