"""Float64 references, error units and the case table of the row-wise encoder kernels of csrc/seq_block.hip (test code, NumPy).

One function per entry point.  Inputs are the device's bf16 (uint16 bit patterns) and float32 arrays; with dt = float64 a function is
the reference, with dt = float32 the same formula evaluated in float32 (the measurement behind every bound: test_seq_block_reference).
Dropout masks come from tests/bayes_stream.py (drop_key / drop_uniform, bit for bit the device's) at the kernels' element indices:

    attention     (((b H + h) S + i) S + j), b the GLOBAL sample
    LayerNorm     r d + c
    act-dropout   the flat index

and an element is kept when u >= float32(p): u sits on the 2^-24 grid, so there is no ambiguous case and no element is ever excluded.

Every function returns {output: (value, unit)}.  The unit is the output's formula with every sum replaced by the sum of the absolute
values of its terms (a first-order running error bound), in units of EPS32 = 2^-24:

    bf16 outputs      |got - ref| <= 1/2 ulp_bf16(ref) + C unit EPS32
    float32 outputs   |got - ref| <= C unit EPS32
    ref == 0          got == 0 (dropped elements, ReLU's negative side, a row whose only key was dropped)

C = 4 x CPU_CONST[output]: CPU_CONST is the largest constant the float32 evaluation shows over the case table (measured and asserted
by tests/test_seq_block_reference.py).  The factor four: the device's __expf / rsqrtf / reciprocal are a few ulp where NumPy's are
correctly rounded, its butterfly and atomic orders differ from NumPy's pairwise sums, and it forms 1 / (1 - p) in float32.
`bug=`: the deliberately wrong variants of the float32 evaluation (the teeth check).
"""
from __future__ import annotations

import numpy as np

from tests import bayes_stream as bs

EPS32 = 2.0 ** -24
SEED = (1 << 62) | 0x2545F491          # bit 62 set: the high word of the seed takes part in the key
COUNTERS = (0, 5, 2 ** 32 + 5)         # the call counter's values: zero, small, and one whose high word is not zero
SENT_F32 = np.float32(-12345.678)
SENT_BF16, SENT_BF16_VALUE = np.uint16(0xC2F7), -123.5

# ---------------------------------------------------------------------------------------------------------------------------------
# the case table (both test files run exactly these inputs)
# ---------------------------------------------------------------------------------------------------------------------------------
ATT_CASES = [(21, 7, 8, 15, 0.1), (21, 7, 8, 15, 0.0), (7, 8, 8, 32, 0.3), (11, 8, 2, 20, 0.5), (6, 8, 16, 16, 0.1), (3, 3, 8, 1, 0.2),
             (10, 5, 64, 4, 0.1), (9, 1, 2, 8, 0.5)]                                            # (Bn, S, H, dh, p)
LN_CASES = [(131, 120, False, 0.1, "both"), (70, 256, True, 0.1, "dy16"), (77, 8, True, 0.25, "dy32"), (33, 65, False, 0.0, "both"),
            (5, 1, False, 0.0, "both"), (8200, 8, False, 0.1, "both")]                          # (T, d, residual bf16, p, gradients)
ACT_CASES = [(n, slope, p) for n in (1, 255, 257, 2048 * 256 + 3) for slope in (0.0, 0.01) for p in (0.0, 0.1, 0.5)]
NOISE_CASES = [(7, 5), (300, 120)]                                                              # (rows, d)
COMBINE_CASES = [(B, Nc, d, gr) for B, Nc, d in ((5, 3, 64), (70, 6, 120), (600, 1, 8)) for gr in ("g", "g16", "both")]
WGRAD_CASES = [(1, 1, 1), (31, 8, 8), (33, 64, 64), (257, 7, 33), (1025, 70, 65)]               # (T, N, K)
COLSUM_CASE = (45, 65)                                                                          # (T, N) of the K = 0 job

# Largest constant of the float32 evaluation per output over the table above (test_seq_block_reference.py asserts that none is
# exceeded and prints the measured values); the bound of the GPU test is four times this.
CPU_CONST = {
    "att.ctx": 6.0, "att.dq": 1.6, "att.dk": 2.0, "att.dv": 5.0,
    "ln.y32": 4.2, "ln.y16": 4.2, "ln.z": 2.8, "ln.mean": 2.5, "ln.rstd": 0.9,
    "ln.dres": 1.4, "ln.dx": 1.8, "ln.dgamma": 0.85, "ln.dbeta": 1.15,
    "act.y": 2.1, "act.dx": 2.25,
    "noise.xn32": 2.5, "noise.xn16": 2.5, "noise.sa": 1.0, "noise.sb": 1.1,
    "comb.z": 2.9, "comb.z16": 2.9, "comb.dm": 3.0, "comb.dcls": 1.9,
    "wgrad.dW": 1.9, "wgrad.dbias": 0.28, "colsum.out": 0.7,
}


def bound_constant(name: str) -> float:
    return 4.0 * CPU_CONST[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(a, truncate: bool = False) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even as lane_common.hpp f32_to_bf16 (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    if not truncate:
        u = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (u >> np.uint32(16)).astype(np.uint16)


def bf16_f32(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_f64(bits) -> np.ndarray:
    return bf16_f32(bits).astype(np.float64)


def ulp_bf16(x) -> np.ndarray:
    """Spacing of bf16 (8 significant bits) in the binade of x; 0 at 0."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    return np.where(x == 0.0, 0.0, np.ldexp(1.0, e - 8))


def rand_bf16(rng, shape, scale=1.0) -> np.ndarray:
    return bf16_bits((scale * rng.standard_normal(shape)).astype(np.float32))


def _rand32(rng, shape, scale=1.0, shift=0.0) -> np.ndarray:
    return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


def keep_mask(seed: int, call: int, idx, p: float) -> np.ndarray:
    p32 = float(np.float32(p))
    idx = np.asarray(idx, dtype=np.uint64)
    if not p32 > 0.0:
        return np.ones(idx.shape, dtype=bool)
    return bs.drop_uniform(bs.drop_key(seed, call), idx) >= p32


def _ks(p, dt):
    return dt(1.0) / (dt(1.0) - dt(np.float32(p))) if np.float32(p) > 0 else dt(1.0)


def error_ratio(got, ref, unit, bf16: bool) -> float:
    """Largest (|got - ref| - [1/2 ulp_bf16(ref)]) / (unit EPS32) over all elements; inf where an error stands against a unit of 0."""
    got, ref, unit = (np.asarray(a, dtype=np.float64) for a in (got, ref, unit))
    err = np.abs(got - ref)
    if bf16:
        err = err - 0.5 * ulp_bf16(ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err <= 0.0, 0.0, err / (unit * EPS32))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def exact_zeros(got, ref) -> bool:
    """Where the reference is exactly zero the output is exactly zero."""
    return bool((np.asarray(got, dtype=np.float64)[np.asarray(ref) == 0.0] == 0.0).all())


def combine_partials(init, partials):
    """float32: init + partials added one by one, in ascending and in descending order (the two extremes of an atomic order)."""
    out = []
    for seq in (partials, partials[::-1]):
        acc = np.array(init, dtype=np.float32, copy=True)
        for part in seq:
            acc = acc + part.astype(np.float32)
        out.append(acc)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def att_samples_per_wg(S, H, dh, backward: bool) -> int:
    """seq_block.hip sa_samples_per_wg (0: refused)."""
    dhp = 16 if dh <= 16 else 32
    per = S * 4 * H * dhp * 2 + 2 * H * S * S * 4 if backward else S * 3 * H * dhp * 2
    return max(0, min(512 // (S * H), (64 * 1024) // per, 8))


def att_inputs(case):
    Bn, S, H, dh, p = case
    rng = np.random.default_rng([Bn, S, H, dh, 1])
    return dict(qkv=rand_bf16(rng, (Bn * S, 3 * H * dh)), dctx=rand_bf16(rng, (Bn * S, H * dh)))


def _att_keep(Bn, S, H, p, seed, call, bug, nb):
    b = np.arange(Bn, dtype=np.uint64)[:, None, None, None]
    if bug == "local_b":
        b = b % np.uint64(nb)
    h = np.arange(H, dtype=np.uint64)[None, :, None, None]
    i = np.arange(S, dtype=np.uint64)[None, None, :, None]
    j = np.arange(S, dtype=np.uint64)[None, None, None, :]
    if bug == "mask_ji":
        i, j = j, i
    return keep_mask(seed, call, ((b * np.uint64(H) + h) * np.uint64(S) + i) * np.uint64(S) + j, p)


def _att_common(qkv, Bn, S, H, dh, p, seed, call, dt, bug, nb):
    a = bf16_f32(qkv).reshape(Bn, S, 3, H, dh).astype(dt)
    q, k, v = (a[:, :, n].transpose(0, 2, 1, 3) for n in range(3))              # [Bn, H, S, dh]
    scale = dt(1.0) / np.sqrt(dt(dh))
    s = (q @ k.transpose(0, 1, 3, 2)) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    keep = _att_keep(Bn, S, H, p, seed, call, bug, nb)
    ks = _ks(p, dt)
    Pt = np.where(keep, P * ks, dt(0.0))
    return q, k, v, scale, P, Pt, keep, ks


def _rows(x, Bn, S, H, dh):
    """[Bn, H, S, dh] -> the kernels' [Bn * S, H * dh]."""
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(Bn * S, H * dh)


def attention_fwd(qkv, Bn, S, H, dh, p, seed, call, dt=np.float64, bug=None, nb=8):
    q, k, v, scale, P, Pt, keep, ks = _att_common(qkv, Bn, S, H, dh, p, seed, call, dt, bug, nb)
    return {"ctx": (_rows(Pt @ v, Bn, S, H, dh), _rows(np.abs(Pt) @ np.abs(v), Bn, S, H, dh))}


def attention_bwd(qkv, dctx, Bn, S, H, dh, p, seed, call, dt=np.float64, bug=None, nb=8):
    q, k, v, scale, P, Pt, keep, ks = _att_common(qkv, Bn, S, H, dh, p, seed, call, dt, bug, nb)
    dO = bf16_f32(dctx).reshape(Bn, S, H, dh).astype(dt).transpose(0, 2, 1, 3)
    dPt = dO @ v.transpose(0, 1, 3, 2)
    dP = np.where(keep, dPt * (dt(1.0) if bug == "no_ks" else ks), dt(0.0))
    D = (P * dP).sum(-1, keepdims=True)
    dS = P * (dP - D) * scale
    T_ = lambda x: x.transpose(0, 1, 3, 2)      # noqa: E731
    dq, dk, dv = dS @ k, T_(dS) @ q, T_(P if bug == "dv_P" else Pt) @ dO
    amp = dt(1.0) + ((np.abs(q) @ T_(np.abs(k))) * scale).max(-1, keepdims=True)
    U = P * (np.abs(dP) + (P * np.abs(dP)).sum(-1, keepdims=True)) * scale * amp
    units = (U @ np.abs(k), T_(U) @ np.abs(q), T_(np.abs(Pt)) @ np.abs(dO))
    r = lambda x: _rows(x, Bn, S, H, dh)        # noqa: E731
    return {n: (r(val), r(u)) for n, val, u in zip(("dq", "dk", "dv"), (dq, dk, dv), units)}


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm(residual + dropout(x))
# ---------------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5


def ln_inputs(case):
    T, d, res16, p, grads = case
    rng = np.random.default_rng([T, d, 2])
    i = dict(x=rand_bf16(rng, (T, d)), gamma=_rand32(rng, d, 0.2, 1.0), beta=_rand32(rng, d, 0.1),
             dgamma0=_rand32(rng, d), dbeta0=_rand32(rng, d))
    i["res"] = rand_bf16(rng, (T, d)) if res16 else _rand32(rng, (T, d))
    i["dy32"] = _rand32(rng, (T, d)) if grads in ("both", "dy32") else None
    i["dy16"] = rand_bf16(rng, (T, d)) if grads in ("both", "dy16") else None
    return i


def _ln_keep(T, d, p, seed, call):
    return keep_mask(seed, call, np.arange(T * d, dtype=np.uint64).reshape(T, d), p)


def layernorm_fwd(x, res, res16, gamma, beta, eps, p, seed, call, dt=np.float64, bug=None):
    T, d = x.shape
    xv = bf16_f32(x).astype(dt)
    rv = (bf16_f32(res) if res16 else res).astype(dt)
    keep, ks = _ln_keep(T, d, p, seed, call), _ks(p, dt)
    if bug == "drop_after_add":
        z = np.where(keep, (rv + xv) * ks, dt(0.0))
        xd = xv
    else:
        xd = np.where(keep, xv * ks, dt(0.0))
        z = rv + xd
    g, b = gamma.astype(dt), beta.astype(dt)
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).mean(-1, keepdims=True)
    rstd = dt(1.0) / np.sqrt(var + dt(np.float32(eps)))
    y = (z - mean) * rstd * g + b
    mabs = np.abs(z).mean(-1, keepdims=True)
    uy = np.abs(g) * rstd * (np.abs(z) + mabs) + np.abs(y)
    urstd = rstd * (dt(1.0) + rstd ** 2 * ((np.abs(z) + mabs) ** 2).mean(-1, keepdims=True))
    return {"y32": (y, uy), "y16": (y, uy), "z": (z, np.abs(rv) + np.abs(xd)), "mean": (mean[:, 0], mabs[:, 0]), "rstd": (rstd[:, 0], urstd[:, 0])}


def layernorm_bwd(dy32, dy16, z, mean, rstd, gamma, p, seed, call, dgamma0, dbeta0, dt=np.float64, bug=None):
    """z, mean, rstd: the forward's saved float32 arrays, taken as given.  float32: dgamma / dbeta come as [ascending, descending]
    workgroup order of the kernel's grouping (32 rows per workgroup, rows w and w + 16 per wave, waves added in order)."""
    T, d = z.shape
    g = np.zeros((T, d), dtype=dt)
    if dy32 is not None:
        g = g + dy32.astype(dt)
    if dy16 is not None:
        g = g + bf16_f32(dy16).astype(dt)
    zz, mu, rs, gm = z.astype(dt), mean.astype(dt)[:, None], rstd.astype(dt)[:, None], gamma.astype(dt)
    keep, ks = _ln_keep(T, d, p, seed, call), (dt(1.0) if bug == "no_ks" else _ks(p, dt))
    xh = (zz - mu) * rs
    gy = g * gm
    m = lambda a: a.mean(-1, keepdims=True)      # noqa: E731
    dz = rs * (gy - m(gy) - xh * m(gy * xh))
    dx = np.where(keep, dz * ks, dt(0.0))
    mabs = m(np.abs(zz))
    udz = rs * (np.abs(gy) + m(np.abs(gy)) + np.abs(xh) * m(np.abs(gy * xh))) + rs ** 2 * (np.abs(zz) + mabs) * (np.abs(gy) + m(np.abs(gy)))
    ug = (np.abs(g) * (np.abs(xh) + rs * (np.abs(zz) + mabs))).sum(0) + np.abs(dgamma0.astype(dt))
    ub = np.abs(g).sum(0) + np.abs(dbeta0.astype(dt))
    if dt is np.float64:
        dgam, dbet = dgamma0.astype(dt) + (g * xh).sum(0), dbeta0.astype(dt) + g.sum(0)
    else:
        nwg = -(-T // 32)
        pad = lambda a: np.concatenate([a, np.zeros((nwg * 32 - T, d), dtype=dt)]).reshape(nwg, 2, 16, d)      # noqa: E731
        tg, tb = pad(g * xh), pad(g)                     # row r0 + 16 k + wave -> [workgroup, k, wave]
        pg, pb = tg[:, 0] + tg[:, 1], tb[:, 0] + tb[:, 1]
        sg, sb_ = np.zeros((nwg, d), dtype=dt), np.zeros((nwg, d), dtype=dt)
        for w in range(16):
            sg, sb_ = sg + pg[:, w], sb_ + pb[:, w]
        dgam, dbet = combine_partials(dgamma0, list(sg)), combine_partials(dbeta0, list(sb_))
    return {"dres": (dz, udz), "dx": (dx, np.where(keep, udz * ks, dt(0.0))), "dgamma": (dgam, ug), "dbeta": (dbet, ub)}


# ---------------------------------------------------------------------------------------------------------------------------------
# dropout(LeakyReLU(x))
# ---------------------------------------------------------------------------------------------------------------------------------
def act_inputs(case):
    n, slope, p = case
    rng = np.random.default_rng([n, int(1000 * slope), int(10 * p), 3])
    return dict(x=rand_bf16(rng, n), dy=rand_bf16(rng, n))


def _slope(slope, dt):
    return dt(np.float32(slope))


def act_dropout_fwd(x, slope, p, seed, call, dt=np.float64, bug=None):
    xv = bf16_f32(x).astype(dt)
    keep, ks = keep_mask(seed, call, np.arange(x.size, dtype=np.uint64), p), _ks(p, dt)
    v = np.where(xv > 0, xv, xv * _slope(slope, dt))
    y = np.where(keep, v * ks, dt(0.0))
    return {"y": (y, np.abs(y))}


def act_dropout_bwd(x, dy, slope, p, seed, call, dt=np.float64, bug=None):
    xv, g = bf16_f32(x).astype(dt), bf16_f32(dy).astype(dt)
    keep, ks = keep_mask(seed, call, np.arange(x.size, dtype=np.uint64), p), (dt(1.0) if bug == "no_ks" else _ks(p, dt))
    g = np.where(keep, g * ks, dt(0.0))
    dx = np.where(xv > 0, g, g * _slope(slope, dt))
    return {"dx": (dx, np.abs(dx))}


def act_exact_bits(x, slope, dy=None) -> np.ndarray:
    """p = 0: the bf16 the kernel must store, bit for bit -- its one float32 product x * slope (correctly rounded by IEEE, so the float64
    product rounded to float32 is that value) rounded to nearest even at bit 16; forward for dy None, else the backward."""
    xv = bf16_f64(x)
    v = xv if dy is None else bf16_f64(dy)
    return bf16_bits(np.where(xv > 0, v, v * float(np.float32(slope))).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# diffusion front end
# ---------------------------------------------------------------------------------------------------------------------------------
def noise_inputs(case):
    rows, d = case
    rng = np.random.default_rng([rows, d, 4])
    acp = np.cumprod(1.0 - np.linspace(1e-4, 0.02, 1000)).astype(np.float32)
    return dict(x=_rand32(rng, (rows, d)), eps=_rand32(rng, (rows, d)), t=rng.integers(0, 1000, rows).astype(np.int64), acp=acp)


def diffusion_noise(x, t, eps, acp, dt=np.float64, bug=None):
    a = acp.astype(dt)[t][:, None]
    sa, sb = np.sqrt(a), np.sqrt(dt(1.0) - a)
    v = sa * x.astype(dt) + sb * eps.astype(dt)
    u = np.abs(sa * x.astype(dt)) + np.abs(sb * eps.astype(dt))
    return {"xn32": (v, u), "xn16": (v, u), "sa": (sa[:, 0], sa[:, 0]), "sb": (sb[:, 0], sb[:, 0])}


def combine_inputs(case):
    B, Nc, d, gr = case
    rng = np.random.default_rng([B, Nc, d, 5])
    sa = rng.uniform(0.1, 1.0, B * Nc).astype(np.float32)
    i = dict(m=rand_bf16(rng, (B * Nc, d)), xn32=_rand32(rng, (B * Nc, d)), sa=sa, sb=np.sqrt(1.0 - sa.astype(np.float64) ** 2).astype(np.float32),
             cls=_rand32(rng, d), pe=_rand32(rng, (Nc + 1, d)), dcls0=_rand32(rng, d))
    i["g"] = _rand32(rng, (B, Nc + 1, d)) if gr in ("g", "both") else None
    i["g16"] = rand_bf16(rng, (B, Nc + 1, d)) if gr in ("g16", "both") else None
    return i


def diffusion_combine_fwd(m, xn32, sa, sb, cls, pe, B, Nc, d, dt=np.float64, bug=None):
    mv, xn = bf16_f32(m).astype(dt).reshape(B, Nc, d), xn32.astype(dt).reshape(B, Nc, d)
    a, b = sa.astype(dt).reshape(B, Nc, 1), sb.astype(dt).reshape(B, Nc, 1)
    pv = pe.astype(dt)
    z = np.empty((B, Nc + 1, d), dtype=dt)
    u = np.empty_like(z)
    z[:, 0], u[:, 0] = cls.astype(dt) + pv[0], np.abs(cls.astype(dt)) + np.abs(pv[0])
    z[:, 1:] = (xn - b * mv) / a + pv[1:]
    u[:, 1:] = (np.abs(xn) + np.abs(b * mv)) / np.abs(a) + np.abs(pv[1:])
    return {"z": (z, u), "z16": (z, u)}


def diffusion_combine_bwd(g, g16, sa, sb, dcls0, B, Nc, d, dt=np.float64, bug=None):
    """float32: dcls as [ascending, descending] order of the 64 workgroups' partials (workgroup w: samples w, w + 64, ... in order)."""
    zero = np.zeros((B, Nc + 1, d), dtype=dt)
    g1 = zero if g is None else g.astype(dt)
    g2 = zero if g16 is None else bf16_f32(g16).astype(dt)
    gs = g1 + g2
    r = (sb.astype(dt) / sa.astype(dt)).reshape(B, Nc, 1)
    dm = -r * gs[:, 1:]
    udm = np.abs(r) * (np.abs(g1) + np.abs(g2))[:, 1:]
    ucls = (np.abs(g1) + np.abs(g2))[:, 0].sum(0) + np.abs(dcls0.astype(dt))
    if dt is np.float64:
        dcls = dcls0.astype(dt) + gs[:, 0].sum(0)
    else:
        parts = []
        for w in range(64):
            acc = np.zeros(d, dtype=dt)
            for b in range(w, B, 64):
                acc = acc + gs[b, 0]
            parts.append(acc)
        dcls = combine_partials(dcls0, parts)
    return {"dm": (dm.reshape(B * Nc, d), udm.reshape(B * Nc, d)), "dcls": (dcls, ucls)}


# ---------------------------------------------------------------------------------------------------------------------------------
# split-row weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def wgrad_inputs(case):
    T, N, K = case
    rng = np.random.default_rng([T, N, K, 6])
    return dict(dY=rand_bf16(rng, (T, N)), X=rand_bf16(rng, (T, K)), dW0=_rand32(rng, (N, K)), dbias0=_rand32(rng, N))


def colsum_inputs(case=COLSUM_CASE):
    T, N = case
    rng = np.random.default_rng([T, N, 7])
    return dict(M=_rand32(rng, (T, N)), out0=_rand32(rng, N))


def wg_rows_per_wave(T, det=False):
    nsplit = 1 if det else -(-T // 1024)
    per = -(-T // nsplit)
    return -(-(-(-per // 4)) // 32) * 32


def wg_row_splits(T, det=False):
    return -(-T // (4 * wg_rows_per_wave(T, det)))


def wgrad(dY, X, dW0, dbias0, dt=np.float64, bug=None, det=False):
    """dW0 + dY^T X, dbias0 + column sums of dY.  float32: in the kernel's grouping -- a wave's rows in 32-row slabs, the four waves of a
    workgroup added owner first, the row splits' partial tiles as [ascending, descending]."""
    a, b = bf16_f32(dY).astype(dt), bf16_f32(X).astype(dt)
    T, N = a.shape
    w0 = np.zeros_like(dW0, dtype=dt) if bug == "dw_overwrite" else dW0.astype(dt)
    uW = np.abs(a).T @ np.abs(b) + np.abs(dW0.astype(dt))
    ub = np.abs(a).sum(0) + np.abs(dbias0.astype(dt))
    if dt is np.float64:
        return {"dW": (w0 + a.T @ b, uW), "dbias": (dbias0.astype(dt) + a.sum(0), ub)}
    rw, ns = wg_rows_per_wave(T, det), wg_row_splits(T, det)
    owner = (np.arange(N) % 64) // 16
    pW, pb = [], []
    for s in range(ns):
        accs, bsum = [], []
        for w in range(4):
            t0 = (4 * s + w) * rw
            t1 = min(t0 + rw, T)
            acc, cs = np.zeros((N, b.shape[1]), dtype=dt), np.zeros((8, N), dtype=dt)
            for ts in range(t0, t1, 32):
                sa_, sb_ = a[ts:min(ts + 32, t1)], b[ts:min(ts + 32, t1)]
                acc = acc + sa_.T @ sb_
                for i in range(0, sa_.shape[0], 8):
                    blk = sa_[i:i + 8]
                    cs[:blk.shape[0]] = cs[:blk.shape[0]] + blk
            idx = np.arange(8)
            for bit in (1, 2, 4):                          # the lanes' butterfly over the eight loaders of a column
                cs = cs + cs[idx ^ bit]
            accs.append(acc)
            bsum.append(cs[0])
        tile = np.zeros_like(accs[0])
        for o in range(4):
            rows = owner == o
            v = accs[o][rows]
            for r in range(4):
                if r != o:
                    v = v + accs[r][rows]
            tile[rows] = v
        pW.append(tile)
        pb.append(((bsum[0] + bsum[1]) + bsum[2]) + bsum[3])
    return {"dW": (combine_partials(w0, pW), uW), "dbias": (combine_partials(dbias0, pb), ub)}


def colsum(M, out0, dt=np.float64, bug=None, det=False):
    """out0 + column sums of the float32 matrix M (the K = 0 job).  float32: 32 rows per workgroup, four stripes of eight rows each."""
    a = M.astype(dt)
    T, N = a.shape
    u = np.abs(a).sum(0) + np.abs(out0.astype(dt))
    if dt is np.float64:
        return {"out": (out0.astype(dt) + a.sum(0), u)}
    nb = -(-T // 32)
    blocks = np.concatenate([a, np.zeros((nb * 32 - T, N), dtype=dt)]).reshape(nb, 8, 4, N)       # row r0 + 4 k + stripe
    parts, acc = [], np.zeros((4, N), dtype=dt)
    for blk in blocks:
        if not det:
            acc = np.zeros((4, N), dtype=dt)
        for k in range(8):
            acc = acc + blk[k]
        if not det:
            parts.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    if det:
        parts.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return {"out": (combine_partials(out0, parts), u)}


# ---------------------------------------------------------------------------------------------------------------------------------
# one case, every output of its kernels: the float64 reference (dt = float64) or the float32 evaluation
# ---------------------------------------------------------------------------------------------------------------------------------
BF16_OUTPUTS = {"att.ctx", "att.dq", "att.dk", "att.dv", "ln.y16", "ln.dx", "act.y", "act.dx", "noise.xn16", "comb.z16", "comb.dm"}
CASES = {"att": ATT_CASES, "ln": LN_CASES, "act": ACT_CASES, "noise": NOISE_CASES, "comb": COMBINE_CASES, "wgrad": WGRAD_CASES,
         "colsum": [COLSUM_CASE]}


def case_counter(kind, case) -> int:
    """The call counter a case runs with: the three values of COUNTERS in turn down each kernel's table."""
    return COUNTERS[CASES[kind].index(case) % 3]


def ln_saved(case):
    """(z, mean, rstd) the backward of a LayerNorm case is given: the float64 forward rounded to float32 (the same arrays for the device
    and for the float32 evaluation)."""
    T, d, res16, p, _ = case
    i = ln_inputs(case)
    f = layernorm_fwd(i["x"], i["res"], res16, i["gamma"], i["beta"], LN_EPS, p, SEED, case_counter("ln", case))
    return tuple(f[k][0].astype(np.float32) for k in ("z", "mean", "rstd"))


def evaluate(kind, case, dt=np.float64, bug=None, det=False):
    """{"<kind>.<output>": (value, unit)} of every kernel of `kind` on the inputs of `case`."""
    call = case_counter(kind, case)
    if kind == "att":
        Bn, S, H, dh, p = case
        i = att_inputs(case)
        out = attention_fwd(i["qkv"], Bn, S, H, dh, p, SEED, call, dt, bug, att_samples_per_wg(S, H, dh, False))
        out.update(attention_bwd(i["qkv"], i["dctx"], Bn, S, H, dh, p, SEED, call, dt, bug, att_samples_per_wg(S, H, dh, True)))
    elif kind == "ln":
        T, d, res16, p, _ = case
        i = ln_inputs(case)
        out = layernorm_fwd(i["x"], i["res"], res16, i["gamma"], i["beta"], LN_EPS, p, SEED, call, dt, bug)
        z, mean, rstd = ln_saved(case)
        out.update(layernorm_bwd(i["dy32"], i["dy16"], z, mean, rstd, i["gamma"], p, SEED, call, i["dgamma0"], i["dbeta0"], dt, bug))
    elif kind == "act":
        n, slope, p = case
        i = act_inputs(case)
        out = act_dropout_fwd(i["x"], slope, p, SEED, call, dt, bug)
        out.update(act_dropout_bwd(i["x"], i["dy"], slope, p, SEED, call, dt, bug))
    elif kind == "noise":
        i = noise_inputs(case)
        out = diffusion_noise(i["x"], i["t"], i["eps"], i["acp"], dt, bug)
    elif kind == "comb":
        B, Nc, d, _ = case
        i = combine_inputs(case)
        out = diffusion_combine_fwd(i["m"], i["xn32"], i["sa"], i["sb"], i["cls"], i["pe"], B, Nc, d, dt, bug)
        out.update(diffusion_combine_bwd(i["g"], i["g16"], i["sa"], i["sb"], i["dcls0"], B, Nc, d, dt, bug))
    elif kind == "wgrad":
        i = wgrad_inputs(case)
        out = wgrad(i["dY"], i["X"], i["dW0"], i["dbias0"], dt, bug, det)
    else:
        i = colsum_inputs(case)
        out = colsum(i["M"], i["out0"], dt, bug, det)
    return {f"{kind}.{k}": v for k, v in out.items()}


def stored(name, value, truncate=False):
    """A float32 evaluation's value as the kernel would leave it in memory, widened: bf16 outputs rounded to bf16."""
    value = np.asarray(value, dtype=np.float32)
    return bf16_f64(bf16_bits(value, truncate)) if name in BF16_OUTPUTS else value.astype(np.float64)
