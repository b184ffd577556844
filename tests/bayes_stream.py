"""NumPy mirror of the Bayesian draws of csrc/bayes_mlp.hip (test code).

    uniform   drop_key / drop_uniform of csrc/dropout_stream.hpp: uint32 arithmetic, bit for bit (the device result is a 24-bit
              integer times 2^-24, exact in float32 and float64)
    normal    bayes_key / bayes_normal: Box-Muller from the uniforms at 2e and 2e + 1, evaluated in float64 with the exact 2 pi
    t         the diffusion step (int)(u * T) with the product rounded in float32 as on the device, clamped to T - 1: bit for bit
    xeps      the diffusion noise of global row row_base + i, column c at element (row_base + i) * K + c of layer 3's stream

Error of the device's float32 normal against `normal` here (the build is -fno-fast-math -ffp-contract=off; u = 2^-24):
    u1 = 1 - U and u2 are exact in float32 (both on the 2^-24 grid), so only the evaluation rounds.
    r = sqrtf(-2 logf(u1)): logf within 2 ulp (<= 4 u relative; its argument is exact), the doubling is exact, sqrtf halves the
        relative error and adds at most 1 u: |dr| <= 3 u r.
    phi = 6.2831855f * u2: the float32 constant differs from 2 pi by 1.75e-7 and the product rounds by at most 1/2 ulp of a value below
        2 pi, i.e. <= 2 pi 2^-24: |dphi| <= 1.75e-7 + 2 pi u; cosf (~2 ulp of a value <= 1) adds 2 u, and cos has slope <= 1.
    the final product rounds by 1/2 ulp of |eps| <= r.
So |eps_dev - eps| <= r (1.75e-7 + 2 pi u + 2 u) + 3 u r + u r = r (1.75e-7 + (2 pi + 6) u) (`normal_with_bound`), ~ 9e-7 r.
"""
from __future__ import annotations

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
LAYER_SALT = 0xD1B54A32D192ED03
U = 2.0 ** -24
TWO_PI_F32_ERR = abs(float(np.float32(6.28318530717958647692)) - 2 * np.pi)       # 1.75e-7


def drop_key(seed: int, call: int):
    """(k0, k1) of csrc/dropout_stream.hpp drop_key (splitmix64 of seed + golden * (call + 1))."""
    z = (int(seed) + GOLDEN * ((int(call) + 1) & MASK64)) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z & 0xFFFFFFFF, z >> 32


def drop_bits(key, idx) -> np.ndarray:
    """The 24-bit integer behind drop_uniform(key, idx); idx any integer array, key (k0, k1) scalars or arrays that broadcast with it."""
    k0, k1 = (np.asarray(k, dtype=np.uint32) for k in key)
    idx = np.asarray(idx, dtype=np.uint64)
    x = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ k0
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= k1 ^ hi
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x >> np.uint32(8)


def drop_uniform(key, idx) -> np.ndarray:
    """[0, 1) on the 2^-24 grid, float64 (exactly the device's float32 value)."""
    return drop_bits(key, idx).astype(np.float64) * U


def bayes_key(seed: int, counter: int, layer: int):
    return drop_key(int(seed) ^ ((LAYER_SALT * (layer + 1)) & MASK64), counter)


def _box_muller(key, e):
    e = np.asarray(e, dtype=np.uint64)
    u1 = 1.0 - drop_uniform(key, e * np.uint64(2))
    u2 = drop_uniform(key, e * np.uint64(2) + np.uint64(1))
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r


def bayes_normal(key, e) -> np.ndarray:
    """float64 Box-Muller normal of element(s) e."""
    return _box_muller(key, e)[0]


def normal_with_bound(key, e):
    """(bayes_normal, per-element bound on |device float32 normal - bayes_normal|); derivation in the module docstring."""
    v, r = _box_muller(key, e)
    return v, r * (TWO_PI_F32_ERR + (2 * np.pi + 6) * U)


def layer_eps(seed: int, counter: int, layer: int, n: int):
    """(eps, bound) of elements 0 .. n - 1 of one layer's stream: the weights row-major, then the biases."""
    return normal_with_bound(bayes_key(seed, counter, layer), np.arange(n, dtype=np.uint64))


def _sample_keys(seed: int, S: int, layer: int):
    """Keys of samples (counters) 0 .. S - 1 of one layer as [S, 1] uint32 columns."""
    ks = [bayes_key(seed, s, layer) for s in range(S)]
    return (np.array([k[0] for k in ks], dtype=np.uint32)[:, None], np.array([k[1] for k in ks], dtype=np.uint32)[:, None])


def _per_sample_normals(seed: int, S: int, layer: int, idx: np.ndarray):
    """(eps, bound) [S, idx.size] of elements idx of every sample's stream of `layer`, vectorised over samples in chunks."""
    k0, k1 = _sample_keys(seed, S, layer)
    idx = np.asarray(idx, dtype=np.uint64).reshape(1, -1)
    eps = np.empty((S, idx.shape[1]))
    bnd = np.empty_like(eps)
    step = max(1, (1 << 22) // max(1, idx.shape[1]))
    for s0 in range(0, S, step):
        sl = slice(s0, s0 + step)
        eps[sl], bnd[sl] = normal_with_bound((k0[sl], k1[sl]), idx)
    return eps, bnd


def mc_eps(seed: int, S: int, K: int, H: int, N: int):
    """Every sample's weight draws of one Monte-Carlo block, in eps_out's layout [S, H K + H + N H + N] (lin1 weights, lin1 biases,
    lin2 weights, lin2 biases): (eps, bound), float64.  Sample s is counter s; lin1 is layer 0, lin2 layer 1."""
    e1, b1 = _per_sample_normals(seed, S, 0, np.arange(H * K + H))
    e2, b2 = _per_sample_normals(seed, S, 1, np.arange(N * H + N))
    return np.concatenate([e1, e2], axis=1), np.concatenate([b1, b2], axis=1)


def diffusion_t(seed: int, S: int, P: int, T: int, row_base: int = 0) -> np.ndarray:
    """[S, P] int64 diffusion steps: (int)(u * (float)T) in float32, clamped to T - 1, keyed by the global row row_base + i."""
    u = drop_uniform(_sample_keys(seed, S, 2), np.arange(row_base, row_base + P, dtype=np.uint64)[None, :]).astype(np.float32)
    return np.minimum((u * np.float32(T)).astype(np.int64), T - 1)


def diffusion_eps(seed: int, S: int, P: int, K: int, row_base: int = 0):
    """([S, P, K], bound) diffusion noise of global rows row_base .. row_base + P - 1: element (row_base + i) * K + c."""
    idx = np.arange(row_base, row_base + P, dtype=np.uint64)[:, None] * np.uint64(K) + np.arange(K, dtype=np.uint64)[None, :]
    eps, bnd = _per_sample_normals(seed, S, 3, idx)
    return eps.reshape(S, P, K), bnd.reshape(S, P, K)
