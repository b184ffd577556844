"""The NumPy mirror of the Bayesian draws (tests/bayes_stream.py) against the host code of the same stream: the sub-stream seeding of
bayes._mix is the dropout key of csrc/dropout_stream.hpp shifted by one golden-ratio step, and uniforms live on the 2^-24 grid."""
import numpy as np

from openpystruct_amd import bayes
from tests import bayes_stream as bs

_SEEDS = [0, 1, 0xFFFFFFFF, 1 << 32, 0x8000000000000001, 0xFFFFFFFFFFFFFFFF, 0xB7E151628AED2A6B, 0xD1B54A32D192ED03]
_CALLS = [0, 1, 2, 0xFFFFFFFF, (1 << 32) + 5, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF]


def test_mirror_key_equals_the_host_mix_and_uniforms_sit_on_the_grid():
    for seed in _SEEDS:
        for call in _CALLS:
            k0, k1 = bs.drop_key(seed, call)
            z = bayes._mix((seed + bs.GOLDEN * call) & bs.MASK64)
            assert (k0, k1) == (z & 0xFFFFFFFF, z >> 32), (hex(seed), hex(call))
    key = bs.bayes_key(0xFEDCBA9876543210, (1 << 32) + 5, 3)
    idx = np.concatenate([np.arange(100_000, dtype=np.uint64), np.uint64(1 << 32) + np.arange(1000, dtype=np.uint64),
                          np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64)])
    u = bs.drop_uniform(key, idx)
    assert u.min() >= 0.0 and u.max() < 1.0
    np.testing.assert_array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    np.testing.assert_array_equal(u, u.astype(np.float32).astype(np.float64))
    # the high index word enters the hash: index i and i + 2^32 do not collide
    assert not np.array_equal(u[:1000], u[100_000:101_000])
    # the layer salt separates the layers' streams; the normals are finite and standard-ish
    e0, b0 = bs.layer_eps(7, 0, 0, 200_000)
    e1, _ = bs.layer_eps(7, 0, 1, 200_000)
    assert not np.array_equal(e0, e1)
    assert np.isfinite(e0).all() and abs(e0.mean()) < 0.02 and abs(e0.std() - 1) < 0.02
    assert (b0 > 0).all() and b0.max() < 1e-5
    # the step draw covers [0, T) and nothing else
    for T in (1, 7, 512):
        t = bs.diffusion_t(3, 4, 5000, T, row_base=123)
        assert t.min() == 0 and t.max() == T - 1
