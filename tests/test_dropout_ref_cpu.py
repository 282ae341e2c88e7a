"""The numpy restatement of the dropout masks (tests/dropout_ref.py) against published constants and its own
definition: the GPU dropout parity tests inject these masks into the oracle, so a slip here would show there as
errors of order 0.1 and be blamed on the kernels."""
import numpy as np
import pytest

import dropout_ref as dr


def test_mix64_is_splitmix64():
    """splitmix64's first output for seed 0 (the state advances by the golden-ratio constant, then is mixed)."""
    assert int(dr.mix64(0)) == 0xE220A8397B1DCDAF
    # wrap-around: a value whose increment overflows 2^64
    z = (0xFFFFFFFFFFFFFFFF + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    assert int(dr.mix64(np.uint64(0xFFFFFFFFFFFFFFFF))) == z ^ (z >> 31)
    assert int(dr.mix64(-1)) == z ^ (z >> 31)          # negative Python ints wrap like the device's casts


def test_fmix32_murmur3_values():
    assert int(dr.fmix32(1)) == 0x514E28B7
    assert int(dr.fmix32(0)) == 0


def test_hash4_and_drop_base_nesting():
    a, b, c, d = 0x1234567890ABCDEF, 7, 299, 41
    want = dr.mix64(np.uint64(a) ^ dr.mix64(np.uint64(b) ^ dr.mix64(np.uint64(c) ^ dr.mix64(d))))
    assert int(dr.hash4(a, b, c, d)) == int(want)
    assert int(dr.drop_base(a, b, c, d)) == int(want) & 0xFFFFFFFF
    # vectorised over keys, scalar elsewhere
    ks = np.arange(5, dtype=np.int64)
    v = dr.drop_base(a, b, ks, d)
    assert v.dtype == np.uint32 and [int(x) for x in v] == [int(dr.drop_base(a, b, int(k), d)) for k in ks]


def test_step_seed_formula():
    base, nb = 0, 3
    assert dr.step_seed(base, nb) == (int(dr.mix64(int(dr.mix64(nb)) ^ base)) >> 1)
    assert 0 <= dr.step_seed(12345, 1) < 2 ** 63
    assert dr.step_seed(0, 1) != dr.step_seed(0, 2)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.6])
def test_threshold_is_an_exact_integer_compare(p):
    """kept <=> (h >> 8) >= ceil(float32(p) 2^24) <=> (h >> 8) 2^-24 >= float32(p), both sides exact."""
    thr = dr.threshold(p)
    p32 = float(np.float32(p))
    assert thr == int(np.ceil(p32 * 2 ** 24)) and (thr - 1) / 2 ** 24 < p32 <= thr / 2 ** 24
    base = dr.drop_base(99, 7, np.arange(4000), 5)
    idx = np.arange(4000) % 3
    h24 = dr.keep_hash(base, idx)
    assert int(h24.max()) < 2 ** 24
    keep = dr.keep32(base, idx, p)
    assert np.array_equal(keep, h24.astype(np.float64) / 2 ** 24 >= p32)
    assert np.array_equal(keep, h24.astype(np.int64) >= thr)
    s = dr.keep_scale(base, idx, p)
    assert set(np.unique(s).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert np.array_equal(s != 0, keep)


def test_keep_hash_index_multiplier_wraps_mod_2_32():
    base = np.uint32(0xDEADBEEF)
    for idx in (0, 1, 171, 172, 271, 2 ** 31 + 5):
        want = int(dr.fmix32(int(base) ^ ((idx * 0x9E3779B9) & 0xFFFFFFFF))) >> 8
        assert int(dr.keep_hash(base, idx)) == want


def test_p_zero_keeps_everything():
    base = dr.drop_base(1, 2, np.arange(12000), 0)
    assert dr.threshold(0.0) == 0 and dr.keep32(base, 0, 0.0).all()
    assert np.array_equal(dr.keep_scale(base, 0, 0.0), np.ones(12000, np.float32))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.6])
def test_dropped_share_over_12000_keys(p):
    base = dr.drop_base(dr.step_seed(0, 1), 7, np.arange(6000), np.arange(6000) * 3 + 1)
    keep = np.stack([dr.keep32(base, 0, p), dr.keep32(base, 1, p)], 1)
    assert keep.size == 12000
    assert abs((1.0 - keep.mean()) - p) <= 0.02
