"""The host references of tests/pointwise_ref.py checked on the CPU, so that tests/test_gpu_pointwise.py does not rest on an
unchecked restatement: Philox against the generator's published known answers, bf16 rounding against torch's CPU cast, the
argmax-routed pool gradient against the oracle's first-maximum form, and the statistics of the reference keep mask."""
import itertools

import numpy as np
import torch

import pointwise_ref as R
from oracle import tf13_ops as T

# Random123 kat_vectors, "philox4x32 10": counter[4], key[2] -> output[4]
PHILOX_KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# bit patterns every cast test feeds: +-0, +-inf, largest finite (rounds to inf), ties down / up to even, just below the
# next value, the last tie before infinity, denormals (a tie, an odd tie, 1e-40), the smallest denormal
SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F808000, 0x3F818000,
                         0x3F80FFFF, 0x7F7F8000, 0x00008000, 0x00018000, 0x000116C2, 0x800116C2, 0x00000001, 0x007FFFFF],
                        np.uint32)
NAN_BITS = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FA00000, 0xFF80FFFF], np.uint32)   # quiet, and signalling patterns


def test_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        got = R.philox4x32_10(ctr, key)
        assert tuple(int(g) for g in got) == want
    # vectorised: the three at once give the same
    ctr = [np.array([k[0][j] for k in PHILOX_KAT], np.uint64) for j in range(4)]
    key = [np.array([k[1][j] for k in PHILOX_KAT], np.uint64) for j in range(2)]
    got = np.stack(R.philox4x32_10(ctr, key), axis=1)
    np.testing.assert_array_equal(got, np.array([k[2] for k in PHILOX_KAT], np.uint64))


def test_keep_uniform_indexing():
    """Element i is word i % 4 of block i // 4; the counter's and key's high words are the high halves of step and seed."""
    seed, step = (7 << 32) | 3000, (5 << 32) | 2
    u = R.keep_uniform(11, seed, step)
    for i in (0, 1, 5, 10):
        words = R.philox4x32_10((i // 4, 0, 2, 5), (3000, 7))
        assert u[i] == np.float32(int(words[i % 4]) >> 8) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()


def test_bf16_round_against_torch_cpu():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(1 << 16).astype(np.float32) * np.float32(3),
                        (rng.standard_normal(4096) * 1e-39).astype(np.float32),          # denormals
                        SPECIAL_BITS.view(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_round(x)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(R.bf16_to_f32(got), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    # the named cases, stated: ties to even, overflow to infinity, signed zero, denormals kept
    named = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F80FFFF: 0x3F81, 0x7F7F8000: 0x7F80, 0x7F7FFFFF: 0x7F80,
             0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002, 0x000116C2: 0x0001}
    for src, dst in named.items():
        assert int(R.bf16_round(np.array([src], np.uint32).view(np.float32))[0]) == dst, hex(src)
    nan = R.bf16_round(NAN_BITS.view(np.float32))
    assert ((nan & 0x7FFF) > 0x7F80).all()                                      # NaN stays NaN
    assert np.isnan(torch.from_numpy(NAN_BITS.view(np.float32).copy()).to(torch.bfloat16).float().numpy()).all()
    flushed = R.bf16_round(np.array([0x00018000, 0x800116C2, 0x00800000], np.uint32).view(np.float32), flush_denormals=True)
    np.testing.assert_array_equal(flushed, np.array([0x0000, 0x8000, 0x0080], np.uint16))


def test_argmax_routing_against_first_maximum_oracle():
    rng = np.random.default_rng(9)
    for n, h, w, c in [(2, 6, 8, 5), (1, 5, 7, 3), (3, 2, 2, 1), (1, 3, 3, 4)]:
        x = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32)
        ho, wo = h // 2, w // 2
        win = x[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, ho, wo, c, 4)
        arg = win.argmax(-1).astype(np.uint8)                                     # first maximum, as T.maxpool2x2_bwd
        pooled = T.maxpool2x2_fwd(x)
        dy = rng.standard_normal(pooled.shape).astype(np.float32)
        np.testing.assert_array_equal(R.maxpool2x2_bwd_from_argmax(arg, pooled, dy, h, w, False), T.maxpool2x2_bwd(x, dy))
        np.testing.assert_array_equal(R.maxpool2x2_bwd_from_argmax(arg, pooled, dy, h, w, True),
                                      T.relu_grad(T.maxpool2x2_bwd(x, dy), x))
    # routed by the byte, not by the values
    dx = R.maxpool2x2_bwd_from_argmax(np.array([3], np.uint8).reshape(1, 1, 1, 1), np.ones((1, 1, 1, 1), np.float32),
                                      np.full((1, 1, 1, 1), 5, np.float32), 3, 3, True)
    assert dx[0, 1, 1, 0] == 5 and dx.sum() == 5


def test_keep_mask_statistics_of_the_reference():
    n = 1 << 20
    for rate in (0.5, 0.25, 0.9):
        p = 1 - rate
        m = R.keep_mask(n, 3000, 2, rate)
        assert set(np.unique(m)) <= {0, 1}
        assert abs(m.mean() - p) < 5 * np.sqrt(p * (1 - p) / n)                  # binomial: sigma = sqrt(p (1 - p) / n)
        np.testing.assert_array_equal(m, R.keep_mask(n, 3000, 2, rate, form='floor'))
    seed, step = 3000, 2
    masks = [R.keep_mask(n, s, t, 0.5) for s, t in [(seed, step), (seed + 1000, step), (seed, step + 1),
                                                    (seed + 2 ** 32, step), (seed, step + 2 ** 32)]]
    for a, b in itertools.combinations(masks, 2):                                # independent fair bits differ in half
        assert abs((a != b).mean() - 0.5) < 5 * np.sqrt(0.25 / n)


def test_keep_mask_forms_differ_only_where_the_sum_rounds_to_two():
    """rate = 0: keep_prob = 1 and u = 1 - 2^-24 give fl(1 + u) = 2 (tie to even).  seed 3000, step 2 draws that u at element
    3768265; the header's mask is {0, 1} there as everywhere."""
    i = 3768265
    u = R.keep_uniform(i + 3, 3000, 2)
    assert u[i] == np.float32(1 - 2.0 ** -24)
    floor, m01 = R.keep_mask(i + 3, 3000, 2, 0.0, form='floor'), R.keep_mask(i + 3, 3000, 2, 0.0)
    assert floor[i] == 2 and m01[i] == 1 and (m01 == 1).all()
    differ = np.flatnonzero(floor != m01)                                         # every element that drew all 24 bits set
    np.testing.assert_array_equal(differ, np.flatnonzero(u == np.float32(1 - 2.0 ** -24)))
    assert i in differ and (floor[differ] == 2).all()


def test_adam_poisoned_statement():
    f = np.float32
    a = np.array([1, np.nan, np.inf, 2], f)
    assert R.adam_poisoned(a, a, a.copy(), a.copy()) == 0                        # nothing changed
    b = a.copy(); b[0] = np.nan
    assert R.adam_poisoned(a, a, b, a) == 1 and R.adam_poisoned(a, a, a, b) == 1
    b = a.copy(); b[2] = np.nan                                                   # an infinity that became NaN
    assert R.adam_poisoned(a, a, b, a) == 1
    b = a.copy(); b[3] = 5                                                        # a finite change is not poison
    assert R.adam_poisoned(a, a, b, a) == 0
