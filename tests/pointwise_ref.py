"""Host references (numpy only) of the exact operations in ann3depth_amd/csrc/pointwise.hip and pool.hip that
oracle/tf13_ops.py does not already restate: the Philox4x32-10 keep mask of a3d_dropout_keep_mask, round-to-nearest-even float32 -> bf16, the
max-pool gradient routed by recorded argmax bytes, and the meaning of a3d_adam_apply_tf1_flag's `poisoned` bit.  Each is a
restatement of the contract in include/a3d.h; tests/test_pointwise_ref.py pins them to published vectors, torch's CPU
cast and the oracle, and tests/test_gpu_pointwise.py holds the kernels to them bit for bit."""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57            # Salmon et al. 2011, Philox4x32 multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments (golden ratio, sqrt(3) - 1)
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: 4 and key: 2 uint64 arrays (or ints) holding 32-bit words, broadcast against
    each other; returns the 4 output words as uint64 arrays."""
    c = [np.asarray(v, np.uint64) & _M32 for v in counter]
    k0, k1 = (np.asarray(v, np.uint64) & _M32 for v in key)
    s = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]                   # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & _M32, (p0 >> s) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return c


def keep_uniform(count, seed, step):
    """The float32 u_i in [0, 1) of a3d_dropout_keep_mask: element i takes word i % 4 of the Philox block whose counter is
    (q lo, q hi, step lo, step hi), q = i // 4, under the key (seed lo, seed hi); u = float32(word >> 8) * 2^-24."""
    nquad = (count + 3) // 4
    q = np.arange(nquad, dtype=np.uint64)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    words = philox4x32_10((q & _M32, q >> np.uint64(32), step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:count]
    return (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(count, seed, step, rate, form='01'):
    """uint8 mask of a3d_dropout_keep_mask.  form '01' (the header's contract): 1 where fl(keep_prob + u) >= 1, else 0;
    form 'floor': floor(fl(keep_prob + u)) as TF-1.3's nn.dropout states it, which differs from '01' only at rate 0, where
    fl(1 + (1 - 2^-24)) = 2.  All arithmetic in float32, keep_prob = float32(1) - float32(rate)."""
    u = keep_uniform(count, seed, step)
    s = (np.float32(1) - np.float32(rate)) + u
    assert s.dtype == np.float32
    if form == 'floor':
        return np.floor(s).astype(np.uint8)
    return (s >= np.float32(1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ bf16
def bf16_round(x, flush_denormals=False):
    """float32 -> the uint16 bits of the nearest bfloat16, ties to even, computed on the bits.  Overflow goes to infinity,
    the sign of zero is kept, denormals round like every other value (flush_denormals=True: float32 denormal inputs give a
    zero of their sign instead), NaN gives a quiet NaN of the same sign (payload: the top 7 bits, bit 6 set)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b.astype(np.uint64) + np.uint64(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), r)
    if flush_denormals:
        den = ((b & np.uint32(0x7F800000)) == 0)
        r = np.where(den, (b >> np.uint32(16)).astype(np.uint16) & np.uint16(0x8000), r)
    return r.astype(np.uint16)


def bf16_to_f32(bits):
    """uint16 bf16 bits -> the float32 of the same value (exact)."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_values(x):
    """float32 -> the float32 array of the bf16-rounded values."""
    return bf16_to_f32(bf16_round(x))


def same_bf16(got_bits, want_bits):
    """True where two bf16 bit patterns are the same value: equal bits, or both NaN (the payload is free)."""
    g, w = np.asarray(got_bits, np.uint16), np.asarray(want_bits, np.uint16)
    gn, wn = (g & 0x7FFF) > 0x7F80, (w & 0x7FFF) > 0x7F80
    return (g == w) | (gn & wn)


# ------------------------------------------------------------------------------------------------ pool gradient by argmax
def maxpool2x2_bwd_from_argmax(arg, pooled, dy, h, w, relu_mask):
    """The a3d_maxpool2x2_bwd_idx* contract: dx[n, h, w, c] (dy's dtype) takes dy[b, p, q, ch] at row 2p + arg // 2, column
    2q + arg % 2 of window (p, q) where (!relu_mask or pooled > 0), zero everywhere else, the odd last row / column that
    VALID flooring cuts included.  arg uint8 [n, h//2, w//2, c] with values 0..3 (another value: the window gets nothing);
    pooled and dy [n, h//2, w//2, c]."""
    n, ho, wo, c = arg.shape
    assert (ho, wo) == (h // 2, w // 2) and pooled.shape == arg.shape == dy.shape
    g = np.where(pooled > 0, dy, dy.dtype.type(0)) if relu_mask else dy
    cells = np.zeros((n, ho, wo, c, 4), dy.dtype)
    for k in range(4):
        cells[..., k] = np.where(arg == k, g, dy.dtype.type(0))
    dx = np.zeros((n, h, w, c), dy.dtype)
    dx[:, :2 * ho, :2 * wo, :] = cells.reshape(n, ho, wo, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, 2 * ho, 2 * wo, c)
    return dx


# ------------------------------------------------------------------------------------------------ ApplyAdam's flag
def adam_poisoned(var_before, v_before, var_after, v_after):
    """Bit 0 of a3d_adam_apply_tf1_flag's `poisoned` word: 1 when the update CHANGED an element of var or v INTO a
    non-finite value (a NaN that stays a NaN and an infinity that stays that infinity are no change).  That is the event a
    rank-sharded frozen optimizer has to tell the other ranks about: their copies of the slice no longer match."""
    def turned(a, b):
        same = (a == b) | (np.isnan(a) & np.isnan(b))
        return bool((~np.isfinite(b) & ~same).any())
    return int(turned(var_before, var_after) or turned(v_before, v_after))
