"""The cases of tests/test_gpu_dense_exact.py: one row per launch of ann3depth_amd/csrc/dense.hip that the suite holds element by
element, with the route the row EXPECTS written out — kernel and template arguments, grid, and for the forward its split count
and span, for the Adam stream kernels the row groups a block walks (gpb).  Nothing here computes a route: the numbers were
worked out by hand from the dispatch and are held to the library's own `a3d dense:` line (A3D_TUNING=1 A3D_PLAN_LOG=1) by
tests/exact_dense_worker.py, so a row that lands somewhere else is a failure, not a silent change of what is tested.
tests/test_dense_cases_cpu.py holds the table to the source: the kernels these rows expect are exactly the instantiations
dense.hip can launch.  No GPU and no torch in here.

Operands are exact_ops.dense_case's ternary integers: every sum is an integer far below 2^24 (asserted when the case is built),
exact in float32 and, ternary, in bf16 — so the bf16 stream kernels are held to the same integers.  adam_steps() states the
two ApplyAdam steps every Adam row runs; their values are multiples of 1/8 below 2^24 / 8, asserted there."""
import collections

import numpy as np

import exact_ops as E

Row = collections.namedtuple('Row', 'entry shape precision align route edge')
FWD, DW, ADAM = 'a3d_dense_fwd', 'a3d_dense_bwd_filter', 'a3d_dense_bwd_filter_adam_tf1_ex'
# what the route line calls the launch site behind each entry point
SITE = {FWD: 'dense_fwd_stream', DW: 'dense_dw_launch', ADAM: 'a3d_dense_bwd_filter_adam_tf1_ex'}

F1, F2 = 'dense_fwd_stream_kernel<1>', 'dense_fwd_stream_kernel<2>'
PLAIN, PLAIN_ADAM = 'dense_dw_kernel<false,4>', 'dense_dw_kernel<true,4>'
ROWS4, ROWS2 = 'dense_dw_adam_rows_kernel<4>', 'dense_dw_adam_rows_kernel<2>'
SLIM, WIDE = 'dense_dw_adam_stream_kernel<2,1,2>', 'dense_dw_adam_stream_kernel<2,2>'
BF4, BF2 = 'dense_dw_adam_stream_kernel<4,2,1,true>', 'dense_dw_adam_stream_kernel<2,2,1,true>'


def fwd(m, k, n, kernel, grid, splits, span, edge):
    assert grid[1] == splits
    return Row(FWD, (m, k, n), 'fp32', {}, dict(kernel=kernel, grid=grid, splits=splits, span=span), edge)


def dw(m, k, n, grid, edge):
    return Row(DW, (m, k, n), 'fp32', {}, dict(kernel=PLAIN, grid=grid), edge)


def adam(m, k, n, kernel, grid, edge, gpb=None, precision='fp32', align=None):
    route = dict(kernel=kernel, grid=grid, **({} if gpb is None else {'gpb': gpb}))
    return Row(ADAM, (m, k, n), precision, align or {}, route, edge)


# ---- forward, split: one slab per split, bias / activation / dropout in the split-K reduction ----
FORWARD_SPLIT = [
    fwd(1, 132, 8193, F1, (65, 3), 3, 64, 'one batch row; n % 128 == 1: a column block of one column; k % 64 == 4: a last split of 4 rows'),
    fwd(31, 260, 4223, F1, (33, 5), 5, 64, 'n % 128 == 127, n % 4 == 3: the last lane\'s 16 bytes run into the next row of W'),
    fwd(32, 256, 4096, F1, (32, 4), 4, 64, 'every one of the 32 MFMA rows live, no tail anywhere'),
    fwd(5, 1028, 1030, F1, (9, 17), 17, 64, 'n % 4 == 2, seventeen splits, a last split of 4 rows'),
    fwd(33, 132, 8193, F2, (65, 3), 3, 64, 'one row in the second batch tile; n % 128 == 1'),
    fwd(63, 260, 4223, F2, (33, 5), 5, 64, 'second batch tile one row short; n % 128 == 127'),
    fwd(64, 128, 8200, F2, (65, 2), 2, 64, 'both batch tiles full; n % 128 == 8'),
    fwd(64, 256, 4096, F2, (32, 4), 4, 64, 'both batch tiles full, no tail anywhere'),
]
# ---- forward, unsplit: bias / activation / dropout inside dense_fwd_stream_kernel ----
FORWARD_UNSPLIT = [
    fwd(4, 64, 16384, F1, (128, 1), 1, 64, 'k <= 64 at n >= 16384: one split, the in-kernel epilogue'),
    fwd(9, 68, 32771, F1, (257, 1), 1, 128, 'n > 32768 and k > 64; k = 68: the third wave takes 4 rows, the fourth none; n % 4 == 3'),
    fwd(2, 4, 262145, F1, (2049, 1), 1, 64, 'k = 4: one wave works, three add zero tiles; n % 128 == 1'),
    fwd(33, 64, 16388, F2, (129, 1), 1, 64, 'one row in the second batch tile; n % 128 == 4'),
    fwd(64, 68, 32771, F2, (257, 1), 1, 128, 'n > 32768 and k > 64, both batch tiles full; n % 4 == 3'),
]
# (bias, activation, dropout): with and without bias, ReLU and none, dropout (x 2 is exact) — run on every forward row
FORWARD_VARIANTS = [(True, None, False), (False, 'relu', False), (True, 'relu', True), (False, None, True)]
# sigmoid (held to float64, not exact): bias + sigmoid on one unsplit and one split row
SIGMOID = [FORWARD_UNSPLIT[0], FORWARD_SPLIT[4]]

# ---- a3d_dense_bwd_filter at k n >= 2^16: dense_dw_kernel<false, 4>, eight batch-row pairs per pass of its loop ----
FILTER_GRADIENT = [
    dw(17, 130, 513, (5, 2), 'two passes of the loop, an odd last pair; n % 128 == 1; k % 128 == 2'),
    dw(33, 200, 383, (3, 2), 'three passes, an odd last pair; n % 128 == 127, n % 4 == 3; k % 128 == 72'),
    dw(64, 132, 511, (4, 2), 'four full passes; n % 128 == 127; k % 128 == 4'),
]

# ---- the fused filter gradient + ApplyAdam ----
ADAM_ONE_GROUP = [      # gpb == 1, and the three forms outside the stream kernels
    adam(32, 384, 520, SLIM, (3, 12), 'whole row groups, a last column block of 8 columns', gpb=1),
    adam(1, 132, 258, SLIM, (2, 5), 'one batch row; a last row group of 4 rows, a last column block of 2 columns', gpb=1),
    adam(31, 260, 1030, SLIM, (5, 9), 'odd batch: the last pair of rows is half empty', gpb=1),
    adam(48, 260, 518, WIDE, (3, 9), '33..64 rows on the float32 stream form, tails in k and n', gpb=1),
    adam(45, 1028, 1030, BF2, (3, 33), 'bf16 arithmetic, 8-byte columns; 45 rows: a partial last 16-row step', gpb=1, precision='bf16'),
    adam(64, 516, 1032, BF4, (3, 17), 'bf16 arithmetic, 16-byte columns', gpb=1, precision='bf16'),
    adam(64, 130, 516, ROWS4, (2, 5), 'k % 4 == 2 leaves the stream kernels; n % 512 == 4, k % 32 == 2'),
    adam(1, 132, 518, ROWS2, (2, 5), 'x one float off the 16-byte grid leaves the stream kernels; n % 4 == 2', align={'x': 4}),
    adam(64, 130, 517, PLAIN_ADAM, (5, 2), 'odd n: no vector form of the m slot at all'),
    adam(64, 132, 518, ROWS2, (2, 5), 'the 8-byte rows form at a batch the poisoned gradient can use; n % 512 == 6, k % 32 == 4', align={'x': 4}),
]
# gpb == 2 on 33 row groups: grid y 17, the last block walks ONE group, and that group has 4 rows (k = 1028)
ADAM_SLIM_MULTI = [
    adam(32, 1028, 8450, SLIM, (34, 17), '34 column blocks x 33 groups; a last column block of 2 columns', gpb=2),
    adam(17, 1028, 8452, SLIM, (34, 17), 'the same walk at an odd batch; a last column block of 4 columns', gpb=2),
]
ADAM_WIDE_MULTI = [
    adam(64, 1028, 4102, WIDE, (17, 17), '17 column blocks x 33 groups; a last column block of 6 columns', gpb=2),
    adam(33, 1028, 4100, WIDE, (17, 17), 'one row in the second batch tile', gpb=2),
]
ADAM_BF16_MULTI = [
    adam(40, 1028, 8200, BF4, (17, 17), '17 column blocks of 512 x 33 groups; a last column block of 8 columns', gpb=2, precision='bf16'),
    adam(64, 1028, 8198, BF2, (17, 17), 'the 8-byte form; a last column block of 6 columns', gpb=2, precision='bf16'),
]
# every Adam row: with the bias slots and without them
ADAM_VARIANTS = [True, False]
GRAD_SCALE = 0.5

# the pytest cases of test_gpu_dense_exact.py: a group is one child process
GROUPS = {
    'forward-split': FORWARD_SPLIT + [SIGMOID[1]._replace(edge='sigmoid')],
    'forward-unsplit': FORWARD_UNSPLIT + [SIGMOID[0]._replace(edge='sigmoid')],
    'filter-gradient-and-one-group': FILTER_GRADIENT + ADAM_ONE_GROUP,
    'adam-slim-multi-group': ADAM_SLIM_MULTI,
    'adam-wide-multi-group': ADAM_WIDE_MULTI,
    'adam-bf16-multi-group': ADAM_BF16_MULTI,
}
# run-to-run bits and the poison semantics: one multi-group row of each stream instantiation, in that row's group
REPEATED = [ADAM_SLIM_MULTI[0], ADAM_WIDE_MULTI[1], ADAM_BF16_MULTI[0], ADAM_BF16_MULTI[1]]
# the poison semantics alone (one poisoned launch, no three-run bit check) on the three forms outside the stream kernels too: the
# smallest rows that reach their tails with a batch of more than one row
POISONED = REPEATED + [ADAM_ONE_GROUP[6], ADAM_ONE_GROUP[8], ADAM_ONE_GROUP[9]]
ALL = FORWARD_SPLIT + FORWARD_UNSPLIT + FILTER_GRADIENT + ADAM_ONE_GROUP + ADAM_SLIM_MULTI + ADAM_WIDE_MULTI + ADAM_BF16_MULTI


def is_sigmoid(row):
    return row.edge == 'sigmoid'


def launches(row):
    """how many route lines a verified row leaves"""
    if row.entry == FWD:
        return 1 if is_sigmoid(row) else len(FORWARD_VARIANTS)
    if row.entry == DW:
        return 2
    # two steps each; repeated: 3 launches for the bits; poisoned: 1 launch
    return 2 * len(ADAM_VARIANTS) + (3 if row in REPEATED else 0) + (1 if row in POISONED else 0)


def case(row):
    return E.dense_case(*row.shape)


def forward_reference(cs, bias, act, drop):
    s = cs.y if bias else cs.y - E.f64(cs.b)
    s = np.maximum(s, 0) if act == 'relu' else s
    return 2.0 * s * cs.keep if drop else s


def second_dz(cs):
    """the gradient of the second Adam step: the first one's, moved by one batch row and three columns"""
    return np.roll(cs.dz, (1, 3), axis=(0, 1))


def adam_steps(cs):
    """[(dz, beta1, beta1_power, m_w, m_b)] of the two steps on the same slots, m from zero, grad_scale 0.5, in float64.
    Step 1 is the off-grid suite's: beta1 = 0 on a zero slot, m becomes the scaled gradient itself.  Step 2 (beta1 = 1/2) must
    read that m back: m + (g - m) / 2.  alpha = 0 and beta2 = 1: var and v stay what they were.  Every value is a multiple of 1/8
    and 8 max|value| < 2^24: each of the kernel's separate float32 operations is exact."""
    out, m_w, m_b = [], np.zeros_like(cs.dw), np.zeros_like(cs.db)
    for dz, beta1, b1p in ((cs.dz, 0.0, 0.0), (second_dz(cs), 0.5, 0.25)):
        g_w, g_b = GRAD_SCALE * (E.f64(cs.x).T @ E.f64(dz)), GRAD_SCALE * E.f64(dz).sum(0)
        m_w, m_b = m_w + (g_w - m_w) * (1.0 - beta1), m_b + (g_b - m_b) * (1.0 - beta1)
        for what, a in (('g_w', g_w), ('g_b', g_b), ('m_w', m_w), ('m_b', m_b)):
            E.require_integers(f'{cs.what} Adam {what} x 8', 8 * a)
            assert 8 * E.amax(a) < E.F32_EXACT, f'{cs.what} Adam {what}'
        out.append((dz, beta1, b1p, m_w, m_b))
    return out


# ---- poison (the POISONED rows): an inf in dz, and a finite value whose scaled square is not finite ----
POISON_COLUMN = 3
HUGE = 2.0 ** 66          # exact in bf16; (0.5 * 2^66)^2 = 2^130 is not finite, 2^65 and the new m are


def poisoned_dz(cs):
    """The rest of the last column is zero, so that no sum with 2^66 in it has anything to round: x^T dz is +-2^66 or 0 there in
    any arithmetic and any order.  (With ternary neighbours the bf16 stream kernels gave 2^66 - 2^42 where float32 addition
    gives 2^66: the bf16 matrix core does not round a sum of sixteen products as sixteen float32 additions would.  Neither is
    wrong, and the poison rule is indifferent to it; exact_ops.py's assumption about that unit is for sums below 2^24.)"""
    m, k, n = cs.shape
    dz = cs.dz.copy()
    dz[0, POISON_COLUMN] = np.inf
    dz[:, n - 1] = 0
    dz[m - 1, n - 1] = HUGE
    return dz


def poison_masks(cs):
    """(kernel [k, n], bias [n]): where v and var must turn NaN — all of column 3 (inf x = +-inf, inf 0 = NaN), and of the last
    column the rows whose x[m - 1] is not zero (there g = +-2^65: finite, its square is not); the bias of both columns"""
    m, k, n = cs.shape
    assert m > 1 and n - 1 != POISON_COLUMN
    w = np.zeros((k, n), bool)
    w[:, POISON_COLUMN] = True
    w[:, n - 1] = cs.x[m - 1] != 0
    assert 0 < w[:, n - 1].sum() < k
    b = np.zeros(n, bool)
    b[[POISON_COLUMN, n - 1]] = True
    return w, b
