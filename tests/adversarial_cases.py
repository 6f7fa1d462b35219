"""Inputs of the adversarial kernel tests (tests/test_gpu_adversarial.py), built on the host.

Plain numpy: tests/test_adversarial_host.py checks on the CPU that these inputs have the
properties the GPU tests rely on (the oracle's class for every special row, subnormal results far
enough from zero, summation orders that the data tells apart).
"""
import numpy as np

from oracle import oracle

# m straddles the 2-, 4-, 16-, 32- and 64-row ownership blocks and the row-pair form's 32-row
# block; k one chunk, a chunk plus a pair, a chunk plus an odd column, k shorter than a tile
SHAPES = [(1, 1), (3, 5), (5, 7), (17, 130), (33, 258), (65, 127), (64, 128), (47, 1000), (257, 1030),
          (130, 4226), (33, 6002), (7, 20001), (9, 16388)]
PADS = (1, 2, 13, 16)  # an odd lda: p = 16 in gemv_rowblock_lines; lda % 16 == 8: p = 2
NVS = (1, 2, 3, 5, 8, 9, 13, 16, 25)
KINDS = ("inf", "nan", "inf_minus_inf", "inf_times_zero")
UNIT = -1074  # the smallest subnormal is 2^UNIT


def signed(A, seed):
    rng = np.random.default_rng(seed)
    return A * rng.choice([-1.0, 1.0], size=A.shape)


def payload(m, k, nv=1, sign=False):
    """The ordinary synthetic A (m x k) and X (nv x k, vector v contiguous)."""
    A, X = oracle.synth(m, k, 42), oracle.synth(nv, k, 4242)
    if sign:
        A, X = signed(A, m * 7 + k), signed(X, k)
    return A, X


def boundary_col(k):
    """A column on a chunk / tile boundary of the kernels: the first column of the last chunk of
    1024 (else 128, else 16) columns that k - 1 lies in, the middle for k < 16."""
    for c in (1024, 128, 16):
        if k - 1 >= c:
            return (k - 1) // c * c
    return k // 2


def col_positions(k):
    return sorted({0, boundary_col(k), k - 1})


def row_positions(m):
    """Rows 0 and 1, a row in the middle of every ownership block (row % 64 == 21: % 32 == 21,
    % 16 == 5, % 4 == 1; 5 or 2 where m is too small), and row m - 1, which clamped lanes re-read."""
    rows = {0, min(1, m - 1), m - 1}
    for mid in (m // 2 // 64 * 64 + 21, 21, 5, 2):
        if 1 < mid < m - 1:
            rows.add(mid)
            break
    return sorted(rows)


def second_col(k, j):
    """Where the second infinity of an inf_minus_inf row goes (k >= 2)."""
    return (j + max(1, k // 2)) % k


def special_x(X, j, kind):
    """X for a special row with its element in column j: positive where an infinity must keep
    its sign, zero for inf_times_zero. The same X serves the all-finite run the special run is
    compared with."""
    X = X.copy()
    k = X.shape[1]
    if kind == "inf_times_zero":
        X[:, j] = 0.0
    else:
        X[:, j] = 0.5
        if k >= 2:
            X[:, second_col(k, j)] = 0.25
    return X


def special_row(row, j, kind):
    """(column, value) pairs that turn the finite `row` of A into a special one. Every class is
    independent of the order of summation: no finite sum or product overflows, and a second
    infinity appears only where NaN is wanted."""
    k = row.shape[0]
    if kind == "inf":
        return [(j, np.inf)]
    if kind == "nan":
        return [(j, np.nan)]
    if kind == "inf_minus_inf":
        assert k >= 2
        return [(j, np.inf), (second_col(k, j), -np.inf)]
    assert kind == "inf_times_zero"
    return [(j, np.inf)]


def kinds_for(k):
    return [kd for kd in KINDS if k >= 2 or kd != "inf_minus_inf"]


def wanted_class(kind):
    return np.inf if kind == "inf" else np.nan


# ------------------------------------------------------------------ exponent range
def exponent_scales(m, k, seed=20250):
    """Per-row scales 2^e_i and per-column scales 2^f_j, e and f uniform integers in [-300, 300]."""
    rng = np.random.default_rng(seed + 131 * m + k)
    e = rng.integers(-300, 301, size=m)
    f = rng.integers(-300, 301, size=k)
    return np.ldexp(1.0, e), np.ldexp(1.0, f), e


# ------------------------------------------------------------------ gradual underflow
def underflow_inputs(m, k, nv=1):
    """A * 2^-600 and X * 2^s: every product is a handful of units of 2^-1074, every sum a
    subnormal. s is -470 (products of about 4 units on average), raised for the shapes where that
    leaves a reference y_i under 2k units (short rows with a small a*x); None where no s <= -440
    reaches it (a zero in the data)."""
    A, X = payload(m, k, nv)
    As = np.ldexp(A, -600)
    for s in range(-470, -439):
        Xs = np.ldexp(X, s)
        ref = np.stack([oracle.multiply_std_rowwise(As, Xs[v]) for v in range(nv)])
        if np.all(units(ref) >= 2 * k):
            return As, Xs, ref
    return None


def units(y):
    """y in units of the smallest subnormal, 2^-1074 (exact for subnormal y)."""
    return np.ldexp(y, -UNIT)


# ------------------------------------------------------------------ overflow and cancel
def overflow_cancel(m, k, j, ordinary, sign_seed=7):
    """Rows whose sequential chain overflows and then cancels: at columns j .. j+3 x is
    [10, 10, -10, -10]; a row of 1e308 there has products +inf, +inf, -inf: the chain goes +inf
    then NaN; a row of 1e307 has finite products whose running sum overflows to +inf and stays
    there. The rest of those rows is zero or (ordinary) the synthetic values; the other rows are
    ordinary. k >= 4. Returns A, x and the rows' indices."""
    assert k >= 4 and 0 <= j <= k - 4
    A, X = payload(m, k, 1, sign=True)
    x = X[0]
    x[j:j + 4] = [10.0, 10.0, -10.0, -10.0]
    rows = row_positions(m)
    for n, r in enumerate(rows):
        if not ordinary:
            A[r] = 0.0
        A[r, j:j + 4] = 1e308 if n % 2 == 0 else 1e307
    return A, x, rows


# ------------------------------------------------------------------ the exact combines
def combine_parts(P, n, seed=99):
    """P partial vectors of n doubles, mixed signs, exponents spread over +-40 binades: sums
    whose bits depend on the association."""
    rng = np.random.default_rng(seed + 1000 * P + n)
    mant = rng.uniform(1.0, 2.0, size=(P, n)) * rng.choice([-1.0, 1.0], size=(P, n))
    return np.ldexp(mant, rng.integers(-40, 41, size=(P, n)))


def binomial_sum(parts):
    """The binomial tree over the vectors in order: ((p0 + p1) + (p2 + p3)) + ..."""
    bufs = [np.array(p, dtype=np.float64) for p in parts]
    mask = 1
    while mask < len(bufs):
        for r in range(0, len(bufs) - mask, 2 * mask):
            bufs[r] = bufs[r] + bufs[r + mask]
        mask *= 2
    return bufs[0]


def fold_sum(parts):
    """MPICH's reduce-scatter + gather order: ranks 2i, 2i + 1 (i < P - pof2) fold into one, then
    the binomial tree over the pof2 ranks left."""
    P = len(parts)
    pof2 = 1
    while pof2 * 2 <= P:
        pof2 *= 2
    rem = P - pof2
    folded = [parts[2 * i] + parts[2 * i + 1] for i in range(rem)] + [parts[r] for r in range(2 * rem, P)]
    return binomial_sum(folded)


def orders_associate_alike(P):
    """Whether the two orders are the same parenthesisation (then no data can tell them apart):
    compared as nested tuples of rank numbers."""
    def tree(items):
        items = list(items)
        mask = 1
        while mask < len(items):
            for r in range(0, len(items) - mask, 2 * mask):
                items[r] = (items[r], items[r + mask])
            mask *= 2
        return items[0]

    pof2 = 1
    while pof2 * 2 <= P:
        pof2 *= 2
    rem = P - pof2
    folded = [(2 * i, 2 * i + 1) for i in range(rem)] + list(range(2 * rem, P))
    return tree(range(P)) == tree(folded)


def grid_rows_sum(parts, gr, gc, reverse=False):
    """y[g*lr + j] = ((0 + p[g*gc]) + p[g*gc + 1]) + ... (reverse: from the last column back)."""
    lr = parts.shape[1]
    y = np.zeros(gr * lr)
    cols = range(gc - 1, -1, -1) if reverse else range(gc)
    for g in range(gr):
        for c in cols:
            y[g * lr:(g + 1) * lr] = y[g * lr:(g + 1) * lr] + parts[g * gc + c]
    return y
