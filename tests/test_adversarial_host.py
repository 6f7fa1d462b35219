"""CPU-side conditions of the adversarial GPU tests (tests/test_gpu_adversarial.py and the
combine tests of tests/test_gpu_exact.py): the inputs built by tests/adversarial_cases.py have the
properties those tests rely on, checked against the oracle without a GPU."""
import numpy as np
import pytest

import adversarial_cases as AC
from oracle import oracle

MPICH_P = [2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17]
MPICH_N = [1, 3, 255, 256, 257, 1000, 70000]
GRIDS = [(1, 2), (2, 2), (2, 3), (2, 4), (3, 5)]


@pytest.mark.parametrize("m,k", AC.SHAPES)
def test_special_rows_have_an_order_independent_class_in_the_oracle(m, k):
    A, X = AC.payload(m, k, 1, sign=True)
    for j in AC.col_positions(k):
        for kind in AC.kinds_for(k):
            x = AC.special_x(X, j, kind)[0]
            base = oracle.multiply_std_rowwise(A, x)
            assert np.isfinite(base).all()
            for r in AC.row_positions(m):
                As = A.copy()
                for c, v in AC.special_row(A[r], j, kind):
                    As[r, c] = v
                for order in (np.arange(k), np.arange(k)[::-1]):  # the class does not depend on the order
                    y = oracle.multiply_std_rowwise(As[:, order], x[order])
                    want = AC.wanted_class(kind)
                    assert np.isnan(y[r]) if np.isnan(want) else y[r] == want, (kind, r, j, y[r])
                y = oracle.multiply_std_rowwise(As, x)
                others = np.arange(m) != r
                assert np.array_equal(y[others], base[others])


def test_row_and_column_positions_sit_on_the_edges():
    assert AC.row_positions(1) == [0] and AC.row_positions(3) == [0, 1, 2]
    assert AC.row_positions(257) == [0, 1, 149, 256] and AC.row_positions(33) == [0, 1, 21, 32]
    assert AC.row_positions(17) == [0, 1, 5, 16] and AC.row_positions(5) == [0, 1, 2, 4]
    assert [AC.boundary_col(k) for k in (1, 5, 130, 258, 127, 1000, 1030, 4226, 20001, 16388)] == \
        [0, 2, 128, 256, 112, 896, 1024, 4096, 19456, 16384]


@pytest.mark.parametrize("m,k", AC.SHAPES)
def test_exponent_scaling_is_exact_in_the_oracle(m, k):
    # the two properties the GPU test asserts of every kernel hold for the reference's own sum
    A, X = AC.payload(m, k, 1, sign=True)
    x = X[0]
    re, cf, e = AC.exponent_scales(m, k)
    assert e.min() >= -300 and e.max() <= 300
    y = oracle.multiply_std_rowwise(A, x)
    assert np.array_equal(oracle.multiply_std_rowwise(A * cf[None, :], x / cf), y)
    assert np.array_equal(oracle.multiply_std_rowwise(A * re[:, None], x), np.ldexp(y, e))
    both = oracle.multiply_std_rowwise(A * re[:, None] * cf[None, :], x / cf)
    assert np.array_equal(both, np.ldexp(y, e)) and np.isfinite(both).all()


@pytest.mark.parametrize("m,k", AC.SHAPES)
def test_underflow_reference_stays_2k_units_above_zero(m, k):
    for nv in (1, 25):
        made = AC.underflow_inputs(m, k, nv)
        assert made is not None, (m, k, nv)
        As, Xs, ref = made
        u = AC.units(ref)
        assert u.min() >= 2 * k and u.max() < 2.0 ** 52  # every sum a subnormal, adds exact
        assert np.array_equal(u, np.round(u))
        assert np.ldexp(1.0, -1022) > ref.max() > 0
        prod = AC.units(As[0] * Xs[0])  # the products are a few units each: rounding is visible
        assert prod.max() <= 64


def test_overflow_rows_go_inf_then_nan_in_the_oracle():
    for m, k in AC.SHAPES:
        if k < 4:
            continue
        for j in sorted({0, min(AC.boundary_col(k), k - 4), k - 4}):
            for ordinary in (False, True):
                A, x, rows = AC.overflow_cancel(m, k, j, ordinary)
                y = oracle.multiply_std_rowwise(A, x)
                for n, r in enumerate(rows):
                    assert np.isnan(y[r]) if n % 2 == 0 else y[r] == np.inf, (m, k, j, r, y[r])
                others = np.setdiff1d(np.arange(m), rows)
                assert np.isfinite(y[others]).all()


# ---------------------------------------------------------------- the exact combines' data
@pytest.mark.parametrize("P", MPICH_P)
def test_combine_data_separates_the_mpich_orders(P):
    """The device test of combine_mpich is vacuous unless the data tells the binomial order from
    the fold order. They are different parenthesisations at P = 5, 9, 17 (and every other P whose
    fold splits a binomial pair); at P = 3, 6, 7, 12 and the powers of two they are the same
    parenthesisation, which no data can separate (oracle/cpu_ref.c says the same), so there the
    two restatements must agree bit for bit."""
    pof2 = 1 << (P.bit_length() - 1)
    for n in MPICH_N:
        parts = AC.combine_parts(P, n)
        bino, fold = AC.binomial_sum(parts), AC.fold_sum(parts)
        want = fold if n * 8 > 2048 and n >= pof2 else bino
        assert np.array_equal(oracle.mpich_reduce(list(parts)), want), (P, n)
        if AC.orders_associate_alike(P):
            assert np.array_equal(bino, fold), (P, n)
        elif n >= 257:
            assert not np.array_equal(bino, fold), (P, n)
        if n >= 257:  # and from the plain left-to-right sum, whatever P > 3 ((p0 + p1) + p2 is both)
            seq = np.zeros(n)
            for p in parts:
                seq = seq + p
            assert P <= 3 or not np.array_equal(seq, want), (P, n)
    assert AC.orders_associate_alike(P) == (P in (2, 3, 4, 6, 7, 8, 12, 16))


@pytest.mark.parametrize("gr,gc", GRIDS)
def test_combine_data_separates_the_grid_row_orders(gr, gc):
    for lr in (1, 257, 1000):
        parts = AC.combine_parts(gr * gc, lr, seed=5)
        fwd = AC.grid_rows_sum(parts, gr, gc)
        assert np.isfinite(fwd).all() and fwd.shape == (gr * lr,)
        if gc > 2 and lr >= 257:  # two columns: a + b == b + a bit for bit
            assert not np.array_equal(fwd, AC.grid_rows_sum(parts, gr, gc, reverse=True))
