"""The guarded-operand checker (tests/gpu_guarded.py) on images corrupted on the host: a mistake
in the harness shows here, on the CPU, not by breaking a kernel on the GPU."""
import numpy as np
import pytest

import gpu_guarded as G

M, NV, LDY = 37, 3, 40  # ldy = m + 3, one spare vector past nv


@pytest.fixture
def lay():
    return G.Layout(NV, M, LDY, nvec=NV + 1)


def clean_image(lay, want):
    return lay.image(want)


def want_of(lay):
    return np.arange(lay.nv * lay.n, dtype=np.float64).reshape(lay.nv, lay.n) + 0.5


def test_layout_places_payload_guards_and_padding(lay):
    assert lay.off == G.GUARD and lay.size == G.GUARD + (NV + 1) * LDY + G.GUARD
    img = lay.image(want_of(lay))
    assert np.isnan(img[:G.GUARD]).all() and np.isnan(img[-G.GUARD:]).all()
    body = img[lay.off:lay.off + (NV + 1) * LDY].reshape(NV + 1, LDY)
    assert np.array_equal(body[:NV, :M], want_of(lay))
    assert np.isnan(body[:NV, M:]).all() and np.isnan(body[NV]).all()
    assert np.array_equal(lay.payload(img), want_of(lay))
    assert lay.payload_mask().sum() == NV * M
    shifted = G.Layout(1, 5, 7, shift=1)
    assert shifted.off == G.GUARD + 1 and shifted.size == G.GUARD + 1 + 7 + G.GUARD
    assert np.isnan(shifted.image(np.ones(5))[:shifted.off]).all()


def test_checker_accepts_a_clean_image(lay):
    want = want_of(lay)
    assert G.check_image(clean_image(lay, want), lay, G.exact_ok(want)) == []
    G.assert_clean(clean_image(lay, want), lay, G.exact_ok(want))


def test_checker_flags_a_store_at_row_m(lay):
    want = want_of(lay)
    img = clean_image(lay, want)
    img[lay.off + 1 * LDY + M] = 4.0  # vector 1, row m
    bad = G.check_image(img, lay, G.exact_ok(want), "k")
    assert len(bad) == 1 and f"vector 1 row {M} " in bad[0] and "padding" in bad[0] and "4.0" in bad[0]
    with pytest.raises(AssertionError):
        G.assert_clean(img, lay, G.exact_ok(want))


def test_checker_flags_a_store_before_row_0(lay):
    want = want_of(lay)
    img = clean_image(lay, want)
    img[lay.off - 1] = 0.0
    bad = G.check_image(img, lay, G.exact_ok(want))
    assert len(bad) == 1 and "1 doubles before vector 0 row 0" in bad[0]
    # before row 0 of a later vector: the padding of the vector in front of it
    img = clean_image(lay, want)
    img[lay.off + 2 * LDY - 1] = -1.0
    bad = G.check_image(img, lay, G.exact_ok(want))
    assert len(bad) == 1 and f"vector 1 row {LDY - 1} " in bad[0]


def test_checker_flags_a_store_in_vector_nv_and_in_the_back_guard(lay):
    want = want_of(lay)
    img = clean_image(lay, want)
    img[lay.off + NV * LDY + 5] = 1.5
    bad = G.check_image(img, lay, G.exact_ok(want))
    assert len(bad) == 1 and f"vector {NV} row 5 " in bad[0] and "past nv" in bad[0]
    img = clean_image(lay, want)
    img[lay.off + (NV + 1) * LDY + 2] = np.inf  # an infinity is a store too
    bad = G.check_image(img, lay, G.exact_ok(want))
    assert len(bad) == 1 and "2 doubles past the last vector" in bad[0]


def test_checker_flags_a_payload_row_turned_nan(lay):
    # what a kernel that summed a padding column of A or x would leave
    want = want_of(lay)
    img = clean_image(lay, want)
    img[lay.off + 2 * LDY + 11] = np.nan
    for compare in (G.exact_ok(want), lambda got: np.abs(got - want) <= 1e-12 * np.abs(want)):
        bad = G.check_image(img, lay, compare)
        assert len(bad) == 1 and "vector 2 row 11" in bad[0] and "nan" in bad[0]
    # a row never written at all is the same failure
    img = clean_image(lay, want)
    img[lay.off + 36] = np.nan
    assert "vector 0 row 36" in G.check_image(img, lay, G.exact_ok(want))[0]


def test_checker_flags_a_wrong_value_and_counts_every_failure(lay):
    want = want_of(lay)
    img = clean_image(lay, want)
    img[lay.off + 3] = np.nextafter(want[0, 3], np.inf)
    img[lay.off - 3] = 1.0
    img[lay.off + M] = 2.0
    bad = G.check_image(img, lay, G.exact_ok(want))
    assert len(bad) == 3 and any("vector 0 row 3:" in b for b in bad)


def test_comparators():
    a = np.array([1.0, np.nan, np.inf, 0.0])
    assert G.same_or_both_nan(a, a.copy())
    neg_nan = np.array([np.nan]).view(np.uint64) | np.uint64(1 << 63)
    b = a.copy()
    b[1] = neg_nan.view(np.float64)[0]  # the negative quiet NaN of x86 against the GPU's positive one
    assert G.same_or_both_nan(a, b) and G.exact_ok(a)(b).all()
    assert not G.same_or_both_nan(a, np.array([1.0, np.nan, np.inf, -0.0]))  # the sign of a zero counts
    assert not G.exact_ok(a)(np.array([1.0, np.nan, np.inf, -0.0]))[3]
    assert not G.same_or_both_nan(a, np.array([1.0, 2.0, np.inf, 0.0]))
    assert not G.same_or_both_nan(a, np.array([1.0, np.nan, -np.inf, 0.0]))
    want = np.array([np.inf, np.nan, -np.inf])
    assert G.same_class(want)(np.array([np.inf, b[1], -np.inf])).all()
    assert not G.same_class(want)(np.array([np.nan, np.inf, np.inf])).any()
    assert not G.same_class(want)(np.array([1e308, 0.0, -1e308])).any()
