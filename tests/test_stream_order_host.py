"""The stream-order suite's host side (tests/stream_order.py): its case table reaches the
dispatch paths it names (the picks are host logic, no device needed), and its comparison
function reports the images a launch on the wrong stream leaves behind."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib

lib = _lib.lib
CASES = {c.id: c for c in SO.cases(lib)}


def test_the_bar_is_the_parity_suites():
    import test_gpu_parity

    assert SO.TOL == test_gpu_parity.TOL == 1e-12


@pytest.mark.parametrize("cid", [c.id for c in CASES.values() if c.reaches])
def test_case_reaches_the_pick_it_names(cid):
    kind, args, how, text = CASES[cid].reaches
    name = SO.pick_name(lib, kind, args)
    assert SO.reaches_ok(name, how, text), (cid, name, how, text)


def test_the_picks_the_table_is_there_for():
    name = lambda cid: SO.pick_name(lib, *CASES[cid].reaches[:2])  # noqa: E731
    assert name("gemv-64x16384") == "rowblk_w4_r2_u4_splitk" and name("gemv-64x16384").endswith("_splitk")
    assert name("gemv-4100x6150").startswith("rowlines_")
    assert name("multi-8203x1058-nv13").startswith("m16_")
    assert name("exact-6144x800-4cu").startswith("hop8e_")
    assert name("exact-6144x800-4cu-refused").startswith("hop8e_")  # what the refusal is of
    # mvg_gemv_exact_multi at 6150 x 64: the group of 4, then what the dispatch says for the 3 left
    em = lambda nv: SO.pick_name(lib, "exact_multi", (64, 64, 6150, 64, nv))  # noqa: E731
    assert em(7).startswith("hopm_") and em(7).endswith("_v4")
    assert em(3).startswith("hopm_") and em(3).endswith("_v2")
    assert em(1) == "auto"  # nv < 2: mvg_gemv_exact
    assert name("exact-multi-257x1000-nv3") == "separate"
    # the multi entries' groups: no 16-vector pass at 130 rows (8 + 3, 8 + 1), one at 8203 x 1058
    # for 9 .. 16 vectors, which is also what is left of 25 after the first 16
    mv = lambda m, k, nv: SO.pick_name(lib, "multi", (k, k, m, k, nv))  # noqa: E731
    assert not mv(130, 4226, 11).startswith("m16_") and not mv(130, 4226, 3).startswith("m16_")
    assert mv(8203, 1058, 9).startswith("m16_") and not mv(8203, 1058, 8).startswith("m16_")
    assert lib.mvg_gemv_multi_auto_variant(1058, 1058, 8203, 1058, 1) == 0  # the tail: single-vector dispatch


def test_every_explicit_split_form_and_8_byte_kernel_is_in_the_table():
    splits = SO.split_variants(lib)
    assert len(splits) >= 2 and all(n.endswith("_splitk") for _, n in splits)
    for _, n in splits:
        assert f"gemv-130x16388-{n}" in CASES
    scalars = SO.scalar_variants(lib)
    assert scalars
    for _, n in scalars:
        assert f"gemv-70x301-off8-{n}" in CASES


def test_the_table_covers_every_entry_point_of_the_issue():
    entries = " ".join(c.entry for c in CASES.values())
    for e in ("mvg_gemv", "mvg_gemv_variant", "mvg_gemv_multi", "mvg_gemv_exact", "mvg_gemv_exact_multi",
              "mvg_panel_relayout", "mvg_gemv_exact_panels", "mvg_debug_combine_mpich", "mvg_debug_combine_grid_rows",
              "mvg_synth_fill_device", "mvg_memcpy_h2d", "mvg_memcpy_d2h"):
        assert e in entries, e


@pytest.mark.parametrize("cid", ["gemv-70x301-lda301-off8", "gemv-16x0", "multi-70x301-lda301-nv5",
                                 "exact-multi-257x1000-nv3", "combine-mpich-P5-n300", "combine-grid-2x3-lr300",
                                 "pinned-copies-gemv-257x1000"])
def test_specs_are_consistent(cid):
    """The cheap specs, built on the CPU: sizes agree, the oracle's y is finite (so that a NaN in
    a result can only come from a NaN operand), and differs from every marker value."""
    spec = CASES[cid].make()
    assert spec.want.shape == (spec.ny,) and np.isfinite(spec.want).all()
    assert not np.any(spec.want == SO.SENTINEL) and not np.any(spec.want == SO.EARLY)
    assert all(v.ndim == 1 and v.dtype == np.float64 and np.isfinite(v).all() for v in spec.ops.values())
    assert spec.bar in ("exact", "tol")
    if cid == "gemv-16x0":
        assert np.array_equal(spec.want, np.zeros(16)) and not spec.ops


# ---------------------------------------------------------------- the comparison function
WANT = np.array([1.5, 2.25, 1000.125, 3.0e-5, 0.0, 12.0])


@pytest.mark.parametrize("bar", ["exact", "tol"])
def test_verdict_accepts_the_result_in_stream_order(bar):
    assert SO.verdict(WANT.copy(), WANT, WANT.copy(), bar) == []
    assert SO.verdict(WANT.copy(), WANT, None, bar) == []


@pytest.mark.parametrize("bar", ["exact", "tol"])
def test_verdict_reports_a_result_left_at_the_sentinel(bar):
    whole = np.full(WANT.size, SO.SENTINEL)
    assert any("sentinel" in b for b in SO.verdict(whole, WANT, WANT, bar))
    one = WANT.copy()
    one[3] = SO.SENTINEL  # one row of many
    bad = SO.verdict(one, WANT, WANT, bar)
    assert any("1 of 6 still at the sentinel" in b for b in bad) and len(bad) >= 2


@pytest.mark.parametrize("bar", ["exact", "tol"])
def test_verdict_reports_a_result_computed_from_nan_operands(bar):
    whole = np.full(WANT.size, np.nan)
    assert any("NaN" in b for b in SO.verdict(whole, WANT, WANT, bar))
    one = WANT.copy()
    one[0] = np.nan
    bad = SO.verdict(one, WANT, None, bar)
    assert any("1 of 6 NaN" in b for b in bad)
    assert any("oracle" in b for b in bad)  # and the bar itself fails on it: NaN passes no comparison


@pytest.mark.parametrize("bar", ["exact", "tol"])
def test_verdict_reports_a_result_the_producer_overwrote(bar):
    y = WANT.copy()
    y[1:3] = SO.EARLY
    assert any("2 of 6 hold the producer's overwrite" in b for b in SO.verdict(y, WANT, WANT, bar))


def test_verdict_bars():
    ulp = WANT.copy()
    ulp[2] = np.nextafter(ulp[2], np.inf)
    assert SO.verdict(ulp, WANT, ulp, "tol") == []  # one ulp: inside 1e-12 relative
    assert any("oracle" in b for b in SO.verdict(ulp, WANT, ulp, "exact"))  # not bit for bit
    assert any("null-stream" in b for b in SO.verdict(ulp, WANT, WANT, "tol"))  # nor the null-stream run's bits
    off = WANT.copy()
    off[2] *= 1 + 3e-12
    assert any("relative" in b for b in SO.verdict(off, WANT, off, "tol"))
    neg0 = WANT.copy()
    neg0[4] = -0.0
    assert SO.verdict(neg0, WANT, neg0, "exact") != []  # bits, not values: -0.0 is not the reference's 0.0
    assert SO.verdict(WANT[:5], WANT, None, "tol") != []  # a short image
    with pytest.raises(AssertionError):
        SO.verdict(WANT, WANT, None, "loose")
