"""The published sweep's shards and the dispatch's picks over them, on the CPU.

tests/test_gpu_sweep_shapes.py runs every shard of tests/sweep_shapes.py on the device. What it
runs there is decided by host logic (the planner, gemv.hip pick_variant, mvg_exact_panel_width),
so the coverage it claims is asserted here by name: the six picks the sweep reaches, and with the
extras every pick the dispatch has. A dispatch change that adds a pick, or moves one away from
every test shape, fails here and not silently on the GPU box.
"""
import collections

import pytest

import sweep_shapes as S
from matvec_mpi_multiplier_amd import _lib

lib = _lib.lib


@pytest.fixture(scope="module")
def shapes():
    return S.distinct_shard_shapes()


def test_all_285_combinations_divide_into_208_shard_shapes(shapes):
    combos = S.combos()
    assert len(combos) == len(set(combos)) == 285
    grids = set()
    for R, C, alg, P in combos:
        sh = S.shards(R, C, alg, P)  # raises where a combination does not divide
        assert len(sh) == P
        assert sum(s.n_rows * s.n_cols for s in sh) == R * C
        assert all(s.n_rows > 0 and s.n_cols > 0 for s in sh)
        if alg == "blockwise":
            grids.add((sh[0].grid_rows, sh[0].grid_cols))
    assert grids == {(1, 1), (1, 2), (2, 3), (3, 4), (4, 6)}
    assert len(shapes) == 208
    assert max(m * k * 8 for m, k in shapes) == 10200 * 10200 * 8  # 0.83 GB


def test_sweep_reaches_exactly_six_tree_picks(shapes):
    count = collections.Counter(S.tree_pick(m, k) for m, k in shapes)
    assert set(count) == set(S.SWEEP_PICKS)
    assert count == {"vec_l64_r1_u4_nt1_o5": 27, "vec_l64_r4_u4_nt1_o0": 9, "rowblk_w2_r2_u4": 78,
                     "rowblk_w4_r2_u4_splitk": 84, "rowblk_w8_r2_u4": 4, "rowlines_w8_u4_x0": 6}
    # the odd-lda four-row form: the N x N/24 strips
    assert {s for s in shapes if S.tree_pick(*s) == "vec_l64_r4_u4_nt1_o0"} == {(n, n // 24) for n, _ in S.SQUARES}
    # the line-aligned row pairs: the four large squares and the P = 2 row shards of the last two,
    # all with lda % 16 == 8 (row-pair distance 2)
    lines = {s for s in shapes if S.tree_pick(*s) == "rowlines_w8_u4_x0"}
    assert lines == {(n, n) for n in (6600, 7800, 9000, 10200)} | {(4500, 9000), (5100, 10200)}
    assert all(k % 16 == 8 for _, k in lines)


def test_extras_have_the_picks_they_are_there_for():
    for m, k, pick in S.EXTRAS:
        assert S.tree_pick(m, k) == pick, (m, k)
    assert sorted(k % 16 for _, k, p in S.EXTRAS if p == "rowlines_w8_u4_x0") == [1, 2, 4]  # p = 16, 8, 4
    assert max(m * k * 8 for m, k, _ in S.EXTRAS) < 1.08e9


def test_sweep_and_extras_reach_every_pick_of_the_dispatch(shapes):
    """Every pick pick_variant has for 8-byte-aligned operands (all but the scl_* forms, which
    take operands off an 8-B boundary only) is the pick of some shape the GPU tests run. The
    dispatch's picks are found here by probing it over a grid that crosses every one of its
    thresholds, for lda in every class it tells apart; a pick that appears there and at no test
    shape is a gap."""
    ms = [1, 2, 1398, 1399, 1400, 1401, 4095, 4096, 4097, 8192, 16384, 87381, 87382, 131072, 1 << 20]
    ks = [1, 255, 256, 767, 768, 769, 1535, 1536, 1537, 1538, 4094, 4095, 4096, 4097, 6143, 6144, 6145, 6146,
          6148, 6152, 6160, 8190, 8191, 8192, 8193, 16383, 16384, 16386, 16400, 60000, 65536]
    probed = {S.tree_pick(m, k, lda) for m in ms for k in ks for lda in (k, k + 1, k + 2, k + 16)}
    tested = {S.tree_pick(m, k) for m, k in shapes} | {S.tree_pick(m, k) for m, k, _ in S.EXTRAS}
    assert not any(n.startswith("scl_") for n in probed)
    assert len(probed) == 10
    assert probed == tested == set(S.SWEEP_PICKS) | set(S.EXTRA_PICKS)


def test_exact_picks_and_panel_widths_over_the_sweep(shapes):
    """The bit-exact dispatch over the same shards, at the MI355X's 256 CUs: the names it
    reaches (recorded: the 8-lane hop form on tall shards, wider lane groups on few rows), and
    the column-panel copy on exactly the four large squares and their N x N/2 strips."""
    _lib.check(lib.mvg_debug_set_cu_count(256), "mvg_debug_set_cu_count")
    try:
        count = collections.Counter(S.exact_pick(m, k) for m, k in shapes)
        extras = {S.exact_pick(m, k) for m, k, _ in S.EXTRAS}
    finally:
        lib.mvg_debug_set_cu_count(0)
    assert count == {"hop8_l32_w8_u4": 108, "hop8_l8_w2_u16": 51, "hop8_l16_w4_u8": 49}
    assert extras == {"hop8_l8_w2_u16", "hop8_l32_w8_u4"}
    assert {s for s in shapes if lib.mvg_exact_panel_width(*s)} == S.PANEL_SHARDS
    assert all(lib.mvg_exact_panel_width(*s) == 256 for s in S.PANEL_SHARDS)
    assert len(S.PANEL_SHARDS) == 8
    assert not any(lib.mvg_exact_panel_width(m, k) for m, k, _ in S.EXTRAS)
