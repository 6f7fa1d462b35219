"""The transposed product's exchange on a host without GPUs: mvg_plan_exchange_t, the mirror image
of mvg_plan_exchange on the same shards.

Every schedule is executed in NumPy: each rank's partial is the oracle's sequential sum on the
transposed shard and its segment of z, members, colours and keys are grouped as the plan says, a
reduce is the sum in communicator-rank order, a gather the pieces in key order. Rank 0's w must be
the oracle's on the whole A^T: within 1e-12 everywhere, and the same bits wherever the schedule
only gathers (the column split, and the block split on one grid row).
"""
import numpy as np
import pytest

from conftest import max_rel
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

ALGS = ("rowwise", "colwise", "blockwise")
R, C = 1560, 792
A = oracle.synth(R, C, 42)
Z = oracle.synth(1, R, 4343)[0]
WANT = oracle.multiply_std_rowwise(np.ascontiguousarray(A.T), Z)


def _inputs(r, c):
    if (r, c) == (R, C):
        return A, Z, WANT
    a, z = oracle.synth(r, c, 42), oracle.synth(1, r, 4343)[0]
    return a, z, oracle.multiply_std_rowwise(np.ascontiguousarray(a.T), z)


def _parts(alg, a, z, P):
    r, c = a.shape
    out = []
    for rank in range(P):
        s = mm.plan_shard(alg, r, c, P, rank)
        blk = a[s.row_off:s.row_off + s.n_rows, s.col_off:s.col_off + s.n_cols]
        out.append(oracle.multiply_std_rowwise(np.ascontiguousarray(blk.T), z[s.row_off:s.row_off + s.n_rows]))
    return out


def _run_plan(alg, r, c, P, parts, force=False):
    """Rank 0's w after every rank ran its steps of mvg_plan_exchange_t."""
    plans = [mm.plan_exchange_t(alg, r, c, P, rank, force_collect=force) for rank in range(P)]
    assert len({len(p) for p in plans}) == 1
    bufs = [{_lib.X_BUF_PART: parts[rank].copy(), _lib.X_BUF_ROW: np.full(c, np.nan), _lib.X_BUF_Y: np.full(c, np.nan)}
            for rank in range(P)]
    for k in range(len(plans[0])):
        assert len({(p[k].op, p[k].comm, p[k].count, p[k].root, p[k].src, p[k].dst) for p in plans}) == 1
        comms = {}
        for rank, p in enumerate(plans):
            if p[k].member:
                comms.setdefault(p[k].color, []).append((p[k].key, rank))
        st = plans[0][k]
        if st.comm == _lib.X_WORLD:
            assert list(comms) == [0] and [key for key, _ in sorted(comms[0])] == list(range(P))
        for members in comms.values():
            order = [rank for _, rank in sorted(members)]
            root, n = order[st.root], st.count
            srcs = [bufs[m][st.src][:n] for m in order]
            if st.op == _lib.X_GATHER:
                bufs[root][st.dst][:n * len(order)] = np.concatenate(srcs)
            else:
                acc = srcs[0].copy()
                for s in srcs[1:]:
                    acc = acc + s
                bufs[root][st.dst][:n] = acc
    return bufs[0][_lib.X_BUF_Y] if plans[0] else bufs[0][_lib.X_BUF_PART]


def _gathers_only(alg, P):
    return alg == "colwise" or (alg == "blockwise" and mm.get_2_most_closest_multipliers(P)[0] == 1)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 6, 8, 12])
@pytest.mark.parametrize("alg", ALGS)
def test_plan_executed_gives_the_oracle_w(alg, P):
    w = _run_plan(alg, R, C, P, _parts(alg, A, Z, P))
    assert w.shape == (C,) and max_rel(w, WANT) <= 1e-12, max_rel(w, WANT)
    if _gathers_only(alg, P):
        np.testing.assert_array_equal(w, WANT)  # a gather adds nothing


@pytest.mark.parametrize("alg", ALGS)
def test_forced_collectives_at_one_rank(alg):
    a, z, want = _inputs(24, 24)
    assert mm.plan_exchange_t(alg, 24, 24, 1, 0) == []
    (st,) = mm.plan_exchange_t(alg, 24, 24, 1, 0, force_collect=True)
    assert (st.comm, st.count, st.src, st.dst, st.member) == (_lib.X_WORLD, 24, _lib.X_BUF_PART, _lib.X_BUF_Y, 1)
    assert st.op == (_lib.X_REDUCE if alg == "rowwise" else _lib.X_GATHER)
    np.testing.assert_array_equal(_run_plan(alg, 24, 24, 1, _parts(alg, a, z, 1), force=True), want)


def _d(st):
    return st.as_dict()


def test_row_split_steps_literally():
    for rank in range(4):
        (st,) = mm.plan_exchange_t("rowwise", R, C, 4, rank)
        assert _d(st) == dict(op=_lib.X_REDUCE, comm=_lib.X_WORLD, color=0, key=rank, member=1, root=0,
                              src=_lib.X_BUF_PART, dst=_lib.X_BUF_Y, count=C)


def test_column_split_steps_literally():
    for rank in range(4):
        (st,) = mm.plan_exchange_t("colwise", R, C, 4, rank)
        assert _d(st) == dict(op=_lib.X_GATHER, comm=_lib.X_WORLD, color=0, key=rank, member=1, root=0,
                              src=_lib.X_BUF_PART, dst=_lib.X_BUF_Y, count=C // 4)


def test_block_split_steps_literally():
    # 6 ranks: a 2 x 3 grid, rank = grid_r * 3 + grid_c
    for rank in range(6):
        gr, gc = divmod(rank, 3)
        red, gat = mm.plan_exchange_t("blockwise", R, C, 6, rank)
        assert _d(red) == dict(op=_lib.X_REDUCE, comm=_lib.X_COL, color=gc, key=gr, member=1, root=0,
                               src=_lib.X_BUF_PART, dst=_lib.X_BUF_ROW, count=C // 3)
        assert _d(gat) == dict(op=_lib.X_GATHER, comm=_lib.X_ROW, color=0, key=gc, member=int(gr == 0), root=0,
                               src=_lib.X_BUF_ROW, dst=_lib.X_BUF_Y, count=C // 3)
    # one grid row (3 ranks: 1 x 3): a single world gather
    for rank in range(3):
        (st,) = mm.plan_exchange_t("blockwise", R, C, 3, rank)
        assert _d(st) == dict(op=_lib.X_GATHER, comm=_lib.X_WORLD, color=0, key=rank, member=1, root=0,
                              src=_lib.X_BUF_PART, dst=_lib.X_BUF_Y, count=C // 3)


def test_the_shards_and_their_refusals_are_plan_shards():
    for alg, r, c, P in [("rowwise", 10, 8, 4), ("colwise", 8, 10, 4), ("blockwise", 9, 8, 4), ("blockwise", 8, 9, 4)]:
        with pytest.raises(mm.IndivisibleError):
            mm.plan_exchange_t(alg, r, c, P, 0)
        with pytest.raises(mm.IndivisibleError):
            mm.plan_shard(alg, r, c, P, 0)
