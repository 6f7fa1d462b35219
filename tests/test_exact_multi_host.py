"""Host side of the bit-exact multi-vector path (no GPU): the variant table of
mvg_gemv_exact_multi, its automatic choice and argument checks, and the block-of-vectors exchange
(csrc/engine.cpp exchange_plan_multi / exchange_exact_multi) as one process driving G devices
issues it, recorded by mvg_debug_trace_exchange_multi and executed here with numpy on the
oracle's per-rank partials.

The executor adds in the reference's orders wherever a call leaves the order open (MPICH's
MPI_Reduce for the column split, colwise.c:124; rank order into a zeroed y for a grid row,
blockwise.c:150-207), per vector, so rank 0's Y must be oracle.multiply's bits in every column, in
tree mode and in exact mode alike.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle
from test_single_process_exchange import SHAPES, _comms, _parts

lib = _lib.lib
ALGS = ("rowwise", "colwise", "blockwise")


# ------------------------------------------------------------------ the variant table
def table():
    return [lib.mvg_gemv_exact_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_exact_multi_variant_count())]


def test_variant_table_keeps_its_names_and_order():
    with open(os.path.join(GOLDEN_DIR, "exact_multi_variant_names.json")) as f:
        golden = json.load(f)
    assert list(golden) == ["mvg_gemv_exact_multi_variant_name"]
    assert table() == golden["mvg_gemv_exact_multi_variant_name"]
    assert lib.mvg_gemv_exact_multi_variant_name(len(table())) == b"invalid"
    assert lib.mvg_gemv_exact_multi_variant_name(-1) == b"invalid"


def test_variant_table_covers_the_three_lane_widths_for_two_and_four_vectors():
    import re

    forms = {(int(m[1]), int(m[4])) for m in (re.fullmatch(r"hopm_l(\d+)_w(\d+)_u(\d+)_v(\d+)", n) for n in table()) if m}
    assert forms >= {(L, nv) for L in (8, 16, 32) for nv in (2, 4)}


@pytest.mark.parametrize("m,k", [(16384, 16384), (65536, 8192), (524288, 512), (4096, 16384), (1024, 32768), (7, 3)])
def test_auto_variant_is_single_below_two_vectors_and_a_table_entry_above(m, k):
    names = table()
    for nv in (-1, 0, 1):
        assert lib.mvg_gemv_exact_multi_auto_variant(k, k, m, k, nv) == 0
    for nv in (2, 3, 4, 8, 16):
        for lda in (k, k + 13):
            v = lib.mvg_gemv_exact_multi_auto_variant(lda, k, m, k, nv)
            assert 0 < v < len(names) and names[v] != "invalid", (m, k, nv, v)


def test_argument_errors_need_no_device():
    p = 4096  # never dereferenced: every call below is refused by its argument checks
    call = lambda lda, ldx, ldy, m, k, nv, var=0, A=p, X=p, Y=p: lib.mvg_gemv_exact_multi_variant(  # noqa: E731
        A, lda, X, ldx, Y, ldy, m, k, nv, var, None)
    bad = _lib.MVG_E_INVALID
    assert call(8, 8, 8, -1, 8, 2) == bad and call(8, 8, 8, 8, -1, 2) == bad and call(8, 8, 8, 8, 8, -1) == bad
    assert call(7, 8, 8, 8, 8, 2) == bad  # lda < k
    assert call(8, 7, 8, 8, 8, 2) == bad  # ldx < k
    assert call(8, 8, 7, 8, 8, 2) == bad  # ldy < m
    assert call(8, 8, 8, 8, 8, 2, var=-1) == bad
    assert call(8, 8, 8, 8, 8, 2, var=lib.mvg_gemv_exact_multi_variant_count()) == bad
    assert call(8, 8, 8, 8, 8, 2, A=None) == bad and call(8, 8, 8, 8, 8, 2, X=None) == bad
    assert call(8, 8, 8, 8, 8, 2, Y=None) == bad
    assert b"mvg_gemv_exact_multi" in lib.mvg_last_error()
    assert lib.mvg_gemv_exact_multi(p, 7, p, 8, p, 8, 8, 8, 2, None) == bad
    # nothing to do: no pointer is looked at
    assert call(0, 0, 0, 0, 8, 2, A=None, X=None, Y=None) == _lib.MVG_OK
    assert call(8, 8, 8, 8, 8, 0, A=None, X=None, Y=None) == _lib.MVG_OK


# ------------------------------------------------------------------ the block's exchange
def trace_multi(alg, R, Cn, ndev, exact, nv):
    cap = (16 * ndev + 16) * (nv + 1)
    calls = (_lib.XCall * cap)()
    n = C.c_int()
    _lib.check(lib.mvg_debug_trace_exchange_multi(_lib.ALG_BY_NAME[alg], R, Cn, ndev, int(exact), nv, calls, cap,
                                                  C.byref(n)), "mvg_debug_trace_exchange_multi")
    return [calls[i].as_dict() for i in range(n.value)]


def reference_sum(alg, parts):
    """The members' vectors added as the reference adds them."""
    if alg == "colwise":
        return oracle.mpich_reduce(list(parts))
    y = np.zeros_like(parts[0])
    for p in parts:
        y = y + p
    return y


def execute_multi(calls, alg, R, Cn, G, parts, nv):
    """Rank 0's Y (nv x R, vector v in row v) after the recorded calls ran on parts[r] (nv x
    y_len). Buffers are column-major, one vector per column, as the header documents: vector v of
    a partial or grid-row buffer at v * y_len, of Y at v * R, of the gather buffer at v * G * y_len;
    gather call v of a member moves vector v."""
    comms = _comms(calls)
    color_of = {(c["group"], c["rank"]): c["color"] for c in calls if c["kind"] == _lib.XCALL_SPLIT}
    bufs = {}
    for r in range(G):
        n = mm.plan_shard(alg, R, Cn, G, r).y_len
        bufs[r] = {_lib.X_BUF_PART: np.array(parts[r], dtype=np.float64).reshape(nv * n),
                   _lib.X_BUF_ROW: np.zeros(nv * n), _lib.X_BUF_Y: np.zeros(nv * R),
                   _lib.X_BUF_GATHERED: np.zeros(nv * G * n)}
    xs = [c for c in calls if c["kind"] in (_lib.XCALL_GATHER, _lib.XCALL_REDUCE)]
    for g in sorted({c["group"] for c in xs}):
        step = [c for c in calls if c["group"] == g]
        assert g >= 0 and {c["kind"] for c in step} in ({_lib.XCALL_GATHER}, {_lib.XCALL_REDUCE}), step
        by_comm = {}
        for c in step:
            members = list(range(G)) if c["comm"] == -1 else comms[c["comm"]][color_of[(c["comm"], c["rank"])]]
            by_comm.setdefault(tuple(members), []).append(c)
        for members, cs in by_comm.items():
            assert len({c["root"] for c in cs}) == 1 and len({c["count"] for c in cs}) == 1, cs
            root = members[cs[0]["root"]]
            per = {m: [c for c in cs if c["rank"] == m] for m in members}
            assert sorted({c["rank"] for c in cs}) == sorted(members), (members, cs)
            dst = per[root][0]["dst"]
            if cs[0]["kind"] == _lib.XCALL_REDUCE:
                # one reduce of count * nv per member
                assert all(len(v) == 1 for v in per.values()), cs
                n, rem = divmod(cs[0]["count"], nv)
                assert rem == 0 and n == mm.plan_shard(alg, R, Cn, G, root).y_len, cs
                for v in range(nv):
                    bufs[root][dst][v * n:(v + 1) * n] = reference_sum(
                        alg, [bufs[m][per[m][0]["src"]][v * n:(v + 1) * n] for m in members])
            else:
                # nv gathers of count per member, vector v in each member's v-th call
                assert all(len(v) == nv for v in per.values()), cs
                n = cs[0]["count"]
                stride = len(members) * n  # Y: a whole y; the gather buffer: every rank's partial
                assert stride == (R if dst == _lib.X_BUF_Y else G * n), (dst, stride)
                for v in range(nv):
                    assert all(per[m][v]["dst"] == dst for m in members if m == root)
                    bufs[root][dst][v * stride:(v + 1) * stride] = np.concatenate(
                        [bufs[m][per[m][v]["src"]][v * n:(v + 1) * n] for m in members])
    combines = [c for c in calls if c["kind"] == _lib.XCALL_COMBINE]
    for v, c in enumerate(combines):
        assert c["rank"] == 0 and c["group"] == -1 and c["src"] == _lib.X_BUF_GATHERED and c["dst"] == _lib.X_BUF_Y
        n = c["count"] // G
        gathered = bufs[0][c["src"]][v * G * n:(v + 1) * G * n].reshape(G, n)
        if alg == "colwise":
            y = reference_sum(alg, list(gathered))
        else:
            gr, gc = mm.get_2_most_closest_multipliers(G)
            y = np.concatenate([reference_sum(alg, list(gathered[i * gc:(i + 1) * gc])) for i in range(gr)])
        bufs[0][c["dst"]][v * R:(v + 1) * R] = y
    return bufs[0][_lib.X_BUF_Y].reshape(nv, R), len(combines)


def signed(A, seed):
    return A * np.random.default_rng(seed).choice([-1.0, 1.0], size=A.shape)


@pytest.mark.parametrize("nv", [1, 3])
@pytest.mark.parametrize("exact", [False, True], ids=["tree", "exact"])
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("G", [2, 4, 8])
def test_block_exchange_gives_the_reference_y_per_column(G, alg, exact, nv):
    R, Cn = SHAPES[G]
    A, X = signed(oracle.synth(R, Cn, 42), 1), signed(oracle.synth(nv, Cn, 4242), 2)
    calls = trace_multi(alg, R, Cn, G, exact, nv)
    per_vector = [_parts(alg, R, Cn, G, A, X[v]) for v in range(nv)]
    parts = [np.stack([per_vector[v][r] for v in range(nv)]) for r in range(G)]
    Y, ncombine = execute_multi(calls, alg, R, Cn, G, parts, nv)
    assert ncombine == (nv if exact and alg != "rowwise" else 0)
    for v in range(nv):
        np.testing.assert_array_equal(Y[v], oracle.multiply(alg, A, X[v], G), err_msg=f"vector {v}")


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("G", [2, 4, 8])
def test_block_exchange_issues_one_group_per_step(G, alg):
    """Tree mode: the schedule's steps, each one group; a reduce is one call of count * nv per
    member, a gather nv calls of count per member. Exact mode (column and block split): one group
    of nv world gathers per rank, then nv combines outside any group."""
    R, Cn = SHAPES[G]
    nv = 3
    plans = [mm.plan_exchange(alg, R, Cn, G, r) for r in range(G)]
    xs = [c for c in trace_multi(alg, R, Cn, G, False, nv) if c["kind"] != _lib.XCALL_SPLIT]
    steps = sorted({c["group"] for c in xs})
    assert len(steps) == len(plans[0])
    for k, g in enumerate(steps):
        cs = [c for c in xs if c["group"] == g]
        for r in range(G):
            mine, st = [c for c in cs if c["rank"] == r], plans[r][k]
            if not st.member:
                assert not mine
            elif st.op == _lib.X_REDUCE:
                assert [(c["kind"], c["count"]) for c in mine] == [(_lib.XCALL_REDUCE, st.count * nv)]
            else:
                assert [(c["kind"], c["count"]) for c in mine] == [(_lib.XCALL_GATHER, st.count)] * nv
    if alg != "rowwise":
        xs = [c for c in trace_multi(alg, R, Cn, G, True, nv) if c["kind"] != _lib.XCALL_SPLIT]
        gathers = [c for c in xs if c["kind"] == _lib.XCALL_GATHER]
        assert len({c["group"] for c in gathers}) == 1 and all(c["comm"] == -1 for c in gathers)
        assert sorted(c["rank"] for c in gathers) == sorted(list(range(G)) * nv)
        assert [c["kind"] for c in xs if c["kind"] != _lib.XCALL_GATHER] == [_lib.XCALL_COMBINE] * nv


def test_one_vector_block_issues_the_single_vector_calls():
    """nv = 1: the same calls, counts and buffers as one mvg_engine_multiply's exchange."""
    for alg in ALGS:
        for exact in (False, True):
            assert trace_multi(alg, 96, 80, 4, exact, 1) == mm.trace_exchange(alg, 96, 80, 4, exact=exact)


def test_trace_refuses_a_block_outside_1_to_16_vectors():
    calls = (_lib.XCall * 64)()
    n = C.c_int()
    for nv in (0, -1, _lib.MAX_VECTORS + 1):
        assert lib.mvg_debug_trace_exchange_multi(0, 96, 80, 2, 0, nv, calls, 64, C.byref(n)) == _lib.MVG_E_INVALID


def test_auto_variant_names_match_the_dispatch_table():
    """The classes the committed sweep (profiles/r07/exact_multi/sweep_all.jsonl) decided, and the
    ones it did not cover, which keep separate passes."""
    pick = lambda m, k, nv: table()[lib.mvg_gemv_exact_multi_auto_variant(k, k, m, k, nv)]  # noqa: E731
    for m, k in ((16384, 16384), (65536, 8192), (524288, 512), (6144, 769)):
        assert pick(m, k, 2) == pick(m, k, 3) == "hopm_l8_w2_u8_v2"
        assert pick(m, k, 4) == pick(m, k, 16) == "hopm_l8_w2_u4_v4"
    assert pick(4096, 16384, 2) == "hopm_l16_w4_u4_v2" and pick(4096, 16384, 8) == "hopm_l16_w4_u4_v4"
    assert pick(1024, 32768, 2) == pick(1024, 32768, 8) == "hopm_l32_w8_u4_v2"
    for m, k in ((8192, 65536), (4096, 8192), (2048, 32768), (1024, 4096), (240, 1260), (624, 1536)):
        assert pick(m, k, 2) == pick(m, k, 16) == "separate", (m, k)
