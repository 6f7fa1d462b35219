"""CPU self-tests of tests/engine_scripts.py, which tests/test_gpu_engine_sequences.py runs on the
device: the scripts are well formed, the host model's answers are spelled out literally (a
rewrite of the model cannot silently change what the GPU tests assert), the comparison rejects
what it must, the runner records a wrong engine without raising, the data tells the combine
orders apart, and the root-send piece list (mvg_debug_shard_pieces) tiles every shard. No GPU."""
import ctypes as C

import numpy as np
import pytest

import engine_scripts as ES
from engine_scripts import D, F, M, O, S, T, X, Y  # noqa: F401
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

lib = _lib.lib
ALL_RUNS = [(n, r) for n, r in ES.SMALL_RUNS.items()] + [("panel/" + n, r) for n, r in ES.PANEL_RUNS.items()]


# ------------------------------------------------------------------ the scripts
@pytest.mark.parametrize("name,run", ALL_RUNS, ids=[n for n, _ in ALL_RUNS])
def test_every_script_is_well_formed(name, run):
    script = run[0]
    assert ES.well_formed(script), ES.spell(script)
    assert sum(op == ES.C for op in script) >= 1
    writes = [op[1] for op in script if op[0] in ES.WRITES]
    assert len(writes) == len(set(writes))  # every write brings a data set no earlier one did


def test_well_formed_rejects_what_it_must():
    assert not ES.well_formed((M, ES.C))                       # no write before the first M
    assert not ES.well_formed((D(0), ES.C))                    # a C with no M before it
    assert not ES.well_formed((D(0), M, D(1), ES.C))           # the C would check a y no multiply made
    assert not ES.well_formed((D(0), M, ES.C, D(0), M, ES.C))  # a data set written twice
    assert ES.well_formed((D(0), M, ES.C, X(1), ES.C))         # exact mode alone leaves y as it is


def test_the_scripts_are_the_ones_agreed():
    assert ES.spell(ES.B2B_EXACT) == "X1 D0 M D1 M D2 M C"
    assert ES.spell(ES.TOGGLE) == "F0 M C X1 M C M C X0 M C X1 M C F1 M C M C"
    assert ES.spell(ES.CHUNKED) == "X1 O3 S0 M C M C O7 S1 S2 M C O0 S3 M C D4 M C"
    assert ES.spell(ES.MIXED_WRITERS) == "O2 S0 F1 M C D2 M X1 M C T1 M M C T-1 M M Y D3 M C T0"
    assert ES.spell(ES.SEND_PIECES) == "D0 M C X1 D1 M M C"
    assert ES.spell(ES.PANEL_RUNS["chunked"][0]) == "X1 O3 S0 M C M C O7 S1 S2 M C O0 S3 M C S4 M C"
    assert [ES.SMALL_RUNS[f"b2b_exact/ring{n}"][1] for n in (1, 2, 8)] == [{"MVG_XRING": str(n)} for n in (1, 2, 8)]
    assert ES.SMALL_RUNS["send_pieces"][2] == 5000 and all(r[2] == 0 for n, r in ES.SMALL_RUNS.items() if n != "send_pieces")


def test_scripts_that_share_an_engine_keep_their_own_answers():
    # groups(): the three ring lengths and the lowered staging need engines of their own, the
    # rest walks one; join() puts X0 O0 T0 between two scripts and moves every script to data
    # sets of its own, so the model gives each script of a group the answers it has alone
    assert [g[0] for g in ES.groups(ES.SMALL_RUNS)] == [
        ["b2b_exact/ring1", "b2b_again/ring1"], ["b2b_exact/ring2", "b2b_again/ring2"],
        ["b2b_exact/ring8", "b2b_again/ring8", "toggle", "chunked", "mixed_writers", "ring_wrap", "timed_chunks"],
        ["send_pieces"]]
    # the exchange's ring slot of the multiply each b2b check reads (multiplies 2 and 5 of the engine)
    assert [n % 2 for n in (2, 5)] == [0, 1] and [n % 8 for n in (2, 5)] == [2, 5]
    assert [g[0] for g in ES.groups(ES.PANEL_RUNS)] == [["toggle", "chunked"], ["chunked/no_panels"]]
    for runs, shape, world in ((ES.SMALL_RUNS, (1200, 960), 2), (ES.SMALL_RUNS, (240, 3072), 1),
                               (ES.PANEL_RUNS, ES.panel_shape("colwise"), 2)):
        for names, env, stage in ES.groups(runs):
            script, owners = ES.join(names, runs)
            assert ES.well_formed(script)
            assert owners == [(n, c) for n in names for c in range(sum(op == ES.C for op in runs[n][0]))]
            for rank in range(world):
                no_panels = env.get("MVG_NO_PANELS") == "1"
                joined = ES.expect(script, "colwise", *shape, world, rank, no_panels)
                alone = []
                for k, n in enumerate(names):
                    for m in ES.expect(runs[n][0], "colwise", *shape, world, rank, no_panels):
                        alone.append(dict(m, set=(m["set"][0], m["set"][1] + ES.SET_STRIDE * k)))
                assert joined == alone, names


# ------------------------------------------------------------------ the model, literally
def answers(script, alg, R, Cn, world, rank, no_panels=False):
    """[(set, exact, width, launches)] per C."""
    return [("%s%d" % m["set"], m["exact"], m["width"], m["launches"])
            for m in ES.expect(script, alg, R, Cn, world, rank, no_panels)]


def test_model_literal_small_shape_colwise_world_2():
    R, Cn = 1200, 960
    for rank in (0, 1):
        def got(s):
            return answers(s, "colwise", R, Cn, 2, rank)

        assert got(ES.B2B_EXACT) == [("D2", True, 0, None)]
        assert got(ES.TOGGLE) == [("F0", False, 0, None), ("F0", True, 0, None), ("F0", True, 0, None),
                                  ("F0", False, 0, None), ("F0", True, 0, None), ("F1", True, 0, None),
                                  ("F1", True, 0, None)]
        assert got(ES.CHUNKED) == [("S0", True, 0, None), ("S0", True, 0, None), ("S2", True, 0, None),
                                   ("S3", True, 0, None), ("D4", True, 0, None)]
        assert got(ES.MIXED_WRITERS) == [("F1", False, 0, None), ("D2", True, 0, None), ("D2", True, 0, 2),
                                         ("D3", True, 0, None)]
        assert got(ES.SEND_PIECES) == [("D0", False, 0, None), ("D1", True, 0, None)]
        assert got(ES.RING_WRAP) == [("D0", False, 0, None), ("D1", True, 0, None), ("D2", True, 0, None)]
        # S0 M M: the first multiply consumes the chunks and is not timed, the second is;
        # S1 M: chunked again, still one launch
        assert got(ES.TIMED_CHUNKS) == [("S0", False, 0, 1), ("S1", False, 0, 1)]


def test_model_literal_panel_shape_colwise_world_2():
    R, Cn = ES.panel_shape("colwise")
    toggle, chunked = ES.PANEL_RUNS["toggle"][0], ES.PANEL_RUNS["chunked"][0]
    for rank in (0, 1):
        # X1 after a multiply of F0: the copy is built by the next multiply at once; X0 releases
        # it; X1 again rebuilds at once; F1 makes it stale: row-major for one multiply, then panels
        assert answers(toggle, "colwise", R, Cn, 2, rank) == [
            ("F0", False, 0, None), ("F0", True, 256, None), ("F0", True, 256, None), ("F0", False, 0, None),
            ("F0", True, 256, None), ("F1", True, 0, None), ("F1", True, 256, None)]
        # only S0 is multiplied twice
        assert answers(chunked, "colwise", R, Cn, 2, rank) == [
            ("S0", True, 0, None), ("S0", True, 256, None), ("S2", True, 0, None), ("S3", True, 0, None),
            ("S4", True, 0, None)]
        assert answers(chunked, "colwise", R, Cn, 2, rank, no_panels=True) == [
            ("S0", True, 0, None), ("S0", True, 0, None), ("S2", True, 0, None), ("S3", True, 0, None),
            ("S4", True, 0, None)]
    # mixed_writers' X1 comes after one multiply of D2: on a panel shard the next multiply builds
    assert [a[2] for a in answers(ES.MIXED_WRITERS, "colwise", R, Cn, 2, 0)] == [0, 256, 256, 0]


def test_model_chunking_follows_the_engine():
    # a D is chunked only when every rank is in one process (world 1); a shard with fewer than
    # two rows per chunk is copied whole
    script = (O(3), T(1), D(0), M, ES.C)
    assert answers(script, "rowwise", 240, 3072, 1, 0)[0][3] == 0
    assert answers(script, "rowwise", 240, 3072, 2, 0)[0][3] == 1
    few = (O(50), T(1), S(0), M, ES.C)
    assert answers(few, "rowwise", 240, 3072, 3, 0)[0][3] == 1   # 80 rows < 2 * 50
    assert answers(few, "colwise", 240, 3072, 3, 0)[0][3] == 0   # 240 rows
    # F and a second T reset what they must
    assert answers((T(1), F(0), M, M, T(1), M, ES.C), "rowwise", 240, 3072, 2, 1)[0][3] == 1


def test_panel_shards_keep_a_copy_and_small_ones_do_not():
    for alg in ES.ALGS:
        R, Cn = ES.panel_shape(alg)
        for rank in range(ES.PANEL_WORLD):
            sh = mm.plan_shard(alg, R, Cn, ES.PANEL_WORLD, rank)
            assert (sh.n_rows, sh.n_cols) == ES.PANEL_SHARD
            assert lib.mvg_exact_panel_width(sh.n_rows, sh.n_cols) == 256 and sh.n_cols % 256 == 2
        for R, Cn in ES.SMALL_SHAPES:
            for world in ES.WORLDS:
                for rank in range(world):
                    sh = mm.plan_shard(alg, R, Cn, world, rank)  # raises if the shape does not divide
                    assert sh.n_rows > 0 and sh.n_cols > 0
                    assert lib.mvg_exact_panel_width(sh.n_rows, sh.n_cols) == 0
    assert {mm.get_2_most_closest_multipliers(p) for p in (3, 4, 6)} == {(1, 3), (2, 2), (2, 3)}


# ------------------------------------------------------------------ the data tells the orders apart
def colwise_parts(A, x, P):
    R, Cn = A.shape
    parts = []
    for r in range(P):
        sh = mm.plan_shard("colwise", R, Cn, P, r)
        cols = slice(sh.col_off, sh.col_off + sh.n_cols)
        parts.append(oracle.multiply_std_rowwise(np.ascontiguousarray(A[:, cols]), x[cols]))
    return parts


def in_order(parts):
    y = parts[0].copy()
    for p in parts[1:]:
        y = y + p
    return y


@pytest.mark.parametrize("R,Cn", ES.SMALL_SHAPES)
def test_signed_sets_separate_the_column_splits_orders(R, Cn):
    """An exact-mode pass at P ranks proves the combine order only if another order would give
    other bits on the same data. On every host-distributed set of the scripts: at P = 4 and 6
    MPICH's order (oracle.multiply) differs from the plain rank-order sum ((p0 + p1) + p2) + ...
    in many rows, on the binomial path (240 rows) and the reduce-scatter path (1200 rows). The
    two paths themselves associate alike at P = 2, 3, 4 and 6 (oracle/cpu_ref.c
    ref_mpich_reduce), so these world sizes run both but cannot tell them apart; P = 5, 9, 10
    can, and the combine kernel is tested there through its hook (tests/test_gpu_exact.py). At
    P = 3 MPICH folds ranks 0 and 1 and then adds rank 2, on both paths: that is the rank-order
    sum, so there the data must separate it from the other association, p0 + (p1 + p2)."""
    assert (R * 8 <= 2048) == (R == 240)
    data = ES.DataSets(R, Cn)
    for i in range(5):
        A, x = data.inputs("D", i)
        assert (A < 0).any() and (A > 0).any() and (x < 0).any()
        for P in (3, 4, 6):
            parts = colwise_parts(A, x, P)
            want = oracle.multiply("colwise", A, x, P)
            assert np.array_equal(oracle.mpich_reduce(parts), want)
            if P == 3:
                assert np.array_equal(in_order(parts), want)
                other = parts[0] + (parts[1] + parts[2])
            else:
                other = in_order(parts)
            assert np.count_nonzero(other != want) >= R // 8, (P, i)


@pytest.mark.parametrize("R,Cn", ES.SMALL_SHAPES)
def test_signed_sets_separate_the_block_splits_order_over_three_columns(R, Cn):
    # 2 x 3 grid: y's slice of a grid row is ((0 + p0) + p1) + p2; the data must tell that from
    # (p2 + p1) + p0, or the rank-order sum over three grid columns is not tested
    data = ES.DataSets(R, Cn)
    for i in range(5):
        A, x = data.inputs("D", i)
        want = oracle.multiply("blockwise", A, x, 6)
        back = np.zeros(R)
        for r in (5, 4, 3, 2, 1, 0):
            sh = mm.plan_shard("blockwise", R, Cn, 6, r)
            blk = np.ascontiguousarray(A[sh.row_off:sh.row_off + sh.n_rows, sh.col_off:sh.col_off + sh.n_cols])
            rows = slice(sh.y_off, sh.y_off + sh.y_len)
            back[rows] = back[rows] + oracle.multiply_std_rowwise(blk, x[sh.col_off:sh.col_off + sh.n_cols])
        assert np.count_nonzero(back != want) >= R // 8, i


def test_every_two_data_sets_differ_everywhere():
    # a y from any other data set of a script misses the bound in (nearly) every row
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    ys = {}
    for kind in ("D", "F"):
        for i in range(5):
            ys[kind, i] = data.want("colwise", 2, kind, i)
    for a in ys:
        for b in ys:
            if a != b:
                assert np.count_nonzero(np.abs(ys[a][0] - ys[b][0]) > ES.TOL * ys[b][1]) >= R - 2, (a, b)


# ------------------------------------------------------------------ the comparison
def test_checker_rejects_a_stale_y_and_one_ulp():
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    want, mag = data.want("colwise", 3, "D", 1)
    prev, _ = data.want("colwise", 3, "D", 0)
    assert ES.check_y(want.copy(), want, mag, True) == (True, 0.0)
    assert ES.check_y(want.copy(), want, mag, False)[0]
    assert not ES.check_y(prev, want, mag, True)[0]
    assert not ES.check_y(prev, want, mag, False)[0]
    one = want.copy()
    one[R // 2] = np.nextafter(one[R // 2], np.inf)
    assert ES.check_y(one, want, mag, True) == (False, 1.0)   # one ulp in one row: not the reference's bits
    assert ES.check_y(one, want, mag, False)[0]               # but well inside the 1e-12 bar
    off = want.copy()
    off[7] += 2e-12 * mag[7]
    ok, figure = ES.check_y(off, want, mag, False)
    assert not ok and 1.5e-12 < figure < 2.5e-12
    bad = want.copy()
    bad[3] = np.nan
    assert not ES.check_y(bad, want, mag, False)[0] and not ES.check_y(bad, want, mag, True)[0]
    assert not ES.check_y(want[:-1], want, mag, False)[0]


# ------------------------------------------------------------------ the runner, on a stand-in engine
class FakeEngine:
    """A Multiplier stand-in on the host: y is the oracle's product of whatever was written last,
    the panel width and launch count follow csrc/engine.cpp's fields. `fault` makes it wrong the
    way a slip in the engine would."""

    def __init__(self, alg, R, Cn, world, rank, data, fault=None):
        self.name, self.R, self.C, self.world, self.rank, self.data, self.fault = alg, R, Cn, world, rank, data, fault
        self.plan = mm.plan_shard(alg, R, Cn, world, rank)
        self.exact = False
        self.panelP, self.dAp, self.panels_fresh, self.uses, self.chunks_pending = 0, False, False, 0, False
        self.overlap, self.timing, self.launches = 0, 0, 0
        self.sets, self.y_set, self.calls = [], None, []

    def shard(self, i=0):
        return self.plan

    def is_root(self):
        return self.rank == 0

    def _write(self, kind, i, chunked):
        self.calls.append(kind)
        if self.fault != "write_keeps_panels":
            self.panels_fresh = False
        self.uses = 0
        self.chunks_pending = chunked and self.overlap > 1 and self.plan.n_rows >= 2 * self.overlap
        self.sets.append((kind, i))

    def _set_of(self, A):
        """Which data set the runner handed over (by identity; -1 off the root, where the
        stand-in never looks at the values)."""
        return -1 if A is None else next(i for i in range(8) if A is self.data.inputs("D", i)[0])

    def distribute(self, A, x):
        assert (A is None) == (self.rank != 0) and (x is None) == (self.rank != 0)  # A, x on the root alone
        self._write("D", self._set_of(A), self.world == 1)

    def distribute_shared(self, A, x):
        assert A is not None and x is not None  # every rank brings the shared A and x
        self._write("S", self._set_of(A), True)

    def fill_synth(self, sa, sx):
        self._write("F", (sa - 42) // 2, False)
        assert ES.seeds(self.sets[-1][1]) == (sa, sx)

    def multiply(self):
        self.calls.append("M")
        if self.exact and self.panelP and not self.panels_fresh and self.uses >= 1 and not self.chunks_pending:
            self.dAp = self.panels_fresh = True
        if self.timing == 1 and not self.chunks_pending:
            self.launches += 1
        self.uses += 1
        self.chunks_pending = False
        self.y_set = self.sets[-2] if self.fault == "stale_y" and len(self.sets) > 1 else self.sets[-1]

    def set_exact(self, on):
        self.exact = on
        if not on:
            self.dAp, self.panelP, self.panels_fresh = False, 0, False
        elif not self.dAp:
            self.panelP, self.panels_fresh = int(lib.mvg_exact_panel_width(self.plan.n_rows, self.plan.n_cols)), False

    def set_overlap(self, n):
        self.overlap = n

    def kernel_timing(self, mode):
        self.timing, self.launches = mode, 0

    def kernel_ms(self):
        return mm.KernelTiming(0.1, self.launches)

    def sync(self):
        self.calls.append("Y")

    def exact_panel_width(self, i=0):
        return self.panelP if self.exact and self.dAp and self.panels_fresh else 0

    def collect(self):
        self.calls.append("C")
        if self.rank:
            return None
        y = self.data.want(self.name, self.world, *self.y_set)[0].copy()
        if self.fault == "one_ulp":
            y[0] = np.nextafter(y[0], np.inf)
        return y


@pytest.mark.parametrize("name,run", list(ES.SMALL_RUNS.items()), ids=list(ES.SMALL_RUNS))
def test_runner_passes_a_right_engine_and_records_a_wrong_one(name, run):
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    script = run[0]
    for alg, world in (("colwise", 3), ("blockwise", 6), ("rowwise", 1)):
        for rank in {0, world - 1}:
            recs = ES.run_script(FakeEngine(alg, R, Cn, world, rank, data), script, data, world)
            assert len(recs) == sum(op == ES.C for op in script)
            assert all(r["ok"] for r in recs), recs
            assert all((r["y_ok"] is None) == (rank != 0) for r in recs)
        # a y from the data set before: recorded on the root, not raised, and the script is
        # walked to its end
        stale = FakeEngine(alg, R, Cn, world, 0, data, fault="stale_y")
        recs = ES.run_script(stale, script, data, world)
        assert len(recs) == sum(op == ES.C for op in script)
        assert [c for c in stale.calls if c in "MCY"] == [op[0] for op in script if op[0] in "MCY"]
        later = [r for r, m in zip(recs, ES.expect(script, alg, R, Cn, world, 0)) if m["set"] != (script_first_write(script))]
        assert later and not any(r["ok"] or r["y_ok"] for r in later), recs
        # one ulp: caught exactly where the model says exact mode is on
        recs = ES.run_script(FakeEngine(alg, R, Cn, world, 0, data, fault="one_ulp"), script, data, world)
        assert [r["ok"] for r in recs] == [not r["want_exact"] for r in recs]


def script_first_write(script):
    return next((op[0], op[1]) for op in script if op[0] in ES.WRITES)


def test_runner_catches_a_panel_copy_that_a_write_leaves_fresh():
    # the stand-in's begin_write slip shows as a width the model does not allow (on the device
    # the stale copy also gives the previous set's y)
    alg = "colwise"
    R, Cn = ES.panel_shape(alg)

    class NoData:
        def inputs(self, kind, i):
            return None, None

    for fault, want_ok in ((None, True), ("write_keeps_panels", False)):
        e = FakeEngine(alg, R, Cn, 2, 1, NoData(), fault=fault)
        recs = ES.run_script(e, ES.TOGGLE, NoData(), 2)
        assert all(r["ok"] for r in recs) == want_ok
        assert [r["want_width"] for r in recs] == [0, 256, 256, 0, 256, 0, 256]
        if fault:
            assert [r["width"] for r in recs] == [0, 256, 256, 0, 256, 256, 256]


# ------------------------------------------------------------------ the root-send piece list
def pieces(alg, R, Cn, P, rank, stage, cap=4096):
    row0, rows, count = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)()
    n = C.c_int(-1)
    rc = lib.mvg_debug_shard_pieces(mm.ALG_BY_NAME[alg], R, Cn, P, rank, stage, row0, rows, count, cap, C.byref(n))
    return rc, [(row0[i], rows[i], count[i]) for i in range(max(n.value, 0))]


@pytest.mark.parametrize("P", [2, 3, 4, 6])
@pytest.mark.parametrize("alg", ES.ALGS)
def test_shard_pieces_tile_every_shard(alg, P):
    for R, Cn in ES.SMALL_SHAPES:
        for rank in range(P):
            sh = mm.plan_shard(alg, R, Cn, P, rank)
            nc = sh.n_cols
            for stage in (nc, nc + 1, 9 * nc - 1, 5000, 0):
                rc, ps = pieces(alg, R, Cn, P, rank, stage)
                assert rc == _lib.MVG_OK, (rank, stage)
                limit = stage or (256 << 20) // 8
                assert ps[0] == (-1, 1, nc)  # the x segment first
                at = 0
                for row0, rows, count in ps[1:]:
                    assert row0 == at and rows >= 1  # in order, no gap, no empty piece
                    assert count == rows * nc and count <= limit
                    # a piece is as long as the staging allows: only the last may be shorter
                    assert rows == min(limit // nc, sh.n_rows - at)
                    at += rows
                assert at == sh.n_rows
                rows_per = limit // nc
                assert len(ps) == 1 + -(-sh.n_rows // rows_per)
            # a row that does not fit the staging: refused for every rank's plan
            for stage in (nc - 1, 1):
                rc, ps = pieces(alg, R, Cn, P, rank, stage)
                assert rc == _lib.MVG_E_INVALID and ps == []
                assert b"row larger than staging" in lib.mvg_last_error()


def test_shard_pieces_of_the_gpu_scripts_shapes():
    # what send_pieces sends at 5000 doubles: 10-row pieces, 120 per peer, at 1200 x 960 in
    # column strips over 2 ranks; single rows at 240 x 3072 in row blocks
    rc, ps = pieces("colwise", 1200, 960, 2, 1, ES.SEND_PIECES_STAGE)
    assert rc == 0 and len(ps) == 121 and all(p[1:] == (10, 4800) for p in ps[1:])
    rc, ps = pieces("rowwise", 240, 3072, 2, 1, ES.SEND_PIECES_STAGE)
    assert rc == 0 and len(ps) == 121 and all(p[1:] == (1, 3072) for p in ps[1:])
    # a receiver that cut with a staging one row larger than the sender's would post other counts
    assert pieces("colwise", 1200, 960, 2, 1, ES.SEND_PIECES_STAGE + 480)[1] != ps
    for alg in ES.ALGS:
        for R, Cn in ES.SMALL_SHAPES:
            for world in ES.WORLDS:
                assert all(mm.plan_shard(alg, R, Cn, world, r).n_cols <= ES.SEND_PIECES_STAGE for r in range(world))


def test_shard_pieces_empty_shards_and_bad_arguments():
    for alg in ES.ALGS:
        assert pieces(alg, 240, 0, 2, 1, 5000) == (_lib.MVG_OK, [])      # no columns: nothing travels
        rc, ps = pieces(alg, 0, 3072, 2, 1, 5000)                        # no rows: the x segment alone
        assert rc == _lib.MVG_OK and len(ps) == 1 and ps[0][0] == -1
    assert pieces("rowwise", 10, 10, 3, 0, 5000)[0] == _lib.MVG_E_INDIVISIBLE
    assert pieces("rowwise", 240, 3072, 2, 1, -1)[0] == _lib.MVG_E_INVALID
    assert pieces("rowwise", 240, 3072, 2, 1, 5000, cap=3)[0] == _lib.MVG_E_INVALID  # 121 pieces
    n = C.c_int()
    assert lib.mvg_debug_shard_pieces(0, 240, 3072, 2, 1, 5000, None, None, None, 8, C.byref(n)) == _lib.MVG_E_INVALID
    assert lib.mvg_debug_shard_pieces(0, 240, 3072, 2, 1, 5000, None, None, None, 0, None) == _lib.MVG_E_INVALID


def test_set_stage_elems_hook():
    try:
        assert lib.mvg_debug_set_stage_elems(-1) == _lib.MVG_E_INVALID
        assert lib.mvg_debug_set_stage_elems(5000) == _lib.MVG_OK
        # the piece list takes its staging as an argument: the hook's value is the engines' alone
        assert len(pieces("rowwise", 240, 3072, 2, 1, 0)[1]) == 2
    finally:
        assert lib.mvg_debug_set_stage_elems(0) == _lib.MVG_OK
