"""CPU self-tests of tests/engine_scripts.py, which tests/test_gpu_engine_sequences.py runs on the
device: the scripts are well formed, the host model's answers are spelled out literally (a
rewrite of the model cannot silently change what the GPU tests assert), the comparison rejects
what it must, the runner records a wrong engine without raising, the data tells the combine
orders apart, and the root-send piece list (mvg_debug_shard_pieces) tiles every shard. No GPU."""
import ctypes as C

import numpy as np
import pytest

import engine_scripts as ES
from engine_scripts import CM, D, F, G, M, MM, O, S, T, V, X, Y  # noqa: F401
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

lib = _lib.lib
ALL_RUNS = ([(n, r) for n, r in ES.SMALL_RUNS.items()] + [("panel/" + n, r) for n, r in ES.PANEL_RUNS.items()]
            + [(n, r) for n, r in ES.BLOCK_RUNS.items()] + [("panel/" + n, r) for n, r in ES.BLOCK_PANEL_RUNS.items()])


# ------------------------------------------------------------------ the scripts
@pytest.mark.parametrize("name,run", ALL_RUNS, ids=[n for n, _ in ALL_RUNS])
def test_every_script_is_well_formed(name, run):
    script = run[0]
    assert ES.well_formed(script), ES.spell(script)
    assert sum(op == ES.C for op in script) >= 1 or sum(op == CM for op in script) >= 1
    writes = [op[1] for op in script if op[0] in ES.WRITES]
    assert len(writes) == len(set(writes))  # every write brings a data set no earlier one did
    vsets = [op[1] for op in script if op[0] in ES.VECTORS]
    assert len(vsets) == len(set(vsets))    # and every V or G a vector set no earlier one did
    assert max(writes + vsets) < ES.SET_STRIDE  # join() keeps the scripts of a group apart


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
        self.vsets, self.vectors, self.Y_of = [], 0, None

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

    # ---- the block: X is told apart by identity, as A is; Y is the oracle's of what the last
    # multiply_multi saw. `fault`: "mm_uses" counts it as a use of A, "mm_timed" times it,
    # "mm_keeps_chunks" leaves a chunked distribution pending, "stale_x" multiplies the vector
    # set before the current one
    def set_vectors(self, Xm, nv=None):
        assert (Xm is None) == (self.rank != 0)  # X on the root alone
        if Xm is not None:
            assert Xm.shape == (self.C, nv) and Xm.T.flags.c_contiguous  # handed over without a copy
            j = next(j for j in range(80) if np.shares_memory(Xm, self.data.vectors("V", j)))
        self.vsets.append(("V", j if Xm is not None else -1, nv))
        self.vectors = nv

    def fill_synth_vectors(self, seed, nv):
        self.vsets.append(("G", (seed - 777) // 2, nv))
        assert ES.seed_of(self.vsets[-1][1]) == seed
        self.vectors = nv

    def multiply_multi(self):
        self.calls.append("MM")
        if self.fault == "mm_uses":
            self.uses += 1
        if self.fault == "mm_timed" and self.timing == 1:
            self.launches += 1
        if self.fault != "mm_keeps_chunks":
            self.chunks_pending = False
        vset = self.vsets[-2] if self.fault == "stale_x" and len(self.vsets) > 1 else self.vsets[-1]
        self.Y_of = (self.sets[-1], vset[:2] + (self.vsets[-1][2],))

    def collect_multi(self):
        self.calls.append("CM")
        if self.rank:
            return None
        Yb = self.data.want_multi(self.name, self.world, *self.Y_of)[0].copy()
        if self.fault == "one_ulp":
            Yb[0, -1] = np.nextafter(Yb[0, -1], np.inf)
        return Yb


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


# ------------------------------------------------------------------ a block of vectors beside the single one
def test_well_formed_rejects_ill_formed_block_scripts():
    assert ES.well_formed((D(0), V(0, 3), MM, CM))
    assert not ES.well_formed((V(0, 3), MM, CM))                        # no write of A before the MM
    assert not ES.well_formed((D(0), MM, CM))                           # no V or G before the MM
    assert not ES.well_formed((D(0), V(0, 3), CM))                      # a CM with no MM before it
    assert not ES.well_formed((D(0), V(0, 3), M, CM))                   # an M is no MM
    assert not ES.well_formed((D(0), V(0, 3), MM, ES.C))                # and an MM no M
    assert not ES.well_formed((D(0), V(0, 3), MM, V(1, 3), CM))         # a V between the MM and its CM
    assert not ES.well_formed((D(0), V(0, 3), MM, G(1, 3), CM))         # a G
    assert not ES.well_formed((D(0), V(0, 3), MM, S(1), CM))            # a write of A
    assert not ES.well_formed((D(0), V(0, 3), MM, CM, G(0, 3), MM, CM))  # a vector set used twice
    assert not ES.well_formed((D(0), V(0, 4), MM, CM))                  # nv outside NVS
    assert ES.well_formed((D(0), V(0, 3), MM, M, X(0), CM, ES.C))       # an M or a mode leaves Y as it is
    assert ES.NVS == (1, 3, 7, 11) and ES.NV_MAX == 11 and ES.seed_of(0) == 777


def test_the_block_scripts_are_the_ones_agreed():
    assert ES.spell(ES.BLK_B2B_EXACT) == "X1 D0 V0:3 MM D1 V1:3 MM D2 V2:3 MM CM"
    assert ES.spell(ES.BLK_MIXED_RING) == ("D0 V0:7 M MM M MM M MM M MM M MM C CM "
                                           "X1 D1 V1:3 MM M MM M MM M MM M MM M CM C")
    assert ES.spell(ES.BLK_GROW_IN_FLIGHT) == "D0 V0:3 MM MM MM V1:11 MM CM V2:1 MM CM X1 MM CM G3:7 MM CM"
    assert ES.spell(ES.BLK_CHUNKED) == ("X1 O3 S0 V0:7 MM CM M C O7 S1 S2 MM CM S3 M MM C CM O0 S4 MM CM D5 MM CM")
    assert ES.spell(ES.BLK_TIMED_CHUNKS) == "O3 T1 S0 V0:3 MM M C S1 M C MM CM T0"
    assert ES.spell(ES.BLK_SEND_PIECES) == "D0 V0:11 MM D1 V1:11 MM CM X1 D2 MM M CM C"
    assert ES.spell(ES.BLK_WRITERS) == ("F0 G0:7 MM CM S1 V1:3 MM CM D2 G2:11 MM CM V3:11 MM CM X1 F3 MM CM G4:3 MM CM "
                                        "S4 V5:7 MM CM D5 MM CM G6:1 V7:1 MM CM")
    assert ES.spell(ES.BLOCK_PANEL_RUNS["blk_panels"][0]) == "X1 S0 V0:3 M M C MM CM S1 MM CM M C M C MM CM X0 MM CM"
    assert ES.spell(ES.BLOCK_PANEL_RUNS["blk_chunked"][0]).endswith("O0 S4 MM CM S5 MM CM")
    rings = {n: r[1]["MVG_XRING"] for n, r in ES.BLOCK_RUNS.items() if "/ring" in n}
    assert rings == {f"{s}/ring{n}": str(n) for s, ns in (("blk_b2b_exact", (1, 2, 8)), ("blk_b2b_again", (1, 2, 8)),
                                                          ("blk_mixed_ring", (2, 3, 8))) for n in ns}
    assert all(ES.BLOCK_RUNS[f"blk_b2b_again/ring{n}"][0] is ES.BLK_B2B_EXACT for n in (1, 2, 8))
    assert [n for n, r in ES.BLOCK_RUNS.items() if r[2]] == ["blk_send_pieces"]
    assert ES.BLOCK_RUNS["blk_send_pieces"][2] == ES.SEND_PIECES_STAGE
    assert all(r[1] == {"MVG_NO_PANELS": "0"} for r in ES.BLOCK_PANEL_RUNS.values())
    # V and G follow one another both ways round, and every writer of A comes before an MM in
    # both modes
    w = ES.spell(ES.BLK_WRITERS)
    assert "G6:1 V7:1" in w and w.index("G2:11") < w.index("V3:11") < w.index("G4:3")
    tree, exact = w.split(" X1 ")
    assert all(k in tree and k in exact for k in "FSD")


def block_answers(script, alg, R, Cn, world, rank, no_panels=False):
    """[(set, vset or None at a C, exact, width, launches)] per C and CM."""
    return [("%s%d" % m["set"], "%s%d:%d" % m["vset"] if "vset" in m else None, m["exact"], m["width"], m["launches"])
            for m in ES.expect(script, alg, R, Cn, world, rank, no_panels)]


def test_block_model_literal_small_shape_colwise_world_2():
    R, Cn = 1200, 960
    for rank in (0, 1):
        def got(s):
            return block_answers(s, "colwise", R, Cn, 2, rank)

        assert got(ES.BLK_B2B_EXACT) == [("D2", "V2:3", True, 0, None)]
        assert got(ES.BLK_MIXED_RING) == [("D0", None, False, 0, None), ("D0", "V0:7", False, 0, None),
                                          ("D1", "V1:3", True, 0, None), ("D1", None, True, 0, None)]
        # set, vector set and mode are the last MM's: V2:1 is still current at the exact MM
        assert got(ES.BLK_GROW_IN_FLIGHT) == [("D0", "V1:11", False, 0, None), ("D0", "V2:1", False, 0, None),
                                              ("D0", "V2:1", True, 0, None), ("D0", "G3:7", True, 0, None)]
        assert got(ES.BLK_CHUNKED) == [("S0", "V0:7", True, 0, None), ("S0", None, True, 0, None),
                                       ("S2", "V0:7", True, 0, None), ("S3", None, True, 0, None),
                                       ("S3", "V0:7", True, 0, None), ("S4", "V0:7", True, 0, None),
                                       ("D5", "V0:7", True, 0, None)]
        # S0 MM M: the MM consumed the chunks, so the M is whole and timed; S1 M: chunked, not
        # timed; the MM after it is never timed
        assert got(ES.BLK_TIMED_CHUNKS) == [("S0", None, False, 0, 1), ("S1", None, False, 0, 1),
                                            ("S1", "V0:3", False, 0, 1)]
        assert got(ES.BLK_SEND_PIECES) == [("D1", "V1:11", False, 0, None), ("D2", "V1:11", True, 0, None),
                                           ("D2", None, True, 0, None)]
        assert got(ES.BLK_WRITERS) == [
            ("F0", "G0:7", False, 0, None), ("S1", "V1:3", False, 0, None), ("D2", "G2:11", False, 0, None),
            ("D2", "V3:11", False, 0, None), ("F3", "V3:11", True, 0, None), ("F3", "G4:3", True, 0, None),
            ("S4", "V5:7", True, 0, None), ("D5", "V5:7", True, 0, None), ("D5", "V7:1", True, 0, None)]
    # the pair the model's second rule rests on: without the MM the M consumes the chunks untimed
    assert [a[4] for a in block_answers((O(3), T(1), S(0), V(0, 3), MM, M, ES.C), "colwise", R, Cn, 2, 0)] == [1]
    assert [a[4] for a in block_answers((O(3), T(1), S(0), M, ES.C), "colwise", R, Cn, 2, 0)] == [0]


def test_block_model_literal_panel_shape_colwise_world_2():
    R, Cn = ES.panel_shape("colwise")
    for rank in (0, 1):
        # 256 only where two M have run since the last write; no MM moves the width, beside a
        # fresh copy (checks 1, 5), a stale one (2) and after X0 released it (6)
        assert block_answers(ES.BLOCK_PANEL_RUNS["blk_panels"][0], "colwise", R, Cn, 2, rank) == [
            ("S0", None, True, 256, None), ("S0", "V0:3", True, 256, None), ("S1", "V0:3", True, 0, None),
            ("S1", None, True, 0, None), ("S1", None, True, 256, None), ("S1", "V0:3", True, 256, None),
            ("S1", "V0:3", False, 0, None)]
        # no set is multiplied by M twice
        assert block_answers(ES.BLOCK_PANEL_RUNS["blk_chunked"][0], "colwise", R, Cn, 2, rank) == [
            ("S0", "V0:7", True, 0, None), ("S0", None, True, 0, None), ("S2", "V0:7", True, 0, None),
            ("S3", None, True, 0, None), ("S3", "V0:7", True, 0, None), ("S4", "V0:7", True, 0, None),
            ("S5", "V0:7", True, 0, None)]
        # an MM between the two M is no use: S0 M MM M builds at the second M, S0 M MM does not
        assert [a[3] for a in block_answers((X(1), S(0), V(0, 3), M, MM, CM, M, ES.C), "colwise", R, Cn, 2, rank)] == [0, 256]
        assert [a[3] for a in block_answers((X(1), S(0), V(0, 3), MM, M, MM, CM), "colwise", R, Cn, 2, rank)] == [0]


def test_block_scripts_that_share_an_engine_keep_their_own_answers():
    assert [g[0] for g in ES.groups(ES.BLOCK_RUNS)] == [
        ["blk_b2b_exact/ring1", "blk_b2b_again/ring1"],
        ["blk_mixed_ring/ring2", "blk_b2b_exact/ring2", "blk_b2b_again/ring2"],
        ["blk_mixed_ring/ring3"],
        ["blk_mixed_ring/ring8", "blk_b2b_exact/ring8", "blk_b2b_again/ring8", "blk_grow_in_flight", "blk_chunked",
         "blk_timed_chunks", "blk_writers"],
        ["blk_send_pieces"]]
    assert [g[0] for g in ES.groups(ES.BLOCK_PANEL_RUNS)] == [["blk_panels", "blk_chunked"]]
    for runs, shape, world in ((ES.BLOCK_RUNS, (1200, 960), 2), (ES.BLOCK_RUNS, (240, 3072), 1),
                               (ES.BLOCK_PANEL_RUNS, ES.panel_shape("colwise"), 2)):
        for names, env, stage in ES.groups(runs):
            script, owners = ES.join(names, runs)
            assert ES.well_formed(script)
            assert owners == [(n, c) for n in names for c in range(ES.n_checks(runs[n][0]))]
            for rank in range(world):
                joined = ES.expect(script, "colwise", *shape, world, rank)
                alone = []
                for k, n in enumerate(names):
                    for m in ES.expect(runs[n][0], "colwise", *shape, world, rank):
                        m = dict(m, set=(m["set"][0], m["set"][1] + ES.SET_STRIDE * k))
                        if "vset" in m:
                            m["vset"] = (m["vset"][0], m["vset"][1] + ES.SET_STRIDE * k, m["vset"][2])
                        alone.append(m)
                assert joined == alone, names


def ring_group(ring):
    """The scripts that walk the engine of ring length `ring`, joined as the runner walks them."""
    names = next(g[0] for g in ES.groups(ES.BLOCK_RUNS) if g[1] == {"MVG_XRING": str(ring)} and g[2] == 0)
    script, owners = ES.join(names, ES.BLOCK_RUNS)
    return names, script


def multiplies_of(names, script, name):
    """ES.slots' entries of the multiplies that script `name` of the group issues."""
    per = {n: sum(op[0] in ("M", "MM") for op in ES.BLOCK_RUNS[n][0]) for n in names}
    start = sum(per[n] for n in names[:names.index(name)])
    return ES.slots(script, int(ES.BLOCK_RUNS[name][1]["MVG_XRING"]))[start:start + per[name]]


@pytest.mark.parametrize("ring", [2, 3, 8])
def test_mixed_ring_takes_the_ring_wait_on_either_kind_behind_the_other(ring):
    names, script = ring_group(ring)
    assert names[0] == f"blk_mixed_ring/ring{ring}"  # the engine's first script: its slots count from 0
    walked = multiplies_of(names, script, names[0])
    # each half issues more multiplies than the ring has slots, the second the other kind first
    assert [w[0] for w in walked] == ["M", "MM"] * 5 + ["MM", "M"] * 5 and 10 > ring
    # slot 0 with an exchange pending (the wait is taken) on an MM right behind an M's exchange ...
    assert any(w == ("MM", 0, "M", True) for w in walked), walked
    # ... and on an M right behind an MM's
    assert any(w == ("M", 0, "MM", True) for w in walked), walked


def test_b2b_walks_end_in_different_slots():
    for ring, ends in ((2, (0, 1)), (8, (6, 1))):
        names, script = ring_group(ring)
        first = multiplies_of(names, script, f"blk_b2b_exact/ring{ring}")
        again = multiplies_of(names, script, f"blk_b2b_again/ring{ring}")
        assert [w[0] for w in first + again] == ["MM"] * 6
        assert (first[-1][1], again[-1][1]) == ends  # the Y that is checked comes out of another slot
    # a ring of one exchanges on the GEMV stream: one slot, no wait
    names, script = ring_group(1)
    assert all(w[1:] == (0, p, False) for w, p in zip(ES.slots(script, 1), [None] + ["MM"] * 5))


def test_slot_replay_follows_the_engine():
    s = (D(0), V(0, 1), M, MM, Y, M, M, T(1), MM, ES.C, MM, T(0), M)
    assert ES.slots(s, 2) == [("M", 0, None, False), ("MM", 1, "M", False), ("M", 0, "MM", False), ("M", 1, "M", False),
                              ("MM", 0, "M", False), ("MM", 1, "MM", False), ("M", 0, "MM", False)]
    assert ES.slots((D(0), M, M, M, ES.C, M, M), 2) == [("M", 0, None, False), ("M", 1, "M", False), ("M", 0, "M", True),
                                                       ("M", 1, "M", False), ("M", 0, "M", True)]


@pytest.mark.parametrize("R,Cn", ES.SMALL_SHAPES)
def test_signed_vector_sets_separate_the_combine_orders(R, Cn):
    """test_signed_sets_separate_the_column_splits_orders and its block-split twin, for the
    vectors of the V sets: an exact-mode pass of a block proves the combine order per vector only
    if another order would give other bits. Every V set of the scripts (j below SET_STRIDE + 3:
    the second walk of blk_b2b_exact included), its first and last vector, on a signed A."""
    data = ES.DataSets(R, Cn)
    A = data.inputs("D", 0)[0]
    for j in list(range(8)) + [10, 11, 12]:
        XT = data.vectors("V", j)
        assert XT.shape == (ES.NV_MAX, Cn) and XT.flags.c_contiguous
        assert np.array_equal(np.abs(XT), data.vectors("G", j))  # the same values, signs apart
        assert np.array_equal(data.vectors("G", j), oracle.synth(ES.NV_MAX, Cn, 777 + 2 * j))
        for v in (0, ES.NV_MAX - 1):
            x = XT[v]
            assert (x < 0).any() and (x > 0).any()
            for P in (3, 4, 6):
                parts = colwise_parts(A, x, P)
                want = oracle.multiply("colwise", A, x, P)
                other = parts[0] + (parts[1] + parts[2]) if P == 3 else in_order(parts)
                assert np.count_nonzero(other != want) >= R // 8, (j, v, P)
            want = oracle.multiply("blockwise", A, x, 6)
            back = np.zeros(R)
            for r in (5, 4, 3, 2, 1, 0):
                sh = mm.plan_shard("blockwise", R, Cn, 6, r)
                blk = np.ascontiguousarray(A[sh.row_off:sh.row_off + sh.n_rows, sh.col_off:sh.col_off + sh.n_cols])
                rows = slice(sh.y_off, sh.y_off + sh.y_len)
                back[rows] = back[rows] + oracle.multiply_std_rowwise(blk, x[sh.col_off:sh.col_off + sh.n_cols])
            assert np.count_nonzero(back != want) >= R // 8, (j, v)


def test_every_two_vector_sets_differ_everywhere():
    # a Y from any other vector set of a script, or from the neighbouring column, misses the bound
    # in (nearly) every element
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    ys = {(k, j): data.want_multi("colwise", 2, ("D", 0), (k, j, 3)) for k in "VG" for j in range(4)}
    for a in ys:
        for b in ys:
            if a != b:
                assert np.count_nonzero(np.abs(ys[a][0] - ys[b][0]) > ES.TOL * ys[b][1]) >= 3 * R - 6, (a, b)
    want, mag = ys["V", 0]
    assert np.count_nonzero(np.abs(want[:, 0] - want[:, 1]) > ES.TOL * mag[:, 1]) >= R - 2
    # a column is the single vector's product of that vector
    A, XT = data.inputs("D", 0)[0], data.vectors("V", 0)
    assert np.array_equal(want[:, 2], oracle.multiply("colwise", A, XT[2], 2))
    assert np.array_equal(mag[:, 2], np.abs(A) @ np.abs(XT[2]))


def test_checker_takes_a_block():
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    want, mag = data.want_multi("colwise", 3, ("D", 0), ("V", 0, 7))
    assert want.shape == mag.shape == (R, 7)
    assert ES.check_y(want.copy(), want, mag, True) == (True, 0.0)
    one = want.copy()
    one[5, 6] = np.nextafter(one[5, 6], np.inf)
    assert ES.check_y(one, want, mag, True) == (False, 1.0) and ES.check_y(one, want, mag, False)[0]
    off = want.copy()
    off[7, 3] += 2e-12 * mag[7, 3]
    ok, figure = ES.check_y(off, want, mag, False)
    assert not ok and 1.5e-12 < figure < 2.5e-12
    assert not ES.check_y(want[:, :6], want, mag, False)[0]              # a column short
    assert not ES.check_y(want[:, ::-1].copy(), want, mag, False)[0]     # the columns in another order


BLOCK_SCRIPTS = [(n, r) for n, r in ES.BLOCK_RUNS.items() if "again" not in n and n.split("/")[-1] not in ("ring3", "ring8")]


@pytest.mark.parametrize("name,run", BLOCK_SCRIPTS, ids=[n for n, _ in BLOCK_SCRIPTS])
def test_runner_walks_the_block_scripts_and_records_a_wrong_engine(name, run):
    R, Cn = 240, 3072
    data = ES.DataSets(R, Cn)
    script = run[0]
    n = ES.n_checks(script)
    blocks = [i for i, m in enumerate(ES.expect(script, "colwise", R, Cn, 3, 0)) if "vset" in m]
    for alg, world in (("colwise", 3), ("blockwise", 6), ("rowwise", 1)):
        for rank in {0, world - 1}:
            e = FakeEngine(alg, R, Cn, world, rank, data)
            recs = ES.run_script(e, script, data, world)
            assert len(recs) == n and all(r["ok"] for r in recs), recs
            assert all((r["y_ok"] is None) == (rank != 0) for r in recs)
            assert [c for c in e.calls if c in ("M", "MM", "C", "CM")] == [op[0] for op in script if op[0] in ("M", "MM", "C", "CM")]
        # one ulp in one element of Y: caught exactly where the model says exact mode is on
        recs = ES.run_script(FakeEngine(alg, R, Cn, world, 0, data, fault="one_ulp"), script, data, world)
        assert [r["ok"] for r in recs] == [not r["want_exact"] for r in recs]
        # the vector set before the current one: every CM after the script's second V or G is wrong
        recs = ES.run_script(FakeEngine(alg, R, Cn, world, 0, data, fault="stale_x"), script, data, world)
        first = next(op for op in script if op[0] in ES.VECTORS)
        later = [recs[i] for i in blocks if recs[i]["vset"] != "%s%d:%d" % first]
        assert not any(r["ok"] or r["y_ok"] for r in later), later
        assert len(recs) == n


def test_runner_catches_a_block_that_counts_is_timed_or_leaves_the_chunks():
    class NoData:
        token = np.zeros(1)

        def inputs(self, kind, i):
            return self.token, self.token

        def vectors(self, kind, j):
            return None

    # off the root the stand-in never looks at values: widths and launches alone
    alg = "colwise"
    R, Cn = ES.panel_shape(alg)
    panels = ES.BLOCK_PANEL_RUNS["blk_panels"][0]
    for fault, want_ok in ((None, True), ("mm_uses", False)):
        recs = ES.run_script(FakeEngine(alg, R, Cn, 2, 1, NoData(), fault=fault), panels, NoData(), 2)
        assert all(r["ok"] for r in recs) == want_ok
        assert [r["want_width"] for r in recs] == [256, 256, 0, 0, 256, 256, 0]
        if fault:  # S1 MM CM M C: the MM counted, so the first M already builds the copy
            assert [r["width"] for r in recs] == [256, 256, 0, 256, 256, 256, 0]
    for fault, launches in ((None, [1, 1, 1]), ("mm_timed", [2, 2, 3]), ("mm_keeps_chunks", [0, 0, 0])):
        recs = ES.run_script(FakeEngine(alg, 1200, 960, 2, 1, NoData(), fault=fault), ES.BLK_TIMED_CHUNKS, NoData(), 2)
        assert [r["want_launches"] for r in recs] == [1, 1, 1]
        assert [r["launches"] for r in recs] == launches
        assert all(r["ok"] for r in recs) == (fault is None)

