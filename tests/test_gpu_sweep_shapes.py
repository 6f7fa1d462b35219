"""The reference's published sweep on the device, shard by shard, and the picks it misses.

Every (size, algorithm, P) of tests/sweep_shapes.py: 19 sizes x 3 algorithms x P in 1, 2, 6, 12,
24. For every rank of a combination the shard the planner gives it is filled on the device from
its global offsets (mvg_synth_fill_device, as mvg_engine_fill_synth does; nothing is uploaded)
and multiplied

  * by the automatic tree kernel (mvg_gemv) into a NaN-guarded y image (tests/gpu_guarded.py);
    once per distinct shard shape the dispatch's own pick, launched by number, must give the
    same bits (so the shape did run the kernel tests/test_sweep_shapes_host.py names);
  * by mvg_gemv_exact into slot r of one guarded buffer of P partials, and where exact mode
    keeps a column-panel copy (mvg_exact_panel_width) also through mvg_panel_relayout and
    mvg_gemv_exact_panels: the same bits.

The exact partials are combined on the device by the engine's combine kernels
(mvg_debug_combine_mpich for the column split, mvg_debug_combine_grid_rows for the block split;
the row split's gathered buffer is y) and y must be oracle.multiply(alg, A, x, P) bit for bit,
every row. The synthetic data separates the orders: at 600^2 about 530 of the 600 rows differ
between P = 1 and any P > 1. The tree partials, summed on the host where the exchange sums them,
must be within 1e-12 relative per element (non-negative data). At P = 1 the engine itself runs
the same sequence as test_full_size_whole_y_against_oracle.

The ranks run from the last to the first: a store past a partial's last row lands in the next
slot, which is already written, and shows in the comparison. A combination's launches queue on
one stream and its images are read back once; the oracle's y is computed on the CPU meanwhile.

EXTRAS: one shape per pick of the tree dispatch that no shard of the sweep reaches (and one just
under a boundary), kernel level, against oracle.multiply_std_rowwise.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gpu_guarded as G
import sweep_shapes as S
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
TOL = 1e-12  # relative per element, non-negative data (BASELINE north star; tests/test_gpu_parity.py)


def sync():
    _lib.check(lib.mvg_stream_sync(None), "sync")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def max_rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))


# ------------------------------------------------------------------ per-size state
_pool = ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0)))))  # the oracle (ctypes releases the GIL)
_inputs = {}  # (R, C) -> future of the host (A, x): the size in use and the next one


def host_inputs(R, C):
    if (R, C) not in _inputs:
        _inputs[R, C] = _pool.submit(lambda: (oracle.synth(R, C, mm.SEED_A), oracle.synth(1, C, mm.SEED_X)[0]))
    return _inputs[R, C]


class Size:
    """Host A and x of one published size, the oracle's y of its 15 combinations (computed once
    each, on the CPU beside the device work, in the order the cases run) and the device buffers
    every shard of it is filled into: A at the start of its own allocation, so every shard is
    line-aligned as the engine's shards are and the automatic dispatch is mvg_gemv_auto_variant's."""

    def __init__(self, R, C):
        self.R, self.C = R, C
        self.A, self.x = host_inputs(R, C).result()
        self.want = {(alg, P): _pool.submit(oracle.multiply, alg, self.A, self.x, P) for alg in S.ALGS for P in S.PS}
        i = S.SIZES.index((R, C))
        if i + 1 < len(S.SIZES):
            host_inputs(*S.SIZES[i + 1])
        self.dA, self.dx = mm.DeviceBuffer(R * C), mm.DeviceBuffer(C)
        self.dAp = None

    def panels(self, n):
        if self.dAp is None or self.dAp.n < n:
            if self.dAp is not None:
                self.dAp.free()
            self.dAp = mm.DeviceBuffer(n)
        return self.dAp

    def free(self):
        for f in self.want.values():
            f.cancel()
        _inputs.pop((self.R, self.C), None)
        for b in (self.dA, self.dx, self.dAp):
            if b is not None:
                b.free()


_current = []        # the one Size alive (the cases are ordered size-major)
_variant_checked = set()  # shard shapes whose pick has been launched by number


def drop_size():
    while _current:
        _current.pop().free()


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    drop_size()
    for f in _inputs.values():
        f.cancel()
    _inputs.clear()


def size_state(R, C):
    if not _current or (_current[0].R, _current[0].C) != (R, C):
        drop_size()
        _current.append(Size(R, C))
    return _current[0]


@pytest.fixture(scope="module")
def comm1():
    c = mm.Comm.init_all([0])
    yield c
    c.destroy()


# ------------------------------------------------------------------ one operand, every check
def fill(dA, dx, m, k, row_off, col_off, C):
    """The shard [row_off, +m) x [col_off, +k) of the global matrix (C columns) packed at dA
    (lda = k) and its x segment at dx: mvg_engine_fill_synth's two calls."""
    _lib.check(lib.mvg_synth_fill_device(dA.ptr, k, m, k, row_off, col_off, C, mm.SEED_A, None), "fill A")
    _lib.check(lib.mvg_synth_fill_device(dx.ptr, k, 1, k, 0, col_off, C, mm.SEED_X, None), "fill x")


def guarded_run(dy, call, what):
    """One launch into the NaN-filled image dy; nothing outside its payload may change."""
    dy.fill()
    _lib.check(call(dy.ptr), what)
    sync()
    img = dy.image()
    bad = G.violations(img, dy.lay)
    assert not bad, (what, bad[:4])
    return dy.lay.payload(img)[0]


def pick_by_number_gives_the_same_bits(dA, dx, dyt, r, dy, m, k):
    """Once per shape: the dispatch's own pick (mvg_gemv_auto_variant, named on the CPU in
    tests/test_sweep_shapes_host.py), launched by number into dy, against the automatic call's
    result in vector r of dyt."""
    v = lib.mvg_gemv_auto_variant(k, m, k)
    name = lib.mvg_gemv_variant_name(v).decode()
    assert v > 0 and name == S.tree_pick(m, k)
    yv = guarded_run(dy, lambda p: lib.mvg_gemv_variant(dA.ptr, k, dx.ptr, p, m, k, v, None), f"{name} {m}x{k}")
    y = np.empty(m)
    _lib.check(lib.mvg_memcpy_d2h(y.ctypes.data, dyt.ptr + 8 * r * dyt.lay.ld, 8 * m, None), "d2h")
    sync()
    assert np.array_equal(bits(y), bits(yv)), (m, k, name, np.flatnonzero(bits(y) != bits(yv))[:8])
    _variant_checked.add((m, k))


def panel_product(dA, dx, dAp, dy, m, k, P):
    """The exact product over the column-panel copy of the packed operand."""
    npan = -(-k // P)
    assert dAp.n >= npan * m * P
    _lib.check(lib.mvg_panel_relayout(dA.ptr, k, m, k, dAp.ptr, m * P, P, None), "mvg_panel_relayout")
    return guarded_run(dy, lambda p: lib.mvg_gemv_exact_panels(dAp.ptr, m * P, P, dx.ptr, p, m, k, 0, None),
                       f"mvg_gemv_exact_panels {m}x{k} P={P}")


# ------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("R,C,alg,P", S.combos())
def test_published_sweep_shard_by_shard(comm1, R, C, alg, P):
    st = size_state(R, C)
    shards = S.shards(R, C, alg, P)
    n = shards[0].y_len
    assert all(s.y_len == n == s.n_rows for s in shards)  # every partial is one slot long
    # the tree partials: vector r of one guarded image, 3 NaN rows and a spare vector behind each
    # payload; the launches of a combination queue on one stream and are read back once
    dyt = G.result(P, n, n + 3, spare=1)
    dy = G.result(1, n, n + 3, spare=1)  # the pick by number, the panel product
    parts = G.result(P, n, n)  # the gathered buffer: P partials of n doubles, contiguous
    dyc = G.result(1, R, R)
    try:
        panel_y = {}
        for s in reversed(shards):
            m, k, r = s.n_rows, s.n_cols, s.rank
            fill(st.dA, st.dx, m, k, s.row_off, s.col_off, C)
            _lib.check(lib.mvg_gemv(st.dA.ptr, k, st.dx.ptr, dyt.ptr + 8 * r * (n + 3), m, k, None), "mvg_gemv")
            if (m, k) not in _variant_checked:
                pick_by_number_gives_the_same_bits(st.dA, st.dx, dyt, r, dy, m, k)
            # exact: slot r of the gathered buffer
            slot = parts.ptr + 8 * r * n
            _lib.check(lib.mvg_gemv_exact(st.dA.ptr, k, st.dx.ptr, slot, m, k, None), "mvg_gemv_exact")
            pw = lib.mvg_exact_panel_width(m, k)
            assert (pw > 0) == ((m, k) in S.PANEL_SHARDS)
            if pw > 0:
                panel_y[r] = panel_product(st.dA, st.dx, st.panels(-(-k // pw) * m * pw), dy, m, k, pw)
        sync()
        img = dyt.image()
        bad = G.violations(img, dyt.lay)
        assert not bad, (R, C, alg, P, "mvg_gemv", bad[:4])
        tree = np.zeros(R)  # summed on the host where the exchange sums (the row split only gathers)
        for s, part in zip(shards, dyt.lay.payload(img)):
            tree[s.y_off:s.y_off + n] += part
        img = parts.image()
        assert not G.violations(img, parts.lay), (R, C, alg, P)
        gathered = parts.lay.payload(img)
        assert np.isfinite(gathered).all(), (R, C, alg, P)  # every slot written
        for r, yp in panel_y.items():
            assert np.array_equal(bits(yp), bits(gathered[r])), (R, C, alg, P, "rank", r, "panel copy differs from row-major")
        want = st.want[alg, P].result()
        if P == 1 or alg == "rowwise":
            y = gathered.reshape(-1)
        else:
            if alg == "colwise":
                rc = lib.mvg_debug_combine_mpich(parts.ptr, P, R, dyc.ptr, None)
            else:
                gr, gc = shards[0].grid_rows, shards[0].grid_cols
                assert gr * n == R
                rc = lib.mvg_debug_combine_grid_rows(parts.ptr, gr, gc, n, dyc.ptr, None)
            _lib.check(rc, "combine")
            sync()
            img = dyc.image()
            assert not G.violations(img, dyc.lay), (R, C, alg, P)
            assert not G.violations(parts.image(), parts.lay), (R, C, alg, P)  # overwritten in place only
            y = dyc.lay.payload(img)[0]
        wrong = np.flatnonzero(bits(y) != bits(want))
        assert wrong.size == 0, (R, C, alg, P, "exact y differs in", wrong.size, "rows, first", wrong[:8])
        assert max_rel(tree, want) <= TOL, (R, C, alg, P, max_rel(tree, want))
    finally:
        for g in (dyt, dy, parts, dyc):
            g.free()
    if P == 1:
        with mm.Multiplier(alg, R, C, comm1) as e:
            e.fill_synth()
            e.multiply()
            y_tree = e.collect()
            e.set_exact(True)
            e.multiply()
            y_rm = e.collect()
            e.multiply()
            y_2 = e.collect()
            width = e.exact_panel_width()
        assert max_rel(y_tree, want) <= TOL, (R, C, alg, max_rel(y_tree, want))
        np.testing.assert_array_equal(bits(y_rm), bits(want))
        np.testing.assert_array_equal(bits(y_2), bits(want))
        assert width == (256 if R == C and R >= 6600 else 0), (R, C, alg, width)


# ------------------------------------------------------------------ the picks the sweep misses
def oracle_rows(m, k, x, block_bytes=64 << 20):
    """oracle.multiply_std_rowwise of the synthetic m x k matrix, generated and summed in row
    blocks on the allowed CPUs (ctypes releases the GIL): A is never held whole."""
    y = np.empty(m)
    rows = max(1, block_bytes // (8 * k))

    def block(r0):
        nr = min(rows, m - r0)
        y[r0:r0 + nr] = oracle.multiply_std_rowwise(oracle.synth_block(r0, nr, 0, k, k, mm.SEED_A), x)

    with ThreadPoolExecutor(max_workers=max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        list(ex.map(block, range(0, m, rows)))
    return y


@pytest.mark.parametrize("m,k,pick", S.EXTRAS)
def test_picks_the_sweep_misses_at_their_smallest_shapes(m, k, pick):
    drop_size()  # the sweep's last size is done with
    assert S.tree_pick(m, k) == pick and lib.mvg_exact_panel_width(m, k) == 0
    x = oracle.synth(1, k, mm.SEED_X)[0]
    want = oracle_rows(m, k, x)
    dA, dx = mm.DeviceBuffer(m * k), mm.DeviceBuffer(k)
    dy = G.result(1, m, m + 3, spare=1)
    try:
        fill(dA, dx, m, k, 0, 0, k)
        dyt = G.result(1, m, m + 3, spare=1)
        try:
            y = guarded_run(dyt, lambda p: lib.mvg_gemv(dA.ptr, k, dx.ptr, p, m, k, None), f"mvg_gemv {m}x{k}")
            pick_by_number_gives_the_same_bits(dA, dx, dyt, 0, dy, m, k)
        finally:
            dyt.free()
        assert max_rel(y, want) <= TOL, (m, k, pick, max_rel(y, want))
        ye = guarded_run(dy, lambda p: lib.mvg_gemv_exact(dA.ptr, k, dx.ptr, p, m, k, None), f"mvg_gemv_exact {m}x{k}")
        wrong = np.flatnonzero(bits(ye) != bits(want))
        assert wrong.size == 0, (m, k, "exact y differs in", wrong.size, "rows, first", wrong[:8])
    finally:
        for b in (dA, dx, dy):
            b.free()
