"""Op sequences for the engine (csrc/engine.cpp), a host model of what each must give, and the
runner that walks one on a Multiplier. Shared by tests/test_engine_scripts_host.py (CPU),
tests/test_gpu_engine_sequences.py and tests/test_gpu_engine_block_sequences.py (world 1, in
process) and tests/rank_worker_sequences.py (worlds 2, 3, 4 and 6 under torch.distributed.run).
Not collected by pytest.

A script is a tuple of ops that every rank walks identically:

  D(i)     distribute of data set i (root-send at more than one rank: A, x are None off the root)
  S(i)     distribute_shared of data set i (every rank makes the same A and x itself)
  F(i)     fill_synth with data set i's seed pair
  M        multiply
  C        collect and check
  X(on)    set_exact
  O(n)     set_overlap
  T(mode)  kernel_timing
  Y        sync
  V(j, nv) set_vectors with vector set j (the root passes X, the other ranks None and nv)
  G(j, nv) fill_synth_vectors with vector set j's seed
  MM       multiply_multi
  CM       collect_multi and check

Data set i is oracle.synth with seeds that depend on i (seeds(i)). Every write in a script uses
an i no earlier write of that script used, and the values of two sets differ in every element
but chance hits, so a stale A, x, panel copy or ring slot gives a y that is wrong in every row.
The sets that travel through the host (D, S) have their signs flipped (signed(), as in
tests/test_gpu_exact.py), with sign seeds for which the column split's combine orders differ
from a plain rank-order sum (tests/test_engine_scripts_host.py asserts it); F sets stay as the
generator gives them.

Vector set j is oracle.synth(NV_MAX, C, seed_of(j)).T, of which a V or G takes the first nv columns;
no script uses a j twice, so a stale X is wrong in every element. V sets have their signs flipped
with a seed of their own, G sets are the generator's: X[j, v] = mvg_synth_value(seed, v * C + j),
as include/matvec_gpu.h says of mvg_engine_fill_synth_vectors.
"""
from __future__ import annotations

import os
import time
from collections import OrderedDict

import numpy as np

ALGS = ("rowwise", "colwise", "blockwise")
TOL = 1e-12  # include/matvec_gpu.h: <= 1e-12 relative per element on non-negative data


# ------------------------------------------------------------------ ops
def D(i):
    return ("D", i)


def S(i):
    return ("S", i)


def F(i):
    return ("F", i)


def X(on):
    return ("X", int(bool(on)))


def O(n):  # noqa: E743
    return ("O", int(n))


def T(mode):
    return ("T", int(mode))


def V(j, nv):
    return ("V", int(j), int(nv))


def G(j, nv):
    return ("G", int(j), int(nv))


M, C, Y, MM, CM = ("M",), ("C",), ("Y",), ("MM",), ("CM",)
WRITES = ("D", "S", "F")
VECTORS = ("V", "G")
CHECKS = ("C", "CM")
NV_MAX = 11
# 7: exact mode's chains of 4 + 2 + 1 vectors; 11: a group of 8 and a group of 3
NVS = (1, 3, 7, 11)


def spell(script) -> str:
    """'X1 D0 V0:3 MM D1 M C CM': a script as the issue and the docstrings write it."""
    return " ".join(op[0] + ("%d:%d" % op[1:] if len(op) == 3 else str(op[1]) if len(op) == 2 else "") for op in script)


def n_checks(script) -> int:
    return sum(op[0] in CHECKS for op in script)


# ------------------------------------------------------------------ the scripts
# ring > 1 with different inputs in flight: exact mode gathers dy_parts[b] of three multiplies
# into the one gbuf on the exchange stream while the next distributions and GEMVs are issued.
# On a new engine its three multiplies use slots 0, 1, 2, or 0, 1, 0 of a ring of two: the y
# that is checked comes out of slot 0 there. So every ring length walks the script a second time
# on the same engine (b2b_again: multiplies 3, 4, 5 end in slot 1 of two, slot 5 of eight).
B2B_EXACT = (X(1), D(0), M, D(1), M, D(2), M, C)
# exact mode on a live engine, on and off and on again, then a write under a built panel copy
TOGGLE = (F(0), M, C, X(1), M, C, M, C, X(0), M, C, X(1), M, C, F(1), M, C, M, C)
# S1 S2 with no multiply between them: a second chunked write onto pending chunks; D4 after
# chunking: the root-send goes through drain_chunks
CHUNKED = (X(1), O(3), S(0), M, C, M, C, O(7), S(1), S(2), M, C, O(0), S(3), M, C, D(4), M, C)
# every writer after every other one; timing of either kind must not change y
MIXED_WRITERS = (O(2), S(0), F(1), M, C, D(2), M, X(1), M, C, T(1), M, M, C, T(-1), M, M, Y, D(3), M, C, T(0))
# run with the root-send staging lowered to SEND_PIECES_STAGE doubles: many pieces per peer,
# alternating the two staging buffers, a second send over the first one's buffers and events
SEND_PIECES = (D(0), M, C, X(1), D(1), M, M, C)
# more multiplies than ring slots, so the once-per-ring wait (slot 0) is taken with an exchange
# pending, in both modes, and a write lands behind a full ring
RING_WRAP = (D(0),) + (M,) * 9 + (C, X(1), D(1)) + (M,) * 9 + (C, D(2), M, C)
# per-launch timing skips exactly the multiplies that consume a chunked distribution
TIMED_CHUNKS = (O(3), T(1), S(0), M, M, C, S(1), M, C, T(0))

SEND_PIECES_STAGE = 5000

# name -> (script, environment for the engine's creation, staging in doubles or 0). Neighbours
# with the same environment and staging walk one engine, one after the other (groups(): creating
# an engine, the block split's communicator splits above all, costs more than walking a script);
# MVG_XRING=8 is the engine's own default.
SMALL_RUNS = OrderedDict([
    ("b2b_exact/ring1", (B2B_EXACT, {"MVG_XRING": "1"}, 0)),
    ("b2b_again/ring1", (B2B_EXACT, {"MVG_XRING": "1"}, 0)),
    ("b2b_exact/ring2", (B2B_EXACT, {"MVG_XRING": "2"}, 0)),
    ("b2b_again/ring2", (B2B_EXACT, {"MVG_XRING": "2"}, 0)),
    ("b2b_exact/ring8", (B2B_EXACT, {"MVG_XRING": "8"}, 0)),
    ("b2b_again/ring8", (B2B_EXACT, {"MVG_XRING": "8"}, 0)),
    ("toggle", (TOGGLE, {"MVG_XRING": "8"}, 0)),
    ("chunked", (CHUNKED, {"MVG_XRING": "8"}, 0)),
    ("mixed_writers", (MIXED_WRITERS, {"MVG_XRING": "8"}, 0)),
    ("ring_wrap", (RING_WRAP, {"MVG_XRING": "8"}, 0)),
    ("timed_chunks", (TIMED_CHUNKS, {"MVG_XRING": "8"}, 0)),
    ("send_pieces", (SEND_PIECES, {"MVG_XRING": "8"}, SEND_PIECES_STAGE)),
])


def with_shared(script):
    """The script with S in place of D (the panel shapes: no 200 MB root-send over sockets)."""
    return tuple(S(op[1]) if op[0] == "D" else op for op in script)


PANEL_RUNS = OrderedDict([
    ("toggle", (with_shared(TOGGLE), {"MVG_NO_PANELS": "0"}, 0)),
    ("chunked", (with_shared(CHUNKED), {"MVG_NO_PANELS": "0"}, 0)),
    ("chunked/no_panels", (with_shared(CHUNKED), {"MVG_NO_PANELS": "1"}, 0)),
])

# ---- a block of vectors (multiply_multi) beside the single vector. Both kinds of multiply share
# the slot counter, the ring's events and the exchange stream; the block has buffers of its own.
# Three exact blocks in flight with different A and X: blk.gathered is one buffer for every ring
# slot, and at more than one rank the root-send, the broadcast of X and the pending exchanges all
# use the world communicator with no sync between them. Walked twice per engine, as B2B_EXACT.
BLK_B2B_EXACT = (X(1), D(0), V(0, 3), MM, D(1), V(1, 3), MM, D(2), V(2, 3), MM, CM)
# M and MM in turn for more multiplies than the longest ring has slots, so slot 0 (the
# once-per-ring wait) falls on a multiply of one kind with an exchange of the other kind pending;
# ten multiplies, then the other kind first: at a ring of two the parity of the slots changes
# sides (tests/test_engine_scripts_host.py replays the slot counter)
BLK_MIXED_RING = ((D(0), V(0, 7)) + (M, MM) * 5 + (C, CM, X(1), D(1), V(1, 3)) + (MM, M) * 5 + (CM, C))
# the block grows (its buffers are freed and remade) with three block exchanges in flight, the slot
# counter runs on; a smaller block in the larger buffers; the first exact MM after tree-mode ones
BLK_GROW_IN_FLIGHT = (D(0), V(0, 3), MM, MM, MM, V(1, 11), MM, CM, V(2, 1), MM, CM, X(1), MM, CM, G(3, 7), MM, CM)
# a multiply_multi consumes a pending chunked distribution whole (drain_chunks), also a second
# chunked write over pending chunks, chunks that an M consumed, and whole writes afterwards
BLK_CHUNKED = (X(1), O(3), S(0), V(0, 7), MM, CM, M, C, O(7), S(1), S(2), MM, CM, S(3), M, MM, C, CM,
               O(0), S(4), MM, CM, D(5), MM, CM)
# an MM is never timed, and the M after it finds no chunks pending: a whole, timed multiply
BLK_TIMED_CHUNKS = (O(3), T(1), S(0), V(0, 3), MM, M, C, S(1), M, C, MM, CM, T(0))
# staging lowered to SEND_PIECES_STAGE: the root-send's many pieces, the broadcast of an 11-vector
# X and the block exchanges on one communicator, then both kinds of multiply behind one send
BLK_SEND_PIECES = (D(0), V(0, 11), MM, D(1), V(1, 11), MM, CM, X(1), D(2), MM, M, CM, C)
# every writer of A before an MM and V after G after V, in both modes
BLK_WRITERS = (F(0), G(0, 7), MM, CM, S(1), V(1, 3), MM, CM, D(2), G(2, 11), MM, CM, V(3, 11), MM, CM,
               X(1), F(3), MM, CM, G(4, 3), MM, CM, S(4), V(5, 7), MM, CM, D(5), MM, CM, G(6, 1), V(7, 1), MM, CM)
# the block beside a fresh panel copy and beside a stale one: it reads the row-major shard and is
# never a use (256 only where two M have run since the last write)
BLK_PANELS = (X(1), S(0), V(0, 3), M, M, C, MM, CM, S(1), MM, CM, M, C, M, C, MM, CM, X(0), MM, CM)

# The ring scripts come first in their group: the host test replays the slot counter from the
# engine's creation.
BLOCK_RUNS = OrderedDict([
    ("blk_b2b_exact/ring1", (BLK_B2B_EXACT, {"MVG_XRING": "1"}, 0)),
    ("blk_b2b_again/ring1", (BLK_B2B_EXACT, {"MVG_XRING": "1"}, 0)),
    ("blk_mixed_ring/ring2", (BLK_MIXED_RING, {"MVG_XRING": "2"}, 0)),
    ("blk_b2b_exact/ring2", (BLK_B2B_EXACT, {"MVG_XRING": "2"}, 0)),
    ("blk_b2b_again/ring2", (BLK_B2B_EXACT, {"MVG_XRING": "2"}, 0)),
    ("blk_mixed_ring/ring3", (BLK_MIXED_RING, {"MVG_XRING": "3"}, 0)),
    ("blk_mixed_ring/ring8", (BLK_MIXED_RING, {"MVG_XRING": "8"}, 0)),
    ("blk_b2b_exact/ring8", (BLK_B2B_EXACT, {"MVG_XRING": "8"}, 0)),
    ("blk_b2b_again/ring8", (BLK_B2B_EXACT, {"MVG_XRING": "8"}, 0)),
    ("blk_grow_in_flight", (BLK_GROW_IN_FLIGHT, {"MVG_XRING": "8"}, 0)),
    ("blk_chunked", (BLK_CHUNKED, {"MVG_XRING": "8"}, 0)),
    ("blk_timed_chunks", (BLK_TIMED_CHUNKS, {"MVG_XRING": "8"}, 0)),
    ("blk_writers", (BLK_WRITERS, {"MVG_XRING": "8"}, 0)),
    ("blk_send_pieces", (BLK_SEND_PIECES, {"MVG_XRING": "8"}, SEND_PIECES_STAGE)),
])

# On the panel shapes the chunked copy of a 200 MB shard takes milliseconds. A build whose
# multiply_multi did not wait for the chunks still passed these at world 2, from pageable and from
# page-locked host arrays (MEASUREMENTS §14); it failed blk_chunked's S1 S2 MM CM at world 1.
BLOCK_PANEL_RUNS = OrderedDict([
    ("blk_panels", (with_shared(BLK_PANELS), {"MVG_NO_PANELS": "0"}, 0)),
    ("blk_chunked", (with_shared(BLK_CHUNKED), {"MVG_NO_PANELS": "0"}, 0)),
])

# Shapes that divide by 2, 3, 4 and 6 in every split. The column split's partial is R doubles:
# 240 * 8 = 1920 B <= 2 KiB takes MPICH's binomial reduce, 1200 * 8 B its reduce-scatter + gather.
SMALL_SHAPES = ((240, 3072), (1200, 960))
WORLDS = (1, 2, 3, 4, 6)
# World 2 only: every rank's shard is 6160 x 4098 (200 MB), which exact mode keeps in column
# panels (mvg_exact_panel_width > 0, with a column tail of 2).
PANEL_WORLD = 2
PANEL_SHARD = (6160, 4098)


def panel_shape(alg):
    return (12320, 4098) if alg == "rowwise" else (6160, 8196)


# ------------------------------------------------------------------ data sets
SIGN_SEED = 20260
VSIGN_SEED = 30260


def seeds(i):
    """(seed of A, seed of x) of data set i; 42 / 4242, the package's defaults, are set 0's."""
    return 42 + 2 * i, 4242 + 2 * i


def seed_of(j):
    """Seed of vector set j; 777 is tests/rank_worker_multi.py's."""
    return 777 + 2 * j


def signed(A, seed):
    """tests/test_gpu_exact.py signed(): mixed signs from a seeded generator."""
    rng = np.random.default_rng(seed)
    return A * rng.choice([-1.0, 1.0], size=A.shape)


class DataSets:
    """A, x and the oracle's y of the data sets of one R x C shape, made once and shared by every
    script and algorithm that needs them (keep: how many sets stay in memory)."""

    def __init__(self, R, Cn, keep=64):
        self.R, self.C, self.keep = R, Cn, keep
        self._inputs = OrderedDict()
        self._want = {}
        self._vectors = {}
        self._want_col = {}

    def vectors(self, kind, j):
        """Vector set j as NV_MAX rows of C (vector v is row v, contiguous: what set_vectors hands
        the engine without a copy when it is given the transpose of the first nv rows). kind
        'G': the generator's values; 'V': the same with flipped signs."""
        from oracle import oracle

        key = ("G" if kind == "G" else "V", j)
        if key not in self._vectors:
            XT = oracle.synth(NV_MAX, self.C, seed_of(j))
            self._vectors[key] = signed(XT, VSIGN_SEED + j) if key[0] == "V" else XT
        return self._vectors[key]

    def want_multi(self, alg, world, aset, vset):
        """(oracle.multiply at `world` ranks per column, |A|·|x_v| per row and column), both
        R x nv, of A set aset = (kind, i) and vector set vset = (kind, j, nv)."""
        from oracle import oracle

        akey = ("F" if aset[0] == "F" else "H", aset[1])
        vkey = ("G" if vset[0] == "G" else "V", vset[1])
        cols = []
        for v in range(vset[2]):
            key = (alg, world, akey, vkey, v)
            if key not in self._want_col:
                A, XT = self.inputs(*aset)[0], self.vectors(*vset[:2])
                self._want_col[key] = (oracle.multiply(alg, A, XT[v], world), np.abs(A) @ np.abs(XT[v]))
            cols.append(self._want_col[key])
        return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)

    def inputs(self, kind, i):
        """kind 'F': the generator's values; 'D' / 'S': the same with flipped signs."""
        from oracle import oracle

        key = ("F" if kind == "F" else "H", i)
        if key not in self._inputs:
            sa, sx = seeds(i)
            A, x = oracle.synth(self.R, self.C, sa), oracle.synth(1, self.C, sx)[0]
            if key[0] == "H":
                A, x = signed(A, SIGN_SEED + 2 * i), signed(x, SIGN_SEED + 2 * i + 1)
            self._inputs[key] = (A, x)
            while len(self._inputs) > self.keep:
                self._inputs.popitem(last=False)
        self._inputs.move_to_end(key)
        return self._inputs[key]

    def want(self, alg, world, kind, i):
        """(oracle.multiply at `world` ranks, |A|·|x| per row) of the set."""
        from oracle import oracle

        key = (alg, world, "F" if kind == "F" else "H", i)
        if key not in self._want:
            A, x = self.inputs(kind, i)
            self._want[key] = (oracle.multiply(alg, A, x, world), np.abs(A) @ np.abs(x))
        return self._want[key]


# ------------------------------------------------------------------ the host model
def well_formed(script):
    """A write before the first M, every C after an M (with no write in between: the y a C
    checks is the last multiply's), and no data set written twice. The block alike: a write and a
    V or G before the first MM, every CM after an MM with no V, G or write in between, no vector
    set used twice, and nv one of NVS."""
    written, multiplied, used = False, False, set()
    vectors, multi, vused = False, False, set()
    for op in script:
        if op[0] in WRITES:
            if op[1] in used:
                return False
            used.add(op[1])
            written, multiplied, multi = True, False, False
        elif op[0] in VECTORS:
            if op[1] in vused or op[2] not in NVS:
                return False
            vused.add(op[1])
            vectors, multi = True, False
        elif op[0] == "M":
            if not written:
                return False
            multiplied = True
        elif op[0] == "MM":
            if not (written and vectors):
                return False
            multi = True
        elif op[0] == "C" and not multiplied:
            return False
        elif op[0] == "CM" and not multi:
            return False
    return True


def expect(script, alg, R, Cn, world, rank, no_panels=False):
    """What every C of the script must see on `rank`, from the engine's rules alone (no device):
    a list of {"set": (kind, i), "exact": bool, "width": int, "launches": int or None}.

    set: the last write before the C.

    width, what exact_panel_width() must report. The engine's rule (csrc/engine.cpp):
      - set_exact(1) gives a shard its panel width W = mvg_exact_panel_width(n_rows, n_cols),
        0 with MVG_NO_PANELS=1, and marks the copy not built; set_exact(0) releases the copy;
      - begin_write, which opens every D, S and F, marks the copy stale and restarts the count
        of multiplies since the write (uses = 0);
      - refresh_panels, at the start of each multiply, builds the copy when exact mode is on,
        W > 0, the copy is not fresh, at least one multiply has run since the last write
        (uses >= 1) and no chunked distribution is pending; the multiply then counts (uses += 1)
        and consumes any pending chunks. So the first multiply after a write always runs the
        row-major kernels (a chunked write's GEMVs run behind its copies there), and the second
        is the earliest that runs on panels; switching exact mode on over a shard that has been
        multiplied since its last write builds the copy at the next multiply.
      The width reported is W while the copy is fresh and exact mode is on, else 0.

    launches, for T(1): the multiplies since the T that did not consume a chunked distribution
    (pool_enter times every other one; kernel_ms() collects them). None in the other modes.
    A write is chunked when an overlap > 1 is set, the shard has at least 2 rows per chunk and
    the write is an S, or a D with every rank in one process (world 1); F and the root-send D
    drain the pending chunks instead.

    The list has one entry per C and per CM, in script order. A CM's entry is {"set", "vset":
    (kind, j, nv), "exact", "width", "launches"}: set and exact are the A set and the mode at the
    last MM (collect_multi returns that multiply's Y), vset the vector set then current; width
    and launches are what the engine reports at the CM, as at a C. The block's rules
    (mvg_engine_multiply_multi): an MM reads the row-major shard and is no use of A (uses and the
    copy's freshness stay), is never timed, and consumes a pending chunked distribution whole
    (drain_chunks), so the M after it is a whole, timed multiply. V and G change the current
    vector set and nothing else."""
    from matvec_mpi_multiplier_amd import _lib
    from matvec_mpi_multiplier_amd import multiplier as mm

    sh = mm.plan_shard(alg, R, Cn, world, rank)
    W = 0 if no_panels else int(_lib.lib.mvg_exact_panel_width(sh.n_rows, sh.n_cols))
    exact = fresh = pending = False
    uses = overlap = timing = launches = 0
    cur, vcur, block, out = None, None, None, []
    for op in script:
        k = op[0]
        if k in WRITES:
            cur, fresh, uses = (k, op[1]), False, 0
            direct = k == "S" or (k == "D" and world == 1)
            pending = direct and overlap > 1 and sh.n_rows >= 2 * overlap
        elif k in VECTORS:
            vcur = op
        elif k == "M":
            if exact and W and not fresh and uses >= 1 and not pending:
                fresh = True
            if timing == 1 and not pending:
                launches += 1
            uses += 1
            pending = False
        elif k == "MM":
            block = {"set": cur, "vset": vcur, "exact": exact}
            pending = False
        elif k == "X":
            exact = bool(op[1])
            if not exact:
                fresh = False
        elif k == "O":
            overlap = op[1]
        elif k == "T":
            timing, launches = op[1], 0
        elif k == "C":
            out.append({"set": cur, "exact": exact, "width": W if exact and fresh else 0,
                        "launches": launches if timing == 1 else None})
        elif k == "CM":
            out.append(dict(block, width=W if exact and fresh else 0, launches=launches if timing == 1 else None))
    return out


def slots(script, ring):
    """The ring slot of every multiply of a script walked on a new engine with an exchange (more
    than one rank, or forced collectives), as the root counts (multiply_step): a list of (kind,
    slot, the previous multiply's kind or None, waits). Both kinds take slot nx % ring of one
    counter. waits: the once-per-ring wait is taken, which needs slot 0, a ring longer than one
    and an exchange pending (x_pending: every multiply sets it, mvg_engine_sync clears it, and
    X, O, T, Y and a check under per-launch timing synchronise)."""
    nx, pending, timing, prev, out = 0, False, 0, None, []
    for op in script:
        k = op[0]
        if k in ("M", "MM"):
            b = nx % ring
            out.append((k, b, prev, ring > 1 and pending and b == 0))
            pending, prev, nx = ring > 1, k, nx + 1
        elif k in ("X", "O", "T", "Y") or (k in CHECKS and timing == 1):
            pending = False
        if k == "T":
            timing = op[1]
    return out


# ------------------------------------------------------------------ the comparison
def check_y(y, want, mag, exact):
    """(ok, figure). Exact mode: np.array_equal, figure = rows that differ. Otherwise
    |y - want| <= 1e-12 * (|A|·|x|) per row, the header's 1e-12 bar on the uncancelled magnitude
    (the relative bar itself on non-negative data); figure = max |y - want| / (|A|·|x|)."""
    y = np.asarray(y, dtype=np.float64)
    if y.shape != want.shape:
        return False, -1.0
    if exact:
        return bool(np.array_equal(y, want)), float(np.count_nonzero(~(y == want)))
    err = np.abs(y - want)
    ok = bool(np.all(err <= TOL * mag))  # a NaN in y compares false
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(mag > 0, err / mag, np.where(err > 0, np.inf, 0.0))
    return ok, float(np.max(ratio)) if ratio.size else 0.0


# ------------------------------------------------------------------ the runner
def groups(runs):
    """[(names, environment, staging)]: neighbouring runs that share an engine."""
    out = []
    for name, (_, env, stage) in runs.items():
        if out and out[-1][1:] == (env, stage):
            out[-1][0].append(name)
        else:
            out.append(([name], env, stage))
    return out


SET_STRIDE = 10  # the k-th script of a group writes data sets 10 k + i


def join(names, runs):
    """(script, owners): the named scripts one after the other for one engine, with X0 O0 T0
    between two of them (every script starts from the modes a new engine has) and data sets
    and vector sets that no earlier script of the group wrote; owners[n] = (name, check) of the
    n-th C or CM."""
    ops, owners = [], []
    for k, name in enumerate(names):
        if k:
            ops += [X(0), O(0), T(0)]
        checks = 0
        for op in runs[name][0]:
            ops.append((op[0], op[1] + SET_STRIDE * k) + op[2:] if op[0] in WRITES + VECTORS else op)
            if op[0] in CHECKS:
                owners.append((name, checks))
                checks += 1
    return tuple(ops), owners


def run_script(e, script, data, world, no_panels=False):
    """Walks the script on Multiplier `e`. Per C and per CM one record: the model's answers
    (want_*), what the engine reported, and on the root the comparison of y with the oracle (at a
    CM every column of Y with oracle.multiply of that vector; off the root Y is None and the
    engine's vector count is the set's nv). A CM's "exact" is the mode the engine reported right
    after the last MM. A failed check is recorded ("ok": False), never raised: the rank keeps
    walking, so no peer is left inside a collective."""
    sh = e.shard(0)
    rank, root = sh.rank, e.is_root()
    model = expect(script, e.name, e.R, e.C, world, rank, no_panels)
    # alive: every host array an engine call was handed (D, S, V) until the next op that
    # synchronises, since a copy out of it may still be queued; the wrapper keeps only the last
    timing, alive, records, block_exact = 0, [], [], None
    for op in script:
        k = op[0]
        if k == "D":
            A, x = data.inputs("D", op[1]) if root else (None, None)
            alive.append((A, x))
            e.distribute(A, x)
        elif k == "S":
            A, x = data.inputs("S", op[1])
            alive.append((A, x))
            e.distribute_shared(A, x)
        elif k == "F":
            e.fill_synth(*seeds(op[1]))
        elif k == "M":
            e.multiply()
        elif k == "X":
            e.set_exact(bool(op[1]))
        elif k == "O":
            e.set_overlap(op[1])
        elif k == "T":
            timing = op[1]
            e.kernel_timing(timing)
        elif k == "Y":
            e.sync()
        elif k == "C":
            m = model[len(records)]
            y = e.collect()
            rec = {"check": len(records), "rank": rank, "set": "%s%d" % m["set"], "want_exact": m["exact"],
                   "exact": e.exact, "want_width": m["width"], "width": e.exact_panel_width(),
                   "want_launches": m["launches"], "launches": e.kernel_ms().launches if timing == 1 else None,
                   "y_ok": None, "figure": None}
            if root:
                want, mag = data.want(e.name, world, *m["set"])
                rec["y_ok"], rec["figure"] = check_y(y, want, mag, m["exact"])
            rec["ok"] = (rec["exact"] == rec["want_exact"] and rec["width"] == rec["want_width"]
                         and rec["launches"] == rec["want_launches"] and rec["y_ok"] is not False)
            rec["t"] = time.perf_counter()
            records.append(rec)
            alive.clear()  # collect has synchronised: no copy still reads the host arrays
        elif k == "V":
            XT = data.vectors("V", op[1])
            alive.append(XT)
            e.set_vectors(XT[:op[2]].T if root else None, op[2])
        elif k == "G":
            e.fill_synth_vectors(seed_of(op[1]), op[2])
        elif k == "MM":
            e.multiply_multi()
            block_exact = e.exact
        elif k == "CM":
            m = model[len(records)]
            nv = m["vset"][2]
            Yb = e.collect_multi()
            rec = {"check": len(records), "rank": rank, "set": "%s%d" % m["set"], "vset": "%s%d:%d" % m["vset"],
                   "want_exact": m["exact"], "exact": block_exact, "want_width": m["width"],
                   "width": e.exact_panel_width(), "want_launches": m["launches"],
                   "launches": e.kernel_ms().launches if timing == 1 else None, "y_ok": None, "figure": None,
                   "vectors": e.vectors}
            if root:
                want, mag = data.want_multi(e.name, world, m["set"], m["vset"])
                rec["y_ok"], rec["figure"] = check_y(Yb, want, mag, m["exact"]) if Yb is not None else (False, -1.0)
            rec["ok"] = (rec["exact"] == rec["want_exact"] and rec["width"] == rec["want_width"]
                         and rec["launches"] == rec["want_launches"] and rec["y_ok"] is not False
                         and rec["vectors"] == nv and (root or Yb is None))
            rec["t"] = time.perf_counter()
            records.append(rec)
            alive.clear()
        if k in ("X", "O", "T", "Y"):
            alive.clear()  # each of them synchronises every stream of the engine
    return records


class environment:
    """os.environ entries for the duration of a block (the engine reads them at creation and at
    set_exact), put back afterwards."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_group(comm, alg, R, Cn, group, runs, data, world):
    """One engine for one (algorithm, shape, group of runs): the records of its scripts, each
    tagged with its case and with the script's wall time on this rank (the engine's creation
    counts with the group's first script)."""
    from matvec_mpi_multiplier_amd import _lib
    from matvec_mpi_multiplier_amd import multiplier as mm

    names, env, stage = group
    script, owners = join(names, runs)
    t0 = time.perf_counter()
    try:
        _lib.check(_lib.lib.mvg_debug_set_stage_elems(stage), "mvg_debug_set_stage_elems")
        with environment(env):
            with mm.Multiplier(alg, R, Cn, comm) as e:
                records = run_script(e, script, data, world, no_panels=env.get("MVG_NO_PANELS") == "1")
    finally:
        _lib.lib.mvg_debug_set_stage_elems(0)
    ends = {}
    for rec, (name, check) in zip(records, owners):
        rec.update(world=world, alg=alg, R=R, C=Cn, script=name, check=check)
        ends[name] = rec.pop("t")
    for rec in records:
        before = [t for n, t in ends.items() if t < ends[rec["script"]]]
        rec["secs"] = round(ends[rec["script"]] - max(before + [t0]), 3)
    return records


def small_cases():
    """(alg, R, C, name) of one small-shape launch, in the order every rank runs them."""
    return [(alg, R, Cn, name) for R, Cn in SMALL_SHAPES for alg in ALGS for name in SMALL_RUNS]


def panel_cases():
    return [(alg,) + panel_shape(alg) + (name,) for alg in ALGS for name in PANEL_RUNS]


def block_cases():
    return [(alg, R, Cn, name) for R, Cn in SMALL_SHAPES for alg in ALGS for name in BLOCK_RUNS]


def block_panel_cases():
    return [(alg,) + panel_shape(alg) + (name,) for alg in ALGS for name in BLOCK_PANEL_RUNS]


def run_cases(comm, world, shapes, runs, emit, keep=64):
    """Every (algorithm, shape, group) in order on this rank; shapes: [(alg, R, C)]. emit(record)
    per check. True when every check held."""
    ok, data = True, None
    for alg, R, Cn in shapes:
        if data is None or (data.R, data.C) != (R, Cn):
            data = DataSets(R, Cn, keep)  # the previous shape's sets are released
        for group in groups(runs):
            for rec in run_group(comm, alg, R, Cn, group, runs, data, world):
                ok &= rec["ok"]
                emit(rec)
    return ok


def small_shapes(algs=ALGS):
    return [(alg, R, Cn) for R, Cn in SMALL_SHAPES for alg in algs]


def panel_shapes(algs=ALGS):
    return [(alg,) + panel_shape(alg) for alg in algs]
