"""The engine's block-of-vectors calls (set_vectors / fill_synth_vectors / multiply_multi /
collect_multi) against the oracle, walked by every rank of a world. Run under
torch.distributed.run it is the worker of tests/test_gpu_engine_multi.py (worlds 2, 4 and 6, every
rank on GPU 0 with a distinct NCCL_HOSTID and loopback sockets, as tests/rank_worker_sequences.py);
imported, run_world() walks the same cases in process (world 1). Not collected by pytest.

One launch walks all three algorithms. Per (algorithm, shape) one engine; per mode (tree, exact)
and nv in NVS: distribute(A, x), set_vectors(X), multiply_multi(), collect_multi(), and on the root
every column against oracle.multiply(alg, A, X[:, v], world): np.array_equal in exact mode (signed
data, so the order of summation shows in the bits; the block split at 3 grid columns is held to
rank order), <= 1e-12 relative in tree mode on the generator's non-negative values. Then, once per
algorithm on the first shape, the checks named in EXTRAS.

Here every load() follows a collect_multi, so it starts on idle streams. Everything
sequence-shaped — blocks in flight with different A and X, both kinds of multiply around the
ring, a block that grows with exchanges pending, chunked distribution, lowered root-send staging,
panel shards, 3 ranks — is walked by the op-sequence scripts instead (BLOCK_RUNS and
BLOCK_PANEL_RUNS in tests/engine_scripts.py, tests/test_gpu_engine_block_sequences.py).

Every rank prints one JSON line per check and a last line {"done": true, ...}. A failed check is
recorded and the rank walks on, so no peer is left inside a collective; the exit status is 1 if any
check of this rank failed.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

ALGS = ("rowwise", "colwise", "blockwise")
# both divide by 1, 2, 4 and 6 and by the 2 x 2 and 2 x 3 grids. The column split's partial is R
# doubles: 240 * 8 B is under MPICH's 2 KiB switch (binomial tree), 624 * 8 B over it
# (reduce-scatter + gather); 1260 / 4 = 315 columns: odd-width strips, 1536: aligned ones
SHAPES = ((240, 1260), (624, 1536))
NVS = (1, 3, 8, 11)
NV_MAX = 11
TOL = 1e-12
EXTRAS = ("ring_wrap", "single_before", "single_kept", "single_after", "grow", "synth", "toggle_tree", "toggle_exact",
          "panel_width", "launches_per_launch", "launches_span")


def signed(A, seed):
    return A * np.random.default_rng(seed).choice([-1.0, 1.0], size=A.shape)


class Data:
    """A, x, X (C x NV_MAX) of one shape, plain (the generator's non-negative values) and signed,
    and the oracle's y per vector, made when first asked for."""

    def __init__(self, R, Cn):
        from oracle import oracle

        self.R, self.C, self.oracle = R, Cn, oracle
        A, x, X = oracle.synth(R, Cn, 42), oracle.synth(1, Cn, 4242)[0], oracle.synth(NV_MAX, Cn, 777).T.copy()
        self.sets = {False: (A, x, X), True: (signed(A, 1), signed(x, 2), signed(X, 3))}
        self._want = {}

    def want(self, alg, world, sign, v):
        """oracle.multiply for vector v of X (v = -1: the single x)."""
        key = (alg, world, sign, v)
        if key not in self._want:
            A, x, X = self.sets[sign]
            self._want[key] = self.oracle.multiply(alg, A, x if v < 0 else X[:, v], world)
        return self._want[key]


def compare(Y, wants, exact):
    """(ok, figure): exact: rows x vectors that differ; else the largest relative error."""
    want = np.stack(wants, axis=1)
    if Y is None or Y.shape != want.shape:
        return False, -1.0
    if exact:
        return bool(np.array_equal(Y, want)), float(np.count_nonzero(~(Y == want)))
    rel = np.abs(Y - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)
    return bool(np.all(rel <= TOL)), float(rel.max()) if rel.size else 0.0


def run_engine(e, alg, data, world, extras, emit):
    root = e.is_root()
    if extras:  # the exact single-vector y of the signed set while the engine has never seen a block
        A, x, _ = data.sets[True]
        e.set_exact(True)
        e.distribute(A if root else None, x if root else None)
        e.multiply()
        y_plain = e.collect()
    base = {"alg": alg, "R": data.R, "C": data.C, "world": world, "rank": e.shard(0).rank}
    ok_all = True

    def record(case, ok, **more):
        nonlocal ok_all
        ok_all &= bool(ok)
        emit(dict(base, case=case, ok=bool(ok), **more))

    def load(sign, nv):
        A, x, X = data.sets[sign]
        e.distribute(A if root else None, x if root else None)
        e.set_vectors(X[:, :nv] if root else None, nv)

    def check_block(case, sign, nv, exact, **more):
        Y = e.collect_multi()
        if root:
            ok, figure = compare(Y, [data.want(alg, world, sign, v) for v in range(nv)], exact)
            record(case, ok and e.vectors == nv, y_ok=ok, figure=figure, nv=nv, **more)
        else:
            record(case, Y is None and e.vectors == nv, y_ok=None, figure=None, nv=nv, **more)

    for exact in (False, True):
        e.set_exact(exact)
        for nv in NVS:
            load(exact, nv)
            e.multiply_multi()
            check_block("block", exact, nv, exact, mode="exact" if exact else "tree")
    if not extras:
        return ok_all

    # ---- once per algorithm, in exact mode on the signed set unless it says otherwise
    sign = True
    A, x, X = data.sets[sign]
    # more multiplies in flight than the ring has slots
    load(sign, 3)
    for _ in range(11):
        e.multiply_multi()
    check_block("ring_wrap", sign, 3, True)
    # the single vector's y is what an engine that never saw a block gives, and the block's
    # multiplies leave it alone
    e.multiply()
    y0 = e.collect()
    e.multiply_multi()
    e.multiply_multi()
    y1 = e.collect()  # no single multiply since y0: still the last one's y
    e.multiply()
    e.multiply_multi()
    y2 = e.collect()
    if root:
        want = data.want(alg, world, sign, -1)
        for case, y in (("single_before", y0), ("single_kept", y1), ("single_after", y2)):
            record(case, np.array_equal(y, y_plain) and np.array_equal(y, want))
    else:
        for case in ("single_before", "single_kept", "single_after"):
            record(case, y0 is None and y1 is None and y2 is None)
    # a larger block on the live engine: its buffers are remade (the smaller blocks after it reuse them)
    load(sign, 2)
    e.multiply_multi()
    e.set_vectors(X[:, :NV_MAX] if root else None, NV_MAX)
    e.multiply_multi()
    check_block("grow", sign, NV_MAX, True)
    # device-generated inputs
    e.fill_synth(42, 4242)
    e.fill_synth_vectors(777, 5)
    e.multiply_multi()
    check_block("synth", False, 5, True)
    # exact mode switched between two multiplies of the same block
    e.set_exact(False)
    e.multiply_multi()
    check_block("toggle_tree", False, 5, False)
    e.set_exact(True)
    e.multiply_multi()
    check_block("toggle_exact", False, 5, True)
    # the panel copy's "second multiply" rule counts single-vector multiplies only
    load(sign, 3)
    w0 = e.exact_panel_width()
    e.multiply_multi()
    e.multiply_multi()
    e.multiply_multi()
    w1 = e.exact_panel_width()
    e.multiply()
    e.multiply_multi()
    w2 = e.exact_panel_width()
    e.sync()
    record("panel_width", w0 == w1 == w2 == 0, widths=[w0, w1, w2])
    # kernel timing counts single-vector multiplies only, in both modes
    e.kernel_timing(1)
    e.multiply()
    n0 = e.kernel_ms().launches
    e.multiply_multi()
    e.multiply_multi()
    n1 = e.kernel_ms().launches
    e.multiply()
    n2 = e.kernel_ms().launches
    record("launches_per_launch", (n0, n1, n2) == (1, 1, 2), launches=[n0, n1, n2])
    e.kernel_timing(-1)
    e.multiply()
    e.multiply()
    n0 = e.kernel_ms().launches
    e.multiply_multi()
    n1 = e.kernel_ms().launches
    e.multiply()
    n2 = e.kernel_ms().launches
    e.kernel_timing(0)
    record("launches_span", (n0, n1, n2) == (2, 2, 3), launches=[n0, n1, n2])
    e.set_exact(False)
    return ok_all


def run_world(comm, world, emit):
    """Every (algorithm, shape) on this rank. True when every check held."""
    from matvec_mpi_multiplier_amd import multiplier as mm

    ok = True
    datas = {}
    for alg in ALGS:
        for i, (R, Cn) in enumerate(SHAPES):
            data = datas.setdefault((R, Cn), Data(R, Cn))
            with mm.Multiplier(alg, R, Cn, comm) as e:
                ok &= run_engine(e, alg, data, world, i == 0, emit)
    return ok


def main():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    os.environ.setdefault("NCCL_HOSTID", f"mvg-multi-{rank}")
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")

    import torch.distributed as dist

    from matvec_mpi_multiplier_amd import multiplier as mm

    def emit(rec):
        sys.stdout.write(json.dumps(rec) + "\n")
        sys.stdout.flush()

    t0 = time.perf_counter()
    dist.init_process_group("gloo")
    comm = mm.Comm.from_process_group(0)
    try:
        ok = run_world(comm, world, emit)
    except BaseException:
        # an engine call failed on this rank alone: its peers may sit in a collective that this
        # rank will never join, and so would an orderly teardown; leave at once, the launcher
        # then ends the peers
        import traceback

        traceback.print_exc()
        sys.stderr.flush()
        os._exit(2)
    comm.destroy()
    emit({"done": True, "rank": rank, "world": world, "ok": ok, "secs": round(time.perf_counter() - t0, 3)})
    # leave together, so a rank whose checks failed does not cut short a peer still printing
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
