"""Worker for tests/test_gpu_engine_sequences.py and tests/test_gpu_engine_block_sequences.py
(run under torch.distributed.run; not collected by pytest).

One process per rank, every rank on GPU 0 (a distinct NCCL_HOSTID per rank and loopback sockets,
as tests/rank_worker_b2b.py). One launch walks every case of its kind, all three algorithms
(start-up of the ranks dominates the cost):

  small             every script of engine_scripts.SMALL_RUNS at the small shapes
  panels [alg ...]  engine_scripts.PANEL_RUNS at the panel shapes (world 2), all algorithms or
                    the named ones
  blocks [alg ...]  every script of engine_scripts.BLOCK_RUNS (a block of vectors beside the
                    single one) at the small shapes, all algorithms or the named ones
  blockpanels [alg ...]  engine_scripts.BLOCK_PANEL_RUNS at the panel shapes (world 2)

Every rank prints one JSON line per (case, check), and a last line {"done": true, ...}. A failed
check is recorded and the rank walks on, so no peer is left inside a collective; the exit status
is 1 if any check of this rank failed.
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

rank = int(os.environ.get("RANK", "0"))
world = int(os.environ.get("WORLD_SIZE", "1"))
os.environ.setdefault("NCCL_HOSTID", f"mvg-seq-{rank}")
os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
os.environ.setdefault("NCCL_IB_DISABLE", "1")

import torch.distributed as dist  # noqa: E402

import engine_scripts as ES  # noqa: E402
from matvec_mpi_multiplier_amd import multiplier as mm  # noqa: E402


def emit(rec):
    sys.stdout.write(json.dumps(rec) + "\n")
    sys.stdout.flush()


def main():
    kind = sys.argv[1]
    if kind == "small":
        shapes, runs, keep = ES.small_shapes(), ES.SMALL_RUNS, 64
    elif kind == "panels":
        shapes, runs, keep = ES.panel_shapes(tuple(sys.argv[2:]) or ES.ALGS), ES.PANEL_RUNS, 6
    elif kind == "blocks":
        shapes, runs, keep = ES.small_shapes(tuple(sys.argv[2:]) or ES.ALGS), ES.BLOCK_RUNS, 64
    elif kind == "blockpanels":
        shapes, runs, keep = ES.panel_shapes(tuple(sys.argv[2:]) or ES.ALGS), ES.BLOCK_PANEL_RUNS, 6
    else:
        raise SystemExit(f"unknown kind {kind!r}")
    t0 = time.perf_counter()
    dist.init_process_group("gloo")
    comm = mm.Comm.from_process_group(0)
    try:
        ok = ES.run_cases(comm, world, shapes, runs, emit, keep)
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
    # the launcher ends every rank as soon as one leaves with a failure: leave together, so a
    # rank whose checks failed does not cut short a peer that is still printing its own
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
