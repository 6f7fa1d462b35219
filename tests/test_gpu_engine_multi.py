"""The engine's block of vectors (mvg_engine_set_vectors / fill_synth_vectors / multiply_multi /
collect_multi) at 1, 2, 4 and 6 ranks, every split, tree and exact mode, against
oracle.multiply per column.

tests/rank_worker_multi.py holds the cases and the runner. World 1 runs in this process on
Comm.init_all([0]), without collectives (the product goes straight into Y) and with them forced
(MVG_ALWAYS_COLLECT=1). Worlds 2, 4 (2 x 2 grid: reduce, then gather) and 6 (2 x 3: the
rank-order sum over three grid columns) run the worker under torch.distributed.run, every rank
on GPU 0: one launch per world walks all three algorithms, and the cases below read its lines
from a module-level cache.

After a launch that hung or was killed by a signal nothing more is started on the GPU: the
remaining launches are reported as not run.
"""
import json
import os
import re
import socket
import subprocess
import sys
import time

import pytest

import engine_scripts as ES
import rank_worker_multi as W

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "rank_worker_multi.py")
WORLDS = (2, 4, 6)

_launches = {}
_stopped = []  # why no further launch is started
FAULT = re.compile(r"exitcode\s*:\s*-(?!15\b)\d+|Signal (?!15\b)\d+|core dumped|illegal memory access|HSA_STATUS_ERROR|Aborted")


def run_world_1(always_collect):
    from matvec_mpi_multiplier_amd import multiplier as mm

    lines = []
    t0 = time.perf_counter()
    with ES.environment({"MVG_ALWAYS_COLLECT": "1" if always_collect else "0"}):
        comm = mm.Comm.init_all([0])
        try:
            ok = W.run_world(comm, 1, lines.append)
        finally:
            comm.destroy()
    return {"returncode": 0 if ok else 1, "lines": lines, "secs": time.perf_counter() - t0, "stderr": ""}


def run_worker(nproc):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER],
                       env=dict(os.environ), capture_output=True, text=True, timeout=110)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return {"returncode": r.returncode, "lines": lines, "secs": time.perf_counter() - t0, "stderr": r.stderr[-3000:]}


def launch(key):
    """The records of one launch, made on first use. key: ("inproc", always_collect) or
    ("ranks", world)."""
    if key not in _launches:
        if _stopped:
            _launches[key] = {"returncode": None, "lines": [], "secs": 0.0, "stderr": "not run: " + _stopped[0]}
        else:
            try:
                res = run_world_1(key[1]) if key[0] == "inproc" else run_worker(key[1])
            except subprocess.TimeoutExpired as exc:
                res = {"returncode": None, "lines": [], "secs": 110.0, "stderr": f"timed out: {exc}"}
            rc = res["returncode"]
            # a time-out, a signal or a GPU fault: the GPU is left alone from here on
            if rc is None or rc < 0 or (rc != 0 and FAULT.search(res["stderr"])):
                _stopped.append(f"launch {key} ended with {rc}: {res['stderr'][-300:]}")
            _launches[key] = res
            print(f"engine multi {key}: {res['secs']:.1f} s wall, {len(res['lines'])} lines")
    return _launches[key]


def keys():
    return [("inproc", False), ("inproc", True)] + [("ranks", w) for w in WORLDS]


def key_id(key):
    return {("inproc", False): "world1", ("inproc", True): "world1_forced_collectives"}.get(key, f"world{key[1]}")


def world_of(key):
    return 1 if key[0] == "inproc" else key[1]


def assert_lines(key, lines, exact=None):
    """One line per rank, all ok; on the root the comparison ran and met its bar."""
    res = launch(key)
    world = world_of(key)
    assert sorted(ln["rank"] for ln in lines) == list(range(world)), (res["returncode"], res["stderr"][-1500:])
    bad = [ln for ln in lines if not ln["ok"]]
    assert not bad, bad[:4]
    for ln in lines:
        assert ln["world"] == world
        if "y_ok" in ln:
            assert (ln["y_ok"] is True) if ln["rank"] == 0 else (ln["y_ok"] is None), ln
            if ln["rank"] == 0 and exact is not None:
                assert ln["figure"] == 0.0 if exact else ln["figure"] <= W.TOL, ln


@pytest.mark.parametrize("key", keys(), ids=key_id)
def test_every_rank_walks_every_case(key):
    res = launch(key)
    assert res["returncode"] == 0, ([ln for ln in res["lines"] if ln.get("ok") is False][:4], res["stderr"][-3000:])
    world = world_of(key)
    per_rank = len(W.ALGS) * (len(W.SHAPES) * 2 * len(W.NVS) + len(W.EXTRAS))
    checks = [ln for ln in res["lines"] if "case" in ln]
    assert len(checks) == world * per_rank
    if key[0] == "ranks":
        done = [ln for ln in res["lines"] if ln.get("done")]
        assert sorted(ln["rank"] for ln in done) == list(range(world)) and all(ln["ok"] for ln in done)


@pytest.mark.parametrize("mode", ["tree", "exact"])
@pytest.mark.parametrize("nv", W.NVS)
@pytest.mark.parametrize("shape", W.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("alg", W.ALGS)
@pytest.mark.parametrize("key", keys(), ids=key_id)
def test_block_of_vectors(key, alg, shape, nv, mode):
    """distribute, set_vectors, multiply_multi, collect_multi: every column of Y is
    oracle.multiply's y for that vector, bit for bit in exact mode, within 1e-12 in tree mode."""
    lines = [ln for ln in launch(key)["lines"] if ln.get("case") == "block" and ln["alg"] == alg
             and (ln["R"], ln["C"]) == shape and ln["nv"] == nv and ln["mode"] == mode]
    assert_lines(key, lines, exact=mode == "exact")


@pytest.mark.parametrize("case", W.EXTRAS)
@pytest.mark.parametrize("alg", W.ALGS)
@pytest.mark.parametrize("key", keys(), ids=key_id)
def test_block_beside_the_single_vector(key, alg, case):
    """Eleven multiplies in flight; the single vector's y before, between and after the block's
    multiplies is the bits of an engine that never saw a block; a larger block on a live engine;
    device-generated vectors; exact mode switched between two multiplies; the panel width and the
    timed-launch counts count single-vector multiplies only."""
    lines = [ln for ln in launch(key)["lines"] if ln.get("case") == case and ln["alg"] == alg]
    exact = {"toggle_tree": False}.get(case, True) if case in ("ring_wrap", "grow", "synth", "toggle_tree", "toggle_exact") else None
    assert_lines(key, lines, exact=exact)
