"""The engine (csrc/engine.cpp) on op sequences that combine its modes, at 1, 2, 3, 4 and 6 ranks.

tests/engine_scripts.py holds the scripts (distribute / distribute_shared / fill_synth, multiply,
collect, exact mode and chunked distribution switched on a live engine, the two kernel-timing
modes, the root-send in many pieces), a host model of what every collect must see, and the
runner. Every write brings a data set no earlier write of the script brought, so a y from a stale
A, x, panel copy or ring slot is wrong in every row. Checked at every collect:

  - on the root, y against oracle.multiply at the same rank count: np.array_equal in exact mode,
    |y - want| <= 1e-12 * (|A|·|x|) per row otherwise;
  - on every rank, exact_panel_width() and (per-launch timing) kernel_ms().launches against the
    model.

World 1 runs in this process on Comm.init_all([0]), with the collectives forced
(MVG_ALWAYS_COLLECT=1) and without. Worlds 2, 3 (1 x 3 grid: one reduce straight into y), 4
(2 x 2: two-level reduce and gather) and 6 (2 x 3: the rank-order sum over three grid columns)
run tests/rank_worker_sequences.py under torch.distributed.run, every rank on GPU 0: one launch
per world walks all algorithms, shapes and scripts, and the cases below read its lines from a
module-level cache. The panel shapes (200 MB shards that exact mode keeps in column panels) run
at world 2 only, with distribute_shared, one launch per algorithm (a launch with all three took
more than twice the slowest case of tests/test_gpu_rank_mode.py).

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

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "rank_worker_sequences.py")

_launches = {}
_stopped = []  # why no further launch is started
FAULT = re.compile(r"exitcode\s*:\s*-(?!15\b)\d+|Signal (?!15\b)\d+|core dumped|illegal memory access|HSA_STATUS_ERROR|Aborted")


def n_checks(name, runs):
    return ES.n_checks(runs[name][0])


def report(key, lines, secs):
    """The launch's wall time and slowest script on stdout (pytest -rP shows it)."""
    per = {}
    for ln in lines:
        if "script" in ln and ln["rank"] == 0:
            per[(ln["alg"], ln["R"], ln["C"], ln["script"])] = ln["secs"]
    slow = max(per.items(), key=lambda kv: kv[1]) if per else None
    print(f"engine sequences {key}: {secs:.1f} s wall, {len(per)} scripts, slowest {slow}")


def run_world_1(always_collect, runs=ES.SMALL_RUNS):
    from matvec_mpi_multiplier_amd import multiplier as mm

    lines = []
    t0 = time.perf_counter()
    with ES.environment({"MVG_ALWAYS_COLLECT": "1" if always_collect else "0"}):
        comm = mm.Comm.init_all([0])
        try:
            ok = ES.run_cases(comm, 1, ES.small_shapes(), runs, lines.append)
        finally:
            comm.destroy()
    return {"returncode": 0 if ok else 1, "lines": lines, "secs": time.perf_counter() - t0, "stderr": ""}


def run_worker(nproc, args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                        "--master-addr", "127.0.0.1", "--master-port", str(port), WORKER] + list(args),
                       env=dict(os.environ), capture_output=True, text=True, timeout=110)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return {"returncode": r.returncode, "lines": lines, "secs": time.perf_counter() - t0, "stderr": r.stderr[-3000:]}


def launch(key):
    """The records of one launch, made on first use. key: ("inproc", always_collect),
    ("small", world) or ("panels", alg); for tests/test_gpu_engine_block_sequences.py, which shares
    this cache and its stop rule: ("blk_inproc", always_collect), ("blocks", world) or
    ("blocks", world, alg), or ("blockpanels", alg)."""
    if key not in _launches:
        if _stopped:
            _launches[key] = {"returncode": None, "lines": [], "secs": 0.0, "stderr": "not run: " + _stopped[0]}
        else:
            try:
                if key[0] == "inproc":
                    res = run_world_1(key[1])
                elif key[0] == "small":
                    res = run_worker(key[1], ["small"])
                elif key[0] == "blk_inproc":
                    res = run_world_1(key[1], ES.BLOCK_RUNS)
                elif key[0] == "blocks":
                    res = run_worker(key[1], ["blocks"] + list(key[2:]))
                else:
                    res = run_worker(ES.PANEL_WORLD, [key[0], key[1]])
            except subprocess.TimeoutExpired as exc:
                res = {"returncode": None, "lines": [], "secs": 110.0, "stderr": f"timed out: {exc}"}
            rc = res["returncode"]
            # a time-out, a signal (the launcher reports a rank's as "exitcode : -11"; -15 is its
            # own SIGTERM to the peers of a rank that left with failed checks) or a GPU fault:
            # the GPU is left alone from here on
            if rc is None or rc < 0 or (rc != 0 and FAULT.search(res["stderr"])):
                _stopped.append(f"launch {key} ended with {rc}: {res['stderr'][-300:]}")
            _launches[key] = res
            report(key, res["lines"], res["secs"])
    return _launches[key]


def case_lines(key, alg, R, Cn, name):
    return [ln for ln in launch(key)["lines"]
            if ln.get("script") == name and (ln["alg"], ln["R"], ln["C"]) == (alg, R, Cn)]


def assert_case(key, world, alg, R, Cn, name, runs):
    res = launch(key)
    lines = case_lines(key, alg, R, Cn, name)
    want = {(rank, c) for rank in range(world) for c in range(n_checks(name, runs))}
    got = {(ln["rank"], ln["check"]) for ln in lines}
    assert got == want, (sorted(want - got)[:6], res["returncode"], res["stderr"][-1500:])
    bad = [ln for ln in lines if not ln["ok"]]
    assert not bad, bad[:4]
    # what "ok" stands for, spelled out: the root compared y at every check, exact mode was what
    # the model says, and widths and launch counts are the model's on every rank
    for ln in lines:
        assert ln["world"] == world
        assert (ln["y_ok"] is True) if ln["rank"] == 0 else (ln["y_ok"] is None), ln
        assert ln["exact"] == ln["want_exact"] and ln["width"] == ln["want_width"], ln
        assert ln["launches"] == ln["want_launches"], ln
        if ln["rank"] == 0 and ln["want_exact"]:
            assert ln["figure"] == 0.0, ln  # no row differs from the oracle's bits
        elif ln["rank"] == 0:
            assert ln["figure"] <= ES.TOL, ln


SMALL_IDS = [f"{alg}-{R}x{Cn}-{name}" for alg, R, Cn, name in ES.small_cases()]
PANEL_IDS = [f"{alg}-{R}x{Cn}-{name}" for alg, R, Cn, name in ES.panel_cases()]


# ------------------------------------------------------------------ world 1, in process
@pytest.mark.parametrize("always_collect", [False, True], ids=["plain", "forced_collectives"])
def test_world_1_walks_every_script(always_collect):
    res = launch(("inproc", always_collect))
    assert res["returncode"] == 0, [ln for ln in res["lines"] if not ln["ok"]][:4]
    assert len(res["lines"]) == sum(n_checks(c[3], ES.SMALL_RUNS) for c in ES.small_cases())


@pytest.mark.parametrize("case", ES.small_cases(), ids=SMALL_IDS)
@pytest.mark.parametrize("always_collect", [False, True], ids=["plain", "forced_collectives"])
def test_world_1_sequence(always_collect, case):
    assert_case(("inproc", always_collect), 1, *case, ES.SMALL_RUNS)


# ------------------------------------------------------------------ worlds 2, 3, 4 and 6
@pytest.mark.parametrize("world", [2, 3, 4, 6])
def test_ranks_walk_every_script(world):
    res = launch(("small", world))
    assert res["returncode"] == 0, ([ln for ln in res["lines"] if ln.get("ok") is False][:4], res["stderr"][-3000:])
    done = [ln for ln in res["lines"] if ln.get("done")]
    assert sorted(ln["rank"] for ln in done) == list(range(world)) and all(ln["ok"] for ln in done)


@pytest.mark.parametrize("case", ES.small_cases(), ids=SMALL_IDS)
@pytest.mark.parametrize("world", [2, 3, 4, 6])
def test_rank_sequence(world, case):
    assert_case(("small", world), world, *case, ES.SMALL_RUNS)


# ------------------------------------------------------------------ the panel shapes, world 2
@pytest.mark.parametrize("alg", ES.ALGS)
def test_panel_ranks_walk_every_script(alg):
    res = launch(("panels", alg))
    assert res["returncode"] == 0, ([ln for ln in res["lines"] if ln.get("ok") is False][:4], res["stderr"][-3000:])
    done = [ln for ln in res["lines"] if ln.get("done")]
    assert sorted(ln["rank"] for ln in done) == [0, 1] and all(ln["ok"] for ln in done)


@pytest.mark.parametrize("case", ES.panel_cases(), ids=PANEL_IDS)
def test_panel_sequence(case):
    """toggle and chunked on shards that keep a panel copy, and chunked once more with
    MVG_NO_PANELS=1: both give the oracle's bits, and the widths are the model's (256 from the
    second multiply of a write on, 0 after a write and with MVG_NO_PANELS)."""
    assert_case(("panels", case[0]), ES.PANEL_WORLD, *case, ES.PANEL_RUNS)
    if case[3] == "toggle":
        widths = [ln["width"] for ln in sorted(case_lines(("panels", case[0]), *case), key=lambda l: l["check"])
                  if ln["rank"] == 1]
        assert widths == [0, 256, 256, 0, 256, 0, 256]
