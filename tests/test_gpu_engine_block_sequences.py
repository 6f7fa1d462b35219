"""The engine's block of vectors (set_vectors / fill_synth_vectors / multiply_multi /
collect_multi) walked through op sequences beside the single vector, at 1, 2, 3, 4 and 6 ranks.

Both kinds of multiply share one slot counter, one ring of events and one exchange stream
(csrc/engine.cpp multiply_step); the block has its own buffers. tests/engine_scripts.py holds the
scripts (BLOCK_RUNS, BLOCK_PANEL_RUNS), the host model and the runner: three exact blocks in
flight with different A and X at rings of 1, 2 and 8; M and MM in turn around rings of 2, 3 and 8,
so the once-per-ring wait falls on one kind with the other kind's exchange pending; a block that
grows with exchanges in flight; multiply_multi on a chunked distribution still copying and the
timed multiply after it; the root-send in 120 pieces per peer, the broadcast of X and the block
exchanges on one communicator; every writer of A and both writers of X; and, on 200 MB shards,
the block beside a fresh and a stale panel copy and on chunks that take milliseconds to land.
Every write and every V or G brings values no earlier one of the script brought. Checked at every
collect and collect_multi:

  - on the root, y (every column of Y) against oracle.multiply at the same rank count:
    np.array_equal in exact mode, |y - want| <= 1e-12 * (|A|·|x|) per element otherwise;
  - on every rank, the mode, exact_panel_width() and (per-launch timing) kernel_ms().launches
    against the model; off the root collect_multi gives None and the vector count is the set's.

The launches, their cache and the rule that nothing more is started on the GPU after a launch
that hung, died of a signal or reported a GPU fault are tests/test_gpu_engine_sequences.py's:
world 1 in this process, plain and with MVG_ALWAYS_COLLECT=1; worlds 2, 3, 4 and 6 through
tests/rank_worker_sequences.py under torch.distributed.run, every rank on GPU 0, one launch per
world (world 6: one per algorithm, its one launch took 34 to 75 s of the 110 s limit from run to
run); the panel shapes at world 2, one launch per algorithm.
"""
import pytest

import engine_scripts as ES
import test_gpu_engine_sequences as SEQ

pytestmark = pytest.mark.gpu

BLOCK_IDS = [f"{alg}-{R}x{Cn}-{name}" for alg, R, Cn, name in ES.block_cases()]
BLOCK_PANEL_IDS = [f"{alg}-{R}x{Cn}-{name}" for alg, R, Cn, name in ES.block_panel_cases()]


# ------------------------------------------------------------------ world 1, in process
@pytest.mark.parametrize("always_collect", [False, True], ids=["plain", "forced_collectives"])
def test_world_1_walks_every_block_script(always_collect):
    res = SEQ.launch(("blk_inproc", always_collect))
    assert res["returncode"] == 0, [ln for ln in res["lines"] if not ln["ok"]][:4]
    assert len(res["lines"]) == sum(SEQ.n_checks(c[3], ES.BLOCK_RUNS) for c in ES.block_cases())


@pytest.mark.parametrize("case", ES.block_cases(), ids=BLOCK_IDS)
@pytest.mark.parametrize("always_collect", [False, True], ids=["plain", "forced_collectives"])
def test_world_1_block_sequence(always_collect, case):
    SEQ.assert_case(("blk_inproc", always_collect), 1, *case, ES.BLOCK_RUNS)


# ------------------------------------------------------------------ worlds 2, 3, 4 and 6
SPLIT_WORLDS = (6,)  # one launch per algorithm


def block_key(world, alg):
    return ("blocks", world, alg) if world in SPLIT_WORLDS else ("blocks", world)


BLOCK_KEYS = [key for world in (2, 3, 4, 6)
              for key in ([("blocks", world, alg) for alg in ES.ALGS] if world in SPLIT_WORLDS else [("blocks", world)])]


@pytest.mark.parametrize("key", BLOCK_KEYS, ids=lambda k: "-".join(str(p) for p in k[1:]))
def test_ranks_walk_every_block_script(key):
    world = key[1]
    res = SEQ.launch(key)
    assert res["returncode"] == 0, ([ln for ln in res["lines"] if ln.get("ok") is False][:4], res["stderr"][-3000:])
    done = [ln for ln in res["lines"] if ln.get("done")]
    assert sorted(ln["rank"] for ln in done) == list(range(world)) and all(ln["ok"] for ln in done)


@pytest.mark.parametrize("case", ES.block_cases(), ids=BLOCK_IDS)
@pytest.mark.parametrize("world", [2, 3, 4, 6])
def test_rank_block_sequence(world, case):
    SEQ.assert_case(block_key(world, case[0]), world, *case, ES.BLOCK_RUNS)


# ------------------------------------------------------------------ the panel shapes, world 2
@pytest.mark.parametrize("alg", ES.ALGS)
def test_panel_ranks_walk_every_block_script(alg):
    res = SEQ.launch(("blockpanels", alg))
    assert res["returncode"] == 0, ([ln for ln in res["lines"] if ln.get("ok") is False][:4], res["stderr"][-3000:])
    done = [ln for ln in res["lines"] if ln.get("done")]
    assert sorted(ln["rank"] for ln in done) == [0, 1] and all(ln["ok"] for ln in done)


@pytest.mark.parametrize("case", ES.block_panel_cases(), ids=BLOCK_PANEL_IDS)
def test_panel_block_sequence(case):
    """blk_panels: the block's Y is the oracle's bits beside a fresh panel copy and beside a stale
    one, and no multiply_multi moves the width (256 only where two M have run since the last
    write). blk_chunked: the block on chunked writes of 200 MB shards, whole writes after them."""
    key = ("blockpanels", case[0])
    SEQ.assert_case(key, ES.PANEL_WORLD, *case, ES.BLOCK_PANEL_RUNS)
    lines = sorted(SEQ.case_lines(key, *case), key=lambda ln: ln["check"])
    for rank in range(ES.PANEL_WORLD):
        widths = [ln["width"] for ln in lines if ln["rank"] == rank]
        if case[3] == "blk_panels":
            assert widths == [256, 256, 0, 0, 256, 256, 0]
        else:
            assert widths == [0] * 7
