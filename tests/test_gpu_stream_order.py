"""Every kernel entry point runs on the caller's stream (include/matvec_gpu.h: "device pointers;
asynchronous on `stream`"), and the split-K workspace map holds under two streams and two host
threads. The gate harness and the case table are tests/stream_order.py; each case there is one
delay of >= 20 ms on a non-blocking stream with the operands' producer, the call and the
result's consumer enqueued behind it, so a launch on any other stream reads NaN or is lost."""
import threading

import numpy as np
import pytest

import stream_order as SO
from conftest import max_rel
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
CASES = {c.id: c for c in SO.cases(lib)}


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        print(f"\nstream-order gate: {g.launches} launches of mvg_stream_read over {g.DELAY_DOUBLES * 8 >> 20} MiB "
              f"= {g.delay_ms:.1f} ms")
        yield g


def test_the_delay_is_calibrated(gate):
    assert gate.launches >= 8 and gate.delay_ms >= SO.DELAY_MS, (gate.launches, gate.delay_ms)
    assert gate.s != gate.t


@pytest.mark.parametrize("cid", ["gemv-257x1000", "exact-2049x512"])
def test_positive_control_a_call_on_another_stream_is_seen(gate, cid):
    """mvg_gemv and mvg_gemv_exact issued on a second non-blocking stream while s is delayed:
    the consumer must not find the expected y (it finds NaN or the producer's overwrite)."""
    spec = CASES[cid].make()
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad


@pytest.mark.parametrize("cid", list(CASES))
def test_entry_point_runs_on_the_callers_stream(gate, cid):
    case = CASES[cid]
    bad, _ = SO.run_case(gate, case.make())
    assert not bad, f"{case.entry} ({case.why}): " + "; ".join(bad)


# ---------------------------------------------------------------- two streams, one workspace map
def _split_name(m, k):
    return lib.mvg_gemv_variant_name(lib.mvg_gemv_auto_variant(k, m, k)).decode()


class _Problem:
    """A (m x k) and nx vectors on the device, y on the null stream per vector as the solo run."""

    def __init__(self, m, k, nx, seed=42, exact=False):
        self.m, self.k, self.nx, self.exact = m, k, nx, exact
        self.bufs = []
        A, X = oracle.synth(m, k, seed), oracle.synth(nx, k, seed + 4200)
        self.A, self.X = self._new(m * k).upload(A), self._new(nx * k).upload(X)
        self.y, self.out = self._new(m), self._new(nx * m)
        self.solo = np.empty((nx, m))
        for i in range(nx):
            self.call(i, None)
            _lib.check(lib.mvg_stream_sync(None), "sync")
            self.solo[i] = self.y.download(m)
        self.y.upload(np.full(m, np.nan))
        self.out.upload(np.full(nx * m, np.nan))
        want = np.stack([oracle.multiply_std_rowwise(A, X[i]) for i in range(nx)])
        assert np.array_equal(self.solo, want) if exact else max_rel(self.solo, want) <= SO.TOL

    def _new(self, n):
        b = mm.DeviceBuffer(n)
        self.bufs.append(b)
        return b

    def call(self, i, s):
        f = lib.mvg_gemv_exact if self.exact else lib.mvg_gemv
        return f(self.A.ptr, self.k, self.X.ptr + 8 * i * self.k, self.y.ptr, self.m, self.k, s)

    def free(self):
        for b in self.bufs:
            b.free()


def test_split_k_calls_interleaved_on_two_streams(gate):
    """Split-K calls of different sizes alternate between two streams with no sync in between:
    64 x 16384 on s1; 32 x 8192 then 700 x 8192 on s2, whose larger rows x splits makes the
    workspace of (device, s2) free and reallocate while s1 has launches queued (hipFree waits for
    the device, which is what makes the regrowth safe). Each y is copied out in stream order and
    must be the solo null-stream run's, bit for bit."""
    rounds = 10
    for m, k in ((64, 16384), (32, 8192), (700, 8192)):
        assert _split_name(m, k).endswith("_splitk"), (m, k)
    probs = []
    s1 = s2 = None
    try:
        s1, s2 = gate.stream(), gate.stream()
        probs = [_Problem(64, 16384, rounds), _Problem(32, 8192, rounds), _Problem(700, 8192, rounds)]
        a, b, c = probs
        for r in range(rounds):
            for p, s in ((a, s1), (b, s2), (c, s2)):
                _lib.check(p.call(r, s), "mvg_gemv")
                gate.copy(p.out.ptr + 8 * r * p.m, p.y.ptr, 8 * p.m, s)
        gate.sync(s1)
        gate.sync(s2)
        for p in probs:
            got = p.out.download().reshape(rounds, p.m)
            assert np.array_equal(got.view(np.uint64), p.solo.view(np.uint64)), (p.m, p.k)
    finally:
        for s in (s1, s2):
            if s:
                lib.mvg_stream_sync(s)
        for p in probs:
            p.free()


def test_two_host_threads_each_on_its_own_stream(gate):
    """Two host threads, each with its own stream and buffers, 20 mixed calls each (split-K of
    varying size, mvg_gemv_exact, mvg_gemv_multi of 3 vectors), results bit-identical to the solo
    runs. One thread makes an invalid call in the middle: its mvg_last_error names mvg_gemv; the
    other thread's last error stays as it was and all its calls return MVG_OK."""
    ncalls = 20
    shapes = [(64, 16384, False), (200, 8192, False), (257, 1000, True), (32, 16384, False)]
    report = [{}, {}]
    probs, multis, streams = [[], []], [None, None], [None, None]
    start = threading.Barrier(2)

    def multi_call(mu, s):
        A, X, Y, m, k = mu
        return lib.mvg_gemv_multi(A.ptr, k, X.ptr, k, Y.ptr, m, m, k, 3, s)

    def work(tid):
        rep, s = report[tid], streams[tid]
        try:
            rep["err_before"] = lib.mvg_last_error()
            rcs = []
            start.wait(timeout=60)
            for i in range(ncalls):
                if i % 5 == 4:
                    rcs.append(multi_call(multis[tid], s))
                else:
                    p = probs[tid][i % 5]
                    j = i // 5
                    rcs.append(p.call(j, s))
                    gate.copy(p.out.ptr + 8 * j * p.m, p.y.ptr, 8 * p.m, s)
                if tid == 1 and i == ncalls // 2:
                    p = probs[tid][0]
                    rep["bad_rc"] = lib.mvg_gemv(p.A.ptr, p.k - 1, p.X.ptr, p.y.ptr, p.m, p.k, s)  # lda < k
                    rep["bad_err"] = lib.mvg_last_error()
            rep["sync"] = lib.mvg_stream_sync(s)
            rep["rcs"] = rcs
            rep["err_after"] = lib.mvg_last_error()
        except BaseException as exc:  # reported by the main thread
            rep["exc"] = exc

    bufs = []
    try:
        for tid in (0, 1):
            streams[tid] = gate.stream()
            probs[tid] = [_Problem(m, k, ncalls // 5, seed=42 + tid, exact=ex) for m, k, ex in shapes]
            m, k = 130, 1058
            A, X = oracle.synth(m, k, 50 + tid), oracle.synth(3, k, 60 + tid)
            dA, dX, dY = mm.DeviceBuffer(m * k).upload(A), mm.DeviceBuffer(3 * k).upload(X), mm.DeviceBuffer(3 * m)
            bufs += [dA, dX, dY]
            multis[tid] = (dA, dX, dY, m, k)
            _lib.check(multi_call(multis[tid], None), "mvg_gemv_multi")
            _lib.check(lib.mvg_stream_sync(None), "sync")
            report[tid]["multi_solo"] = dY.download()
            dY.upload(np.full(3 * m, np.nan))
        threads = [threading.Thread(target=work, args=(tid,)) for tid in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
            assert not t.is_alive()
        for tid in (0, 1):
            rep = report[tid]
            assert "exc" not in rep, rep.get("exc")
            assert rep["rcs"] == [_lib.MVG_OK] * ncalls and rep["sync"] == _lib.MVG_OK, (tid, rep["rcs"])
            for p in probs[tid]:
                got = p.out.download().reshape(p.nx, p.m)
                assert np.array_equal(got.view(np.uint64), p.solo.view(np.uint64)), (tid, p.m, p.k)
            got = multis[tid][2].download()
            assert np.array_equal(got.view(np.uint64), rep["multi_solo"].view(np.uint64)), tid
        assert report[1]["bad_rc"] == _lib.MVG_E_INVALID and b"mvg_gemv" in report[1]["bad_err"], report[1]
        assert report[1]["err_after"] == report[1]["bad_err"]  # later successes leave the text alone
        # the error text is the calling thread's own: the other thread never sees it
        assert report[0]["err_after"] == report[0]["err_before"] and b"lda" not in report[0]["err_after"], report[0]
    finally:
        for s in streams:
            if s:
                lib.mvg_stream_sync(s)
        for tid in (0, 1):
            for p in probs[tid]:
                p.free()
        for b in bufs:
            b.free()
