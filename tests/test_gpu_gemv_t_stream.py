"""mvg_gemv_t runs on the caller's stream (stream contract): the strip kernel, the band
reduce out of the per-(device, stream) workspace and the m == 0 zeroing. The gate, Spec and
run_case are tests/stream_order.py's, unchanged: one delay of >= 20 ms on a non-blocking stream
with the operands' producer, the call and the result's consumer enqueued behind it, so a launch on
any other stream computes from NaN or is overwritten."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib


def _spec(m, k):
    fa, fz = SO._synth_flat(m * k, 42), SO._synth_flat(m, 4343)
    want = oracle.multiply_std_rowwise(np.ascontiguousarray(fa.reshape(m, k).T), fz) if m else np.zeros(k)

    def call(lib, p, s):
        SO._ok(lib, lib.mvg_gemv_t(p["A"], k, p["z"], p["Y"], m, k, s), "mvg_gemv_t")

    # m == 0: nothing to read; the buffers exist so the pointers are real
    return SO.Spec(ops={"A": fa, "z": fz} if m else {}, scratch={} if m else {"A": 2, "z": 2}, ny=k, call=call,
                   want=want, bar="tol")


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        yield g


def test_the_multi_band_shape_has_more_than_one_band():
    assert mm.gemv_t_plan(257, 1000, 257)[1] > 1  # strip kernel into the workspace, then the reduce


@pytest.mark.parametrize("m,k", [(1000, 257), (0, 257)], ids=["bands-1000x257", "zeroing-m0"])
def test_gemv_t_runs_on_the_callers_stream(gate, m, k):
    bad, _ = SO.run_case(gate, _spec(m, k))
    assert not bad, "; ".join(bad)


def test_positive_control_a_call_on_another_stream_is_seen(gate):
    spec = _spec(1000, 257)
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad
