"""mvg_gemv_ata runs on the caller's stream (stream contract): the composed pair, the
fused kernels, the band reduce out of the per-(device, stream) workspace and the zeroing of the
empty sums. The gate, Spec and run_case are tests/stream_order.py's, unchanged: one delay of
>= 20 ms on a non-blocking stream with the operands' producer, the call and the result's consumer
enqueued behind it, so a launch on any other stream computes from NaN or is overwritten. The two
results share one output buffer of m + k doubles, t = Y and w = Y + m, so the single-output Spec
serves."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
NAMES = [lib.mvg_gemv_ata_variant_name(v).decode() for v in range(lib.mvg_gemv_ata_variant_count())]
WROW, WGROW = NAMES.index("wrow_w8_c8_u4"), NAMES.index("wgrow_w8_c8_r2")
M, K = 1000, 257


def _spec(m, k, variant=0):
    fa, fx = SO._synth_flat(m * k, 42), SO._synth_flat(k, 4242)
    if m and k:
        A = fa.reshape(m, k)
        t = oracle.multiply_std_rowwise(A, fx)
        want = np.concatenate([t, oracle.multiply_std_rowwise(np.ascontiguousarray(A.T), t)])
    else:
        want = np.zeros(m + k)

    def call(lib, p, s):
        SO._ok(lib, lib.mvg_gemv_ata_variant(p["A"], k, p["x"], p["Y"], p["Y"] + 8 * m, m, k, variant, s), "mvg_gemv_ata")

    # an empty sum: nothing to read; the buffers exist so the pointers are real
    full = bool(m and k)
    return SO.Spec(ops={"A": fa, "x": fx} if full else {}, scratch={} if full else {"A": 2, "x": 2}, ny=m + k, call=call,
                   want=want, bar="tol")


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        yield g


def test_the_fused_variants_cut_the_shape_into_more_than_one_band():
    for v in (WROW, WGROW):
        assert mm.gemv_ata_plan(K, M, K, v)[1] > 1  # fused kernel into the workspace, then the reduce
    assert mm.gemv_t_plan(K, M, K)[1] > 1  # two_pass: the transposed half too


@pytest.mark.parametrize("m,k,variant", [(M, K, 0), (M, K, 1), (M, K, WROW), (M, K, WGROW), (0, K, 0), (M, 0, 0)],
                         ids=["auto", "two_pass", "wrow", "wgrow", "zeroing-m0", "zeroing-k0"])
def test_gemv_ata_runs_on_the_callers_stream(gate, m, k, variant):
    bad, _ = SO.run_case(gate, _spec(m, k, variant))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("variant", [1, WROW], ids=["two_pass", "wrow"])
def test_positive_control_a_call_on_another_stream_is_seen(gate, variant):
    spec = _spec(M, K, variant)
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad
