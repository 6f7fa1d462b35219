"""mvg_gemv_ata_multi runs on the caller's stream (stream contract): the fused kernel, the
band reduce out of the per-(device, stream) workspace, every group, the single leftover vector, both
halves of two_pass and the zeroings of the empty sums. The gate, Spec and run_case are
tests/stream_order.py's, unchanged: one delay of >= 20 ms on a non-blocking stream with the
operands' producer, the call and the result's consumer enqueued behind it, so a launch on any other
stream computes from NaN or is overwritten. The two results share one output buffer of
(m + k) * nv doubles, T = Y and W = Y + m * nv, so the single-output Spec serves."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
NAMES = [lib.mvg_gemv_ata_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_ata_multi_variant_count())]
WROWM, WGROWM = NAMES.index("wrowm_w8_c8_u2_v2"), NAMES.index("wgrowm_w16_c4_r2_v2")
M, K, NV = 1000, 257, 3  # a full group of two, bands through the workspace, and one vector through mvg_gemv_ata


def _spec(m, k, nv, variant=0):
    fa, fx = SO._synth_flat(m * k, 42), SO._synth_flat(k * nv, 4242)  # X: vector v at v * k
    if m and k:
        A = fa.reshape(m, k)
        At = np.ascontiguousarray(A.T)
        T = [oracle.multiply_std_rowwise(A, fx[v * k:(v + 1) * k]) for v in range(nv)]
        want = np.concatenate(T + [oracle.multiply_std_rowwise(At, t) for t in T])
    else:
        want = np.zeros((m + k) * nv)

    def call(lib, p, s):
        rc = lib.mvg_gemv_ata_multi_variant(p["A"], k, p["X"], k, p["Y"], m, p["Y"] + 8 * m * nv, k, m, k, nv, variant, s)
        SO._ok(lib, rc, "mvg_gemv_ata_multi")

    # an empty sum: nothing to read; the buffers exist so the pointers are real
    full = bool(m and k)
    return SO.Spec(ops={"A": fa, "X": fx} if full else {}, scratch={} if full else {"A": 2, "X": 2}, ny=(m + k) * nv,
                   call=call, want=want, bar="tol")


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        yield g


def test_the_fused_cases_are_a_full_group_in_several_bands_then_a_single_vector():
    for v in (WROWM, WGROWM):
        band_rows, bands, max_k, group = mm.gemv_ata_multi_plan(K, M, K, NV, v)
        assert bands > 1 and group == 2 and K <= max_k  # fused kernel into the workspace, then the reduce
        assert mm.gemv_ata_multi_plan(K, M, K, NV - group, v)[3] == 1  # then one vector through mvg_gemv_ata
    assert mm.gemv_t_multi_plan(K, M, K, NV)[1] > 1  # two_pass: the transposed half too


@pytest.mark.parametrize("m,k,variant", [(M, K, 0), (M, K, 1), (M, K, WROWM), (M, K, WGROWM), (0, K, 0), (M, 0, 0),
                                         (0, K, WROWM), (M, 0, WGROWM)],
                         ids=["auto", "two_pass", "wrowm", "wgrowm", "zeroing-m0", "zeroing-k0", "zeroing-m0-fused",
                              "zeroing-k0-fused"])
def test_gemv_ata_multi_runs_on_the_callers_stream(gate, m, k, variant):
    bad, _ = SO.run_case(gate, _spec(m, k, NV, variant))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("variant", [1, WROWM], ids=["two_pass", "wrowm"])
def test_positive_control_a_call_on_another_stream_is_seen(gate, variant):
    spec = _spec(M, K, NV, variant)
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad
