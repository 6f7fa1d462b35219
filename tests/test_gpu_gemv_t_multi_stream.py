"""mvg_gemv_t_multi runs on the caller's stream (stream contract): a fused group's strip
kernel, its band reduce out of the per-(device, stream) workspace, the single leftover vector, the
m == 0 zeroing and `separate`. The gate, Spec and run_case are tests/stream_order.py's, unchanged:
one delay of >= 20 ms on a non-blocking stream with the operands' producer, the call and the
result's consumer enqueued behind it, so a launch on any other stream computes from NaN or is
overwritten."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib
from matvec_mpi_multiplier_amd import multiplier as mm
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib
NAMES = [lib.mvg_gemv_t_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_t_multi_variant_count())]
FUSED4 = NAMES.index("tstripm_w4_c2_u4_v4")
SEPARATE = NAMES.index("separate")
M, K, NV = 1000, 257, 5  # a group of four, bands through the workspace, and one vector through mvg_gemv_t


def _spec(m, k, nv, variant):
    fa, fz = SO._synth_flat(m * k, 42), SO._synth_flat(m * nv, 4343)  # Z: vector v at v * m
    if m:
        At = np.ascontiguousarray(fa.reshape(m, k).T)
        want = np.concatenate([oracle.multiply_std_rowwise(At, fz[v * m:(v + 1) * m]) for v in range(nv)])
    else:
        want = np.zeros(nv * k)

    def call(lib, p, s):
        SO._ok(lib, lib.mvg_gemv_t_multi_variant(p["A"], k, p["Z"], m, p["Y"], k, m, k, nv, variant, s), "mvg_gemv_t_multi")

    # m == 0: nothing to read; the buffers exist so the pointers are real
    return SO.Spec(ops={"A": fa, "Z": fz} if m else {}, scratch={} if m else {"A": 2, "Z": 2}, ny=nv * k, call=call,
                   want=want, bar="tol")


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        yield g


def test_the_multi_band_shape_has_more_than_one_band():
    band_rows, bands, strip_cols, group = mm.gemv_t_multi_plan(K, M, K, NV, FUSED4)
    assert bands > 1 and group == 4  # strip kernel into the workspace, then the reduce
    assert mm.gemv_t_multi_plan(K, M, K, NV - group, FUSED4)[3] == 1  # then one vector through mvg_gemv_t


@pytest.mark.parametrize("m,variant", [(M, FUSED4), (0, FUSED4), (0, 0), (M, SEPARATE), (M, 0)],
                         ids=["fused-bands-1000x257x5", "zeroing-m0-fused", "zeroing-m0", "separate", "auto"])
def test_gemv_t_multi_runs_on_the_callers_stream(gate, m, variant):
    bad, _ = SO.run_case(gate, _spec(m, K, NV, variant))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("variant", [FUSED4, SEPARATE], ids=["fused", "separate"])
def test_positive_control_a_call_on_another_stream_is_seen(gate, variant):
    spec = _spec(M, K, NV, variant)
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad
