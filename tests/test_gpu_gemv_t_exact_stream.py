"""mvg_gemv_t_exact and mvg_gemv_t_exact_multi run on the caller's stream (stream
contract): the strip kernel over several tiles and strips, a staged form's second launch for the
strip cut by k, the groups and the single-vector tail of the multi call, and the m == 0 zeroing.
The gate, Spec, run_case and run_control are tests/stream_order.py's, unchanged, with the bar at
exact equality: the result behind the gate has the oracle's bits."""
import numpy as np
import pytest

import stream_order as SO
from matvec_mpi_multiplier_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu
lib = _lib.lib


def _names(count, name):
    return [name(v).decode() for v in range(count())]


STAGED = [v for v, n in enumerate(_names(lib.mvg_gemv_t_exact_variant_count, lib.mvg_gemv_t_exact_variant_name))
          if n.startswith("tseqx_")]
FUSED = [v for v, n in enumerate(_names(lib.mvg_gemv_t_exact_multi_variant_count, lib.mvg_gemv_t_exact_multi_variant_name))
         if n.startswith("tseqm_")]


def _ref(fa, m, k, z):
    return oracle.multiply_std_rowwise(np.ascontiguousarray(fa.reshape(m, k).T), z) if m else np.zeros(k)


def _spec(m, k, variant=0):
    fa, fz = SO._synth_flat(m * k, 42), SO._synth_flat(m, 4343)

    def call(lib, p, s):
        SO._ok(lib, lib.mvg_gemv_t_exact_variant(p["A"], k, p["z"], p["Y"], m, k, variant, s), "mvg_gemv_t_exact")

    # m == 0: nothing to read; the buffers exist so the pointers are real
    return SO.Spec(ops={"A": fa, "z": fz} if m else {}, scratch={} if m else {"A": 2, "z": 2}, ny=k, call=call,
                   want=_ref(fa, m, k, fz), bar="exact")


def _multi_spec(m, k, nv, variant=0):
    fa, fz = SO._synth_flat(m * k, 42), SO._synth_flat(max(m, 1) * nv, 4343)
    want = np.concatenate([_ref(fa, m, k, fz[v * m:(v + 1) * m]) for v in range(nv)])

    def call(lib, p, s):
        SO._ok(lib, lib.mvg_gemv_t_exact_multi_variant(p["A"], k, p["Z"], m, p["Y"], k, m, k, nv, variant, s),
               "mvg_gemv_t_exact_multi")

    return SO.Spec(ops={"A": fa, "Z": fz[:m * nv]} if m else {}, scratch={} if m else {"A": 2, "Z": 2}, ny=nv * k,
                   call=call, want=want, bar="exact")


@pytest.fixture(scope="module")
def gate():
    with SO.Gate(lib) as g:
        yield g


CASES = [("auto-1000x257", lambda: _spec(1000, 257)), ("zeroing-m0", lambda: _spec(0, 257))]
CASES += [(f"staged{v}-1000x258", lambda v=v: _spec(1000, 258, v)) for v in STAGED[:2]]  # whole strips + the cut strip
CASES += [("multi-auto-1000x257-nv5", lambda: _multi_spec(1000, 257, 5)), ("multi-zeroing-m0-nv3", lambda: _multi_spec(0, 257, 3))]
CASES += [(f"multi{v}-1000x257-nv7", lambda v=v: _multi_spec(1000, 257, 7, v)) for v in FUSED[:2]]  # groups + the tail


@pytest.mark.parametrize("make", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_runs_on_the_callers_stream(gate, make):
    bad, _ = SO.run_case(gate, make())
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("make", [lambda: _spec(1000, 257), lambda: _multi_spec(1000, 257, 5)], ids=["single", "multi"])
def test_positive_control_a_call_on_another_stream_is_seen(gate, make):
    spec = make()
    bad, y2, pending = SO.run_control(gate, spec)
    assert pending, "delay too short"
    assert not np.array_equal(y2, spec.want)
    assert bad and any(("NaN" in b) or ("overwrite" in b) or ("sentinel" in b) for b in bad), bad
