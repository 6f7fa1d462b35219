"""Stream order as a tested property: the case table and the gate harness.

include/matvec_gpu.h says of every kernel entry point "device pointers; asynchronous on
`stream`". Several entry points are more than one launch (split-K and its reduce through a
workspace, groups of vectors and a single-vector tail, a refused launch re-dispatched, a relayout
chained to the panel product); a piece issued on another stream than the caller's is invisible
on the null stream with a sync after every call. Here every call runs behind a gate:

  on the caller's non-blocking stream s, in this order and with no host wait in between
    1. a delay: pure GPU work (mvg_stream_read over one buffer, repeated) of >= DELAY_MS that
       always ends by itself (no host callback, nothing the host has to release);
    2. the producer: stream-ordered device-to-device copies of the real operands into operand
       buffers that hold NaN until then, and of EARLY over y;
    3. the library call(s) under test, given s;
    4. the consumer: a stream-ordered copy y -> y2 (y2 holds SENTINEL until then);
  and an event recorded right after the delay must still be pending once all of this has been
  enqueued ("delay too short" otherwise: a failure, never a skip).

A launch on any other stream runs while s is still inside the delay: it reads NaN operands, or
its result is overwritten by the producer's EARLY, or y2 keeps SENTINEL. `verdict` names which.
The result must be bit-identical to the same call made on the null stream with a sync after it,
and meet the oracle's bar of tests/test_gpu_parity.py (bit-exact for the exact, panel and combine
entries, TOL relative for the tree and multi entries on the non-negative oracle.synth data).

Before the gated run the same call runs once on s with NaN operands and a sync: the split-K
workspace of (device, s) is then allocated (its growth frees, and hipFree waits for the device:
behind the gate it would wait for the delay) and holds NaN partials, not an earlier run's sums.
"""
import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from conftest import max_rel

TOL = 1e-12          # tests/test_gpu_parity.py: relative, per element, on non-negative data
DELAY_MS = 20.0      # the gate's delay: three orders of magnitude over a launch's latency
DELAY_MARGIN = 2.5   # calibrated to DELAY_MARGIN x DELAY_MS: room for a host thread that is descheduled while it enqueues
SENTINEL = -1.0      # y2 before the consumer's copy
EARLY = 7.0          # what the producer writes over y: a result written before it is lost

HIP_STREAM_NON_BLOCKING = 1
HIP_MEMCPY_D2D = 3
HIP_SUCCESS = 0
HIP_ERROR_NOT_READY = 600


# ---------------------------------------------------------------- the NumPy side (no GPU)
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def verdict(y2, want, y_null, bar):
    """The failures of one gated result, named; empty for a result in stream order.
    y2: what the consumer copied out. want: the oracle's y. y_null: the same call on the null
    stream with a sync (None: not compared). bar: "exact" (bit for bit) or "tol" (TOL relative)."""
    assert bar in ("exact", "tol"), bar
    y2, want = np.asarray(y2, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if y2.shape != want.shape:
        return [f"shape {y2.shape} against {want.shape}"]
    bad = []
    n_sent = int(np.sum(_bits(y2) == _bits(np.array([SENTINEL]))[0]))
    if n_sent:
        bad.append(f"{n_sent} of {y2.size} still at the sentinel: the result was not there when the consumer ran")
    n_nan = int(np.sum(np.isnan(y2) & ~np.isnan(want)))
    if n_nan:
        bad.append(f"{n_nan} of {y2.size} NaN: computed from operands the producer had not written yet, or never written")
    n_early = int(np.sum((y2 == EARLY) & (want != EARLY)))
    if n_early:
        bad.append(f"{n_early} of {y2.size} hold the producer's overwrite: the result was written before the producer ran")
    if y_null is not None:
        y_null = np.asarray(y_null, dtype=np.float64).ravel()
        if y_null.shape != y2.shape or not np.array_equal(_bits(y2), _bits(y_null)):
            n = int(np.sum(_bits(y2) != _bits(y_null))) if y_null.shape == y2.shape else -1
            bad.append(f"{n} elements differ in bits from the null-stream run")
    if bar == "exact":
        if not np.array_equal(_bits(y2), _bits(want)):
            bad.append(f"{int(np.sum(_bits(y2) != _bits(want)))} elements differ in bits from the oracle")
    else:
        with np.errstate(invalid="ignore"):
            rel = max_rel(y2, want)
        if not rel <= TOL:  # NaN fails
            bad.append(f"max relative error {rel:.3e} against the oracle, bar {TOL:g}")
    return bad


# ---------------------------------------------------------------- the case table
@dataclass
class Spec:
    """One case's data: `ops` name -> real operand (flat; its device buffer holds NaN until the
    producer's copy), `scratch` name -> doubles of a NaN-filled device buffer no producer writes
    (an intermediate, or an operand the chain itself produces), ny doubles of y, call(lib, p, s)
    issuing the chain on stream s with p = name -> device address ("Y": y), `want` the oracle's
    y. arm(lib) runs before every run of the call (test hooks), disarm(lib) in a finally;
    pinned: name -> host array registered for the case; host_results() -> [(name, array)] the
    chain wrote on the host, held to the same bar."""
    ops: dict
    ny: int
    call: Callable
    want: np.ndarray
    bar: str
    scratch: dict = field(default_factory=dict)
    arm: Optional[Callable] = None
    disarm: Optional[Callable] = None
    pinned: dict = field(default_factory=dict)
    host_reset: Optional[Callable] = None
    host_results: Optional[Callable] = None
    after: Optional[Callable] = None  # after(lib): asserts on the library's state after the gated run


@dataclass
class Case:
    id: str
    entry: str
    why: str
    make: Callable  # () -> Spec (needs the oracle, not the GPU)
    reaches: Optional[tuple] = None  # (kind, args, how, text): the dispatch pick the case is there for


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.mvg_last_error().decode(errors="replace"))


def _synth_flat(n, seed):
    from oracle import oracle

    return oracle.synth(1, n, seed)[0] if n else np.zeros(0)


def _view(flat, off, m, k, lda):
    """Rows of k columns, lda apart, starting `off` doubles into `flat`."""
    return np.ascontiguousarray(flat[off + np.arange(m)[:, None] * lda + np.arange(k)[None, :]])


def _gemv_spec(entry, m, k, lda=None, off=0, variant=None, bar="tol"):
    """mvg_gemv / mvg_gemv_variant / mvg_gemv_exact on an m x k A with leading dimension lda, A and
    x starting `off` doubles into their buffers."""
    def make():
        from oracle import oracle

        ld = lda or k
        fa, fx = _synth_flat(m * ld + off, 42), _synth_flat(k + off, 4242)
        A, x = _view(fa, off, m, k, ld), fx[off:off + k]
        want = oracle.multiply_std_rowwise(A, x) if k else np.zeros(m)

        def call(lib, p, s):
            a, xx = p["A"] + 8 * off, p["x"] + 8 * off
            if entry == "mvg_gemv_variant":
                _ok(lib, lib.mvg_gemv_variant(a, ld, xx, p["Y"], m, k, variant, s), entry)
            else:
                _ok(lib, getattr(lib, entry)(a, ld, xx, p["Y"], m, k, s), entry)

        # k == 0: nothing to read; the buffers exist so the pointers are real
        return Spec(ops={"A": fa, "x": fx} if k else {}, scratch={} if k else {"A": 2, "x": 2}, ny=m, call=call,
                    want=want, bar=bar)
    return make


def _multi_spec(entry, m, k, nv, lda=None, bar="tol"):
    """mvg_gemv_multi / mvg_gemv_exact_multi: X nv x k (vector v at v*k), Y nv x m (ldy = m)."""
    def make():
        from oracle import oracle

        ld = lda or k
        fa = _synth_flat(m * ld, 42)
        A = _view(fa, 0, m, k, ld)
        X = oracle.synth(nv, k, 4242)
        want = np.concatenate([oracle.multiply_std_rowwise(A, X[v]) for v in range(nv)])

        def call(lib, p, s):
            _ok(lib, getattr(lib, entry)(p["A"], ld, p["X"], k, p["Y"], m, m, k, nv, s), entry)

        return Spec(ops={"A": fa, "X": X.ravel()}, ny=nv * m, call=call, want=want, bar=bar)
    return make


def _exact_hooked_spec(m, k, refuse):
    """mvg_gemv_exact planned for 4 CUs: the evenly placed form with its dynamic LDS; refuse: its
    LDS request set above the CU's 160 KiB, so that the runtime refuses the launch and the call
    re-dispatches to the one-wave form, every run anew (setting the hook forgets the refusal)."""
    def make():
        spec = _gemv_spec("mvg_gemv_exact", m, k, bar="exact")()
        name = lambda lib: lib.mvg_gemv_exact_variant_name(lib.mvg_gemv_exact_auto_variant(k, m, k)).decode()  # noqa: E731

        def arm(lib):
            _ok(lib, lib.mvg_debug_set_cu_count(4), "mvg_debug_set_cu_count")
            _ok(lib, lib.mvg_debug_set_exact_even_lds(200 * 1024 if refuse else 0), "mvg_debug_set_exact_even_lds")
            assert name(lib) == "hop8e_l8_w2_u16_n8", name(lib)

        def after(lib):  # the gated run itself took the path the case is there for
            assert name(lib) == ("hop8_l8_w2_u16" if refuse else "hop8e_l8_w2_u16_n8"), name(lib)

        def disarm(lib):
            lib.mvg_debug_set_cu_count(0)
            lib.mvg_debug_set_exact_even_lds(0)

        spec.arm, spec.after, spec.disarm = arm, after, disarm
        return spec
    return make


def _panel_spec(m, k, P):
    """mvg_panel_relayout then mvg_gemv_exact_panels, chained with no sync between them; the panel
    image holds NaN until the relayout writes it."""
    def make():
        from oracle import oracle

        assert k % P == 0  # no padded last panel: every double of the image is the relayout's
        A, x = oracle.synth(m, k, 42), _synth_flat(k, 4242)

        def call(lib, p, s):
            _ok(lib, lib.mvg_panel_relayout(p["A"], k, m, k, p["Ap"], m * P, P, s), "mvg_panel_relayout")
            _ok(lib, lib.mvg_gemv_exact_panels(p["Ap"], m * P, P, p["x"], p["Y"], m, k, 0, s), "mvg_gemv_exact_panels")

        return Spec(ops={"A": A.ravel(), "x": x}, scratch={"Ap": m * k}, ny=m, call=call,
                    want=oracle.multiply_std_rowwise(A, x), bar="exact")
    return make


def _combine_mpich_spec(P, n):
    def make():
        from oracle import oracle

        parts = oracle.synth(P, n, 42)

        def call(lib, p, s):  # overwrites the partials: every run gets them afresh
            _ok(lib, lib.mvg_debug_combine_mpich(p["parts"], P, n, p["Y"], s), "mvg_debug_combine_mpich")

        return Spec(ops={"parts": parts.ravel()}, ny=n, call=call, want=oracle.mpich_reduce(list(parts)), bar="exact")
    return make


def _combine_grid_spec(gr, gc, lr):
    def make():
        import adversarial_cases as AC
        from oracle import oracle

        parts = oracle.synth(gr * gc, lr, 42)

        def call(lib, p, s):
            _ok(lib, lib.mvg_debug_combine_grid_rows(p["parts"], gr, gc, lr, p["Y"], s), "mvg_debug_combine_grid_rows")

        return Spec(ops={"parts": parts.ravel()}, ny=gr * lr, call=call, want=AC.grid_rows_sum(parts, gr, gc),
                    bar="exact")
    return make


def _fill_then_gemv_spec(m, k):
    """mvg_synth_fill_device on s is the producer of A."""
    def make():
        from oracle import oracle

        A, x = oracle.synth(m, k, 42), _synth_flat(k, 4242)

        def call(lib, p, s):
            _ok(lib, lib.mvg_synth_fill_device(p["A"], k, m, k, 0, 0, k, 42, s), "mvg_synth_fill_device")
            _ok(lib, lib.mvg_gemv(p["A"], k, p["x"], p["Y"], m, k, s), "mvg_gemv")

        return Spec(ops={"x": x}, scratch={"A": m * k}, ny=m, call=call, want=oracle.multiply_std_rowwise(A, x),
                    bar="tol")
    return make


def _pinned_copies_spec(m, k):
    """mvg_memcpy_h2d of A and x from pinned host memory, mvg_gemv, mvg_memcpy_d2h of y into pinned
    host memory, all on s: the copies are the producer and a second consumer."""
    def make():
        from oracle import oracle

        A, x = oracle.synth(m, k, 42), _synth_flat(k, 4242)
        hA, hx, hy = np.ascontiguousarray(A.ravel()), np.ascontiguousarray(x), np.full(m, np.nan)

        def call(lib, p, s):
            _ok(lib, lib.mvg_memcpy_h2d(p["A"], hA.ctypes.data, hA.nbytes, s), "mvg_memcpy_h2d A")
            _ok(lib, lib.mvg_memcpy_h2d(p["x"], hx.ctypes.data, hx.nbytes, s), "mvg_memcpy_h2d x")
            _ok(lib, lib.mvg_gemv(p["A"], k, p["x"], p["Y"], m, k, s), "mvg_gemv")
            _ok(lib, lib.mvg_memcpy_d2h(hy.ctypes.data, p["Y"], hy.nbytes, s), "mvg_memcpy_d2h")

        def host_reset():
            hy[:] = np.nan

        return Spec(ops={}, scratch={"A": m * k, "x": k}, ny=m, call=call, want=oracle.multiply_std_rowwise(A, x),
                    bar="tol", pinned={"A": hA, "x": hx, "y": hy}, host_reset=host_reset,
                    host_results=lambda: [("pinned y", hy.copy())])
    return make


def split_variants(lib):
    """The tree variants that are two launches and a workspace."""
    names = [(v, lib.mvg_gemv_variant_name(v).decode()) for v in range(1, lib.mvg_gemv_variant_count())]
    return [(v, n) for v, n in names if n.endswith("_splitk")]


def scalar_variants(lib):
    return [(v, lib.mvg_gemv_variant_name(v).decode()) for v in range(1, lib.mvg_gemv_variant_count())
            if lib.mvg_gemv_variant_name(v).decode().startswith("scl_")]


def cases(lib):
    """The table. Shapes are the smallest that reach each multi-launch path, hand-derived from
    pick_variant, pick_multi_variant (csrc/gemv.hip), pick_seq_variant and pick_seq_multi_variant
    (csrc/gemv_exact.hip); `reaches` restates the pick, tests/test_stream_order_host.py holds it."""
    G, M, E, EM = "gemv", "multi", "exact", "exact_multi"
    out = [
        Case("gemv-64x16384", "mvg_gemv", "auto split-K: two kernels and the workspace",
             _gemv_spec("mvg_gemv", 64, 16384), (G, (16384, 64, 16384), "eq", "rowblk_w4_r2_u4_splitk")),
        Case("gemv-2049x512", "mvg_gemv", "one row per wave",
             _gemv_spec("mvg_gemv", 2049, 512), (G, (512, 2049, 512), "eq", "vec_l64_r1_u4_nt1_o5")),
        Case("gemv-257x1000", "mvg_gemv", "row per workgroup",
             _gemv_spec("mvg_gemv", 257, 1000), (G, (1000, 257, 1000), "prefix", "rowblk_")),
        Case("gemv-4100x6150", "mvg_gemv", "rows off the 128-B lines (lda % 16 != 0)",
             _gemv_spec("mvg_gemv", 4100, 6150), (G, (6150, 4100, 6150), "eq", "rowlines_w8_u4_x0")),
        Case("gemv-70x301-lda301", "mvg_gemv", "odd lda: unaligned 16-B loads",
             _gemv_spec("mvg_gemv", 70, 301, lda=301), (G, (301, 70, 301), "eq", "vec_l64_r4_u4_nt1_o0")),
        # 8 bytes off a 16-B boundary is still 8-B aligned: the dispatch keeps the 16-B kernels'
        # unaligned loads (the 8-B kernels serve only pointers off 8 B; they run by name below)
        Case("gemv-70x301-lda301-off8", "mvg_gemv", "odd lda, A and x 8 B off a 16-B boundary",
             _gemv_spec("mvg_gemv", 70, 301, lda=301, off=1)),
        Case("gemv-16x0", "mvg_gemv", "k = 0: zero_kernel, y must be zeros", _gemv_spec("mvg_gemv", 16, 0, bar="exact")),
    ]
    for v, name in scalar_variants(lib):
        out.append(Case(f"gemv-70x301-off8-{name}", "mvg_gemv_variant", "the 8-B kernels",
                        _gemv_spec("mvg_gemv_variant", 70, 301, lda=301, off=1, variant=v)))
    for v, name in split_variants(lib):
        out.append(Case(f"gemv-130x16388-{name}", "mvg_gemv_variant", "explicit split form",
                        _gemv_spec("mvg_gemv_variant", 130, 16388, variant=v)))
    out += [
        Case("multi-130x4226-nv11", "mvg_gemv_multi", "8 + 3: two passes",
             _multi_spec("mvg_gemv_multi", 130, 4226, 11), (M, (4226, 4226, 130, 4226, 11), "noprefix", "m16_")),
        Case("multi-130x4226-nv9", "mvg_gemv_multi", "8, then the single-vector tail through mvg_gemv_variant",
             _multi_spec("mvg_gemv_multi", 130, 4226, 9), (M, (4226, 4226, 130, 4226, 9), "noprefix", "m16_")),
        Case("multi-8203x1058-nv13", "mvg_gemv_multi", "m16_*: one pass of 13",
             _multi_spec("mvg_gemv_multi", 8203, 1058, 13), (M, (1058, 1058, 8203, 1058, 13), "prefix", "m16_")),
        # what is left after a pass of 16 goes out as another m16 pass while it is 9 .. 16 vectors,
        # so 25 is 16 + 9; the single-vector tail after an m16 pass is nv = 17
        Case("multi-8203x1058-nv25", "mvg_gemv_multi", "m16_*: 16 + 9",
             _multi_spec("mvg_gemv_multi", 8203, 1058, 25), (M, (1058, 1058, 8203, 1058, 25), "prefix", "m16_")),
        Case("multi-8203x1058-nv17", "mvg_gemv_multi", "m16_*: 16, then the single-vector tail",
             _multi_spec("mvg_gemv_multi", 8203, 1058, 17), (M, (1058, 1058, 8203, 1058, 17), "prefix", "m16_")),
        Case("multi-70x301-lda301-nv5", "mvg_gemv_multi", "odd lda: per-vector fallback, five launches",
             _multi_spec("mvg_gemv_multi", 70, 301, 5, lda=301)),
        Case("exact-6144x800-4cu", "mvg_gemv_exact", "evenly placed form, dynamic LDS",
             _exact_hooked_spec(6144, 800, refuse=False), ("exact@4cu", (800, 6144, 800), "eq", "hop8e_l8_w2_u16_n8")),
        Case("exact-6144x800-4cu-refused", "mvg_gemv_exact", "LDS refusal, then re-dispatch on the same stream",
             _exact_hooked_spec(6144, 800, refuse=True), ("exact@4cu", (800, 6144, 800), "eq", "hop8e_l8_w2_u16_n8")),
        Case("exact-2049x512", "mvg_gemv_exact", "hop form", _gemv_spec("mvg_gemv_exact", 2049, 512, bar="exact"),
             (E, (512, 2049, 512), "prefix", "hop")),
        Case("exact-300x5000", "mvg_gemv_exact", "hop form, few long rows",
             _gemv_spec("mvg_gemv_exact", 300, 5000, bar="exact"), (E, (5000, 300, 5000), "prefix", "hop")),
        Case("exact-multi-6150x64-nv7", "mvg_gemv_exact_multi", "4 + 2 + mvg_gemv_exact for the last",
             _multi_spec("mvg_gemv_exact_multi", 6150, 64, 7, bar="exact"), (EM, (64, 64, 6150, 64, 7), "hopm_v", "4")),
        Case("exact-multi-257x1000-nv3", "mvg_gemv_exact_multi", "separate: three single passes",
             _multi_spec("mvg_gemv_exact_multi", 257, 1000, 3, bar="exact"),
             (EM, (1000, 1000, 257, 1000, 3), "eq", "separate")),
        Case("panels-6144x1024-P256", "mvg_panel_relayout -> mvg_gemv_exact_panels", "chained, NaN panel image",
             _panel_spec(6144, 1024, 256)),
        Case("panels-6144x1024-P32", "mvg_panel_relayout -> mvg_gemv_exact_panels", "chained, NaN panel image",
             _panel_spec(6144, 1024, 32)),
        Case("combine-mpich-P5-n100", "mvg_debug_combine_mpich", "binomial tree (<= 2 KiB)", _combine_mpich_spec(5, 100)),
        Case("combine-mpich-P5-n300", "mvg_debug_combine_mpich", "reduce-scatter + gather (> 2 KiB)",
             _combine_mpich_spec(5, 300)),
        Case("combine-grid-2x3-lr300", "mvg_debug_combine_grid_rows", "grid rows", _combine_grid_spec(2, 3, 300)),
        Case("fill-gemv-257x1000", "mvg_synth_fill_device -> mvg_gemv", "the fill on s is the producer",
             _fill_then_gemv_spec(257, 1000)),
        Case("pinned-copies-gemv-257x1000", "mvg_memcpy_h2d -> mvg_gemv -> mvg_memcpy_d2h", "the copies on s",
             _pinned_copies_spec(257, 1000)),
    ]
    assert len({c.id for c in out}) == len(out)
    return out


def pick_name(lib, kind, args):
    """The name of the automatic pick a case's `reaches` is about (host logic: no device)."""
    if kind == "gemv":
        return lib.mvg_gemv_variant_name(lib.mvg_gemv_auto_variant(*args)).decode()
    if kind == "multi":
        return lib.mvg_gemv_multi_variant_name(lib.mvg_gemv_multi_auto_variant(*args)).decode()
    if kind == "exact":
        return lib.mvg_gemv_exact_variant_name(lib.mvg_gemv_exact_auto_variant(*args)).decode()
    if kind == "exact@4cu":
        assert lib.mvg_debug_set_cu_count(4) == 0
        try:
            return lib.mvg_gemv_exact_variant_name(lib.mvg_gemv_exact_auto_variant(*args)).decode()
        finally:
            lib.mvg_debug_set_cu_count(0)
    if kind == "exact_multi":
        return lib.mvg_gemv_exact_multi_variant_name(lib.mvg_gemv_exact_multi_auto_variant(*args)).decode()
    raise ValueError(kind)


def reaches_ok(name, how, text):
    if how == "eq":
        return name == text
    if how == "prefix":
        return name.startswith(text)
    if how == "noprefix":
        return not name.startswith(text)
    if how == "hopm_v":  # hopm_l<L>_w<W>_u<U>_v<NV>
        return name.startswith("hopm_") and name.endswith("_v" + text)
    raise ValueError(how)


# ---------------------------------------------------------------- the HIP runtime, through ctypes
def hip_runtime():
    """The HIP runtime the library is bound to (tests/test_gpu_exact.py's handle), with the
    signatures of the calls the harness makes."""
    from test_gpu_exact import _hip_runtime

    hip = _hip_runtime()
    p, pp, u = C.c_void_p, C.POINTER(C.c_void_p), C.c_uint
    for name, args in {
        "hipStreamCreateWithFlags": [pp, u], "hipStreamGetFlags": [p, C.POINTER(u)], "hipStreamDestroy": [p],
        "hipMemcpyAsync": [p, p, C.c_size_t, C.c_int, p], "hipEventCreate": [pp], "hipEventRecord": [p, p],
        "hipEventQuery": [p], "hipEventSynchronize": [p], "hipEventDestroy": [p],
        "hipEventElapsedTime": [C.POINTER(C.c_float), p, p],
    }.items():
        fn = getattr(hip, name)
        fn.restype, fn.argtypes = C.c_int, args
    return hip


class Gate:
    """Two non-blocking streams (s: the caller's; t: the wrong one of the positive control), the
    delay's buffer and the number of mvg_stream_read launches that make DELAY_MS. Use as a
    context manager: streams, events and buffers are released on the way out."""

    DELAY_DOUBLES = 1 << 26  # 512 MiB per launch: far above a launch's enqueue cost, so the
    #                          delay is the kernels' run time and not the host's enqueueing

    def __init__(self, lib):
        self.lib = lib
        self.hip = hip_runtime()
        self.streams, self.events, self.buffers = [], [], []
        self.launches, self.delay_ms = 0, 0.0

    def __enter__(self):
        from matvec_mpi_multiplier_amd import multiplier as mm

        try:
            self.s, self.t = self.stream(), self.stream()
            self.delay_buf, self.sink = mm.DeviceBuffer(self.DELAY_DOUBLES), mm.DeviceBuffer(1024)
            self.buffers += [self.delay_buf, self.sink]
            side = 1 << 13
            assert side * side == self.DELAY_DOUBLES
            _ok(self.lib, self.lib.mvg_synth_fill_device(self.delay_buf.ptr, side, side, side, 0, 0, side, 1, None),
                "fill delay")
            _ok(self.lib, self.lib.mvg_stream_sync(None), "sync")
            self.ev_delay, self.ev_done = self.event(), self.event()
            self.calibrate()
        except BaseException:
            self.close()
            raise
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for s in self.streams:
            self.lib.mvg_stream_sync(s)
        for e in self.events:
            self.hip.hipEventDestroy(e)
        for s in self.streams:
            self.hip.hipStreamDestroy(s)
        for b in self.buffers:
            b.free()
        self.streams, self.events, self.buffers = [], [], []

    def stream(self):
        s = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(s), HIP_STREAM_NON_BLOCKING) == HIP_SUCCESS
        assert s.value
        self.streams.append(s.value)
        flags = C.c_uint(0xFFFF)
        assert self.hip.hipStreamGetFlags(s.value, C.byref(flags)) == HIP_SUCCESS
        # a blocking stream would synchronise with the null stream and hide what is looked for
        assert flags.value & HIP_STREAM_NON_BLOCKING, flags.value
        return s.value

    def event(self):
        e = C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(e)) == HIP_SUCCESS
        self.events.append(e.value)
        return e.value

    def delay(self, s, launches=None):
        for _ in range(launches or self.launches):
            _ok(self.lib, self.lib.mvg_stream_read(self.delay_buf.ptr, self.DELAY_DOUBLES, self.sink.ptr, s),
                "mvg_stream_read")

    def timed_delay(self, launches):
        hip, a, b = self.hip, self.ev_delay, self.ev_done
        assert hip.hipEventRecord(a, self.s) == HIP_SUCCESS
        self.delay(self.s, launches)
        assert hip.hipEventRecord(b, self.s) == HIP_SUCCESS
        assert hip.hipEventSynchronize(b) == HIP_SUCCESS
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), a, b) == HIP_SUCCESS
        return float(ms.value)

    def calibrate(self):
        """The launch count whose measured run time is >= DELAY_MARGIN x DELAY_MS (clocks that rise
        after the calibration shorten it; the event query of every gated run is the guard)."""
        self.timed_delay(16)  # first use: code object load, clocks
        per = self.timed_delay(32) / 32
        assert per > 0
        target = DELAY_MARGIN * DELAY_MS
        n = max(int(math.ceil(target / per)), 8)
        for _ in range(4):
            ms = self.timed_delay(n)
            if ms >= target:
                self.launches, self.delay_ms = n, ms
                return
            n = int(math.ceil(n * target / ms)) + 1
        raise AssertionError(f"no delay of {target} ms from {n} launches of mvg_stream_read")

    def copy(self, dst, src, nbytes, s):
        if nbytes:
            assert self.hip.hipMemcpyAsync(dst, src, nbytes, HIP_MEMCPY_D2D, s) == HIP_SUCCESS

    def sync(self, s):
        _ok(self.lib, self.lib.mvg_stream_sync(s), "mvg_stream_sync")


class CaseBuffers:
    """The device side of one Spec: per operand a buffer the calls read and a source holding the
    real values, the scratch buffers, y, y2 and the source of the producer's overwrite of y."""

    def __init__(self, spec):
        from matvec_mpi_multiplier_amd import multiplier as mm

        self.spec, self.all = spec, []
        try:
            new = lambda n: self._keep(mm.DeviceBuffer(n + 32))  # noqa: E731  (slack: clamped loads past a last row)
            self.dst = {k: new(v.size) for k, v in spec.ops.items()}
            self.src = {k: new(v.size).upload(v) for k, v in spec.ops.items()}
            self.scratch = {k: new(n) for k, n in spec.scratch.items()}
            self.y, self.y2 = new(spec.ny), new(spec.ny)
            self.early = new(spec.ny).upload(np.full(spec.ny, EARLY))
        except BaseException:
            self.free()
            raise
        self.p = {**{k: b.ptr for k, b in self.dst.items()}, **{k: b.ptr for k, b in self.scratch.items()}, "Y": self.y.ptr}

    def _keep(self, b):
        self.all.append(b)
        return b

    def free(self):
        for b in self.all:
            b.free()
        self.all = []

    def reset(self):
        """The start state, synchronised: NaN in every operand, scratch buffer and y, the
        sentinel in y2."""
        for b in list(self.dst.values()) + list(self.scratch.values()) + [self.y]:
            b.upload(np.full(b.n, np.nan))
        self.y2.upload(np.full(self.y2.n, SENTINEL))
        if self.spec.host_reset:
            self.spec.host_reset()

    def load(self):
        """The real operands where the calls read them (for the null-stream run)."""
        for k, v in self.spec.ops.items():
            self.dst[k].upload(v)

    def produce(self, gate, s):
        for k, v in self.spec.ops.items():
            gate.copy(self.dst[k].ptr, self.src[k].ptr, v.size * 8, s)
        gate.copy(self.y.ptr, self.early.ptr, self.spec.ny * 8, s)

    def consume(self, gate, s):
        gate.copy(self.y2.ptr, self.y.ptr, self.spec.ny * 8, s)


def gated_run(gate, bufs, on=None):
    """Steps 2-7 on gate.s from the synchronised start state; the call under test goes to stream
    `on` (default gate.s; gate.t is the positive control's wrong stream). Returns (y2, pending):
    pending is whether the event after the delay had not completed when everything was enqueued."""
    lib, hip, s, spec = gate.lib, gate.hip, gate.s, bufs.spec
    f_stream = s if on is None else on
    try:
        gate.delay(s)
        assert hip.hipEventRecord(gate.ev_delay, s) == HIP_SUCCESS
        bufs.produce(gate, s)
        spec.call(lib, bufs.p, f_stream)
        bufs.consume(gate, s)
        assert hip.hipEventRecord(gate.ev_done, s) == HIP_SUCCESS
        q = hip.hipEventQuery(gate.ev_delay)
    finally:  # nothing stays queued behind a failure
        lib.mvg_stream_sync(f_stream)
        lib.mvg_stream_sync(s)
    assert q in (HIP_SUCCESS, HIP_ERROR_NOT_READY), q
    return bufs.y2.download(spec.ny), q == HIP_ERROR_NOT_READY


def run_case(gate, spec):
    """The null-stream run, the run on s that allocates (NaN operands), the gated run. Returns
    (failures, y2): the verdict's list, with "delay too short" in it where the guard failed."""
    lib = gate.lib
    arm = spec.arm or (lambda _lib: None)
    pinned = []
    bufs = None
    try:
        for a in spec.pinned.values():
            _ok(lib, lib.mvg_host_register(a.ctypes.data, a.nbytes), "mvg_host_register")
            pinned.append(a)
        bufs = CaseBuffers(spec)
        arm(lib)
        bufs.reset()
        bufs.load()
        spec.call(lib, bufs.p, None)
        gate.sync(None)
        y_null = bufs.y.download(spec.ny)
        arm(lib)
        bufs.reset()
        spec.call(lib, bufs.p, gate.s)
        gate.sync(gate.s)
        arm(lib)
        bufs.reset()
        y2, pending = gated_run(gate, bufs)
        if spec.after:
            spec.after(lib)
        bad = [] if pending else ["delay too short: the event after the delay had completed when the consumer was enqueued"]
        bad += verdict(y2, spec.want, y_null, spec.bar)
        for name, arr in (spec.host_results() if spec.host_results else []):
            bad += [f"{name}: {b}" for b in verdict(arr, spec.want, y_null, spec.bar)]
        return bad, y2
    finally:
        if bufs is not None:
            bufs.free()
        for a in pinned:
            lib.mvg_host_unregister(a.ctypes.data)
        if spec.disarm:
            spec.disarm(lib)


def run_control(gate, spec):
    """The positive control: the same sequence with the call on gate.t while gate.s is delayed.
    Returns (failures, y2, pending); the failures must not be empty."""
    bufs = CaseBuffers(spec)
    try:
        bufs.reset()
        spec.call(gate.lib, bufs.p, gate.t)  # allocations outside the gate, NaN operands
        gate.sync(gate.t)
        bufs.reset()
        y2, pending = gated_run(gate, bufs, on=gate.t)
        return verdict(y2, spec.want, None, spec.bar), y2, pending
    finally:
        bufs.free()
