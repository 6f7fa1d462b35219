"""Wide views for the kernels' address arithmetic: small payloads inside one large, sparsely
written device allocation.

The kernel tests elsewhere use lda <= k + 16 and a few hundred rows, so every offset a kernel
computes fits 32 bits with room to spare. Here a row, a vector or a panel sits 2^31 .. 2^35 bytes
from its operand's base, and the forms that keep 32-bit per-lane offsets on purpose (gemv_seq,
gemv_seq_x, gemv_mdma, gemv_mdma16) run at the largest strides their host checks let through.

The arena is one allocation of 2^32 + 2^28 doubles (34 GiB), every byte 0xFF: each double a NaN.
A `WideOperand` holds `nvec` vectors of `n` payload doubles, `ld` doubles apart, and writes, poisons
and reads them vector by vector, each with a fringe of 16 NaNs on either side; the span between the
vectors is never touched by the host and never materialised. What a kernel reads from a wrong
address is therefore another vector's payload (the payloads differ in every element:
adversarial_cases.payload(sign=True)) or NaN, and a store to a wrong address lands in another
vector's payload, in a fringe, or in the untouched fill.

The views, and what each crosses (`thresholds`: the first vector index whose offset reaches the
limit, None where no vector does; tests/test_wide_views_host.py asserts this table):

    view         ld         vectors     2^31 B  2^32 B  2^31 el  2^32 el
    LIMIT_A      2^23 - 2   67 rows       33      65      -        -      rows 33..63 of tile 0
    LIMIT_A64    2^22 - 2   67 rows       65       -      -        -      64 * lda * 8 = 2^31 - 1024
    LIMIT_A16    2^24 - 2   67 rows       17      33      -        -      16 * lda * 8 = 2^31 - 256
    FAR_A        2^26       67 rows        4       8     32       64
    FAR_A_ODD    2^26 - 3   67 rows        5       9     33       65      odd lda
    FAR_A_OFF8   2^26 + 2   67 rows        4       8     32       64      A and x 8 B off 16 B
    LIMIT_X16    2^24 - 2   16 vectors     -       -      -        -      16 * ldx * 8 = 2^31 - 256
    LIMIT_X8     2^25 - 2    8 vectors     -       -      -        -       8 * ldx * 8 = 2^31 - 128
    FAR_X        2^28       16 vectors     1       2      8        -
    FAR_Y        2^28       16 vectors     1       2      8        -
    FAR_PANELS   2^29        9 panels      1       1      4        8      (P = 16, k = 130)

LIMIT_A is the largest even lda the LDS-DMA exact forms (lda < 2^23) and the 32-row DMA multi forms
(32 * lda * 8 < 2^31) accept: row 63 of a 64-row tile is 4 227 857 424 bytes from the tile's base,
past 2^31 and under 2^32, so the per-lane offset must be zero-extended. LIMIT_A64 and LIMIT_A16
are the same for the 64-row and the 16-row DMA multi forms, so that each of them runs at the
largest lda its own check lets through. The LIMIT_X views are the largest ldx of the 16- and the
8-vector DMA forms (nvec * ldx * 8 < 2^31): by construction nothing in them passes 2^31 bytes,
they show that the limit the host enforces is one the kernel can take.
FAR_A's power-of-two stride is deliberate: an offset truncated to 32 bits lands on another row's
payload (row 8 on row 0).

`TRUNCATIONS` is the host model of the four mistakes (the byte offset or the element index of a
vector, kept in an int32 or a uint32); `gather` / `scatter` apply one to a `SparseImage`, the host
stand-in for the arena (a dict of written ranges, NaN elsewhere). tests/test_wide_views_host.py
shows with them that every far view tells every truncation from the right answer.
"""
import re

import numpy as np

import gpu_guarded as G

ARENA_DOUBLES = (1 << 32) + (1 << 28)
FRINGE = G.GUARD
M = 67  # rows of every A here: one 64-row tile and three rows of the next


class View:
    """nvec vectors ld doubles apart; shift (doubles) moves the operand off its 16-B boundary."""

    def __init__(self, name, ld, nvec, shift=0):
        self.name, self.ld, self.nvec, self.shift = name, int(ld), int(nvec), int(shift)

    def __repr__(self):
        return self.name

    def offset(self, v):
        """Vector v's first double, in doubles from the operand's base."""
        return v * self.ld

    def first_at(self, limit_bytes=None, limit_elems=None):
        """The first vector whose offset reaches the limit, None when none does."""
        limit = limit_elems if limit_bytes is None else -(-limit_bytes // 8)
        v = -(-limit // self.ld)
        return v if v < self.nvec else None

    def thresholds(self):
        return {"2^31 B": self.first_at(limit_bytes=1 << 31), "2^32 B": self.first_at(limit_bytes=1 << 32),
                "2^31 el": self.first_at(limit_elems=1 << 31), "2^32 el": self.first_at(limit_elems=1 << 32)}


LIMIT_A = View("LIMIT_A", (1 << 23) - 2, M)
LIMIT_A64 = View("LIMIT_A64", (1 << 22) - 2, M)
LIMIT_A16 = View("LIMIT_A16", (1 << 24) - 2, M)
FAR_A = View("FAR_A", 1 << 26, M)
FAR_A_ODD = View("FAR_A_ODD", (1 << 26) - 3, M)
FAR_A_OFF8 = View("FAR_A_OFF8", (1 << 26) + 2, M, shift=1)
LIMIT_X16 = View("LIMIT_X16", (1 << 24) - 2, 16)
LIMIT_X8 = View("LIMIT_X8", (1 << 25) - 2, 8)
FAR_X = View("FAR_X", 1 << 28, 16)
FAR_Y = View("FAR_Y", 1 << 28, 16)
PANEL_K = 130
FAR_PANELS = View("FAR_PANELS", 1 << 29, -(-PANEL_K // 16))

A_VIEWS = (LIMIT_A, LIMIT_A64, LIMIT_A16, FAR_A, FAR_A_ODD, FAR_A_OFF8)
X_VIEWS = (LIMIT_X16, LIMIT_X8, FAR_X)
FAR_VIEWS = (FAR_A, FAR_A_ODD, FAR_A_OFF8, FAR_X, FAR_Y, FAR_PANELS)
LIMIT_VIEWS = (LIMIT_A, LIMIT_A64, LIMIT_A16, LIMIT_X16, LIMIT_X8)
VIEWS = FAR_VIEWS + LIMIT_VIEWS


# ------------------------------------------------------------------ the truncation model
def _wrap32(v, signed):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if signed and v >= (1 << 31) else v


# offset in doubles -> the offset a kernel with that mistake would use
TRUNCATIONS = {
    "int32 bytes": lambda e: _wrap32(8 * e, True) // 8,
    "uint32 bytes": lambda e: _wrap32(8 * e, False) // 8,
    "int32 elements": lambda e: _wrap32(e, True),
    "uint32 elements": lambda e: _wrap32(e, False),
}


def moved(view, trunc):
    """The vectors whose address the truncation changes."""
    return [v for v in range(view.nvec) if TRUNCATIONS[trunc](view.offset(v)) != view.offset(v)]


class SparseImage:
    """The arena on the host: the written ranges, NaN everywhere else (outside it too: a model of
    what is read, not of what faults)."""

    def __init__(self):
        self.ranges = {}

    def write(self, start, values):
        self.ranges[int(start)] = np.array(values, dtype=np.float64)

    def read(self, start, n):
        out = np.full(n, np.nan)
        for s, vals in self.ranges.items():
            lo, hi = max(s, start), min(s + vals.size, start + n)
            if lo < hi:
                out[lo - start:hi - start] = vals[lo - s:hi - s]
        return out


def place(view, payload, base=0):
    """A SparseImage with the payload's vectors where the view puts them."""
    img = SparseImage()
    for v in range(view.nvec):
        img.write(base + view.shift + view.offset(v), payload[v])
    return img


def gather(img, view, n, trunc=None, base=0):
    """What a kernel reads as the view's vectors (nvec x n), its vector offsets truncated."""
    f = TRUNCATIONS[trunc] if trunc else (lambda e: e)
    return np.stack([img.read(base + view.shift + f(view.offset(v)), n) for v in range(view.nvec)])


def scatter(view, values, trunc=None, base=0):
    """The image a kernel leaves that stores the view's vectors with truncated vector offsets
    (later vectors overwrite earlier ones, as a store that lands on vector 0 or 1 would)."""
    f = TRUNCATIONS[trunc] if trunc else (lambda e: e)
    img = SparseImage()
    for v in range(view.nvec):
        img.write(base + view.shift + f(view.offset(v)), values[v])
    return img


def operand_image(img, view, n, base=0):
    """The payload-plus-fringe image WideOperand.image() would download from `img`, and its
    layout for gpu_guarded's checkers."""
    rows = [img.read(base + view.shift + view.offset(v) - FRINGE, n + 2 * FRINGE) for v in range(view.nvec)]
    return np.concatenate(rows + [np.full(2 * FRINGE, np.nan)]), G.Layout(view.nvec, n, n + 2 * FRINGE)


# ------------------------------------------------------------------ which form takes which layout
def dma_rows(name):
    """Rows per workgroup of the LDS-DMA multi forms, from the name: mdma_r<RQ>..., m16_r<RQ>... ->
    16 * RQ; None for every other form."""
    mt = re.match(r"(mdma|m16)_r(\d+)_", name)
    return 16 * int(mt.group(2)) if mt else None


def dma_ok(name, lda, ldx):
    """The host check of the DMA multi forms (gemv.hip dma_ok): the workgroup's rows of A and the
    pass's vectors of X (16 for m16_*, else 8) within 2^31 bytes."""
    nvec = 16 if name.startswith("m16_") else 8
    return dma_rows(name) * lda * 8 < (1 << 31) and nvec * ldx * 8 < (1 << 31)


def needs_16b(name):
    """test_gpu_exact.needs_16b (restated: this module is imported without a device too)."""
    return name.startswith(("seq_r", "seqx_", "hop_"))


def lds_dma_exact(name):
    """The exact forms with 32-bit per-lane offsets over 64 rows of lda: lda < 2^23."""
    return name.startswith(("seq_r", "seqx_"))


def refuses(family, name, lda, ldx=2, off16=False, k=0):
    """Whether the form turns the layout down (MVG_E_INVALID, nothing launched). off16: A or x
    is 8 bytes off a 16-B boundary."""
    if name == "auto" or family in ("tree", "exact_multi"):
        return False
    if family == "exact":
        return bool((needs_16b(name) and (lda % 2 or off16)) or (lds_dma_exact(name) and lda >= (1 << 23)) or
                    (name.startswith("hopxl_") and k > 8192))
    assert family == "multi", family
    return bool(lda % 2 or ldx % 2 or off16 or (dma_rows(name) and not dma_ok(name, lda, ldx)))


def family_names(family):
    """Every variant name of the family, from the library's own count and name calls."""
    from matvec_mpi_multiplier_amd import _lib

    lib = _lib.lib
    count, name = {"tree": (lib.mvg_gemv_variant_count, lib.mvg_gemv_variant_name),
                   "exact": (lib.mvg_gemv_exact_variant_count, lib.mvg_gemv_exact_variant_name),
                   "multi": (lib.mvg_gemv_multi_variant_count, lib.mvg_gemv_multi_variant_name),
                   "exact_multi": (lib.mvg_gemv_exact_multi_variant_count, lib.mvg_gemv_exact_multi_variant_name),
                   "panels": (lib.mvg_gemv_exact_panel_variant_count, lib.mvg_gemv_exact_panel_variant_name)}[family]
    names = [name(v).decode() for v in range(count())]
    assert names[0] == "auto" and len(set(names)) == len(names) > 1, names
    return names


def live_names(family, view, role, k):
    """The names that run (do not refuse) with the view as operand `role` ("A" or "X"), the other
    operands narrow: lda resp. ldx = k + 2, aligned unless the view shifts (then A and x both)."""
    lda, ldx = (view.ld, k + 2) if role == "A" else (k + 2, view.ld)
    return [n for n in family_names(family) if not refuses(family, n, lda, ldx, bool(view.shift), k)]


# ------------------------------------------------------------------ device side
def default_base(span):
    """Where an operand of `span` doubles starts in the arena: 2^28 doubles in when it fits, so
    that an offset sign-extended from 32 bits (up to 2^31 bytes backwards) stays inside the
    allocation; else the largest power of two that fits."""
    for lg in range(28, 9, -1):
        if (1 << lg) + span + 2 * FRINGE <= ARENA_DOUBLES:
            return 1 << lg
    raise AssertionError(f"{span} doubles do not fit the arena")


class Arena:
    """The 34 GiB allocation, all ones. A failed allocation is an error, never a skip."""

    def __init__(self):
        import ctypes

        from matvec_mpi_multiplier_amd import _lib
        from test_gpu_exact import _hip_runtime

        p = ctypes.c_void_p()
        _lib.check(_lib.lib.mvg_malloc(ctypes.byref(p), ARENA_DOUBLES * 8), "mvg_malloc (the 34 GiB arena)")
        self.ptr = p.value
        hip = _hip_runtime()
        hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        rc = hip.hipMemset(self.ptr, 0xFF, ARENA_DOUBLES * 8)
        assert rc == 0 and hip.hipDeviceSynchronize() == 0, rc
        self.live = []  # [start, end) in doubles of the operands in use

    def claim(self, lo, hi):
        assert 0 <= lo and hi <= ARENA_DOUBLES, (lo, hi)
        self.live.append((lo, hi))

    def free(self):
        from matvec_mpi_multiplier_amd import _lib

        if self.ptr:
            _lib.check(_lib.lib.mvg_free(self.ptr), "mvg_free")
            self.ptr = None


class WideOperand:
    """nvec vectors of n payload doubles, ld apart, inside the arena. `ptr` is vector 0's payload.
    Every transfer is per vector: the payload with its two fringes, n + 32 doubles."""

    def __init__(self, arena, nvec, n, ld, shift=0, base=None):
        self.arena, self.nvec, self.n, self.ld = arena, int(nvec), int(n), int(ld)
        span = (self.nvec - 1) * self.ld + self.n + int(shift)
        base = default_base(span) if base is None else base
        assert ld >= n + 2 * FRINGE and base % 32 == 0 and base >= FRINGE, (ld, n, base)
        self.first = base + int(shift)  # vector 0's payload, in doubles from the arena's start
        assert self.first + span - int(shift) + FRINGE <= ARENA_DOUBLES, (base, span)
        mine = [(self.first + v * self.ld - FRINGE, self.first + v * self.ld + self.n + FRINGE) for v in range(self.nvec)]
        for lo, hi in mine:  # two live operands never share a double (relayout: source and panels)
            assert all(hi <= a or b <= lo for a, b in arena.live), (lo, hi)
        self._mine = mine
        for lo, hi in mine:
            arena.claim(lo, hi)
        self.ptr = arena.ptr + 8 * self.first
        self.lay = G.Layout(self.nvec, self.n, self.n + 2 * FRINGE)

    def _copy(self, host, to_device):
        from matvec_mpi_multiplier_amd._lib import check, lib

        assert host.shape == (self.nvec, self.n + 2 * FRINGE) and host.flags.c_contiguous
        for v in range(self.nvec):
            dev = self.ptr + 8 * (v * self.ld - FRINGE)
            if to_device:
                check(lib.mvg_memcpy_h2d(dev, host[v].ctypes.data, 8 * host.shape[1], None), "h2d")
            else:
                check(lib.mvg_memcpy_d2h(host[v].ctypes.data, dev, 8 * host.shape[1], None), "d2h")
        check(lib.mvg_stream_sync(None), "sync")

    def write(self, payload):
        host = np.full((self.nvec, self.n + 2 * FRINGE), np.nan)
        host[:, FRINGE:FRINGE + self.n] = np.asarray(payload, dtype=np.float64).reshape(self.nvec, self.n)
        self._copy(host, True)
        return self

    def poison(self):
        """Payloads and fringes back to NaN (a result operand before each call; every operand
        when its test is done, so the arena is all NaN again)."""
        self._copy(np.full((self.nvec, self.n + 2 * FRINGE), np.nan), True)
        return self

    def read(self):
        """(nvec, 16 + n + 16): every vector's payload between its fringes."""
        host = np.zeros((self.nvec, self.n + 2 * FRINGE))
        self._copy(host, False)
        return host

    def image(self):
        """read() as a gpu_guarded image of layout `lay` (violations, check_image, exact_ok)."""
        return np.concatenate([self.read().ravel(), np.full(2 * FRINGE, np.nan)])

    def release(self):
        self.poison()
        for r in self._mine:
            self.arena.live.remove(r)
        self._mine = []
