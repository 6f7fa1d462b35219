"""Guarded operands for the GPU kernel tests: every operand sits inside NaN.

A device image of an operand is

    [ GUARD NaNs | shift NaNs | nvec vectors of ld doubles | GUARD NaNs ]

with the payload (the part a kernel may read, or must write) the first `n` doubles of each of
the first `nv` vectors; everything else — the guards, the padding n..ld-1 of every vector, the
vectors nv..nvec-1 — is NaN. A row-major A (m x k, lda) is such an image with m vectors of k
payload doubles, X (k x nv column-major, ldx) one with nv vectors of k, and y / Y one with nv
vectors of m whose payload too is prefilled with NaN.

A kernel that reads a padding column of A or x into a sum turns that row of y into NaN; a store
past row m, past vector nv or in front of row 0 replaces a NaN of the y image. `violations` and
`check_image` find both in the downloaded image with numpy alone (no GPU): tests/test_guarded_host.py
runs them on images corrupted on the host.

GUARD is 16 doubles (128 B), so the payload keeps the alignment class of the allocation (256 B
from the allocator) unless `shift` (in doubles) moves it: shift = 1 puts it 8 bytes off a 16-B
boundary. Guards are read and written only inside the image's own allocation.
"""
import numpy as np

GUARD = 16


class Layout:
    """Where the payload sits in a guarded image (all sizes in doubles)."""

    def __init__(self, nv, n, ld, nvec=None, shift=0):
        nvec = nv if nvec is None else nvec
        assert ld >= n and nvec >= nv and shift >= 0
        self.nv, self.n, self.ld, self.nvec, self.shift = int(nv), int(n), int(ld), int(nvec), int(shift)
        self.off = GUARD + self.shift  # the payload's first double
        self.size = self.off + self.nvec * self.ld + GUARD
        self._index = self._mask = None

    def payload_index(self):
        """Flat indices of the payload, shape (nv, n)."""
        if self._index is None:
            self._index = self.off + np.arange(self.nv)[:, None] * self.ld + np.arange(self.n)[None, :]
        return self._index

    def payload_mask(self):
        if self._mask is None:
            self._mask = np.zeros(self.size, dtype=bool)
            self._mask[self.payload_index().reshape(-1)] = True
        return self._mask

    def image(self, payload=None):
        """The host image: NaN everywhere, `payload` (nv x n) in its place when given."""
        img = np.full(self.size, np.nan)
        if payload is not None:
            payload = np.asarray(payload, dtype=np.float64).reshape(self.nv, self.n)
            img[self.payload_index()] = payload
        return img

    def payload(self, img):
        return np.asarray(img)[self.payload_index()]

    def describe(self, idx):
        """Names the position of flat index idx of the image."""
        idx = int(idx)
        if idx < self.off:
            return f"{self.off - idx} doubles before vector 0 row 0 (front guard)"
        rel = idx - self.off
        v, i = divmod(rel, self.ld)
        if v >= self.nvec:
            return f"{rel - self.nvec * self.ld} doubles past the last vector (back guard)"
        if v >= self.nv:
            return f"vector {v} row {i} (a vector past nv = {self.nv})"
        if i >= self.n:
            return f"vector {v} row {i} (padding: row {i - self.n} past n = {self.n})"
        return f"vector {v} row {i}"


def violations(img, lay):
    """Every position outside the payload that is no longer NaN, named."""
    img = np.asarray(img)
    assert img.shape == (lay.size,), (img.shape, lay.size)
    bad = np.flatnonzero(~np.isnan(img) & ~lay.payload_mask())
    return [f"{lay.describe(i)} = {img[i]!r}" for i in bad]


def check_image(img, lay, compare, what=""):
    """The checker: every position outside the payload still NaN, and the payload (nv x n)
    accepted by `compare(payload) -> boolean array, True where the value is accepted` (or a
    single bool). Returns the list of named failures, empty for a clean image."""
    out = [f"{what}: stored outside y: {v}" for v in violations(img, lay)]
    got = lay.payload(img)
    ok = np.broadcast_to(np.asarray(compare(got), dtype=bool), got.shape)
    for v, i in zip(*np.nonzero(~ok)):
        out.append(f"{what}: wrong value at vector {v} row {i}: {got[v, i]!r}")
    return out


def assert_clean(img, lay, compare, what=""):
    bad = check_image(img, lay, compare, what)
    assert not bad, f"{len(bad)} failures, first: " + "; ".join(bad[:6])


# ------------------------------------------------------------------ comparators
def same_or_both_nan(a, b):
    """The exact comparison where NaN results are allowed: equal values, NaN where the other is
    NaN (sign and payload of a NaN are not compared), and the same sign bit on everything else
    (so -0.0 is not +0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a, b, equal_nan=True):
        return False
    live = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[live]), np.signbit(b[live])))


def exact_ok(want):
    """Elementwise form of same_or_both_nan against `want` (for check_image)."""
    want = np.asarray(want)

    def compare(got):
        both_nan = np.isnan(got) & np.isnan(want)
        return both_nan | ((got == want) & (np.signbit(got) == np.signbit(want)))

    return compare


def same_class(want):
    """Where `want` is not finite: the same class (+inf, -inf, or NaN in any encoding)."""
    want = np.asarray(want)

    def compare(got):
        return np.where(np.isnan(want), np.isnan(got), got == want)

    return compare


# ------------------------------------------------------------------ device side
class Guarded:
    """A guarded operand on the device. `ptr` is the payload's address."""

    def __init__(self, lay, payload=None):
        from matvec_mpi_multiplier_amd import multiplier as mm

        self.lay = lay
        self._nan = None
        self.buf = mm.DeviceBuffer(lay.size)
        self.ptr = self.buf.ptr + 8 * lay.off
        self.fill(payload)

    def fill(self, payload=None):
        """(Re)write the whole image: NaN, and the payload if given."""
        if payload is None:
            if self._nan is None:
                self._nan = self.lay.image()
            self.buf.upload(self._nan)
        else:
            self.buf.upload(self.lay.image(payload))
        return self

    def poke(self, v, i, values):
        """Overwrite payload doubles i .. of vector v (inside the payload only)."""
        from matvec_mpi_multiplier_amd._lib import check, lib

        values = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64)
        assert 0 <= v < self.lay.nv and 0 <= i and i + values.size <= self.lay.n, (v, i, values.size)
        check(lib.mvg_memcpy_h2d(self.ptr + 8 * (v * self.lay.ld + i), values.ctypes.data, 8 * values.size, None), "h2d")
        check(lib.mvg_stream_sync(None), "sync")

    def image(self):
        return self.buf.download(self.lay.size)

    def free(self):
        self.buf.free()


def matrix(A, pad, shift=0):
    """Row-major A (m x k) with lda = k + pad inside NaN."""
    m, k = A.shape
    return Guarded(Layout(m, k, k + pad, shift=shift), A)


def vectors(X, ld, shift=0):
    """nv vectors of k doubles (nv x k: vector v contiguous), ld apart, inside NaN."""
    X = np.atleast_2d(X)
    return Guarded(Layout(X.shape[0], X.shape[1], ld, shift=shift), X)


def result(nv, m, ldy, spare=0):
    """The y / Y image, NaN throughout: nv vectors of m rows, ldy apart, `spare` more vectors
    after them that no kernel may touch."""
    return Guarded(Layout(nv, m, ldy, nvec=nv + spare))
