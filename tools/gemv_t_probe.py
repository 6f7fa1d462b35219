"""Launch mvg_gemv_t (automatic kernel choice, or a named variant) on one device-resident shape,
for a rocprofv3 kernel trace of its two kernels (development tool).

    python tools/gemv_t_probe.py [M] [K] [launches] [variant name]      e.g. 524288 512 200
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd import multiplier as mm  # noqa: E402
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    names = [lib.mvg_gemv_t_variant_name(v).decode() for v in range(lib.mvg_gemv_t_variant_count())]
    v = names.index(sys.argv[4]) if len(sys.argv) > 4 else 0
    dA, dz, dy = mm.DeviceBuffer(M * K), mm.DeviceBuffer(M), mm.DeviceBuffer(K)
    check(lib.mvg_synth_fill_device(dA.ptr, K, M, K, 0, 0, K, 42, None), "fill A")
    check(lib.mvg_synth_fill_device(dz.ptr, M, 1, M, 0, 0, M, 4343, None), "fill z")
    for _ in range(n):
        check(lib.mvg_gemv_t_variant(dA.ptr, K, dz.ptr, dy.ptr, M, K, v, None), "mvg_gemv_t")
    check(lib.mvg_stream_sync(None), "sync")
    band_rows, bands, strip_cols = mm.gemv_t_plan(K, M, K, v)
    print(f"gemv_t_probe {M}x{K}: {n} launches of {names[v or lib.mvg_gemv_t_auto_variant(K, M, K)]} "
          f"({bands} bands of {band_rows} rows, strips of {strip_cols} columns)")


if __name__ == "__main__":
    main()
