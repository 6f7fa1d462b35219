"""Launch mvg_gemv_t_multi (automatic choice, or a named variant) on one device-resident shape, for
a rocprofv3 kernel trace of its strip and reduce kernels (development tool).

    python tools/gemv_t_multi_probe.py [M] [K] [NV] [launches] [variant name]    e.g. 524288 512 16 100
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd import multiplier as mm  # noqa: E402
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 524288
    K = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    NV = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    names = [lib.mvg_gemv_t_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_t_multi_variant_count())]
    v = names.index(sys.argv[5]) if len(sys.argv) > 5 else 0
    dA, dZ, dY = mm.DeviceBuffer(M * K), mm.DeviceBuffer(M * NV), mm.DeviceBuffer(K * NV)
    check(lib.mvg_synth_fill_device(dA.ptr, K, M, K, 0, 0, K, 42, None), "fill A")
    check(lib.mvg_synth_fill_device(dZ.ptr, M, NV, M, 0, 0, M, 4343, None), "fill Z")
    for _ in range(n):
        mm.gemv_t_multi(dA.ptr, K, dZ.ptr, M, dY.ptr, K, M, K, NV, None, v)
    check(lib.mvg_stream_sync(None), "sync")
    band_rows, bands, strip_cols, group = mm.gemv_t_multi_plan(K, M, K, NV, v)
    print(f"gemv_t_multi_probe {M}x{K} nv={NV}: {n} launches of {names[v or lib.mvg_gemv_t_multi_auto_variant(K, M, M, K, NV)]} "
          f"(first group {group}: {bands} bands of {band_rows} rows, strips of {strip_cols} columns)")


if __name__ == "__main__":
    main()
