"""mvg_gemv_exact_multi (several vectors per bit-exact pass over A): every variant of its table
against nv back-to-back mvg_gemv_exact calls in the same process, one MI355X (development tool,
not part of the product; its records decide the automatic choice in csrc/gemv_exact.hip).

    python tools/exact_multi_sweep.py [rounds] [shape,shape,...] [variant-name-prefix,...]

Per shape and nv in 2, 4, 8, 16: the two forms interleaved (every round times each candidate
once, `reps` calls between two HIP events), after waiting for VRAM freed earlier to be cleared and
after a settle of untimed separate passes; medians over the rounds. A is one buffer reused by every
shape, so nothing is freed between timings. Every candidate's Y is compared with the separate
passes' bit for bit. One JSON object per (shape, nv, variant): the pass's median, the time per
vector, the fraction of the 8 TB/s HBM peak that A's bytes per vector-time are, and the ratio of
the separate passes' time to this one's (> 1: the multi form is faster).
"""
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402

SHAPES = [
    ("cfg2_16384sq", 16384, 16384),
    ("cfg3_strip_65536x8192", 65536, 8192),
    ("cfg5_shard_524288x512", 524288, 512),
    ("l16_4096x16384", 4096, 16384),
    ("l32_1024x32768", 1024, 32768),
]
NVS = (2, 4, 8, 16)
HBM_PEAK = 8e12  # bytes per second


def wait_for_cleared_vram():
    try:
        from bench import wait_vram_cleared

        return wait_vram_cleared(0)
    except Exception as exc:  # no sysfs count on this box: say so, time anyway
        return {"error": f"{type(exc).__name__}: {exc}"}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    only = sys.argv[2].split(",") if len(sys.argv) > 2 and sys.argv[2] != "all" else None
    prefixes = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * k for _, m, k in shapes), dtype=torch.float64, device=dev)
    nvmax = max(NVS)
    names = [lib.mvg_gemv_exact_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_exact_multi_variant_count())]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": rounds, "vram": wait_for_cleared_vram()}),
          flush=True)
    for shape, M, K in shapes:
        A = buf[: M * K].view(M, K)
        X = torch.empty(nvmax, K, dtype=torch.float64, device=dev)
        Y = torch.empty(nvmax, M, dtype=torch.float64, device=dev)
        check(lib.mvg_synth_fill_device(A.data_ptr(), K, M, K, 0, 0, K, 42, s), "fill A")
        check(lib.mvg_synth_fill_device(X.data_ptr(), K, nvmax, K, 0, 0, K, 4242, s), "fill X")

        def separate(nv):
            for v in range(nv):
                check(lib.mvg_gemv_exact(A.data_ptr(), K, X[v].data_ptr(), Y[v].data_ptr(), M, K, s), "mvg_gemv_exact")

        def multi(nv, var):
            check(lib.mvg_gemv_exact_multi_variant(A.data_ptr(), K, X.data_ptr(), K, Y.data_ptr(), M, M, K, nv, var, s),
                  names[var])

        # settle: untimed separate passes until a second has passed
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:
            separate(4)
            torch.cuda.synchronize()
        separate(nvmax)
        torch.cuda.synchronize()
        want = Y.clone()
        for nv in NVS:
            cands = {"separate": lambda nv=nv: separate(nv)}
            for var in range(2, len(names)):  # 0 auto, 1 separate: the line above
                if not prefixes or any(names[var].startswith(p) for p in prefixes):
                    cands[names[var]] = lambda nv=nv, var=var: multi(nv, var)
            same = {}
            for key, fn in cands.items():
                Y.zero_()
                fn()
                torch.cuda.synchronize()
                same[key] = bool(torch.equal(Y[:nv], want[:nv]))
            reps = 3 if M * K >= 1 << 27 else 10
            times = {key: [] for key in cands}
            for _ in range(rounds):
                for key, fn in cands.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1) / reps)
            med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
            for key in cands:
                per_vec = med[key] / nv
                print(json.dumps({"shape": shape, "M": M, "K": K, "nv": nv, "variant": key,
                                  "median_us": round(med[key] * 1e3, 2), "min_us": round(min(times[key]) * 1e3, 2),
                                  "per_vector_us": round(per_vec * 1e3, 2),
                                  "peak_fraction": round(8 * M * K / (per_vec * 1e-3) / HBM_PEAK, 3),
                                  "separate_over_this": round(med["separate"] / med[key], 3),
                                  "bit_identical": same[key]}), flush=True)
        del X, Y, want


if __name__ == "__main__":
    main()
