"""Transposed-GEMV variant sweep on one MI355X (development tool, not part of the product).

For each shape every variant of mvg_gemv_t_variant is timed alternating, in one process and on one
buffer, with mvg_gemv (the forward product over the same A) and mvg_stream_read (the read-only
ceiling over the same bytes). The device is warmed first; every window holds at least WINDOW_S
seconds of back-to-back launches between two device events; ROUNDS windows per kernel, interleaved.
Each variant is first checked against rocBLAS fp64 (torch.mv on A^T) to 1e-12.

One JSON object per (shape, kernel): us per call (median and best window), the share of 8 TB/s on
8 (m k + m + k) bytes, the workspace bytes, and the ratio to mvg_gemv's and mvg_stream_read's time
in the same run. Usage: gemv_t_sweep.py [out.jsonl] [rounds] [shape,shape,...]
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402

PEAK = 8.0e12
WINDOW_S = 0.3
# (name, m, k, lda): the four dispatch shapes, then the two hazards — rows a power of two apart
# against the same rows 16 doubles further apart, and a k that leaves half of every wave idle
SHAPES = [
    ("cfg2_16384sq", 16384, 16384, 16384),
    ("cfg3_g8_strip_65536x8192", 65536, 8192, 8192),
    ("cfg4_block_65536x32768", 65536, 32768, 32768),
    ("cfg5_shard_524288x512", 524288, 512, 512),
    ("hazard1_16384sq_lda16400", 16384, 16384, 16400),
    ("hazard2_4194304x64", 4194304, 64, 64),
]


def window(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r07/gemv_t/sweep.jsonl"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * lda for _, m, _, lda in shapes), dtype=torch.float64, device=dev)
    sink = torch.zeros(256 * 16 * 256, dtype=torch.float64, device=dev)
    nvar = lib.mvg_gemv_t_variant_count()
    # settle and warm: a second of the read-only stream over the buffer
    n_warm = buf.numel() & ~1
    t = window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), 2)
    window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), max(2, int(1.0 / t)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as out:
        for name, m, k, lda in shapes:
            A = buf[: m * lda].view(m, lda)
            check(lib.mvg_synth_fill_device(A.data_ptr(), lda, m, lda, 0, 0, lda, 42, s), "fill A")
            z = torch.empty(m, dtype=torch.float64, device=dev)
            x = torch.empty(k, dtype=torch.float64, device=dev)
            check(lib.mvg_synth_fill_device(z.data_ptr(), m, 1, m, 0, 0, m, 4343, s), "fill z")
            check(lib.mvg_synth_fill_device(x.data_ptr(), k, 1, k, 0, 0, k, 4242, s), "fill x")
            yt = torch.empty(k, dtype=torch.float64, device=dev)
            y = torch.empty(m, dtype=torch.float64, device=dev)
            ref = torch.mv(A[:, :k].t(), z)
            a, zp, xp, ytp, yp = A.data_ptr(), z.data_ptr(), x.data_ptr(), yt.data_ptr(), y.data_ptr()
            calls = {}
            info = {}
            for v in range(nvar):
                vname = lib.mvg_gemv_t_variant_name(v).decode()
                yt.fill_(float("nan"))
                check(lib.mvg_gemv_t_variant(a, lda, zp, ytp, m, k, v, s), vname)
                rel = ((yt - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
                assert rel <= 1e-12, (name, vname, rel)
                b, n, sc = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
                check(lib.mvg_gemv_t_plan(lda, m, k, v, ctypes.byref(b), ctypes.byref(n), ctypes.byref(sc)), "plan")
                pick = lib.mvg_gemv_t_variant_name(lib.mvg_gemv_t_auto_variant(lda, m, k)).decode() if v == 0 else None
                info[vname] = {"max_rel_vs_rocblas": rel, "band_rows": b.value, "bands": n.value, "strip_cols": sc.value,
                               "workspace_bytes": 8 * n.value * k if n.value > 1 else 0, "picks": pick}
                calls[vname] = (lambda v=v: lib.mvg_gemv_t_variant(a, lda, zp, ytp, m, k, v, s))
            calls["mvg_gemv"] = lambda: lib.mvg_gemv(a, lda, xp, yp, m, k, s)
            n_read = (m * lda) & ~1
            calls["mvg_stream_read"] = lambda: lib.mvg_stream_read(a, n_read, sink.data_ptr(), s)
            iters = {}
            for key, call in calls.items():  # a first window sizes the timed ones
                call()
                t = window(call, 3)
                iters[key] = max(3, int(WINDOW_S / t) + 1)
            times = {key: [] for key in calls}
            for _ in range(rounds):
                for key, call in calls.items():
                    times[key].append(window(call, iters[key]))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
            nbytes = 8 * (m * k + m + k)
            for key in calls:
                rec = {"shape": name, "m": m, "k": k, "lda": lda, "kernel": key, "us": round(med[key] * 1e6, 2),
                       "us_best": round(min(times[key]) * 1e6, 2), "windows": rounds, "launches_per_window": iters[key],
                       "share_of_8TBps": round((8 * m * lda if key == "mvg_stream_read" else nbytes) / med[key] / PEAK, 4),
                       "ratio_to_mvg_gemv": round(med[key] / med["mvg_gemv"], 4),
                       "ratio_to_stream_read": round(med[key] / med["mvg_stream_read"] * (m * lda) / (m * k), 4)}
                rec.update(info.get(key, {}))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del ref


if __name__ == "__main__":
    main()
