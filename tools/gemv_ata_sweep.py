"""Fused A^T A product variant sweep on one MI355X (development tool, not part of the product).

For each shape every variant of mvg_gemv_ata_variant that takes its k is timed alternating, in one
process and on the same buffers, with the pair issued by hand (mvg_gemv into t, then mvg_gemv_t
into w: the baseline) and mvg_stream_read (the read-only ceiling over the same bytes). The device is
warmed first by a second of reads; every window holds at least WINDOW_S seconds of back-to-back
launches between two device events; ROUNDS windows per kernel, interleaved. Before it is timed each
variant's t and w are checked against the pair's on the oracle.synth data: max_rel <= 1e-12.

One JSON object per (shape, kernel): us per call (median and best window), the ratio to the pair in
the same run, the share of 8 TB/s on 8 (m k + 2 k + m) bytes, the bands and the workspace share
2 bands / m. Usage: gemv_ata_sweep.py [out.jsonl] [rounds] [shape,shape,...]
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
TOL = 1e-12
SHAPES = [  # (name, m, k)
    ("cfg2_16384sq", 16384, 16384),
    ("cfg3_g8_strip_65536x8192", 65536, 8192),
    ("cfg5_shard_524288x512", 524288, 512),
    ("tall_4194304x64", 4194304, 64),
    ("short_2048x16384", 2048, 16384),
    ("cfg4_block_65536x32768", 65536, 32768),  # beyond every fused cap: two_pass alone
    # a k inside each picked variant's bracket, not at its max_k: the kernels cut by k
    ("cut_16384x12288", 16384, 12288),
    ("cut_65536x6144", 65536, 6144),
    ("cut_524288x384", 524288, 384),
    ("cut_4194304x192", 4194304, 192),
]


def window(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def rel(a, b):
    return ((a - b).abs() / b.abs().clamp_min(1e-300)).max().item()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r08/gemv_ata/sweep.jsonl"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * k for _, m, k in shapes), dtype=torch.float64, device=dev)
    sink = torch.zeros(256 * 16 * 256, dtype=torch.float64, device=dev)
    nvar = lib.mvg_gemv_ata_variant_count()
    # settle and warm: a second of the read-only stream over the buffer
    n_warm = buf.numel() & ~1
    t0 = window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), 2)
    window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), max(2, int(1.0 / t0)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as out:
        for name, m, k in shapes:
            A = buf[: m * k]
            check(lib.mvg_synth_fill_device(A.data_ptr(), k, m, k, 0, 0, k, 42, s), "fill A")
            x = torch.empty(k, dtype=torch.float64, device=dev)
            check(lib.mvg_synth_fill_device(x.data_ptr(), k, 1, k, 0, 0, k, 4242, s), "fill x")
            t = torch.empty(m, dtype=torch.float64, device=dev)
            w = torch.empty(k, dtype=torch.float64, device=dev)
            a, xp, tp, wp = A.data_ptr(), x.data_ptr(), t.data_ptr(), w.data_ptr()

            def pair():
                check(lib.mvg_gemv(a, k, xp, tp, m, k, s), "mvg_gemv")
                check(lib.mvg_gemv_t(a, k, tp, wp, m, k, s), "mvg_gemv_t")

            pair()
            t_pair, w_pair = t.clone(), w.clone()
            calls, info = {}, {}
            for v in range(nvar):
                vname = lib.mvg_gemv_ata_variant_name(v).decode()
                b, n, mk = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
                if lib.mvg_gemv_ata_plan(k, m, k, v, ctypes.byref(b), ctypes.byref(n), ctypes.byref(mk)) != 0:
                    continue  # k beyond this variant's max_k
                t.fill_(float("nan"))
                w.fill_(float("nan"))
                check(lib.mvg_gemv_ata_variant(a, k, xp, tp, wp, m, k, v, s), vname)
                rt, rw = rel(t, t_pair), rel(w, w_pair)
                assert rt <= TOL and rw <= TOL, (name, vname, rt, rw)
                pick = lib.mvg_gemv_ata_variant_name(lib.mvg_gemv_ata_auto_variant(k, m, k)).decode() if v == 0 else None
                info[vname] = {"max_rel_t_vs_pair": rt, "max_rel_w_vs_pair": rw, "band_rows": b.value, "bands": n.value,
                               "workspace_share": round(2 * n.value / m, 5) if n.value > 1 else 0.0, "picks": pick}
                calls[vname] = (lambda v=v: lib.mvg_gemv_ata_variant(a, k, xp, tp, wp, m, k, v, s))
            calls["pair_by_hand"] = pair
            n_read = (m * k) & ~1
            calls["mvg_stream_read"] = lambda: lib.mvg_stream_read(a, n_read, sink.data_ptr(), s)
            iters = {}
            for key, call in calls.items():  # a first window sizes the timed ones
                call()
                t1 = window(call, 3)
                iters[key] = max(3, int(WINDOW_S / t1) + 1)
            times = {key: [] for key in calls}
            for _ in range(rounds):
                for key, call in calls.items():
                    times[key].append(window(call, iters[key]))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
            nbytes = 8 * (m * k + 2 * k + m)
            for key in calls:
                rec = {"shape": name, "m": m, "k": k, "kernel": key, "us": round(med[key] * 1e6, 2),
                       "us_best": round(min(times[key]) * 1e6, 2), "windows": rounds, "launches_per_window": iters[key],
                       "share_of_8TBps": round((8 * m * k if key == "mvg_stream_read" else nbytes) / med[key] / PEAK, 4),
                       "ratio_to_pair": round(med[key] / med["pair_by_hand"], 4)}
                rec.update(info.get(key, {}))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del t_pair, w_pair


if __name__ == "__main__":
    main()
