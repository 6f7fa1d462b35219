"""Fused A^T A product for a block of vectors: variant sweep on one MI355X (development tool, not
part of the product).

For each shape and nv every fused variant of mvg_gemv_ata_multi_variant that takes the shape's k and
has no more chains than nv is timed alternating, in one process and on the same buffers, with
two_pass issued by hand (mvg_gemv_multi into T, then mvg_gemv_t_multi into W: the baseline) and
mvg_stream_read (the read-only ceiling over A's bytes). The device is warmed first by a second of
reads; every window holds at least WINDOW_S seconds of back-to-back launches between two device
events; ROUNDS windows per kernel, interleaved. Before it is timed each variant's T and W are
checked against two_pass's on the oracle.synth data: max_rel <= 1e-12.

One JSON object per (shape, nv, kernel): us per call (median and best window), the ratio to two_pass
in the same run, the ratio to the read-only stream, the passes over A the call makes, the bands and
the workspace share 2 NV bands / m.
Usage: gemv_ata_multi_sweep.py [out.jsonl] [rounds] [shape,shape,...] [nv,nv,...]
"""
import ctypes
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402

WINDOW_S = 0.2
TOL = 1e-12
NVS = [2, 4, 8, 16]
SHAPES = [  # (name, m, k): MEASUREMENTS §17's ten
    ("cfg2_16384sq", 16384, 16384),
    ("cfg3_g8_strip_65536x8192", 65536, 8192),
    ("cfg5_shard_524288x512", 524288, 512),
    ("tall_4194304x64", 4194304, 64),
    ("short_2048x16384", 2048, 16384),
    ("cfg4_block_65536x32768", 65536, 32768),
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r10/gemv_ata_multi/sweep.jsonl"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3].split(",") if len(sys.argv) > 3 and sys.argv[3] else None
    nvs = [int(n) for n in sys.argv[4].split(",")] if len(sys.argv) > 4 else NVS
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * k for _, m, k in shapes), dtype=torch.float64, device=dev)
    sink = torch.zeros(256 * 16 * 256, dtype=torch.float64, device=dev)
    nvar = lib.mvg_gemv_ata_multi_variant_count()
    names = [lib.mvg_gemv_ata_multi_variant_name(v).decode() for v in range(nvar)]
    # settle and warm: a second of the read-only stream over the buffer
    n_warm = buf.numel() & ~1
    t0 = window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), 2)
    window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), max(2, int(1.0 / t0)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as out:
        for name, m, k in shapes:
            A = buf[: m * k]
            check(lib.mvg_synth_fill_device(A.data_ptr(), k, m, k, 0, 0, k, 42, s), "fill A")
            for nv in nvs:
                X = torch.empty(k * nv, dtype=torch.float64, device=dev)
                check(lib.mvg_synth_fill_device(X.data_ptr(), k, nv, k, 0, 0, k, 4242, s), "fill X")
                T = torch.empty(m * nv, dtype=torch.float64, device=dev)
                W = torch.empty(k * nv, dtype=torch.float64, device=dev)
                a, xp, tp, wp = A.data_ptr(), X.data_ptr(), T.data_ptr(), W.data_ptr()

                def pair():
                    check(lib.mvg_gemv_multi(a, k, xp, k, tp, m, m, k, nv, s), "mvg_gemv_multi")
                    check(lib.mvg_gemv_t_multi(a, k, tp, m, wp, k, m, k, nv, s), "mvg_gemv_t_multi")

                pair()
                T_pair, W_pair = T.clone(), W.clone()
                calls, info = {"two_pass_by_hand": pair}, {}
                pick = names[lib.mvg_gemv_ata_multi_auto_variant(k, k, m, k, nv)]
                for v in range(2, nvar):
                    chains = int(re.search(r"_v(\d+)$", names[v]).group(1))
                    b, n, mk, g = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
                    out_args = (ctypes.byref(b), ctypes.byref(n), ctypes.byref(mk), ctypes.byref(g))
                    if chains > nv or lib.mvg_gemv_ata_multi_plan(k, m, k, nv, v, *out_args) != 0:
                        continue  # a short group, or k beyond this variant's max_k
                    T.fill_(float("nan"))
                    W.fill_(float("nan"))
                    check(lib.mvg_gemv_ata_multi_variant(a, k, xp, k, tp, m, wp, k, m, k, nv, v, s), names[v])
                    rt, rw = rel(T, T_pair), rel(W, W_pair)
                    assert rt <= TOL and rw <= TOL, (name, nv, names[v], rt, rw)
                    info[names[v]] = {"max_rel_T_vs_two_pass": rt, "max_rel_W_vs_two_pass": rw, "band_rows": b.value,
                                      "bands": n.value, "passes_over_A": -(-nv // chains),
                                      "workspace_share": round(2 * chains * n.value / m, 5) if n.value > 1 else 0.0}
                    calls[names[v]] = (lambda v=v: lib.mvg_gemv_ata_multi_variant(a, k, xp, k, tp, m, wp, k, m, k, nv, v, s))
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
                for key in calls:
                    rec = {"shape": name, "m": m, "k": k, "nv": nv, "kernel": key, "us": round(med[key] * 1e6, 2),
                           "us_best": round(min(times[key]) * 1e6, 2), "windows": rounds, "launches_per_window": iters[key],
                           "ratio_to_two_pass": round(med[key] / med["two_pass_by_hand"], 4),
                           "ratio_to_stream_read": round(med[key] / med["mvg_stream_read"], 4), "auto_picks": pick}
                    rec.update(info.get(key, {}))
                    line = json.dumps(rec)
                    print(line, flush=True)
                    out.write(line + "\n")
                    out.flush()
                del T_pair, W_pair, X, T, W


if __name__ == "__main__":
    main()
