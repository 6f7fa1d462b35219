"""Bit-exact transposed-GEMV variant sweep on one MI355X (development tool, not part of the product).

For each shape every variant of mvg_gemv_t_exact_variant, and every variant of
mvg_gemv_t_exact_multi_variant at nv = 2 and 4, is timed alternating, in one process and on one
buffer, with mvg_gemv_t (the tree-summed transposed product of the same tree) and mvg_stream_read
(the read-only ceiling over the same bytes). The device is warmed first; every window holds at
least WINDOW_S seconds of back-to-back launches between two device events; ROUNDS windows per
kernel, interleaved. Before it is timed every variant's result is compared bit for bit with variant
1's (every column of a multi variant with variant 1 on that vector), and variant 1 with rocBLAS
fp64 (torch.mv on A^T) to 1e-12.

One JSON object per (shape, kernel, nv): us per call (median and best window), the ratio to
mvg_gemv_t's and to variant 1's (or separate's) time in the same run, and the share of the model
floor max(mvg_stream_read's time over the same bytes, m chain steps of CHAIN_NS): floor / time.
Usage: gemv_t_exact_sweep.py [out.jsonl] [rounds] [shape,shape,...]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402

WINDOW_S = 0.2
CHAIN_NS = 2.71  # a dependent fp64 multiply-then-add step (profiles/r02/micro/fp64_chain.jsonl)
NVS = (2, 4)
# (name, m, k, lda): the four shapes of MEASUREMENTS §16-18, the chain-bound 4194304 x 64 and one padded lda
SHAPES = [
    ("cfg2_16384sq", 16384, 16384, 16384),
    ("cfg3_g8_strip_65536x8192", 65536, 8192, 8192),
    ("cfg4_block_65536x32768", 65536, 32768, 32768),
    ("cfg5_shard_524288x512", 524288, 512, 512),
    ("tall_4194304x64", 4194304, 64, 64),
    ("cfg2_16384sq_lda16400", 16384, 16384, 16400),
]


def window(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r09/gemv_t_exact/sweep.jsonl"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * lda for _, m, _, lda in shapes), dtype=torch.float64, device=dev)
    sink = torch.zeros(256 * 16 * 256, dtype=torch.float64, device=dev)
    nvar = lib.mvg_gemv_t_exact_variant_count()
    nmvar = lib.mvg_gemv_t_exact_multi_variant_count()
    nvmax = max(NVS)
    # settle and warm: a second of the read-only stream over the buffer
    n_warm = buf.numel() & ~1
    t = window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), 2)
    window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), max(2, int(1.0 / t)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as out:
        for name, m, k, lda in shapes:
            A = buf[: m * lda].view(m, lda)
            check(lib.mvg_synth_fill_device(A.data_ptr(), lda, m, lda, 0, 0, lda, 42, s), "fill A")
            Z = torch.empty(nvmax, m, dtype=torch.float64, device=dev)
            check(lib.mvg_synth_fill_device(Z.data_ptr(), m, nvmax, m, 0, 0, m, 4343, s), "fill Z")
            y1 = torch.empty(nvmax, k, dtype=torch.float64, device=dev)
            y = torch.empty(k, dtype=torch.float64, device=dev)
            Y = torch.empty(nvmax, k, dtype=torch.float64, device=dev)
            a, zp, yp, Yp = A.data_ptr(), Z.data_ptr(), y.data_ptr(), Y.data_ptr()
            for v in range(nvmax):  # variant 1 defines the result
                check(lib.mvg_gemv_t_exact_variant(a, lda, zp + 8 * v * m, y1[v].data_ptr(), m, k, 1, s), "variant 1")
            ref = torch.mv(A[:, :k].t(), Z[0])
            rel = ((y1[0] - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
            assert rel <= 1e-12, (name, rel)
            del ref
            calls, info = {}, {}
            auto = lib.mvg_gemv_t_exact_variant_name(lib.mvg_gemv_t_exact_auto_variant(lda, m, k)).decode()
            for v in range(nvar):
                vname = lib.mvg_gemv_t_exact_variant_name(v).decode()
                y.fill_(float("nan"))
                check(lib.mvg_gemv_t_exact_variant(a, lda, zp, yp, m, k, v, s), vname)
                assert same_bits(y, y1[0]), (name, vname)
                key = (vname, 1)
                info[key] = {"bits_equal_variant_1": True, "max_rel_vs_rocblas": rel, "picks": auto if v == 0 else None}
                calls[key] = (lambda v=v: lib.mvg_gemv_t_exact_variant(a, lda, zp, yp, m, k, v, s))
            for nv in NVS:
                mauto = lib.mvg_gemv_t_exact_multi_variant_name(
                    lib.mvg_gemv_t_exact_multi_auto_variant(lda, m, m, k, nv)).decode()
                for v in range(nmvar):
                    vname = "multi:" + lib.mvg_gemv_t_exact_multi_variant_name(v).decode()
                    Y.fill_(float("nan"))
                    check(lib.mvg_gemv_t_exact_multi_variant(a, lda, zp, m, Yp, k, m, k, nv, v, s), vname)
                    assert same_bits(Y[:nv], y1[:nv]), (name, vname, nv)
                    key = (vname, nv)
                    info[key] = {"bits_equal_variant_1": True, "picks": mauto if v == 0 else None}
                    calls[key] = (lambda v=v, nv=nv: lib.mvg_gemv_t_exact_multi_variant(a, lda, zp, m, Yp, k, m, k, nv, v, s))
            calls[("mvg_gemv_t", 1)] = lambda: lib.mvg_gemv_t(a, lda, zp, yp, m, k, s)
            n_read = (m * lda) & ~1
            calls[("mvg_stream_read", 1)] = lambda: lib.mvg_stream_read(a, n_read, sink.data_ptr(), s)
            iters = {}
            for key, call in calls.items():  # a first window sizes the timed ones
                call()
                t = window(call, 2)
                iters[key] = max(2, int(WINDOW_S / t) + 1)
            times = {key: [] for key in calls}
            for _ in range(rounds):
                for key, call in calls.items():
                    times[key].append(window(call, iters[key]))
            med = {key: sorted(ts)[len(ts) // 2] for key, ts in times.items()}
            read_us = med[("mvg_stream_read", 1)] * 1e6 * (m * k) / (m * lda)  # the same bytes: 8 m k
            floor_us = max(read_us, m * CHAIN_NS * 1e-3)
            for key in calls:
                kname, nv = key
                base = ("multi:separate", nv) if kname.startswith("multi:") else ("tseq_c64_u16", 1)
                rec = {"shape": name, "m": m, "k": k, "lda": lda, "kernel": kname, "nv": nv,
                       "us": round(med[key] * 1e6, 2), "us_best": round(min(times[key]) * 1e6, 2), "windows": rounds,
                       "launches_per_window": iters[key],
                       "ratio_to_mvg_gemv_t": round(med[key] / (nv * med[("mvg_gemv_t", 1)]), 4),  # nv calls of it
                       "ratio_to_variant_1": round(med[key] / med[base], 4),
                       "model_floor_us": round(floor_us, 2), "floor_is": "memory" if floor_us == read_us else "chain",
                       "share_of_model_floor": round(floor_us / (med[key] * 1e6), 4)}
                rec.update(info.get(key, {}))
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
