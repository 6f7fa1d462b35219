"""Transposed block-of-vectors sweep on one MI355X (development tool, not part of the product).

For each shape and each nv in 2, 4, 8, 16 every fused variant of mvg_gemv_t_multi_variant whose
chain count is at most nv is timed alternating, in one process and on the same buffers, with three
baselines: `separate` (nv launches of mvg_gemv_t), mvg_gemv_multi at the same nv over the same A
(the forward block product) and mvg_stream_read (the read-only ceiling over A's bytes). The device
is warmed with a second of reads first; every window holds at least WINDOW_S seconds of
back-to-back launches between two device events; ROUNDS windows per kernel, interleaved; the
median window counts. Each variant is first checked against rocBLAS fp64 (torch.mm on A^T) to 1e-12.

One JSON line per (shape, nv): "us" maps every kernel timed there (the fused variants by name,
separate, mvg_gemv_multi, mvg_stream_read) to its median us per call; ratios follow from the line.
A variant's cut is not recorded: mvg_gemv_t_multi_plan gives it on the host.
Usage: gemv_t_multi_sweep.py [out.jsonl] [rounds] [shape,shape,...] [nv,nv,...]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matvec_mpi_multiplier_amd._lib import check, lib  # noqa: E402

WINDOW_S = 0.3
NVS = [2, 4, 8, 16]
# (name, m, k, lda): tools/gemv_t_sweep.py's: the four dispatch shapes, then the two hazards — rows a
# power of two apart against the same rows 16 doubles further apart, and a k below 128
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
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r07/gemv_t_multi/sweep.jsonl"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3].split(",") if len(sys.argv) > 3 and sys.argv[3] else None
    nvs = [int(t) for t in sys.argv[4].split(",")] if len(sys.argv) > 4 else NVS
    shapes = [s for s in SHAPES if not only or s[0] in only]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(max(m * lda for _, m, _, lda in shapes), dtype=torch.float64, device=dev)
    sink = torch.zeros(256 * 16 * 256, dtype=torch.float64, device=dev)
    names = [lib.mvg_gemv_t_multi_variant_name(v).decode() for v in range(lib.mvg_gemv_t_multi_variant_count())]
    chains = {v: int(n.rsplit("_v", 1)[1]) for v, n in enumerate(names) if n.startswith("t") and "_v" in n}
    # settle and warm: a second of the read-only stream over the buffer
    n_warm = buf.numel() & ~1
    t = window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), 2)
    window(lambda: lib.mvg_stream_read(buf.data_ptr(), n_warm, sink.data_ptr(), s), max(2, int(1.0 / t)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as out:
        for name, m, k, lda in shapes:
            A = buf[: m * lda].view(m, lda)
            check(lib.mvg_synth_fill_device(A.data_ptr(), lda, m, lda, 0, 0, lda, 42, s), "fill A")
            nvmax = max(nvs)
            Z = torch.empty(nvmax * m, dtype=torch.float64, device=dev)  # column-major: vector v at v * m
            X = torch.empty(nvmax * k, dtype=torch.float64, device=dev)
            check(lib.mvg_synth_fill_device(Z.data_ptr(), m, nvmax, m, 0, 0, m, 4343, s), "fill Z")
            check(lib.mvg_synth_fill_device(X.data_ptr(), k, nvmax, k, 0, 0, k, 4242, s), "fill X")
            Yt = torch.empty(nvmax * k, dtype=torch.float64, device=dev)
            Y = torch.empty(nvmax * m, dtype=torch.float64, device=dev)
            a, zp, xp, ytp, yp = A.data_ptr(), Z.data_ptr(), X.data_ptr(), Yt.data_ptr(), Y.data_ptr()
            n_read = (m * lda) & ~1
            for nv in nvs:
                ref = torch.mm(Z[: nv * m].view(nv, m), A[:, :k])  # nv x k: row v is A^T z_v
                calls, worst = {}, 0.0
                for v, vname in enumerate(names):
                    if v == 0 or chains.get(v, 1) > nv:
                        continue
                    Yt.fill_(float("nan"))
                    check(lib.mvg_gemv_t_multi_variant(a, lda, zp, m, ytp, k, m, k, nv, v, s), vname)
                    rel = ((Yt[: nv * k].view(nv, k) - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
                    assert rel <= 1e-12, (name, nv, vname, rel)
                    worst = max(worst, rel)
                    calls[vname] = (lambda v=v, nv=nv: lib.mvg_gemv_t_multi_variant(a, lda, zp, m, ytp, k, m, k, nv, v, s))
                calls["mvg_gemv_multi"] = lambda nv=nv: lib.mvg_gemv_multi(a, lda, xp, k, yp, m, m, k, nv, s)
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
                rec = {"shape": name, "m": m, "k": k, "lda": lda, "nv": nv, "windows": rounds, "max_rel_vs_rocblas": worst,
                       "us": {key: round(sorted(ts)[len(ts) // 2] * 1e6, 2) for key, ts in times.items()}}
                line = json.dumps(rec, separators=(",", ":"))
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
                del ref


if __name__ == "__main__":
    main()
