// Communicators (RCCL over xGMI) and the distributed multiplier engine.
//
// The engine is the MI355X replacement for what the three reference drivers do around the
// local product, one algorithm per object:
//
//   ROWWISE   distribute: MPI_Scatter(rows) + MPI_Bcast(x)          rowwise.c:12-51
//             exchange  : MPI_Gather(y pieces, rank order)          rowwise.c:141
//             here      : H2D row shard (or root->peer ncclSend), ncclGather of y to rank 0
//   COLWISE   distribute: MPI_Type_vector + MPI_Pack + MPI_Send strips, MPI_Scatter(x)
//                                                                   colwise.c:11-102
//             exchange  : MPI_Reduce(SUM) of partial y              colwise.c:124
//             here      : 2-D H2D into a packed strip, ncclReduce(fp64, sum) to rank 0
//   BLOCKWISE distribute: block Pack + Send, x segment Send         blockwise.c:17-141
//             exchange  : root Recv(ANY_SOURCE) + y[(src/c)*lr+j] += partial
//                                                                   blockwise.c:144-210
//             here      : ncclReduce(sum) over each grid-row communicator to the row leader
//                         (grid column 0), then ncclGather of the r leader slices to rank 0.
//                         Fixed order: deterministic, unlike the reference's arrival order.
//
// One process may drive several devices (mvg_comm_init_all: the executables) or exactly one
// (mvg_comm_init_rank: one process per GPU under torch.distributed.run). Every collective
// is issued for all local devices inside ncclGroupStart/End, so both models share one path.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"

using namespace mvg;

namespace {

int nccl_fail(ncclResult_t r, const char* what) {
    set_error(std::string(what) + ": " + ncclGetErrorString(r));
    return MVG_E_RCCL;
}

#define MVG_NCCL(call)                                                  \
    do {                                                                \
        ncclResult_t _r = (call);                                       \
        if (_r != ncclSuccess) return nccl_fail(_r, #call);             \
    } while (0)

// a step of this file (an int MVG_* code): leave the calling function with its error
#define MVG_TRY(call)                                                   \
    do {                                                                \
        const int _rc = (call);                                         \
        if (_rc != MVG_OK) return _rc;                                  \
    } while (0)

struct LocalRank {
    int rank = 0;
    int device = 0;
    ncclComm_t comm = nullptr;
};

}  // namespace

struct mvg_comm {
    int nranks = 0;
    std::vector<LocalRank> locals;
};

namespace {

constexpr int kRing = 8;
// Root-send staging: a peer's shard goes out in pieces of at most this many doubles (256 MiB
// unless mvg_debug_set_stage_elems lowers it). An engine reads the value once, at creation
// (mvg_engine::stage_elems): the staging allocation, every offset into it and both sides' piece
// lists (shard_pieces) take it from there, so it cannot change under a live buffer.
constexpr int64_t kStageElems = (256ll << 20) / (int64_t)sizeof(double);
int64_t g_stage_elems = kStageElems;  // what the next mvg_engine_create reads

// One set of a rank's exchange buffers, by MVG_X_BUF_*, for nv vectors: every buffer is
// column-major, one vector per column. The local product (ld = y_len) in a ring when an exchange
// follows: multiply n writes parts[n % ring] while earlier exchanges still read the others.
struct XBufs {
    double* parts[kRing] = {};   // MVG_X_BUF_PART
    double* row = nullptr;       // block-split row leader: the reduced slice (ld = y_len)
    double* y = nullptr;         // rank 0: the full y (ld = R)
    double* gathered = nullptr;  // rank 0, exact mode: vector v's P partials in rank order at v * P * y_len
    double*& at(int id, int b) {
        return id == MVG_X_BUF_PART ? parts[b] : id == MVG_X_BUF_ROW ? row : id == MVG_X_BUF_Y ? y : gathered;
    }
};

// One rank's streams, events, buffers and communicators. The handles are plain values and
// free_shard is the one place that releases them (a block's buffers also when the block grows,
// make_vector_buffers): frees need the shard's device current, and the trace
// (mvg_debug_trace_exchange) builds Shards whose pointers are stand-in addresses that must
// never reach hipFree.
struct Shard {
    mvg_shard plan{};
    int device = 0;
    int rank = 0;
    ncclComm_t world = nullptr;
    // exchange schedule (mvg_plan_exchange) and the communicator each step runs on:
    // the world, or a split of it (block-split: grid-row comm, grid-column-0 leaders' comm)
    mvg_xstep steps[MVG_MAX_XSTEPS];
    int nsteps = 0;
    ncclComm_t xcomm[MVG_MAX_XSTEPS] = {};
    bool owns_xcomm[MVG_MAX_XSTEPS] = {};
    hipStream_t stream = nullptr;       // GEMV (and the root's distribution sends)
    hipStream_t copy_stream = nullptr;  // H2D staging
    hipStream_t xstream = nullptr;      // the exchange step (collectives), overlapping the next GEMV
    double* dA = nullptr;
    double* dx = nullptr;
    // exact mode, tall long-row shards: the same A in column panels (mvg_gemv_exact_panels),
    // allocated and rebuilt from dA by the second multiply after a write to dA
    double* dAp = nullptr;
    int64_t panelP = 0, pstride = 0;
    bool panels_fresh = false;
    int64_t uses = 0;  // multiplies since dA was last written
    // the single vector's exchange buffers (gathered: mvg_engine_set_exact) and the ring's events,
    // which both kinds of multiply share: one slot counter (mvg_engine::nx)
    XBufs one;
    hipEvent_t gemv_done[kRing] = {};  // product into slot b's partial finished
    hipEvent_t x_done[kRing] = {};     // exchange reading slot b's partial finished
    // chunked distribution (mvg_engine_set_overlap): row chunk c of A landed (copy_stream); the
    // next multiply runs the GEMV of chunk c behind it, while later chunks are still copying
    std::vector<hipEvent_t> chunk_ev;
    std::vector<int64_t> chunk_row;   // chunk c = rows [chunk_row[c], chunk_row[c + 1])
    hipEvent_t copy_ready = nullptr;  // s.stream's work before the copies (the last GEMV reads dA)
    bool chunks_pending = false;
    // a block of vectors (mvg_engine_set_vectors): the whole X (C x nv, ld = C) on every rank, and
    // exchange buffers of nv_cap columns, their own so that the single vector's y and its ring stay
    // what the last mvg_engine_multiply left (gathered: the first exact mvg_engine_multiply_multi)
    double* dX = nullptr;
    XBufs blk;
    // root, one process per GPU (root_send_shards): two staging buffers of stage_elems doubles in
    // one allocation, and the events that order their H2D copies and sends; made on first use
    double* stage = nullptr;
    hipEvent_t copied[2] = {}, sent[2] = {}, ready = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    hipEvent_t span_t0 = nullptr, span_t1 = nullptr;  // span timing (mvg_engine_kernel_timing(-1))
};

}  // namespace

struct mvg_engine {
    int alg = 0;
    int64_t R = 0, C = 0;
    int nranks = 0;
    bool single_process = false;  // all ranks in this process
    bool always_collect = false;  // run the collectives even at nranks == 1 (tests)
    bool distributed = false;
    bool exact = false;         // bit-exact mode: mvg_gemv_exact + the reference's combine orders
    int overlap_chunks = 0;     // > 1: distribute in row chunks, each chunk's GEMV behind its copy
    int timing_every = 0;       // record kernel events on every Nth multiply (0 = off, -1 = span)
    int64_t span_multiplies = 0;  // span timing: multiplies since the span's first event (0 = none open)
    bool span_valid = true;       // no chunked distribution's copies inside the open span
    int64_t nx = 0;             // multiplies with an exchange issued so far
    bool x_pending = false;     // an exchange may still run (slot (nx - 1) % ring)
    int ring = kRing;           // ring length in use (MVG_XRING, 1 = exchange on the GEMV stream)
    int64_t stage_elems = kStageElems;  // root-send staging, doubles per buffer (fixed at creation)
    int nv = 0;      // vectors of the block last set (0: none yet)
    int nv_cap = 0;  // vectors the block's buffers hold
    int64_t multiply_calls = 0;
    double kernel_ms_sum = 0.0;
    int64_t kernel_launches = 0;
    std::vector<Shard> shards;
};

namespace {

// The exchange's device-side calls — RCCL's communicator splits and collectives, and exact
// mode's combine kernel on rank 0 — go through one interface: RCCL and the kernels on the
// devices (DeviceXOps), or a recorder that lists them in issue order (TraceXOps,
// mvg_debug_trace_exchange: the single-process G-device schedule, run on a host without GPUs).
struct XOps {
    virtual ~XOps() = default;
    virtual ncclResult_t group_start() = 0;
    virtual ncclResult_t group_end() = 0;
    virtual void set_device(int dev) = 0;
    virtual ncclResult_t split(ncclComm_t world, int color, int key, ncclComm_t* out) = 0;
    // op: MVG_X_GATHER or MVG_X_REDUCE (fp64 sum) of `count` doubles to `root`
    virtual ncclResult_t collective(int op, const double* src, double* dst, size_t count, int root, ncclComm_t comm,
                                    hipStream_t st) = 0;
    // exact mode's combine of one vector: rank 0's gathered partials of it -> its y
    virtual int combine(const mvg_engine* e, const Shard& s, double* parts, double* y, hipStream_t st) = 0;
};

struct DeviceXOps final : XOps {
    ncclResult_t group_start() override { return ncclGroupStart(); }
    ncclResult_t group_end() override { return ncclGroupEnd(); }
    void set_device(int dev) override { (void)hipSetDevice(dev); }
    ncclResult_t split(ncclComm_t world, int color, int key, ncclComm_t* out) override {
        return ncclCommSplit(world, color, key, out, nullptr);
    }
    ncclResult_t collective(int op, const double* src, double* dst, size_t count, int root, ncclComm_t comm,
                            hipStream_t st) override {
        return op == MVG_X_GATHER ? ncclGather(src, dst, count, ncclFloat64, root, comm, st)
                                  : ncclReduce(src, dst, count, ncclFloat64, ncclSum, root, comm, st);
    }
    int combine(const mvg_engine* e, const Shard& s, double* parts, double* y, hipStream_t st) override {
        return e->alg == MVG_ALG_COLWISE ? launch_combine_mpich_reduce(parts, e->nranks, e->R, y, st)
                                         : launch_combine_grid_rows(parts, s.plan.grid_rows, s.plan.grid_cols,
                                                                    s.plan.y_len, y, st);
    }
};

DeviceXOps g_device_ops;

// A shard keeps a grid-row buffer when a step of its schedule reads or writes one.
bool needs_row_buffer(const Shard& s) {
    bool need = false;
    for (int k = 0; k < s.nsteps; ++k)
        need |= s.steps[k].member && (s.steps[k].dst == MVG_X_BUF_ROW || s.steps[k].src == MVG_X_BUF_ROW);
    return need;
}

// Which exchange buffers a rank keeps, and how many doubles each holds, by MVG_X_BUF_*
// (-1: the rank keeps none). The engine allocates from this and the trace hands out its
// stand-in addresses from it, so the two cannot disagree. `exact` is the mode asked for.
struct XBufLens {
    int64_t len[4];
};
XBufLens exchange_buffers(const mvg_engine& e, const Shard& s, bool exact) {
    // the planner makes y_len = R for the column split: the partial is a whole y there
    const int64_t part = s.plan.y_len;
    XBufLens b;
    b.len[MVG_X_BUF_PART] = part;
    b.len[MVG_X_BUF_ROW] = needs_row_buffer(s) ? part : -1;
    b.len[MVG_X_BUF_Y] = s.rank == 0 ? e.R : -1;
    // exact mode: every rank's partial in rank order (the row split's gather is already exact)
    const bool gathers = exact && e.alg != MVG_ALG_ROWWISE && s.rank == 0 && s.nsteps > 0;
    b.len[MVG_X_BUF_GATHERED] = gathers ? part * e.nranks : -1;
    return b;
}

// One ncclGroupStart/End with every local shard's call in it. A failing call still closes the
// group before the error is reported.
template <class Call>
int grouped(std::vector<Shard>& shards, XOps& ops, const char* what, Call call) {
    MVG_NCCL(ops.group_start());
    ncclResult_t r = ncclSuccess;
    for (auto& s : shards)
        if ((r = call(s)) != ncclSuccess) break;
    const ncclResult_t r2 = ops.group_end();
    if (r != ncclSuccess) return nccl_fail(r, what);
    if (r2 != ncclSuccess) return nccl_fail(r2, (std::string(what) + ": ncclGroupEnd").c_str());
    return MVG_OK;
}

// Sub-communicators of the exchange schedule. ncclCommSplit is collective over the world, so
// every local rank calls it for every split step, inside one group per step.
int split_steps(std::vector<Shard>& shards, XOps& ops) {
    const int nsteps = shards.empty() ? 0 : shards[0].nsteps;
    for (int k = 0; k < nsteps; ++k) {
        if (shards[0].steps[k].comm == MVG_X_WORLD) {
            for (auto& s : shards) s.xcomm[k] = s.world;
            continue;
        }
        MVG_TRY(grouped(shards, ops, "ncclCommSplit", [&](Shard& s) {
            ops.set_device(s.device);
            const mvg_xstep& st = s.steps[k];
            s.owns_xcomm[k] = true;
            return ops.split(s.world, st.member ? st.color : NCCL_SPLIT_NOCOLOR, st.key, &s.xcomm[k]);
        }));
    }
    return MVG_OK;
}

// Exact mode's column-panel copy of a shard (s.panelP > 0), allocated when first needed if it
// fits in free HBM with 8 GiB to spare; otherwise the shard keeps the row-major exact kernels
// (panelP = 0 until exact mode is switched on again).
void alloc_panels(Shard& s) {
    const int64_t elems = s.pstride * ((s.plan.n_cols + s.panelP - 1) / s.panelP);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess ||
        (double)elems * sizeof(double) + (double)(8ll << 30) > (double)free_b ||
        hipMalloc((void**)&s.dAp, (size_t)elems * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        s.dAp = nullptr;
        s.panelP = s.pstride = 0;
    }
}

bool getenv_flag(const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '1';
}

struct DeviceGuard {
    int prev = 0;
    DeviceGuard() { (void)hipGetDevice(&prev); }
    ~DeviceGuard() { (void)hipSetDevice(prev); }
};

// n doubles of device memory; n <= 0 (an empty shard, a buffer this rank does not keep): none.
int alloc_doubles(double** p, int64_t n) {
    *p = nullptr;
    if (n <= 0) return MVG_OK;
    const hipError_t e = hipMalloc((void**)p, (size_t)n * sizeof(double));
    if (e == hipSuccess) return MVG_OK;
    *p = nullptr;
    hip_fail(e, "hipMalloc");
    return MVG_E_NOMEM;
}

// A shard's exchange buffers for nv vectors with a ring of `ring` partials (its device current),
// all but exact mode's gather buffer, which alloc_gathered makes when the mode first needs it.
int alloc_xbufs(const mvg_engine& e, const Shard& s, XBufs& x, int nv, int ring) {
    const XBufLens xb = exchange_buffers(e, s, false);
    for (int b = 0; b < ring; ++b) MVG_TRY(alloc_doubles(&x.parts[b], xb.len[MVG_X_BUF_PART] * nv));
    MVG_TRY(alloc_doubles(&x.row, xb.len[MVG_X_BUF_ROW] * nv));
    return alloc_doubles(&x.y, xb.len[MVG_X_BUF_Y] * nv);
}
int alloc_gathered(const mvg_engine& e, const Shard& s, XBufs& x, int nv, bool exact) {
    if (x.gathered) return MVG_OK;
    return alloc_doubles(&x.gathered, exchange_buffers(e, s, exact).len[MVG_X_BUF_GATHERED] * nv);
}

// The shard's device current, nothing in flight on the buffers: free_shard, and
// make_vector_buffers when the block grows.
void free_xbufs(XBufs& x) {
    for (double* p : x.parts)
        if (p) (void)hipFree(p);
    for (double* p : {x.row, x.y, x.gathered})
        if (p) (void)hipFree(p);
    x = XBufs{};
}

void free_shard(Shard& s) {
    (void)hipSetDevice(s.device);
    for (hipStream_t st : {s.stream, s.copy_stream, s.xstream})
        if (st) (void)hipStreamSynchronize(st);
    free_xbufs(s.one);
    free_xbufs(s.blk);
    for (double* p : {s.dA, s.dAp, s.dx, s.dX, s.stage})
        if (p) (void)hipFree(p);
    std::vector<hipEvent_t> events = {s.span_t0, s.span_t1, s.copy_ready, s.copied[0], s.copied[1],
                                      s.sent[0], s.sent[1],  s.ready};
    events.insert(events.end(), s.chunk_ev.begin(), s.chunk_ev.end());
    for (int b = 0; b < kRing; ++b) events.insert(events.end(), {s.gemv_done[b], s.x_done[b]});
    for (auto& pair : s.ev_pool) events.insert(events.end(), {pair.first, pair.second});
    for (hipEvent_t ev : events)
        if (ev) (void)hipEventDestroy(ev);
    for (int k = 0; k < MVG_MAX_XSTEPS; ++k)
        if (s.owns_xcomm[k] && s.xcomm[k]) (void)ncclCommDestroy(s.xcomm[k]);
    for (hipStream_t st : {s.stream, s.copy_stream, s.xstream})
        if (st) (void)hipStreamDestroy(st);
    s = Shard{};
}

// 2-D host -> device copy of a shard region into a packed device buffer (pitch = cols).
int h2d_region(double* dst, const double* host, int64_t ld_host, int64_t rows, int64_t cols, hipStream_t s) {
    if (rows == 0 || cols == 0) return MVG_OK;
    const size_t row_bytes = (size_t)cols * sizeof(double);
    if (cols == ld_host)
        MVG_HIP(hipMemcpyAsync(dst, host, (size_t)rows * row_bytes, hipMemcpyHostToDevice, s));
    else
        MVG_HIP(hipMemcpy2DAsync(dst, row_bytes, host, (size_t)ld_host * sizeof(double), row_bytes, (size_t)rows,
                                 hipMemcpyHostToDevice, s));
    return MVG_OK;
}

// The x segment of a shard (full x for the row split, the strip's or block's columns
// otherwise) and rows [r0, r0 + rows) of its A, from the host's whole x and A to `dst` on `st`.
int h2d_x(double* dst, const mvg_shard& p, const double* x, hipStream_t st) {
    return h2d_region(dst, x + p.col_off, p.n_cols, 1, p.n_cols, st);
}
int h2d_rows(double* dst, const mvg_shard& p, const double* A, int64_t r0, int64_t rows, hipStream_t st) {
    return h2d_region(dst, A + (p.row_off + r0) * p.C + p.col_off, p.C, rows, p.n_cols, st);
}

// A chunked distribution's copies into dA / dx may still be running on the copy stream. Any
// other writer of those buffers on s.stream (the synthetic fill, the root-send receives) first
// waits for the last of them (the copy stream runs in order), and the pending chunks are dropped:
// the next multiply then reads the whole new shard.
int drain_chunks(Shard& s) {
    if (s.chunks_pending && !s.chunk_ev.empty()) {
        const size_t last = s.chunk_row.size() >= 2 ? s.chunk_row.size() - 2 : 0;
        MVG_HIP(hipStreamWaitEvent(s.stream, s.chunk_ev[last], 0));
    }
    s.chunks_pending = false;
    return MVG_OK;
}

// An untimed event of a shard, made when first needed; free_shard releases it.
int ensure_event(hipEvent_t* ev) {
    if (!*ev) MVG_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return MVG_OK;
}

// Every shard-writing entry point starts here: the panel copies of A are stale, and a write
// while a kernel-timing span is open would land on the GEMV stream between the span's events,
// so the span no longer times GEMVs alone.
bool span_is_open(const mvg_engine* e) { return e->timing_every == -1 && e->span_multiplies > 0; }
void begin_write(mvg_engine* e) {
    if (span_is_open(e)) e->span_valid = false;
    for (auto& s : e->shards) s.panels_fresh = false, s.uses = 0;
}

// One shard's rows in `nch` chunks on the copy stream, each followed by an event; the next
// multiply runs each chunk's GEMV as soon as the chunk has landed: only
// the last chunk's GEMV is left after the transfer.
int distribute_chunked(Shard& s, const double* A, const double* x, int nch) {
    MVG_TRY(ensure_event(&s.copy_ready));
    if ((int)s.chunk_ev.size() < nch) s.chunk_ev.resize(nch, nullptr);
    // the copies overwrite dA and dx, which the GEMV last queued on s.stream still reads
    MVG_HIP(hipEventRecord(s.copy_ready, s.stream));
    MVG_HIP(hipStreamWaitEvent(s.copy_stream, s.copy_ready, 0));
    MVG_TRY(h2d_x(s.dx, s.plan, x, s.copy_stream));
    s.chunk_row.assign(nch + 1, 0);
    for (int c = 0; c <= nch; ++c) s.chunk_row[c] = s.plan.n_rows * c / nch;
    for (int c = 0; c < nch; ++c) {
        const int64_t r0 = s.chunk_row[c];
        MVG_TRY(h2d_rows(s.dA + r0 * s.plan.n_cols, s.plan, A, r0, s.chunk_row[c + 1] - r0, s.copy_stream));
        MVG_TRY(ensure_event(&s.chunk_ev[c]));
        MVG_HIP(hipEventRecord(s.chunk_ev[c], s.copy_stream));
    }
    s.chunks_pending = true;
    return MVG_OK;
}

// Every local device pulls its own shard (and x segment) from host memory that holds the
// whole A and x, over its own PCIe link, concurrently (one stream per device); in row chunks
// on the copy stream with overlap_chunks > 1. The whole of mvg_engine_distribute_shared, and of
// mvg_engine_distribute when all ranks are in this process.
int distribute_direct(mvg_engine* e, const double* A, const double* x) {
    begin_write(e);
    DeviceGuard g;
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        MVG_TRY(drain_chunks(s));
        if (e->overlap_chunks > 1 && s.plan.n_rows >= 2 * (int64_t)e->overlap_chunks) {
            MVG_TRY(distribute_chunked(s, A, x, e->overlap_chunks));
        } else {
            MVG_TRY(h2d_rows(s.dA, s.plan, A, 0, s.plan.n_rows, s.stream));
            MVG_TRY(h2d_x(s.dx, s.plan, x, s.stream));
        }
    }
    e->distributed = true;
    return MVG_OK;
}

// ---- root-send: rank 0 holds A and x and sends every peer its shard (one process per GPU)
// A shard travels as its x segment (row0 = -1), then its rows in runs of whole rows of at
// most `stage` doubles (the engine's stage_elems). The root's sends and the peer's receives
// both walk this list, so their counts agree call for call; empty pieces are left out on both
// sides.
struct Piece {
    int64_t row0, rows, count;
};
int shard_pieces(const mvg_shard& p, int64_t stage, std::vector<Piece>* out) {
    out->clear();
    if (p.n_cols == 0) return MVG_OK;
    if (p.n_cols > stage) return fail(MVG_E_INVALID, "row larger than staging");
    out->push_back({-1, 1, p.n_cols});
    const int64_t rows_per = stage / p.n_cols;
    for (int64_t r0 = 0; r0 < p.n_rows; r0 += rows_per) {
        const int64_t rows = std::min(rows_per, p.n_rows - r0);
        out->push_back({r0, rows, rows * p.n_cols});
    }
    return MVG_OK;
}

hipEvent_t last_x_done(const mvg_engine* e, const Shard& s) { return s.x_done[(e->nx - 1) % e->ring]; }

// Rank 0's shard, where this process holds it: the root's arguments are checked and y is
// collected only there.
Shard* root_shard(mvg_engine* e) {
    for (auto& s : e->shards)
        if (s.rank == 0) return &s;
    return nullptr;
}

// The synthetic fills return with the data in place.
int sync_gemv_streams(mvg_engine* e) {
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        MVG_HIP(hipStreamSynchronize(s.stream));
    }
    return MVG_OK;
}

// Rank 0 stages each peer's shard through two device buffers and ncclSend's it over xGMI (the
// reference's sequential root Send loop, colwise.c:33-57), overlapping the next piece's H2D
// with the current piece's send; then copies its own shard.
int root_send_shards(mvg_engine* e, Shard& s, const double* A, const double* x) {
    if (!s.stage) MVG_TRY(alloc_doubles(&s.stage, 2 * e->stage_elems));
    for (hipEvent_t* ev : {&s.copied[0], &s.copied[1], &s.sent[0], &s.sent[1], &s.ready}) MVG_TRY(ensure_event(ev));
    // sent[b] starts recorded on s.stream, behind the previous GEMV (which reads dA, dx)
    // and the caller's exchange wait: every copy_stream write below is ordered after those
    for (int b = 0; b < 2; ++b) MVG_HIP(hipEventRecord(s.sent[b], s.stream));
    // the own shard's copy into dA/dx needs that order even when no peer piece is sent
    // (every peer shard empty); waiting on the initial record keeps it overlapping the
    // last peer sends
    MVG_HIP(hipEventRecord(s.ready, s.stream));
    int buf = 0;
    std::vector<Piece> pieces;
    for (int peer = 1; peer < e->nranks; ++peer) {
        mvg_shard p;
        MVG_TRY(mvg_plan_shard(e->alg, e->R, e->C, e->nranks, peer, &p));
        MVG_TRY(shard_pieces(p, e->stage_elems, &pieces));
        for (const Piece& pc : pieces) {
            double* stage = s.stage + buf * e->stage_elems;
            MVG_HIP(hipStreamWaitEvent(s.copy_stream, s.sent[buf], 0));
            MVG_TRY(pc.row0 < 0 ? h2d_x(stage, p, x, s.copy_stream)
                                : h2d_rows(stage, p, A, pc.row0, pc.rows, s.copy_stream));
            MVG_HIP(hipEventRecord(s.copied[buf], s.copy_stream));
            MVG_HIP(hipStreamWaitEvent(s.stream, s.copied[buf], 0));
            MVG_NCCL(ncclSend(stage, (size_t)pc.count, ncclFloat64, peer, s.world, s.stream));
            MVG_HIP(hipEventRecord(s.sent[buf], s.stream));
            buf ^= 1;
        }
    }
    // own shard last (MPI_Pack of the root's own strip comes last too, colwise.c:61-69)
    MVG_HIP(hipStreamWaitEvent(s.copy_stream, s.ready, 0));
    MVG_TRY(h2d_rows(s.dA, s.plan, A, 0, s.plan.n_rows, s.copy_stream));
    MVG_TRY(h2d_x(s.dx, s.plan, x, s.copy_stream));
    MVG_HIP(hipEventRecord(s.copied[0], s.copy_stream));
    MVG_HIP(hipStreamWaitEvent(s.stream, s.copied[0], 0));
    return MVG_OK;
}

// A peer receives its shard's pieces from rank 0 straight into dx and dA.
int recv_shard(const mvg_engine* e, Shard& s) {
    std::vector<Piece> pieces;
    MVG_TRY(shard_pieces(s.plan, e->stage_elems, &pieces));
    for (const Piece& pc : pieces)
        MVG_NCCL(ncclRecv(pc.row0 < 0 ? s.dx : s.dA + pc.row0 * s.plan.n_cols, (size_t)pc.count, ncclFloat64, 0, s.world,
                          s.stream));
    return MVG_OK;
}

// ---- one multiply's exchange out of ring slot b of a buffer set (Shard::one: mvg_engine_multiply,
// nv = 1; Shard::blk: mvg_engine_multiply_multi over a block of nv vectors), as the engine and the
// trace both issue it. Every buffer is column-major, one vector per column.
// The steps of the shared schedule (mvg_plan_exchange): one group per step, every local member
// issuing its calls in it. A reduce step moves the nv columns as one contiguous run of count * nv
// doubles; a gather step moves vector v with its own call, into column v of the root's Y (ld = R:
// the members' pieces of one vector make up a whole y), so Y needs no transposing pass.
int exchange_plan(mvg_engine* e, XBufs Shard::*set, int b, int nv, bool serial, XOps& ops) {
    for (int k = 0; k < e->shards[0].nsteps; ++k) {
        const char* what = e->shards[0].steps[k].op == MVG_X_GATHER ? "ncclGather" : "ncclReduce";
        MVG_TRY(grouped(e->shards, ops, what, [&](Shard& s) {
            const mvg_xstep& st = s.steps[k];
            if (!st.member) return ncclSuccess;
            ops.set_device(s.device);
            XBufs& x = s.*set;
            const double* src = x.at(st.src, b);
            const bool writes = x.at(st.dst, b) != nullptr;  // recvbuff is only written on the root
            double* dst = writes ? x.at(st.dst, b) : x.parts[b];
            hipStream_t stream = serial ? s.stream : s.xstream;
            if (st.op == MVG_X_REDUCE)
                return ops.collective(st.op, src, dst, (size_t)st.count * nv, st.root, s.xcomm[k], stream);
            ncclResult_t r = ncclSuccess;
            for (int v = 0; v < nv && r == ncclSuccess; ++v)
                r = ops.collective(st.op, src + v * st.count, writes ? dst + v * e->R : dst, (size_t)st.count, st.root,
                                   s.xcomm[k], stream);
            return r;
        }));
    }
    return MVG_OK;
}

// Exact mode (mvg_engine_set_exact): per vector every partial gathered to rank 0 in rank order
// (all nv in one group), then added there in the reference's order, once per vector, each as if
// that vector were alone (the MPICH algorithm switch looks at one y's length).
int exchange_exact(mvg_engine* e, XBufs Shard::*set, int b, int nv, bool serial, XOps& ops) {
    MVG_TRY(grouped(e->shards, ops, "ncclGather (exact)", [&](Shard& s) {
        ops.set_device(s.device);
        XBufs& x = s.*set;
        const int64_t n = s.plan.y_len;
        ncclResult_t r = ncclSuccess;
        for (int v = 0; v < nv && r == ncclSuccess; ++v)  // recvbuff is only written on the root
            r = ops.collective(MVG_X_GATHER, x.parts[b] + v * n, s.rank == 0 ? x.gathered + v * e->nranks * n : x.parts[b],
                               (size_t)n, 0, s.world, serial ? s.stream : s.xstream);
        return r;
    }));
    for (auto& s : e->shards) {
        if (s.rank != 0) continue;
        ops.set_device(s.device);
        XBufs& x = s.*set;
        for (int v = 0; v < nv; ++v)
            MVG_TRY(ops.combine(e, s, x.gathered + v * e->nranks * s.plan.y_len, x.y + v * e->R,
                                serial ? s.stream : s.xstream));
    }
    return MVG_OK;
}

int exchange(mvg_engine* e, XBufs Shard::*set, int b, int nv, bool serial, XOps& ops) {
    return e->exact && e->alg != MVG_ALG_ROWWISE ? exchange_exact(e, set, b, nv, serial, ops)
                                                 : exchange_plan(e, set, b, nv, serial, ops);
}

// The recorder behind mvg_debug_trace_exchange. Communicators and buffers are stand-in handles
// the trace hands out; every call is listed with the group it was issued in.
struct TraceXOps final : XOps {
    std::vector<mvg_xcall> calls;
    int group = -1, depth = 0, device = 0;
    std::vector<std::pair<uintptr_t, int>> comm_step;  // handle -> group that created it (-1 world)
    std::vector<std::pair<uintptr_t, std::pair<int, int>>> buffers;  // address -> (rank, MVG_X_BUF_*)
    uintptr_t next_comm = 0x7e0000;

    int comm_of(ncclComm_t c) const {
        for (auto& kv : comm_step)
            if (kv.first == (uintptr_t)c) return kv.second;
        return -2;
    }
    static constexpr uintptr_t kBufSpan = (uintptr_t)1 << 40;  // bytes a stand-in buffer spans
    int buf_of(const double* p) const {  // a vector's part of a block's buffer is an offset into it
        for (auto& kv : buffers)
            if ((uintptr_t)p >= kv.first && (uintptr_t)p - kv.first < kBufSpan) return kv.second.second;
        return -1;
    }
    mvg_xcall base(int kind) const {
        mvg_xcall c{};
        c.group = depth > 0 ? group : -1;  // -1: outside any group (the combine kernel)
        c.kind = kind;
        c.rank = device;  // the trace's devices are its ranks
        c.comm = -1;
        c.color = c.key = c.root = -1;
        c.src = c.dst = -1;
        return c;
    }
    ncclResult_t group_start() override {
        if (depth++ == 0) ++group;
        return ncclSuccess;
    }
    ncclResult_t group_end() override {
        if (depth > 0) --depth;
        return ncclSuccess;
    }
    void set_device(int dev) override { device = dev; }
    ncclResult_t split(ncclComm_t world, int color, int key, ncclComm_t* out) override {
        mvg_xcall c = base(MVG_XCALL_SPLIT);
        c.comm = comm_of(world);
        c.color = color == NCCL_SPLIT_NOCOLOR ? -1 : color;
        c.key = key;
        calls.push_back(c);
        *out = (ncclComm_t)(next_comm++);
        comm_step.push_back({(uintptr_t)*out, group});
        return ncclSuccess;
    }
    ncclResult_t collective(int op, const double* src, double* dst, size_t count, int root, ncclComm_t comm,
                            hipStream_t) override {
        mvg_xcall c = base(op == MVG_X_GATHER ? MVG_XCALL_GATHER : MVG_XCALL_REDUCE);
        c.comm = comm_of(comm);
        c.root = root;
        c.count = (int64_t)count;
        c.src = buf_of(src);
        c.dst = buf_of(dst);
        calls.push_back(c);
        return ncclSuccess;
    }
    int combine(const mvg_engine* e, const Shard& s, double* parts, double* y, hipStream_t) override {
        mvg_xcall c = base(MVG_XCALL_COMBINE);
        c.count = s.plan.y_len * e->nranks;
        c.src = buf_of(parts);
        c.dst = buf_of(y);
        calls.push_back(c);
        return MVG_OK;
    }
};

// ---- the steps of mvg_engine_create, per local rank
// Plan, streams, buffers and the ring's events.
int init_shard(mvg_engine* e, Shard& s, const LocalRank& l) {
    s.device = l.device;
    s.rank = l.rank;
    s.world = l.comm;
    MVG_TRY(mvg_plan_shard(e->alg, e->R, e->C, e->nranks, l.rank, &s.plan));
    MVG_HIP(hipSetDevice(s.device));
    MVG_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    MVG_HIP(hipStreamCreateWithFlags(&s.copy_stream, hipStreamNonBlocking));
    MVG_TRY(alloc_doubles(&s.dA, s.plan.n_rows * s.plan.n_cols));
    MVG_TRY(alloc_doubles(&s.dx, s.plan.n_cols));
    MVG_TRY(mvg_plan_exchange(e->alg, e->R, e->C, e->nranks, l.rank, e->always_collect, s.steps, MVG_MAX_XSTEPS,
                              &s.nsteps));
    MVG_TRY(alloc_xbufs(*e, s, s.one, 1, s.nsteps > 0 ? e->ring : 1));
    if (s.nsteps > 0) {
        MVG_HIP(hipStreamCreateWithFlags(&s.xstream, hipStreamNonBlocking));
        for (int b = 0; b < e->ring; ++b) {
            // GEMV -> exchange kernel on the same device: no system-scope fence needed (the
            // marker with one cost ~2 us of idle GPU per multiply); exchange -> collect's
            // D2H copy keeps the default (host-visible) fence
            MVG_HIP(hipEventCreateWithFlags(&s.gemv_done[b], hipEventDisableTiming | hipEventDisableSystemFence));
            MVG_TRY(ensure_event(&s.x_done[b]));
        }
    }
    return MVG_OK;
}

// Warm the device before any timed loop: first-touch every buffer (the first H2D into
// never-touched HBM ran at 11 GB/s instead of 56, profiles/r01/e2e_small/numa_h2d.jsonl) and launch the
// shard's GEMV once (loads its code object and any split-K workspace). These one-time
// costs are the GPU runtime's analogue of MPI_Init; without this they landed in the
// executables' first timed iteration (+0.1 ms on the mean at 600 x 600).
int warm_shard(mvg_engine* e, Shard& s) {
    const mvg_shard& p = s.plan;
    auto zero = [&](double* d, int64_t n) -> int {
        if (d && n > 0) MVG_HIP(hipMemsetAsync(d, 0, (size_t)n * sizeof(double), s.stream));
        return MVG_OK;
    };
    MVG_TRY(zero(s.dA, p.n_rows * p.n_cols));
    MVG_TRY(zero(s.dx, p.n_cols));
    for (double* part : s.one.parts) MVG_TRY(zero(part, p.y_len));
    MVG_TRY(zero(s.one.row, p.y_len));
    MVG_TRY(zero(s.one.y, e->R));
    MVG_TRY(mvg_gemv(s.dA, p.n_cols, s.dx, s.one.parts[0], p.n_rows, p.n_cols, s.stream));
    // ... and one page-locked H2D into A's buffer and D2H out of y's, as large as those
    // transfers will be up to 4 MiB, on each stream that distributes or collects. The
    // runtime brings its large-copy path up on the first such transfer of the process:
    // 8.2 ms once (tools/probes/first_copy.py: 2.88 MB from any page-locked buffer, 8.2 ms first,
    // 66 us after; 512-B copies do not trigger it), which otherwise landed in the
    // executables' first timed iteration (bin/multiplier_rowwise 600 600, MVG_ITER_LOG).
    const int64_t a_elems = std::min<int64_t>(p.n_rows * p.n_cols, 1 << 19);
    const int64_t y_elems = std::min<int64_t>(p.y_len, 1 << 19);
    const size_t wbytes = (size_t)std::max<int64_t>({a_elems, y_elems, 1}) * sizeof(double);
    double* pinned = nullptr;
    if (hipHostMalloc((void**)&pinned, wbytes, hipHostMallocDefault) != hipSuccess)
        return fail(MVG_E_NOMEM, "hipHostMalloc (engine warm-up)");
    memset(pinned, 0, wbytes);
    hipError_t we = hipSuccess;
    for (hipStream_t st : {s.stream, s.copy_stream}) {
        if (we == hipSuccess && a_elems > 0)
            we = hipMemcpyAsync(s.dA, pinned, (size_t)a_elems * sizeof(double), hipMemcpyHostToDevice, st);
        if (we == hipSuccess && y_elems > 0)
            we = hipMemcpyAsync(pinned, s.one.parts[0], (size_t)y_elems * sizeof(double), hipMemcpyDeviceToHost, st);
        if (we == hipSuccess) we = hipStreamSynchronize(st);
    }
    (void)hipHostFree(pinned);
    return we == hipSuccess ? MVG_OK : hip_fail(we, "engine warm-up");
}

// ---- the steps of mvg_engine_multiply, per local rank
// Exact mode's panel copy of A, rebuilt from dA by the second multiply after a write: the
// rebuild moves the shard twice through HBM (about ten multiplies' worth of the panels'
// gain), so a distribution that is multiplied once (the reference's timed loop: distribute +
// multiply per iteration) never pays for it, and repeated multiplies of the same A
// (device-resident) run on panels from the second one on.
int refresh_panels(mvg_engine* e, Shard& s, bool span_opens) {
    if (!e->exact || !s.panelP || s.panels_fresh || s.uses < 1 || s.chunks_pending) return MVG_OK;
    if (!s.dAp) alloc_panels(s);
    if (!s.dAp) return MVG_OK;
    const mvg_shard& p = s.plan;
    MVG_TRY(mvg_panel_relayout(s.dA, p.n_cols, p.n_rows, p.n_cols, s.dAp, s.pstride, s.panelP, s.stream));
    s.panels_fresh = true;
    // a relayout after the span's first event would be counted as GEMV time
    if (e->timing_every == -1 && !span_opens) e->span_valid = false;
    return MVG_OK;
}

// The shard's product into `out`: one GEMV, or one per row chunk of a pending chunked
// distribution (independent products: each runs once its rows have landed).
int local_product(mvg_engine* e, Shard& s, double* out) {
    const mvg_shard& p = s.plan;
    const bool panels = e->exact && s.dAp && s.panels_fresh;
    auto gemv = [&](int64_t r0, int64_t rows) {
        if (panels)
            return mvg_gemv_exact_panels(s.dAp + r0 * s.panelP, s.pstride, s.panelP, s.dx, out + r0, rows, p.n_cols, 0,
                                         s.stream);
        return e->exact ? mvg_gemv_exact(s.dA + r0 * p.n_cols, p.n_cols, s.dx, out + r0, rows, p.n_cols, s.stream)
                        : mvg_gemv(s.dA + r0 * p.n_cols, p.n_cols, s.dx, out + r0, rows, p.n_cols, s.stream);
    };
    if (!s.chunks_pending) return gemv(0, p.n_rows);
    s.chunks_pending = false;
    for (size_t c = 0; c + 1 < s.chunk_row.size(); ++c) {
        MVG_HIP(hipStreamWaitEvent(s.stream, s.chunk_ev[c], 0));
        MVG_TRY(gemv(s.chunk_row[c], s.chunk_row[c + 1] - s.chunk_row[c]));
    }
    return MVG_OK;
}

// ---- kernel timing (mvg_engine_kernel_timing). A multiply whose GEMVs wait on a chunked
// distribution's copies (`chunked`) is not timed in either mode.
// Span mode (-1): one event before the first GEMV of the span, one at the next sync, no marker
// between the GEMVs in between (a timing marker costs the stream ~6 us around the kernel it
// brackets, profiles/r05/t5c); a chunked distribution's copies inside the span void it.
// Counts the multiply; true when it opens the span (span_start on every shard).
bool span_enter(mvg_engine* e, bool chunked) {
    if (e->timing_every != -1) return false;
    if (chunked) e->span_valid = false;
    return e->span_multiplies++ == 0 && !chunked;
}
int span_start(Shard& s) {
    if (!s.span_t0) MVG_HIP(hipEventCreate(&s.span_t0));
    if (!s.span_t1) MVG_HIP(hipEventCreate(&s.span_t1));
    MVG_HIP(hipEventRecord(s.span_t0, s.stream));
    return MVG_OK;
}
// After a sync that recorded span_t1 on every GEMV stream: the span's GEMV time per multiply is
// the first GEMV's start to the stream's end, max over the local devices (the GEMV stream holds
// nothing else at one rank per process; with an exchange it also holds the once-per-ring waits
// on the exchange stream).
int span_close(mvg_engine* e) {
    float worst = 0.f;
    for (auto& s : e->shards) {
        if (!s.span_t0 || !s.span_t1) continue;
        float ms = 0.f;
        MVG_HIP(hipEventElapsedTime(&ms, s.span_t0, s.span_t1));
        worst = std::max(worst, ms);
    }
    if (e->span_valid) {
        e->kernel_ms_sum += worst;
        e->kernel_launches += e->span_multiplies;
    }
    e->span_multiplies = 0;
    e->span_valid = true;
    return MVG_OK;
}

// Per-launch mode (N > 0): every Nth multiply is bracketed by a pair of events from a pool.
bool pool_enter(mvg_engine* e, bool chunked) {
    return e->timing_every > 0 && (e->multiply_calls++ % e->timing_every) == 0 && !chunked;
}
// Records the pair's first event on the GEMV stream; the caller records *stop after the product.
int pool_start(Shard& s, hipEvent_t* stop) {
    if (s.ev_used == s.ev_pool.size()) {
        hipEvent_t a, b;
        MVG_HIP(hipEventCreate(&a));
        MVG_HIP(hipEventCreate(&b));
        s.ev_pool.emplace_back(a, b);
    }
    const auto& pair = s.ev_pool[s.ev_used++];
    *stop = pair.second;
    MVG_HIP(hipEventRecord(pair.first, s.stream));
    return MVG_OK;
}
// After a sync: per timed multiply the max over the local devices, summed; the pool is free again.
int pool_collect(mvg_engine* e) {
    const size_t n = e->timing_every > 0 && !e->shards.empty() ? e->shards[0].ev_used : 0;
    for (size_t k = 0; k < n; ++k) {
        float worst = 0.f;
        for (auto& s : e->shards) {
            if (k >= s.ev_used) continue;
            float ms = 0.f;
            MVG_HIP(hipEventElapsedTime(&ms, s.ev_pool[k].first, s.ev_pool[k].second));
            worst = std::max(worst, ms);
        }
        e->kernel_ms_sum += worst;
        ++e->kernel_launches;
    }
    for (auto& s : e->shards) s.ev_used = 0;
    return MVG_OK;
}

// ---- the frame of both multiplies: product(s, out) queues the shard's product into
// `out` on s.stream; the exchange out of buffer set `set` follows on the exchange stream,
// overlapping the next multiply's product. Both kinds share the slot counter and the events, so the
// once-per-ring wait, x_pending and the collects' waits cover them in any mix.
template <class Product>
int multiply_step(mvg_engine* e, XBufs Shard::*set, int nv, Product product) {
    const bool solo = e->shards[0].nsteps == 0;  // P == 1: the product goes straight into y
    const bool serial = e->ring == 1;
    const int b = solo ? 0 : (int)(e->nx % e->ring);
    // The product writes parts[b]; the exchange that last read it was multiply nx - ring's. The
    // GEMV stream waits once per ring, on the latest exchange (nx - 1): every slot is then free
    // for the next `ring` GEMVs (the exchange stream runs in order), so one cross-stream wait is
    // paid per ring instead of per multiply (measured: a wait per multiply cost more than the
    // overlap saved at world size 1).
    const bool wait_ring = !solo && !serial && e->x_pending && b == 0;
    // 1) local product on every device
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        if (wait_ring) MVG_HIP(hipStreamWaitEvent(s.stream, last_x_done(e, s), 0));
        MVG_TRY(product(s, solo ? (s.*set).y : (s.*set).parts[b]));
        if (!solo && !serial) {  // hand over to the exchange stream
            MVG_HIP(hipEventRecord(s.gemv_done[b], s.stream));
            MVG_HIP(hipStreamWaitEvent(s.xstream, s.gemv_done[b], 0));
        }
    }
    if (solo) return MVG_OK;
    // 2) the exchange step
    MVG_TRY(exchange(e, set, b, nv, serial, g_device_ops));
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        if (!serial) MVG_HIP(hipEventRecord(s.x_done[b], s.xstream));
    }
    e->x_pending = !serial;
    ++e->nx;
    return MVG_OK;
}

// Both collects on rank 0's shard: y is complete once the last exchange is; copy(s) queues the
// device-to-host copy on s.stream.
template <class Copy>
int collect_from(mvg_engine* e, Shard& s, Copy copy) {
    DeviceGuard g;
    MVG_HIP(hipSetDevice(s.device));
    if (e->x_pending) MVG_HIP(hipStreamWaitEvent(s.stream, last_x_done(e, s), 0));
    if (e->R > 0) MVG_TRY(copy(s));
    MVG_HIP(hipStreamSynchronize(s.stream));
    return MVG_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ bound runtimes
int mvg_runtime_versions(int* rccl_version, int* hip_runtime_version) {
    if (rccl_version) MVG_NCCL(ncclGetVersion(rccl_version));
    if (hip_runtime_version) MVG_HIP(hipRuntimeGetVersion(hip_runtime_version));
    return MVG_OK;
}

// The object that defines one symbol of each runtime as this library resolved it: the copy the
// process actually calls, whichever loaded first with the same soname.
const char* mvg_runtime_path(int which) {
    const void* sym = which == 0 ? (const void*)&hipGetDeviceCount
                    : which == 1 ? (const void*)&ncclGetVersion : nullptr;
    Dl_info info;
    if (!sym || dladdr(sym, &info) == 0 || !info.dli_fname) return "";
    return info.dli_fname;
}

// ------------------------------------------------------------------ communicators
int mvg_comm_unique_id(unsigned char out[MVG_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == MVG_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!out) return fail(MVG_E_INVALID, "null");
    ncclUniqueId id;
    MVG_NCCL(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return MVG_OK;
}

int mvg_comm_init_all(mvg_comm** out, int ndev, const int* devlist) {
    if (!out || ndev <= 0) return fail(MVG_E_INVALID, "mvg_comm_init_all: bad arguments");
    *out = nullptr;
    std::vector<int> devs(ndev);
    for (int i = 0; i < ndev; ++i) devs[i] = devlist ? devlist[i] : i;
    std::vector<ncclComm_t> comms(ndev, nullptr);
    DeviceGuard g;
    // One device needs no collective (the exchange plan is empty), so RCCL is not initialised
    // at all — no bootstrap cost, no RCCL banner on the executables' stdout — unless
    // MVG_ALWAYS_COLLECT=1 asks for the collectives to run anyway.
    if (ndev > 1 || getenv_flag("MVG_ALWAYS_COLLECT")) {
        MVG_NCCL(ncclCommInitAll(comms.data(), ndev, devs.data()));
    } else {
        MVG_HIP(hipSetDevice(devs[0]));
    }
    mvg_comm* c = new mvg_comm;
    c->nranks = ndev;
    for (int i = 0; i < ndev; ++i) c->locals.push_back(LocalRank{i, devs[i], comms[i]});
    *out = c;
    return MVG_OK;
}

int mvg_comm_init_rank(mvg_comm** out, const unsigned char id[MVG_UNIQUE_ID_BYTES], int nranks,
                       int rank, int device) {
    if (!out || !id || nranks <= 0 || rank < 0 || rank >= nranks)
        return fail(MVG_E_INVALID, "mvg_comm_init_rank: bad arguments");
    *out = nullptr;
    MVG_HIP(hipSetDevice(device));
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclComm_t comm;
    MVG_NCCL(ncclCommInitRank(&comm, nranks, uid, rank));
    mvg_comm* c = new mvg_comm;
    c->nranks = nranks;
    c->locals.push_back(LocalRank{rank, device, comm});
    *out = c;
    return MVG_OK;
}

int mvg_comm_size(const mvg_comm* c, int* n) {
    if (!c || !n) return fail(MVG_E_INVALID, "null");
    *n = c->nranks;
    return MVG_OK;
}
int mvg_comm_local_count(const mvg_comm* c, int* n) {
    if (!c || !n) return fail(MVG_E_INVALID, "null");
    *n = (int)c->locals.size();
    return MVG_OK;
}
int mvg_comm_local_rank(const mvg_comm* c, int i, int* rank, int* device) {
    if (!c || i < 0 || i >= (int)c->locals.size()) return fail(MVG_E_INVALID, "bad local index");
    if (rank) *rank = c->locals[i].rank;
    if (device) *device = c->locals[i].device;
    return MVG_OK;
}
int mvg_comm_destroy(mvg_comm* c) {
    if (!c) return MVG_OK;
    DeviceGuard g;
    for (auto& l : c->locals) {
        (void)hipSetDevice(l.device);
        if (l.comm) (void)ncclCommDestroy(l.comm);
    }
    delete c;
    return MVG_OK;
}

// ------------------------------------------------------------------ engine
int mvg_engine_destroy(mvg_engine* e) {
    if (!e) return MVG_OK;
    DeviceGuard g;
    for (auto& s : e->shards) free_shard(s);
    delete e;
    return MVG_OK;
}

int mvg_engine_create(mvg_engine** out, int alg, int64_t R, int64_t C, mvg_comm* comm) {
    if (!out || !comm || R < 0 || C < 0) return fail(MVG_E_INVALID, "mvg_engine_create: bad arguments");
    *out = nullptr;
    // Validate the whole grid first (the reference's root-only divisibility check).
    mvg_shard probe;
    int rc = mvg_plan_shard(alg, R, C, comm->nranks, 0, &probe);
    if (rc != MVG_OK) return rc;

    DeviceGuard g;
    mvg_engine* e = new mvg_engine;
    e->alg = alg;
    e->R = R;
    e->C = C;
    e->nranks = comm->nranks;
    e->single_process = (int)comm->locals.size() == comm->nranks;
    // forced collectives need an RCCL communicator (a one-device comm made without the
    // variable has none)
    e->always_collect = getenv_flag("MVG_ALWAYS_COLLECT") && comm->locals[0].comm != nullptr;
    e->stage_elems = g_stage_elems;
    if (const char* v = getenv("MVG_XRING")) e->ring = std::max(1, std::min(kRing, atoi(v)));
    if (const char* ov = getenv("MVG_OVERLAP")) e->overlap_chunks = std::max(0, atoi(ov));

    e->shards.resize(comm->locals.size());
    for (size_t i = 0; i < comm->locals.size() && rc == MVG_OK; ++i) {
        rc = init_shard(e, e->shards[i], comm->locals[i]);
        if (rc == MVG_OK) rc = warm_shard(e, e->shards[i]);
    }
    if (rc == MVG_OK) rc = split_steps(e->shards, g_device_ops);
    if (rc == MVG_OK && getenv_flag("MVG_EXACT")) rc = mvg_engine_set_exact(e, 1);
    if (rc != MVG_OK) {
        mvg_engine_destroy(e);
        return rc;
    }
    *out = e;
    return MVG_OK;
}

// Exact mode: the local products come from mvg_gemv_exact (the reference's sequential sums) and
// the exchange reproduces the reference's combine order instead of RCCL's: every rank's partial
// is gathered to rank 0 in rank order (one ncclGather) and a small kernel there adds them as
// the reference does — MPI_Reduce's tree as MPICH picks it for the column split (colwise.c:124), the
// grid row's blocks into a zeroed y in rank order for the block split (blockwise.c:150-207).
// The row split's gather is a copy and stays as it is. y is then bit-identical to the
// reference's (block split: to its result for rank-order arrival, which is every arrival order
// when the grid has at most two columns).
int mvg_engine_set_exact(mvg_engine* e, int on) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    MVG_TRY(mvg_engine_sync(e));
    const bool exact = on != 0;
    DeviceGuard g;
    // whatever can fail comes first: an error leaves the mode and the panel fields as they were
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        MVG_TRY(alloc_gathered(*e, s, s.one, 1, exact));
    }
    e->exact = exact;
    for (auto& s : e->shards) {
        (void)hipSetDevice(s.device);
        if (!exact) {
            if (s.dAp) (void)hipFree(s.dAp);
            s.dAp = nullptr;
            s.panelP = s.pstride = 0;
        } else if (!s.dAp && !getenv_flag("MVG_NO_PANELS")) {
            // the panel copy where it pays (mvg_exact_panel_width); allocated by the multiply that
            // first needs it (alloc_panels), so a distribute-per-multiply loop never holds one
            s.panelP = mvg_exact_panel_width(s.plan.n_rows, s.plan.n_cols);
            s.pstride = s.plan.n_rows * s.panelP;
            s.panels_fresh = false;
        }
    }
    return MVG_OK;
}

int mvg_engine_exact_panels(const mvg_engine* e, int i, int64_t* P) {
    if (!e || !P || i < 0 || i >= (int)e->shards.size()) return fail(MVG_E_INVALID, "bad index");
    // a copy that a write has made stale is kept allocated, but the shard runs the row-major
    // kernels until the second multiply rebuilds it
    const Shard& s = e->shards[i];
    *P = e->exact && s.dAp && s.panels_fresh ? s.panelP : 0;
    return MVG_OK;
}

int mvg_engine_exact(const mvg_engine* e, int* on) {
    if (!e || !on) return fail(MVG_E_INVALID, "null");
    *on = e->exact ? 1 : 0;
    return MVG_OK;
}

int mvg_engine_set_overlap(mvg_engine* e, int chunks) {
    if (!e || chunks < 0) return fail(MVG_E_INVALID, "mvg_engine_set_overlap: bad arguments");
    MVG_TRY(mvg_engine_sync(e));
    e->overlap_chunks = chunks;
    return MVG_OK;
}

int mvg_engine_shard(const mvg_engine* e, int i, mvg_shard* out) {
    if (!e || !out || i < 0 || i >= (int)e->shards.size()) return fail(MVG_E_INVALID, "bad index");
    *out = e->shards[i].plan;
    return MVG_OK;
}

int mvg_engine_stream(const mvg_engine* e, int i, void** stream) {
    if (!e || !stream || i < 0 || i >= (int)e->shards.size()) return fail(MVG_E_INVALID, "bad index");
    *stream = (void*)e->shards[i].stream;
    return MVG_OK;
}

int mvg_engine_fill_synth(mvg_engine* e, uint64_t seed_a, uint64_t seed_x) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    begin_write(e);
    DeviceGuard g;
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        MVG_TRY(drain_chunks(s));
        const mvg_shard& p = s.plan;
        MVG_TRY(mvg_synth_fill_device(s.dA, p.n_cols, p.n_rows, p.n_cols, p.row_off, p.col_off, e->C, seed_a, s.stream));
        MVG_TRY(mvg_synth_fill_device(s.dx, p.n_cols, 1, p.n_cols, 0, p.col_off, e->C, seed_x, s.stream));
    }
    MVG_TRY(sync_gemv_streams(e));
    e->distributed = true;
    return MVG_OK;
}

// Root (rank 0's process) holds A and x in host memory, as in every reference driver.
// Single-process: each device pulls its own shard over its own PCIe link (distribute_direct).
// One process per GPU: rank 0 sends every peer its shard (root_send_shards / recv_shard).
int mvg_engine_distribute(mvg_engine* e, const double* A, const double* x) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    const bool root = root_shard(e) != nullptr;
    if (root && (!x || (!A && e->R * e->C > 0))) return fail(MVG_E_INVALID, "root needs A and x");
    if (e->single_process) return distribute_direct(e, A, x);
    begin_write(e);
    DeviceGuard g;
    Shard& s = e->shards[0];  // exactly one local shard
    MVG_HIP(hipSetDevice(s.device));
    // the root-send form always lands whole shards on s.stream, after any chunked copies
    MVG_TRY(drain_chunks(s));
    // the sends/recvs use the world communicator on s.stream: order them after any exchange
    // still running on s.xstream (one communicator, one order of operations)
    if (e->x_pending) MVG_HIP(hipStreamWaitEvent(s.stream, last_x_done(e, s), 0));
    MVG_TRY(s.rank == 0 ? root_send_shards(e, s, A, x) : recv_shard(e, s));
    e->distributed = true;
    return MVG_OK;
}

int mvg_engine_distribute_shared(mvg_engine* e, const double* A, const double* x) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    if (!x || (!A && e->R * e->C > 0)) return fail(MVG_E_INVALID, "every rank needs the shared A and x");
    return distribute_direct(e, A, x);
}

int mvg_engine_kernel_timing(mvg_engine* e, int enable) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    MVG_TRY(mvg_engine_sync(e));
    e->timing_every = enable > 0 ? enable : enable == -1 ? -1 : 0;
    e->span_multiplies = 0;
    e->span_valid = true;
    e->multiply_calls = 0;
    e->kernel_ms_sum = 0.0;
    e->kernel_launches = 0;
    return MVG_OK;
}

int mvg_engine_multiply(mvg_engine* e) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    if (!e->distributed) return fail(MVG_E_STATE, "mvg_engine_multiply before distribute/fill");
    DeviceGuard g;
    bool chunked = false;  // a chunked distribution is pending: the GEMVs wait on copies, not timed
    for (auto& s : e->shards) chunked |= s.chunks_pending;
    const bool timed = pool_enter(e, chunked);
    const bool span_opens = span_enter(e, chunked);
    return multiply_step(e, &Shard::one, 1, [&](Shard& s, double* out) -> int {
        MVG_TRY(refresh_panels(e, s, span_opens));
        ++s.uses;
        hipEvent_t stop = nullptr;
        if (span_opens) MVG_TRY(span_start(s));
        if (timed) MVG_TRY(pool_start(s, &stop));
        MVG_TRY(local_product(e, s, out));
        if (stop) MVG_HIP(hipEventRecord(stop, s.stream));
        return MVG_OK;
    });
}

int mvg_engine_sync(mvg_engine* e) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    DeviceGuard g;
    const bool span = span_is_open(e);
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        if (span && s.span_t1) MVG_HIP(hipEventRecord(s.span_t1, s.stream));
        MVG_HIP(hipStreamSynchronize(s.copy_stream));
        MVG_HIP(hipStreamSynchronize(s.stream));
        if (s.xstream) MVG_HIP(hipStreamSynchronize(s.xstream));
    }
    e->x_pending = false;
    if (span) MVG_TRY(span_close(e));
    return pool_collect(e);
}

int mvg_engine_kernel_ms(mvg_engine* e, double* avg_ms, int64_t* launches) {
    if (!e || !avg_ms) return fail(MVG_E_INVALID, "null");
    MVG_TRY(mvg_engine_sync(e));
    *avg_ms = e->kernel_launches ? e->kernel_ms_sum / (double)e->kernel_launches : 0.0;
    if (launches) *launches = e->kernel_launches;
    return MVG_OK;
}

int mvg_engine_collect(mvg_engine* e, double* y) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    Shard* root = root_shard(e);
    if (!root) return MVG_OK;
    if (!y) return fail(MVG_E_INVALID, "root needs a y buffer");
    return collect_from(e, *root, [&](Shard& s) -> int {
        MVG_HIP(hipMemcpyAsync(y, s.one.y, (size_t)e->R * sizeof(double), hipMemcpyDeviceToHost, s.stream));
        return MVG_OK;
    });
}

// ------------------------------------------------------------------ a block of vectors
// Y = A X for X = [x_0 ... x_{nv-1}] on the distributed A: per vector what distribute's x gets
// from multiply — matr_utils.c:86-96 on the shard, then rowwise.c:141, colwise.c:124 or
// blockwise.c:144-210 — with one pass over the shard and one exchange for the whole block.
namespace {

// The block's buffers on every local shard, for at least nv vectors: made by the first
// set_vectors / fill_synth_vectors and remade when nv grows. Nothing may still read the old
// ones: the shard's streams are drained first.
int make_vector_buffers(mvg_engine* e, int nv) {
    if (nv <= e->nv_cap) return MVG_OK;
    e->nv_cap = e->nv = 0;
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        MVG_HIP(hipStreamSynchronize(s.stream));
        if (s.xstream) MVG_HIP(hipStreamSynchronize(s.xstream));
        free_xbufs(s.blk);
        if (s.dX) (void)hipFree(s.dX);
        MVG_TRY(alloc_doubles(&s.dX, e->C * nv));
        // alone (no exchange) the product goes straight into Y: no ring
        MVG_TRY(alloc_xbufs(*e, s, s.blk, nv, s.nsteps > 0 ? e->ring : 0));
    }
    e->nv_cap = nv;
    return MVG_OK;
}

// set_vectors and fill_synth_vectors write dX on the GEMV stream: inside an open kernel-timing
// span that is no longer GEMVs alone.
int begin_vectors(mvg_engine* e, int nv, const char* who) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    if (nv < 1 || nv > MVG_MAX_VECTORS) return fail(MVG_E_INVALID, std::string(who) + ": nv outside 1 .. MVG_MAX_VECTORS");
    if (span_is_open(e)) e->span_valid = false;
    return MVG_OK;
}

}  // namespace

int mvg_engine_set_vectors(mvg_engine* e, const double* X, int64_t ldx, int nv) {
    MVG_TRY(begin_vectors(e, nv, "mvg_engine_set_vectors"));
    const bool root = root_shard(e) != nullptr;
    if (root && e->C > 0 && (!X || ldx < e->C)) return fail(MVG_E_INVALID, "mvg_engine_set_vectors: root needs X with ldx >= C");
    DeviceGuard g;
    MVG_TRY(make_vector_buffers(e, nv));
    for (auto& s : e->shards) {
        MVG_HIP(hipSetDevice(s.device));
        if (e->single_process) {  // every device pulls the whole X itself
            MVG_TRY(h2d_region(s.dX, X, ldx, nv, e->C, s.stream));
            continue;
        }
        // one process per GPU: the root's copy, then a broadcast on the world communicator, in
        // order behind any exchange still running on it (as the root-send distribution)
        if (e->x_pending) MVG_HIP(hipStreamWaitEvent(s.stream, last_x_done(e, s), 0));
        if (s.rank == 0) MVG_TRY(h2d_region(s.dX, X, ldx, nv, e->C, s.stream));
        if (e->C > 0) MVG_NCCL(ncclBroadcast(s.dX, s.dX, (size_t)e->C * nv, ncclFloat64, 0, s.world, s.stream));
    }
    e->nv = nv;
    return MVG_OK;
}

int mvg_engine_fill_synth_vectors(mvg_engine* e, uint64_t seed_x, int nv) {
    MVG_TRY(begin_vectors(e, nv, "mvg_engine_fill_synth_vectors"));
    DeviceGuard g;
    MVG_TRY(make_vector_buffers(e, nv));
    for (auto& s : e->shards) {  // X as nv rows of C: element (v, j) is index v * C + j
        MVG_HIP(hipSetDevice(s.device));
        MVG_TRY(mvg_synth_fill_device(s.dX, e->C, nv, e->C, 0, 0, e->C, seed_x, s.stream));
    }
    MVG_TRY(sync_gemv_streams(e));
    e->nv = nv;
    return MVG_OK;
}

int mvg_engine_vectors(const mvg_engine* e, int* nv) {
    if (!e || !nv) return fail(MVG_E_INVALID, "null");
    *nv = e->nv;
    return MVG_OK;
}

// Always on the row-major shard (never the panel copy), never timed, and no "use" of A for the
// panel copy's second-multiply rule. The block's ring shares the single vector's slot counter
// and events: one order of exchanges on the exchange stream, so the once-per-ring wait, x_pending
// and the collects' waits cover both kinds of multiply.
int mvg_engine_multiply_multi(mvg_engine* e) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    if (!e->distributed || e->nv == 0)
        return fail(MVG_E_STATE, "mvg_engine_multiply_multi needs distribute/fill and set_vectors/fill_synth_vectors first");
    DeviceGuard g;
    if (span_is_open(e)) e->span_valid = false;  // not a GEMV of the span
    const int nv = e->nv;
    return multiply_step(e, &Shard::blk, nv, [&](Shard& s, double* out) -> int {
        MVG_TRY(drain_chunks(s));  // a chunked distribution still copying: wait, then multiply whole
        if (e->exact) MVG_TRY(alloc_gathered(*e, s, s.blk, e->nv_cap, true));
        const mvg_shard& p = s.plan;
        const double* X = s.dX ? s.dX + p.col_off : nullptr;
        return e->exact ? mvg_gemv_exact_multi(s.dA, p.n_cols, X, e->C, out, p.y_len, p.n_rows, p.n_cols, nv, s.stream)
                        : mvg_gemv_multi(s.dA, p.n_cols, X, e->C, out, p.y_len, p.n_rows, p.n_cols, nv, s.stream);
    });
}

int mvg_engine_collect_multi(mvg_engine* e, double* Y, int64_t ldy) {
    if (!e) return fail(MVG_E_INVALID, "null engine");
    if (e->nv == 0) return fail(MVG_E_STATE, "mvg_engine_collect_multi before set_vectors/fill_synth_vectors");
    Shard* root = root_shard(e);
    if (!root) return MVG_OK;
    if (!Y || ldy < e->R) return fail(MVG_E_INVALID, "root needs a Y buffer with ldy >= R");
    return collect_from(e, *root, [&](Shard& s) -> int {
        MVG_HIP(hipMemcpy2DAsync(Y, (size_t)ldy * sizeof(double), s.blk.y, (size_t)e->R * sizeof(double),
                                 (size_t)e->R * sizeof(double), (size_t)e->nv, hipMemcpyDeviceToHost, s.stream));
        return MVG_OK;
    });
}

// Test hooks of the root-send staging (no device needed). The staging size that engines created
// from now on use (0: the default), and the pieces shard_pieces cuts one rank's shard into at a
// given staging size: what root_send_shards sends that rank and recv_shard receives there.
int mvg_debug_set_stage_elems(int64_t n) {
    if (n < 0) return fail(MVG_E_INVALID, "mvg_debug_set_stage_elems: negative size");
    g_stage_elems = n == 0 ? kStageElems : n;
    return MVG_OK;
}

int mvg_debug_shard_pieces(int alg, int64_t R, int64_t C, int nranks, int rank, int64_t stage_elems, int64_t* row0,
                           int64_t* rows, int64_t* count, int max, int* n) {
    if (!n || max < 0 || stage_elems < 0 || (max > 0 && (!row0 || !rows || !count)))
        return fail(MVG_E_INVALID, "mvg_debug_shard_pieces: bad arguments");
    *n = 0;
    mvg_shard p;
    MVG_TRY(mvg_plan_shard(alg, R, C, nranks, rank, &p));
    std::vector<Piece> pieces;
    MVG_TRY(shard_pieces(p, stage_elems == 0 ? kStageElems : stage_elems, &pieces));
    if ((int64_t)pieces.size() > max) return fail(MVG_E_INVALID, "mvg_debug_shard_pieces: piece buffer too small");
    for (size_t i = 0; i < pieces.size(); ++i) {
        row0[i] = pieces[i].row0;
        rows[i] = pieces[i].rows;
        count[i] = pieces[i].count;
    }
    *n = (int)pieces.size();
    return MVG_OK;
}

// The single-process G-device exchange (the executables' MVG_NGPUS=G form) without devices:
// the shards the engine would create over G local devices (the same planner, the same buffer
// choices), their communicator splits and one multiply's exchange, issued through the recorder
// instead of RCCL (exchange_buffers, split_steps, exchange: the engine's own code).
// nv = 0: one multiply's exchange out of the single vector's buffer set; nv >= 1: one
// multiply_multi's out of the block's. The stand-in addresses go into that set through XBufs::at.
static int trace_exchange(int alg, int64_t R, int64_t C, int ndev, int exact, int nv, mvg_xcall* calls, int max_calls,
                          int* ncalls) {
    if (!calls || !ncalls || ndev <= 0 || max_calls < 0 || nv < 0 || nv > MVG_MAX_VECTORS)
        return fail(MVG_E_INVALID, "mvg_debug_trace_exchange: bad arguments");
    *ncalls = 0;
    mvg_engine e;
    e.alg = alg;
    e.R = R;
    e.C = C;
    e.nranks = ndev;
    e.single_process = true;
    e.exact = exact != 0;
    e.shards.resize(ndev);
    TraceXOps ops;
    XBufs Shard::*set = nv > 0 ? &Shard::blk : &Shard::one;
    auto fake = [&](int r, int id) {
        const uintptr_t a = ((uintptr_t)(r + 1) << 44) + (uintptr_t)(id + 1) * TraceXOps::kBufSpan;
        ops.buffers.push_back({a, {r, id}});
        return (double*)a;
    };
    for (int r = 0; r < ndev; ++r) {
        Shard& s = e.shards[r];
        s.device = r;
        s.rank = r;
        s.world = (ncclComm_t)((uintptr_t)0x7d0000 + r);
        ops.comm_step.push_back({(uintptr_t)s.world, -1});
        MVG_TRY(mvg_plan_shard(alg, R, C, ndev, r, &s.plan));
        MVG_TRY(mvg_plan_exchange(alg, R, C, ndev, r, 0, s.steps, MVG_MAX_XSTEPS, &s.nsteps));
        const XBufLens xb = exchange_buffers(e, s, e.exact);
        for (int id = 0; id < 4; ++id)
            if (xb.len[id] >= 0) (s.*set).at(id, 0) = fake(r, id);
    }
    MVG_TRY(split_steps(e.shards, ops));
    if (e.shards[0].nsteps > 0) MVG_TRY(exchange(&e, set, 0, std::max(nv, 1), false, ops));
    if ((int)ops.calls.size() > max_calls) return fail(MVG_E_INVALID, "mvg_debug_trace_exchange: calls buffer too small");
    for (size_t i = 0; i < ops.calls.size(); ++i) calls[i] = ops.calls[i];
    *ncalls = (int)ops.calls.size();
    return MVG_OK;
}

int mvg_debug_trace_exchange(int alg, int64_t R, int64_t C, int ndev, int exact, mvg_xcall* calls, int max_calls,
                             int* ncalls) {
    return trace_exchange(alg, R, C, ndev, exact, 0, calls, max_calls, ncalls);
}

int mvg_debug_trace_exchange_multi(int alg, int64_t R, int64_t C, int ndev, int exact, int nv, mvg_xcall* calls,
                                   int max_calls, int* ncalls) {
    if (nv < 1) return fail(MVG_E_INVALID, "mvg_debug_trace_exchange_multi: nv outside 1 .. MVG_MAX_VECTORS");
    return trace_exchange(alg, R, C, ndev, exact, nv, calls, max_calls, ncalls);
}

}  // extern "C"
