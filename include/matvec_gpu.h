/*
 * matvec_gpu.h — C-ABI of libmatvec_gpu.so, the MI355X (gfx950) replacement for the
 * compute + communication core of yaroslav-i-am/MatVec_MPI_Multiplier.
 *
 * Plain C types only (pointers, int64_t sizes, int return codes). No torch, no HIP
 * types in any signature: streams are passed as `void*` (a hipStream_t, NULL = the
 * library's own stream for that device).
 *
 * Every function returns MVG_OK (0) on success or a negative MVG_E* code; the text of
 * the last failure on the calling thread is available from mvg_last_error().
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   mvg_gemv                 <- multiply_std_rowwise          src/matr_utils.c:86-96
 *                               (also the strip GEMV that multiply_colwise computes as
 *                                scale-then-row-sum,          src/multiplier_colwise.c:105-122)
 *   mvg_gemv_exact           <- the same, bit for bit (the reference's sequential sum)
 *   mvg_multiply_std_rowwise <- multiply_std_rowwise itself on host pointers (matr_utils.h:4-10)
 *   mvg_grid_shape           <- get_2_most_closest_multipliers src/utils.c:26-37
 *   mvg_plan_shard           <- local_n / local_n_rows / local_n_cols arithmetic
 *                               src/multiplier_rowwise.c:93, src/multiplier_colwise.c:349,
 *                               src/multiplier_blockwise.c:299-306 (+ divisibility checks
 *                               rowwise.c:72-75, colwise.c:151-154, blockwise.c:277-281)
 *   mvg_engine_distribute    <- distribute_data (Scatter/Bcast | Type_vector+Pack+Send |
 *                               block Pack+Send)  rowwise.c:12-51, colwise.c:11-102,
 *                               blockwise.c:17-141
 *   mvg_engine_multiply      <- local multiply + MPI_Gather / MPI_Reduce(SUM) /
 *                               gather_local_results
 *                               rowwise.c:140-141, colwise.c:105-129, blockwise.c:144-210,367-368
 *   mvg_engine_collect       <- root owning `result` after the timed region (the reference
 *                               never writes y; this is the opt-in y hand-back)
 *   mvg_load_matr / mvg_load_vec <- load_matr / load_vec       src/matr_utils.c:42-83
 *   mvg_comm_*               <- MPI_Init/Comm_size/Comm_rank/Finalize + the collectives
 *                               (RCCL over xGMI instead of MPI)
 */
#ifndef MATVEC_GPU_H
#define MATVEC_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
#define MVG_OK              0
#define MVG_E_INVALID      -1   /* bad argument (null pointer, negative size, ...)   */
#define MVG_E_INDIVISIBLE  -2   /* shape does not split over the rank count          */
#define MVG_E_HIP          -3   /* HIP runtime failure                                */
#define MVG_E_RCCL         -4   /* RCCL failure                                       */
#define MVG_E_IO           -5   /* file missing / unreadable                          */
#define MVG_E_NOMEM        -6   /* host or device allocation failed                   */
#define MVG_E_STATE        -7   /* call out of order (e.g. multiply before distribute)*/

/* ------------------------------------------------------------------ algorithms   */
#define MVG_ALG_ROWWISE    0    /* src/multiplier_rowwise.c   */
#define MVG_ALG_COLWISE    1    /* src/multiplier_colwise.c   */
#define MVG_ALG_BLOCKWISE  2    /* src/multiplier_blockwise.c */

const char* mvg_version(void);
const char* mvg_strerror(int code);
const char* mvg_last_error(void);

/* The runtimes this library is bound to in the calling process (no counterpart in the
 * reference, whose MPI is fixed at build time). The library needs libamdhip64.so.7 and
 * librccl.so.1 by soname, so a process that loaded another copy first (PyTorch's ROCm wheel
 * bundles its own HIP and RCCL) runs the library on that copy. mvg_runtime_versions: RCCL's
 * ncclGetVersion code (e.g. 22705 = 2.27.5) and HIP's hipRuntimeGetVersion; either pointer may
 * be NULL. mvg_runtime_path: the file the bound copy was loaded from (which: 0 = the HIP
 * runtime, 1 = RCCL), "" when unknown. Neither call runs anything on a device (asking for the
 * HIP version may start the HIP runtime; mvg_runtime_path and the RCCL version do not). */
int mvg_runtime_versions(int* rccl_version, int* hip_runtime_version);
const char* mvg_runtime_path(int which);

/* ------------------------------------------------------------------ planner (host only, no GPU)
 * get_2_most_closest_multipliers (src/utils.c:26-37): rows = largest d <= floor(sqrt(p))
 * with p % d == 0, cols = p / d.  p <= 0 -> MVG_E_INVALID. */
int mvg_grid_shape(int64_t p, int* grid_rows, int* grid_cols);

/* The slice of the global R x C problem that rank `rank` of `nranks` owns.
 * row_off/col_off/n_rows/n_cols: the block of A (and col_off/n_cols: the x segment);
 * y_off/y_len: the slice of y its partial result contributes to.
 * grid_r/grid_c: rank's coordinate in the grid (row-split: (rank,0), col-split: (0,rank)).
 * Returns MVG_E_INDIVISIBLE exactly where the reference prints "ERROR!!!", and also
 * (deliberate deviation) where the reference would silently compute a
 * wrong y: block-split with R % r != 0 or C % c != 0. */
typedef struct mvg_shard {
    int     alg, nranks, rank;
    int     grid_rows, grid_cols, grid_r, grid_c;
    int64_t R, C;
    int64_t row_off, col_off, n_rows, n_cols;
    int64_t y_off, y_len;
} mvg_shard;
int mvg_plan_shard(int alg, int64_t R, int64_t C, int nranks, int rank, mvg_shard* out);

/* The exchange step after the local product, as the collective schedule rank `rank` runs
 * (the engine drives RCCL from exactly this plan; tests replay it over gloo).
 *   row  : GATHER(world, count = R/P, PART -> Y)                    rowwise.c:141
 *   col  : REDUCE(world, count = R, PART -> Y)                       colwise.c:124
 *   block: REDUCE(row comm: color grid_r, key grid_c; count = R/r, PART -> ROW on the leader),
 *          GATHER(col comm: the grid-column-0 leaders, key grid_r; ROW -> Y)  blockwise.c:144-210
 *          (one grid row: a single REDUCE straight into Y).
 * P == 1 has no steps (the product is written straight into Y) unless force_collect != 0.
 * A communicator is identified by (comm kind, color); ranks order by key; root is the rank
 * within that communicator (always 0, i.e. world rank 0 / the grid-row leader). */
#define MVG_X_GATHER    0
#define MVG_X_REDUCE    1
#define MVG_X_WORLD     0
#define MVG_X_ROW       1
#define MVG_X_COL       2
#define MVG_X_BUF_PART  0   /* the local product (y_len doubles; R for column split) */
#define MVG_X_BUF_ROW   1   /* the grid-row sum on the row leader (y_len doubles)       */
#define MVG_X_BUF_Y     2   /* the full y on world rank 0 (R doubles)                   */
typedef struct mvg_xstep {
    int     op, comm, color, key, member, root, src, dst;
    int64_t count;
} mvg_xstep;
#define MVG_MAX_XSTEPS 4
int mvg_plan_exchange(int alg, int64_t R, int64_t C, int nranks, int rank, int force_collect,
                      mvg_xstep* steps, int max_steps, int* nsteps);

/* The exchange after a local transposed product (mvg_gemv_t on each rank's shard): the mirror image of
 * the schedule above on the same shards (mvg_plan_shard, the same divisibility refusals). The
 * partial has n_cols doubles, the result C doubles on rank 0:
 *   row  : REDUCE(world, count = C, PART -> Y)
 *   col  : GATHER(world, count = C/P, key rank, PART -> Y)
 *   block: REDUCE(comm MVG_X_COL: color grid_c, key grid_r, every rank a member; count = C/c,
 *                 PART -> ROW on the grid_r == 0 leader),
 *          GATHER(comm MVG_X_ROW: color 0, key grid_c, the grid-row-0 leaders; ROW -> Y)
 *          (one grid row: a single GATHER(world, PART -> Y)).
 * P == 1 has no steps unless force_collect != 0. */
int mvg_plan_exchange_t(int alg, int64_t R, int64_t C, int nranks, int rank, int force_collect,
                        mvg_xstep* steps, int max_steps, int* nsteps);

/* Test hook: the calls one process driving `ndev` devices issues (the executables'
 * MVG_NGPUS=G form: ncclCommSplit of the schedule's sub-communicators, then one multiply's
 * exchange), produced by the engine's own exchange code with a recorder in place of RCCL, so no
 * device is needed. `exact` != 0: exact mode's exchange (rank-order gather to rank 0 + the
 * combine kernel there). Calls are listed in issue order; `group` numbers the
 * ncclGroupStart/End bracket each was issued in (-1: outside any, the combine kernel); `comm`
 * is -1 for the world communicator, else the group whose split created it;
 * color -1 = NCCL_SPLIT_NOCOLOR; src/dst are MVG_X_BUF_*
 * (MVG_X_BUF_GATHERED: rank 0's gather buffer in exact mode), -1 where the call has none.
 * Reference interface it stands for: multiplier_blockwise.c:144-210 (gather_local_results),
 * multiplier_colwise.c:124, multiplier_rowwise.c:141. */
#define MVG_XCALL_SPLIT   0
#define MVG_XCALL_GATHER  1
#define MVG_XCALL_REDUCE  2
#define MVG_XCALL_COMBINE 3
#define MVG_X_BUF_GATHERED 3
typedef struct mvg_xcall {
    int     group, kind, rank, comm, color, key, root, src, dst;
    int64_t count;
} mvg_xcall;
int mvg_debug_trace_exchange(int alg, int64_t R, int64_t C, int ndev, int exact, mvg_xcall* calls, int max_calls,
                             int* ncalls);
/* The same for one mvg_engine_multiply_multi over a block of nv vectors (1 .. MVG_MAX_VECTORS):
 * one group per step as above; a reduce is one call of count * nv doubles (the block's buffers
 * are column-major, one vector per column), a gather nv calls of count doubles per member, vector
 * v in call v of the member (into column v of the root's Y); exact mode: nv rank-order gathers per
 * rank in one group, then nv combines on rank 0 (blockwise.c:144-210 / colwise.c:124 per vector;
 * rowwise.c:141's gather is exact as it is). */
int mvg_debug_trace_exchange_multi(int alg, int64_t R, int64_t C, int ndev, int exact, int nv, mvg_xcall* calls,
                                   int max_calls, int* ncalls);

/* ------------------------------------------------------------------ synthetic inputs
 * value(seed, idx) = (double)k / 10000.0, k = floor(splitmix64(s0 + idx*gamma) * 10000 / 2^64),
 * s0 = splitmix64(seed), gamma = 0x9E3779B97F4A7C15. Every value is exactly what "%.4f" text
 * of it parses back to (the reference's data format, README.md:32), so synthetic and text
 * inputs are interchangeable bit for bit. A uses idx = i*C + j of the GLOBAL matrix; x uses
 * its own seed.  The device fill writes a shard [row_off, +m) x [col_off, +k) of a global
 * R x C matrix (n_cols_global = C) into dst with leading dimension ld. */
#define MVG_SEED_A 42u
#define MVG_SEED_X 4242u
double mvg_synth_value(uint64_t seed, uint64_t idx);
int    mvg_synth_fill_host(double* dst, int64_t ld, int64_t m, int64_t k,
                           int64_t row_off, int64_t col_off, int64_t n_cols_global, uint64_t seed);
int    mvg_synth_fill_device(double* d_dst, int64_t ld, int64_t m, int64_t k,
                             int64_t row_off, int64_t col_off, int64_t n_cols_global,
                             uint64_t seed, void* stream);

/* ------------------------------------------------------------------ device helpers */
int mvg_device_count(int* n);
int mvg_set_device(int dev);
int mvg_malloc(void** dptr, size_t bytes);
int mvg_free(void* dptr);
int mvg_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int mvg_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int mvg_stream_sync(void* stream);
int mvg_host_register(void* ptr, size_t bytes);     /* pin caller-owned host memory */
int mvg_host_unregister(void* ptr);
/* NUMA node of GPU `device` (from its PCI address; -1 when unknown). */
int mvg_device_numa_node(int device, int* node);
/* Zero [ptr, ptr + bytes) from threads bound to the CPUs of GPU `device`'s NUMA node, so the
 * pages land in that socket's DRAM (first-touch placement of host memory the GPU will pull
 * from; the executables' shared window). Falls back to the caller's CPUs. */
int mvg_host_first_touch(void* ptr, size_t bytes, int device);

/* ------------------------------------------------------------------ the hot kernel
 * y[i] = sum_j A[i*lda + j] * x[j], i < m, j < k (fp64, row-major, lda >= k).
 * Device pointers; asynchronous on `stream`. Results match the reference's sequential
 * left-to-right sum (src/matr_utils.c:87-93) to <= 1e-12 relative per element for
 * non-negative data (different, fixed, run-to-run deterministic summation order).
 * m == 0 or k == 0 is valid (k == 0 writes zeros, as the reference's `sum = 0`). */
int mvg_gemv(const double* d_A, int64_t lda, const double* d_x, double* d_y,
             int64_t m, int64_t k, void* stream);

/* Same, with an explicit kernel variant (benchmarks / tests):
 *   0 = auto (shape-adaptive), 1.. = the table in csrc/gemv.hip (names via
 *   mvg_gemv_variant_name: vec_* wave-owns-rows, rowblk_* row-per-workgroup, scl_* 8-B loads). */
int mvg_gemv_variant(const double* d_A, int64_t lda, const double* d_x, double* d_y,
                     int64_t m, int64_t k, int variant, void* stream);
int mvg_gemv_variant_count(void);
/* the variant mvg_gemv picks for a 16-B-aligned A, x with this lda, m and k */
int mvg_gemv_auto_variant(int64_t lda, int64_t m, int64_t k);
const char* mvg_gemv_variant_name(int variant);

/* Several x per pass over A (beyond the reference's surface):
 * Y[:, v] = A X[:, v] for v < nv, X k x nv and Y m x nv column-major (vector v at X + v*ldx,
 * Y + v*ldy; ldx >= k, ldy >= m). A is streamed once per group of 8 vectors (16 from 8192 rows
 * of >= 1024 columns, on the matrix cores), so the HBM cost
 * of nv products approaches that of one. Same numerics contract as mvg_gemv. */
int mvg_gemv_multi(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_Y,
                   int64_t ldy, int64_t m, int64_t k, int nv, void* stream);
/* mvg_gemv_multi with an explicit kernel variant (0 = automatic; tests and sweeps). A variant
 * needs 16-B aligned A and X, even lda and ldx and k > 0; the LDS-DMA forms (mdma_r<RQ>_*,
 * m16_r<RQ>_*: 16*RQ rows per workgroup) also 16*RQ * lda * 8 < 2^31 and nvec * ldx * 8 < 2^31
 * (nvec 8, 16 for m16_*): MVG_E_INVALID otherwise, decided from the arguments alone. */
int mvg_gemv_multi_variant(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_Y,
                           int64_t ldy, int64_t m, int64_t k, int nv, int variant, void* stream);
int mvg_gemv_multi_variant_count(void);
/* the variant mvg_gemv_multi picks for the first group of nv >= 2 vectors (16-B aligned A and X,
 * even lda and ldx): up to 16 vectors per pass on long enough shapes, else up to 8; 0 for nv < 2
 * (the single-vector dispatch) */
int mvg_gemv_multi_auto_variant(int64_t lda, int64_t ldx, int64_t m, int64_t k, int nv);
const char* mvg_gemv_multi_variant_name(int variant);

/* Bit-exact form of mvg_gemv: every row is the reference's own chain
 *   sum = 0; for j < k: sum = round(sum + round(A[i*lda + j] * x[j]))
 * (src/matr_utils.c:87-93: a rounded multiply then a rounded add, left to right, no FMA), so
 * y is bit-identical to multiply_std_rowwise on the same inputs (and to the strip sums of
 * multiply_colwise, src/multiplier_colwise.c:107-122). Tall shapes whose rows start on 128-B
 * lines: one lane per row, rows streamed through LDS; everything else: several lanes per row,
 * the running sum handed lane to lane in column order (csrc/gemv_exact.hip). Any lda >= k and
 * any alignment. */
int mvg_gemv_exact(const double* d_A, int64_t lda, const double* d_x, double* d_y,
                   int64_t m, int64_t k, void* stream);
/* The reference's in-process call on host pointers, src/matr_utils.h:4-10:
 *   void multiply_std_rowwise(double* matrix, double* vector, long n_rows, long n_cols, double* result);
 * row-major matrix (n_rows x n_cols), vector (n_cols), result (n_rows), all caller-owned host
 * memory, on the calling thread's current device: copies A and x over, runs mvg_gemv_exact
 * (exact != 0: result bit-identical to the reference's) or mvg_gemv (exact == 0: within 1e-12),
 * copies y back and waits. Device buffers are kept per thread and grown as needed; all-zero /
 * null arguments release them. */
int mvg_multiply_std_rowwise(const double* matrix, const double* vector, int64_t n_rows, int64_t n_cols,
                             double* result, int exact);
/* explicit exact variant (0 = auto; names via mvg_gemv_exact_variant_name: seq_r<RW>_t<T>_b<NB>
 * and seqx_* RW-row LDS-DMA tiles of 2T columns with NB buffers, hop_l<L>_w<W>_u<U> L lanes per
 * row holding W columns each with U segments in flight, hop8_* the same with 8-B loads (any
 * alignment, any lda), seq_scalar a lane per row with 8-B loads). A variant whose operand rules the
 * call breaks (seq_*, seqx_*, hop_*: 16-B aligned A and x, even lda; seq_*, seqx_*: lda < 2^23;
 * hopxl_*: k <= 8192) is MVG_E_INVALID, decided from the arguments alone. */
int mvg_gemv_exact_variant(const double* d_A, int64_t lda, const double* d_x, double* d_y,
                           int64_t m, int64_t k, int variant, void* stream);
int mvg_gemv_exact_variant_count(void);
int mvg_gemv_exact_auto_variant(int64_t lda, int64_t m, int64_t k);
const char* mvg_gemv_exact_variant_name(int variant);
/* Bit-exact form of mvg_gemv_multi (same layout and argument rules: vector v at d_X + v*ldx and
 * d_Y + v*ldy, ldx >= k, ldy >= m, any nv >= 0; m == 0 or nv == 0 is a no-op, k == 0 writes
 * zeros): column v of Y is bit-identical to mvg_gemv_exact on x_v, i.e. to multiply_std_rowwise
 * (src/matr_utils.c:86-96) per vector. The multi kernels carry 2 or 4 independent chains per
 * row over one read of A (csrc/gemv_exact.hip, gemv_seq_hop_multi); the vectors go out in groups
 * of the variant's chain count, a last single vector through mvg_gemv_exact. Any lda, ldx and
 * alignment. The automatic choice takes a multi kernel only where a committed sweep showed it
 * faster than separate passes, and separate mvg_gemv_exact passes everywhere else. */
int mvg_gemv_exact_multi(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_Y, int64_t ldy,
                         int64_t m, int64_t k, int nv, void* stream);
/* explicit variant (0 = auto; names via mvg_gemv_exact_multi_variant_name: "separate" = one
 * mvg_gemv_exact per vector, hopm_l<L>_w<W>_u<U>_v<NV> = NV chains per row, L lanes per row
 * holding W columns each, U segments in flight) */
int mvg_gemv_exact_multi_variant(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_Y,
                                 int64_t ldy, int64_t m, int64_t k, int nv, int variant, void* stream);
int mvg_gemv_exact_multi_variant_count(void);
/* the variant mvg_gemv_exact_multi picks for nv >= 2 vectors; 0 for nv < 2 (mvg_gemv_exact) */
int mvg_gemv_exact_multi_auto_variant(int64_t lda, int64_t ldx, int64_t m, int64_t k, int nv);
const char* mvg_gemv_exact_multi_variant_name(int variant);
/* Test hooks of the exact dispatch (no counterpart in the reference). mvg_debug_set_cu_count:
 * the CU count the dispatch plans whole rounds of workgroups for (0 = the current device's).
 * mvg_debug_set_exact_even_lds: the LDS reservation of the evenly placed form in bytes (0 = its
 * own 96 KiB); above the CU's 160 KiB the runtime refuses the launch, which drives the fallback
 * to the one-wave form (same sums); it also forgets earlier refusals. */
int mvg_debug_set_cu_count(int n);
int mvg_debug_set_exact_even_lds(int64_t bytes);
/* 1 when the runtime has refused the evenly placed exact form's LDS on `device` in this process
 * (a request above the device's per-workgroup LDS, confirmed against
 * hipDeviceAttributeMaxSharedMemoryPerBlock, logged once on stderr): the auto dispatch there
 * then runs the one-wave forms. 0 otherwise; MVG_E_INVALID for a device index outside 0..63. */
int mvg_gemv_exact_even_refused(int device);
/* Test hooks: exact mode's combine kernels on their own, as the engine launches them on rank 0
 * after the gather of the partials (device pointers, asynchronous on `stream`).
 * mvg_debug_combine_mpich: d_parts[r*n + i] = rank r's partial y (P ranks of n doubles); d_y[i] =
 * their sum in the order MPICH 3.3.2's MPI_Reduce adds them (colwise.c:124). d_parts is
 * overwritten. mvg_debug_combine_grid_rows: d_parts[r*lr + j] = rank r's partial on a gr x gc
 * grid; d_y[g*lr + j] = ((0 + p[g*gc]) + p[g*gc + 1]) + ... (blockwise.c:150-207). */
int mvg_debug_combine_mpich(double* d_parts, int P, int64_t n, double* d_y, void* stream);
int mvg_debug_combine_grid_rows(const double* d_parts, int gr, int gc, int64_t lr, double* d_y, void* stream);

/* The same bit-exact product over A in column panels (the engine's device layout in exact mode,
 * DESIGN §4b): panel p holds columns [p*P, p*P + P) of all m rows, row i of it at
 * d_Ap + p*pstride + i*P (pstride >= m*P doubles; the last panel may be narrower than P and is
 * padded to P). Same sums in the same order as mvg_gemv_exact (multiply_std_rowwise,
 * src/matr_utils.c:86-96), so y is the same bit for bit; streaming the rows panel by panel reads
 * one contiguous region at a time instead of m scattered ones. P a power of two, a multiple of
 * 16 (32 for panel_l16_*); d_Ap and d_x 16-B aligned. variant 0 = auto (names:
 * mvg_gemv_exact_panel_variant_name, panel_l<L>_w<W>_u<U> as the hop forms). */
int mvg_gemv_exact_panels(const double* d_Ap, int64_t pstride, int64_t P, const double* d_x, double* d_y,
                          int64_t m, int64_t k, int variant, void* stream);
/* Rows [0, m) of a row-major A (lda) into rows [0, m) of the panel layout above (device to
 * device, HBM-bound; any lda and alignment). Row ranges map onto row ranges: offset d_A by
 * r0*lda and d_Ap by r0*P, keep pstride. */
int mvg_panel_relayout(const double* d_A, int64_t lda, int64_t m, int64_t k, double* d_Ap, int64_t pstride,
                       int64_t P, void* stream);
/* P the engine uses for an m x k shard in exact mode (0: it keeps the row-major kernels). */
int64_t mvg_exact_panel_width(int64_t m, int64_t k);
int mvg_gemv_exact_panel_variant_count(void);
int mvg_gemv_exact_panel_auto_variant(int64_t m, int64_t k);
const char* mvg_gemv_exact_panel_variant_name(int variant);

/* The transposed product on the same row-major A (beyond the reference, whose drivers only form
 * A x; least squares, power iteration on A^T A and bidiagonalisation need both on one copy of A):
 *   y[j] = sum_i A[i*lda + j] * z[i],  j < k, i < m   (lda >= k; z has m entries, y has k).
 * Device pointers; asynchronous on `stream`. A is streamed once (csrc/gemv_t.hip): a workgroup
 * sums a band of rows over a strip of columns, a lane per column, and a second kernel adds the
 * bands out of the per-(device, stream) workspace mvg_gemv's split-K form also uses. Same accuracy
 * contract as mvg_gemv: within 1e-12 relative per element of the sequential sum over i (what
 * multiply_std_rowwise, src/matr_utils.c:86-96, gives on a transposed copy) on non-negative data.
 * No atomics: FMAs in a fixed per-lane order, waves added in wave order, bands in band order
 * within 16 runs of consecutive bands and the runs in run order, so y is the same bits from run to
 * run whatever the workspace held. m == 0 writes k zeros, k == 0 is a no-op. Any lda >= k and any
 * 8-byte alignment of A, z, y; nothing is read outside A[i, 0..k) and z[0..m) or stored outside
 * y[0..k); a special value in column j of A reaches y[j] alone. */
int mvg_gemv_t(const double* d_A, int64_t lda, const double* d_z, double* d_y, int64_t m, int64_t k, void* stream);
/* explicit kernel variant (0 = auto; names via mvg_gemv_t_variant_name:
 * strip_w<NW>_c<CPL>_u<UNR>_b<cap>: NW waves per workgroup, CPL columns per lane in 16-B loads,
 * UNR rows in flight, bands of at most <cap> rows (256 unless named); scalar_*: the same with 8-B
 * loads, a lane per column, which the automatic choice takes at any lda and alignment: they were
 * the faster forms wherever swept). A launch is one grid of
 * bands x strips workgroups; bands grow until it fits gridDim.x * blockDim.x < 2^32, and a k with
 * more strips than one grid holds (2^31 / workgroup size of them) is MVG_E_INVALID, decided from the arguments alone
 * before any HIP call. */
int mvg_gemv_t_variant(const double* d_A, int64_t lda, const double* d_z, double* d_y, int64_t m, int64_t k,
                       int variant, void* stream);
int mvg_gemv_t_variant_count(void);
/* the variant mvg_gemv_t picks for this lda, m and k (the pointers' alignment plays no part) */
int mvg_gemv_t_auto_variant(int64_t lda, int64_t m, int64_t k);
const char* mvg_gemv_t_variant_name(int variant);
/* host only, decided from the arguments alone: how `variant` (0 = auto) cuts the problem into
 * `bands` bands of `band_rows` rows (the last one shorter) and strips of `strip_cols` columns.
 * One band: the sums go straight into y; more: 8 * bands * k bytes of workspace. */
int mvg_gemv_t_plan(int64_t lda, int64_t m, int64_t k, int variant, int64_t* band_rows, int64_t* bands,
                    int64_t* strip_cols);

/* The transposed product for a block of vectors (what subspace iteration, block Lanczos and
 * randomized range finders need beside mvg_gemv_multi), mvg_gemv_multi's layout mirrored:
 *   Y[j + v*ldy] = sum_i A[i*lda + j] * Z[i + v*ldz],  j < k, i < m, v < nv
 * A row-major m x k (lda >= k), Z m x nv column-major (vector v at d_Z + v*ldz, ldz >= m), Y k x nv
 * column-major (vector v at d_Y + v*ldy, ldy >= k). Device pointers; asynchronous on `stream`; the
 * band partials live in the per-(device, stream) workspace. The fused variants (csrc/gemv_t_multi.hip)
 * send the vectors out in groups of the variant's chain count NV and stream A once per group: a
 * workgroup sums a band of rows over a strip of columns, a lane per column with NV sums, row i's NV
 * values of Z read as wave-uniform scalars; a second kernel adds the bands of the whole group. The
 * last group may be shorter than NV (it runs the same kernel; its spare chains read the group's last
 * vector again and are never stored); a single leftover vector goes through mvg_gemv_t.
 * Accuracy: mvg_gemv_t's contract per column (within 1e-12 relative per element of the sequential
 * sum over i on non-negative data). With `separate`, and for the single leftover vector of a fused
 * variant, column v is bit-identical to mvg_gemv_t on z_v. A column that a fused group computes has
 * bits that depend on A, z_v, the variant, m and k alone: not on the other vectors' values, on nv or
 * the column's place in its group, or on what the workspace held. No atomics; deterministic from
 * run to run.
 * Any 8-byte alignment of A, Z and Y and any lda >= k, ldz >= m, ldy >= k; row and vector offsets
 * are 64-bit; nothing is read outside A[i, 0..k) and Z[0..m, v) or stored outside Y[0..k, v),
 * v < nv: the gaps between columns (ldy > k) and past the last column are not touched. No two
 * operands may overlap. A special value in A[i, j] reaches row j of Y only, one in Z[i, v] column v
 * of Y only. m == 0 writes k zeros into each of the nv columns; k == 0 or nv == 0 is a no-op, also
 * on null pointers. There is no upper limit on nv. MVG_E_INVALID, decided from the arguments alone
 * before any HIP call (messages start "mvg_gemv_t_multi"): a negative size or nv, lda < k, ldz < m
 * or ldy < k, a null pointer where data would be touched, a variant out of range, more column
 * strips than one grid holds (2^31 / workgroup size of them; mvg_gemv_t's own limit where a vector
 * goes through it). */
int mvg_gemv_t_multi(const double* d_A, int64_t lda, const double* d_Z, int64_t ldz, double* d_Y, int64_t ldy,
                     int64_t m, int64_t k, int nv, void* stream);
/* explicit variant (0 = auto; names via mvg_gemv_t_multi_variant_name):
 *   1 = separate: one mvg_gemv_t per vector on `stream`; defines the result for every shape;
 *   tstripm_w<NW>_c<CPL>_u<UNR>_v<NV>: NV chains per column, NW waves per workgroup, strips of
 *       64 * CPL columns (8-B loads, a lane per 64-column stride), UNR consecutive rows per wave
 *       and step.
 * The automatic choice takes a fused variant only for a class of (m, k, nv) where a committed sweep
 * showed it more than 2 % faster than separate in every kept run: m >= 16384, k >= 64 and
 * m * k >= 2^28, the range that was swept. It chooses group by group, a variant with no more chains
 * than vectors are left (16, then 8, from 128 columns on, then 4 and 2), so every
 * group it launches is a full one and a last single vector goes through mvg_gemv_t; a column's
 * bits are those of its group's variant. Everything else takes separate. The fused variants stay
 * callable by number. */
int mvg_gemv_t_multi_variant(const double* d_A, int64_t lda, const double* d_Z, int64_t ldz, double* d_Y,
                             int64_t ldy, int64_t m, int64_t k, int nv, int variant, void* stream);
int mvg_gemv_t_multi_variant_count(void);
/* the variant mvg_gemv_t_multi picks for these sizes (the pointers' alignment plays no part) */
int mvg_gemv_t_multi_auto_variant(int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv);
const char* mvg_gemv_t_multi_variant_name(int variant);
/* host only, decided from the arguments alone: the first group that `variant` (0 = auto) cuts
 * from nv vectors. *group is its vector count: min(nv, NV) for a fused variant while at least two
 * vectors are left, else 1 (0 for nv == 0); auto: the group of the variant that
 * mvg_gemv_t_multi_auto_variant names for nv; band_rows, bands and strip_cols describe that group's
 * launch (bands * band_rows >= m > (bands - 1) * band_rows). A fused variant's bands are
 * 128 * NV rows, so that the partials' traffic 16 * bands * k * NV stays within 2 % of A's
 * 8 * m * k, shrink (down to 32 rows) until the grid has 512 workgroups and grow until
 * gridDim.x * blockDim.x < 2^32; they do not depend on nv. separate, and a fused variant with one
 * vector left, report what mvg_gemv_t_plan reports, with group = 1. Walk a call group by group by
 * asking again with nv - *group. */
int mvg_gemv_t_multi_plan(int64_t lda, int64_t m, int64_t k, int nv, int variant, int64_t* band_rows,
                          int64_t* bands, int64_t* strip_cols, int* group);

/* The bit-exact transposed product: y = A^T z on the row-major A (m x k, lda >= k) with the bits of
 * the reference's sequential rounded sum,
 *   y[j]: sum = +0.0; for i = 0 .. m-1: sum = round(sum + round(A[i*lda + j] * z[i]))
 * the multiply and the add each rounded (no FMA), rows strictly in order: what multiply_std_rowwise
 * (src/matr_utils.c:86-96) gives on a contiguous transposed copy of A. mvg_gemv_t promises that sum
 * to 1e-12 with bits that depend on variant, band cut and shape; here y is the same bits for every
 * variant, every shape, every lda, every 8-byte alignment and every run, so a transposed result can
 * be compared with array_equal against a CPU run. mvg_gemv_exact followed by mvg_gemv_t_exact is
 * the exact form of the A^T A pair (there is no fused exact mvg_gemv_ata, and the engine does not
 * run transposed products).
 * Device pointers; asynchronous on `stream`; no workspace. A chain cannot be cut into bands, so a
 * workgroup owns a strip of columns over all m rows and a lane that owns a column carries its
 * chain (csrc/gemv_t_exact.hip): the time is at least max(8*m*k / HBM rate, m chain steps).
 * Nothing is read outside A[i, 0..k) and z[0..m), nothing is stored outside y[0..k); row offsets
 * are 64-bit. m == 0 writes k values of +0.0; k == 0 is a no-op, also on null pointers. A special
 * value in A[i, j] reaches y[j] alone; one in z[i] reaches every column, as the chain itself has it
 * (0 * Inf = NaN in every column; signed zeros as the adds give them, +0.0 + -0.0 = +0.0).
 * MVG_E_INVALID, decided from the arguments alone before any HIP call (messages start
 * "mvg_gemv_t_exact"): a negative size, lda < k, a null pointer where data would be touched, a
 * variant out of range, an explicit staged variant whose operand rules the call breaks, more column
 * strips than one grid holds (2^31 / workgroup size of them). */
int mvg_gemv_t_exact(const double* d_A, int64_t lda, const double* d_z, double* d_y, int64_t m, int64_t k,
                     void* stream);
/* explicit kernel variant (0 = auto; names via mvg_gemv_t_exact_variant_name):
 *   1 = tseq_c64_u16, the direct form that defines the result: any lda, any 8-byte alignment;
 *   tseq_c<SC>_u<U>: direct forms, a lane per column of a strip of SC columns, U rows of 8-byte
 *       loads in flight in registers;
 *   tseqx_w<NW>_c<SC>_t<T>_b<NB>: staged forms, NW waves fetch tiles of T rows x SC columns into a
 *       ring of NB LDS buffers by LDS-DMA while SC chain lanes sum the tile before; they need A and
 *       z 16-byte aligned, an even lda and lda < 2^29 / T (32-bit per-lane offsets over a tile's
 *       rows), and are MVG_E_INVALID by number otherwise. The k % SC columns of a strip cut by k
 *       go through variant 1 in a second launch on `stream`.
 * The automatic choice takes another form than variant 1 only for a class of shapes where both
 * kept sweep runs showed it more than 2 % ahead (m >= 16384, 64 <= k <= 32768, 2^28 <= m * k <= 2^31:
 * a staged form by the width of k), and variant 1 wherever that form's operand rules are broken;
 * every variant gives the same bits. */
int mvg_gemv_t_exact_variant(const double* d_A, int64_t lda, const double* d_z, double* d_y, int64_t m, int64_t k,
                             int variant, void* stream);
int mvg_gemv_t_exact_variant_count(void);
/* the variant mvg_gemv_t_exact picks for this lda, m and k on 16-byte aligned operands (operands
 * 8 bytes off take variant 1 wherever this names a staged form) */
int mvg_gemv_t_exact_auto_variant(int64_t lda, int64_t m, int64_t k);
const char* mvg_gemv_t_exact_variant_name(int variant);
/* host only: the variant mvg_gemv_t_exact runs for these operands, their alignment included: the
 * pick of mvg_gemv_t_exact_auto_variant, or 1 where d_A, d_z or lda break that pick's rules */
int mvg_gemv_t_exact_resolve_variant(const double* d_A, int64_t lda, const double* d_z, int64_t m, int64_t k);
/* test hook: min_rows and min_size (m * k) stand in for the lower bounds of the swept range of the
 * automatic choices of mvg_gemv_t_exact and mvg_gemv_t_exact_multi, so that a small problem takes
 * the picks; 0 restores a bound */
int mvg_debug_set_gemv_t_exact_swept(int64_t min_rows, int64_t min_size);

/* The bit-exact transposed product for a block of vectors, in mvg_gemv_t_multi's layout and with
 * its argument rules: A row-major m x k (lda >= k), Z m x nv column-major (vector v at d_Z + v*ldz,
 * ldz >= m), Y k x nv column-major (vector v at d_Y + v*ldy, ldy >= k). Column v of Y is
 * bit-identical to mvg_gemv_t_exact on z_v, whatever nv, the group and the other vectors are. The
 * fused variants carry NV independent chains per column over one read of A and send the vectors
 * out in groups of NV; a last group shorter than NV runs the same kernel (its spare chains read the
 * group's last vector again and are never stored), a last single vector goes through
 * mvg_gemv_t_exact. Nothing is read outside A[i, 0..k) and Z[0..m, v) or stored outside
 * Y[0..k, v), v < nv. m == 0 writes k values of +0.0 into each column; k == 0 or nv == 0 is a
 * no-op, also on null pointers. MVG_E_INVALID, decided from the arguments alone before any HIP call
 * (messages start "mvg_gemv_t_exact_multi"): a negative size or nv, lda < k, ldz < m or ldy < k, a
 * null pointer where data would be touched, a variant out of range, more column strips than one
 * grid holds. */
int mvg_gemv_t_exact_multi(const double* d_A, int64_t lda, const double* d_Z, int64_t ldz, double* d_Y, int64_t ldy,
                           int64_t m, int64_t k, int nv, void* stream);
/* explicit variant (0 = auto; names via mvg_gemv_t_exact_multi_variant_name):
 *   1 = separate: one mvg_gemv_t_exact per vector on `stream`;
 *   tseqm_c<SC>_u<U>_v<NV>: the direct form with NV chains per column.
 * The automatic choice takes a fused form only where both kept sweep runs showed it more than 2 %
 * ahead of separate; everything else takes separate. */
int mvg_gemv_t_exact_multi_variant(const double* d_A, int64_t lda, const double* d_Z, int64_t ldz, double* d_Y,
                                   int64_t ldy, int64_t m, int64_t k, int nv, int variant, void* stream);
int mvg_gemv_t_exact_multi_variant_count(void);
/* the variant mvg_gemv_t_exact_multi picks for the group that opens nv vectors */
int mvg_gemv_t_exact_multi_auto_variant(int64_t lda, int64_t ldz, int64_t m, int64_t k, int nv);
const char* mvg_gemv_t_exact_multi_variant_name(int variant);

/* The fused normal-equations product on the same row-major A: what CGNR, LSQR-style solvers and power
 * iteration on A^T A form every iteration, mvg_gemv and mvg_gemv_t back to back, in one call:
 *   t[i] = sum_j A[i*lda + j] * x[j],  i < m
 *   w[j] = sum_i A[i*lda + j] * t[i],  j < k, with t[i] the rounded value that was stored
 * (lda >= k; x and w have k entries, t has m). Both t and w are always written. t meets mvg_gemv's
 * accuracy contract against A x, and w meets mvg_gemv_t's against A^T (the returned t): w is
 * defined on the stored t, so no compounded bound is needed.
 * Device pointers; asynchronous on `stream`. The fused variants (csrc/gemv_ata.hip) stream A once
 * for both products: a workgroup owns a band of whole rows, forms t[i] from the row it has just
 * loaded, adds t[i] times that row to k column sums it keeps in registers, and the band reduce of
 * mvg_gemv_t adds the bands out of the per-(device, stream) workspace (16 * bands * k bytes of
 * traffic; one band goes straight into w). Algorithmic bytes 8 * (m*k + 2*k + m) + 16 * bands * k.
 * No atomics: every sum has one fixed order for a given (variant, m, k), so t and w are the same
 * bits from run to run whatever the workspace held. Any lda >= k and any 8-byte alignment of A, x,
 * t and w; 64-bit row offsets; nothing is read outside A[i, 0..k) and x[0..k) or stored outside
 * t[0..m) and w[0..k). No two operands may overlap: in particular w == x is not allowed (w is
 * written while other workgroups still read x). Special values behave as in the composed pair: a
 * NaN in A[i, j] makes t[i] NaN and no other entry of t, and through t[i] every entry of w.
 * m == 0 writes k zeros to w and nothing to t; k == 0 writes m zeros to t and nothing to w; both
 * zero is a no-op. MVG_E_INVALID, decided from the arguments alone before any HIP call (messages
 * start "mvg_gemv_ata"): a negative size, lda < k, a null pointer where data would be touched, a
 * variant out of range, an explicit fused variant on a k beyond its max_k, a grid that cannot fit
 * (two_pass: more column strips than one launch of mvg_gemv_t holds). */
int mvg_gemv_ata(const double* d_A, int64_t lda, const double* d_x, double* d_t, double* d_w, int64_t m, int64_t k,
                 void* stream);
/* explicit variant (0 = auto; names via mvg_gemv_ata_variant_name):
 *   1 = two_pass: mvg_gemv into t, then mvg_gemv_t from t, both on `stream`; defines the result
 *       for every shape and is the only form for a k beyond every fused cap;
 *   wrow_w<NW>_c<CPL>_u<UNR>: a wave per row, NW waves per workgroup, CPL columns per lane
 *       (k <= max_k = 64 * CPL), UNR rows of loads in flight per wave;
 *   wgrow_w<NW>_c<CPL>_r<RB>: a workgroup per row, wave w owning columns [w * 64 * CPL, +64 * CPL)
 *       (k <= max_k = 64 * NW * CPL), RB rows per barrier.
 * The automatic choice takes a fused form only for a class of shapes where the sweep showed it more
 * than 2 % faster than two_pass in both kept runs; everything else takes two_pass. The fused
 * variants stay callable by number. */
int mvg_gemv_ata_variant(const double* d_A, int64_t lda, const double* d_x, double* d_t, double* d_w, int64_t m,
                         int64_t k, int variant, void* stream);
int mvg_gemv_ata_variant_count(void);
/* the variant mvg_gemv_ata picks for this lda, m and k (the pointers' alignment plays no part) */
int mvg_gemv_ata_auto_variant(int64_t lda, int64_t m, int64_t k);
const char* mvg_gemv_ata_variant_name(int variant);
/* host only, decided from the arguments alone: how `variant` (0 = auto) cuts the m rows into
 * `bands` bands of `band_rows` rows (the last one shorter; bands * band_rows >= m >
 * (bands - 1) * band_rows), one workgroup each, and the widest k it takes. Bands shrink (down to
 * 32 rows) until the grid fills the chip and grow until gridDim.x * blockDim.x < 2^32. two_pass
 * reports band_rows = bands = 0 and max_k = INT64_MAX. */
int mvg_gemv_ata_plan(int64_t lda, int64_t m, int64_t k, int variant, int64_t* band_rows, int64_t* bands,
                      int64_t* max_k);

/* The fused normal-equations product for a block of vectors (what subspace iteration, block Lanczos
 * and randomized range finders form in every step), in the layout of mvg_gemv_multi and
 * mvg_gemv_t_multi:
 *   T[i + v*ldt] = sum_j A[i*lda + j] * X[j + v*ldx],  i < m, v < nv
 *   W[j + v*ldw] = sum_i A[i*lda + j] * T[i + v*ldt],  j < k, with the T[i, v] that was stored
 * A row-major m x k (lda >= k); X k x nv, T m x nv and W k x nv column-major (vector v at d_X + v*ldx,
 * d_T + v*ldt, d_W + v*ldw; ldx >= k, ldt >= m, ldw >= k). Both T and W are always written.
 * Device pointers; asynchronous on `stream`: the fused kernel, the band reduce out of the
 * per-(device, stream) workspace, every group, the single leftover vector, both halves of two_pass
 * and the zeroings of the empty sums all run there. The fused variants (csrc/gemv_ata_multi.hip)
 * send the vectors out in groups of the variant's chain count NV and stream A once per group: the
 * kernels of mvg_gemv_ata with NV column sets, a loaded row serving all NV chains; the band reduce of
 * mvg_gemv_t_multi adds the bands of the whole group in one launch. The last group may be shorter
 * than NV (it runs the same kernel; its spare chains hold the group's last vector again and store
 * nothing); a single leftover vector goes through mvg_gemv_ata (automatic).
 * Accuracy: column v of T meets mvg_gemv's contract against A x_v, and column v of W meets
 * mvg_gemv_t's against A^T (the returned column of T). No atomics: every sum has one fixed order
 * for a given (kernel, m, k). A column's bits depend on A, x_v, m, k and the kernel that ran its
 * group (the fused variant, or mvg_gemv_ata for a single leftover vector) alone: never on the other
 * vectors' values, on the column's place in its group, or on what the workspace held. A NaN in
 * X[j, v] or produced in T[i, v] stays in column v; a NaN in A[i, j] reaches row i of T in every
 * column and, through it, all of W.
 * Any 8-byte alignment and any leading dimensions within the rules above; row and vector offsets are
 * 64-bit; nothing is read outside A[i, 0..k) and X[0..k, v) or stored outside T[0..m, v) and
 * W[0..k, v), v < nv. No two operands may overlap. nv == 0 is a no-op; m == 0 writes k x nv zeros to
 * W and nothing to T; k == 0 writes m x nv zeros to T and nothing to W; both zero is a no-op.
 * MVG_E_INVALID, decided from the arguments alone before any HIP call (messages start
 * "mvg_gemv_ata_multi"): a negative size or nv, lda < k, ldx < k, ldt < m or ldw < k, a null pointer
 * where data would be touched, a variant out of range, an explicit fused variant on a k beyond its
 * max_k, a grid that cannot fit (more column strips than one launch of the transposed half holds). */
int mvg_gemv_ata_multi(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_T, int64_t ldt,
                       double* d_W, int64_t ldw, int64_t m, int64_t k, int nv, void* stream);
/* explicit variant (0 = auto; names via mvg_gemv_ata_multi_variant_name):
 *   1 = two_pass: mvg_gemv_multi into T, then mvg_gemv_t_multi from T, both automatic, on `stream`,
 *       all nv vectors at once; defines the result for every shape, serves the empty sums and is
 *       the only form for a k beyond every fused cap (8192);
 *   wrowm_w<NW>_c<CPL>_u<UNR>_v<NV>: a wave per row, NW waves per workgroup, CPL columns per lane
 *       (k <= max_k = 64 * CPL), UNR rows of loads in flight per wave, NV chains;
 *   wgrowm_w<NW>_c<CPL>_r<RB>_v<NV>: a workgroup per row, wave w owning columns
 *       [w * 64 * CPL, +64 * CPL) (k <= max_k = 64 * NW * CPL), RB rows per barrier, NV chains.
 * The automatic choice goes group by group and names a fused form, with no more chains than vectors
 * are left, only for a class of shapes where two kept sweep runs both showed it more than 2 % ahead
 * of two_pass. No sweep has been run: the automatic choice is two_pass for every shape, and its last
 * single vector (nv == 1 included) is mvg_gemv_ata bit for bit. The fused variants are callable by
 * number. */
int mvg_gemv_ata_multi_variant(const double* d_A, int64_t lda, const double* d_X, int64_t ldx, double* d_T, int64_t ldt,
                               double* d_W, int64_t ldw, int64_t m, int64_t k, int nv, int variant, void* stream);
int mvg_gemv_ata_multi_variant_count(void);
/* the variant mvg_gemv_ata_multi picks for the group that opens nv vectors (the pointers' alignment
 * plays no part; one vector alone goes through mvg_gemv_ata whatever this names) */
int mvg_gemv_ata_multi_auto_variant(int64_t lda, int64_t ldx, int64_t m, int64_t k, int nv);
const char* mvg_gemv_ata_multi_variant_name(int variant);
/* host only, decided from the arguments alone: the first group that `variant` (0 = auto) cuts from
 * nv vectors. *group is its vector count: min(nv, NV) for a fused variant while at least two
 * vectors are left; nv for two_pass (the pair takes them all at once); 1 for a single leftover
 * vector (0 for nv == 0). band_rows, bands and max_k describe that group's launch: mvg_gemv_ata_plan's
 * rule per variant (bands * band_rows >= m > (bands - 1) * band_rows, one workgroup each), never a
 * function of nv; two_pass reports band_rows = bands = 0 and max_k = INT64_MAX; a single vector
 * reports what mvg_gemv_ata_plan reports for the automatic choice. Walk a call group by group by
 * asking again with nv - *group. */
int mvg_gemv_ata_multi_plan(int64_t lda, int64_t m, int64_t k, int nv, int variant, int64_t* band_rows, int64_t* bands,
                            int64_t* max_k, int* group);

/* Read-only streaming microkernel over `bytes` of device memory (HBM ceiling calibration). */
int mvg_stream_read(const double* d_src, int64_t n, double* d_sink, void* stream);

/* ------------------------------------------------------------------ communicators (RCCL)
 * One communicator object per process covers all devices this process drives:
 *   mvg_comm_init_all : single process, G devices (the executables' model; ncclCommInitAll)
 *   mvg_comm_init_rank: one process per device (torch.distributed.run model); the caller
 *                       moves the 128-byte unique id from rank 0 to every rank. */
typedef struct mvg_comm mvg_comm;
#define MVG_UNIQUE_ID_BYTES 128
int mvg_comm_unique_id(unsigned char out[MVG_UNIQUE_ID_BYTES]);
int mvg_comm_init_all(mvg_comm** out, int ndev, const int* devlist);
int mvg_comm_init_rank(mvg_comm** out, const unsigned char id[MVG_UNIQUE_ID_BYTES],
                       int nranks, int rank, int device);
int mvg_comm_size(const mvg_comm* c, int* nranks);
int mvg_comm_local_count(const mvg_comm* c, int* nlocal);
int mvg_comm_local_rank(const mvg_comm* c, int local_index, int* rank, int* device);
int mvg_comm_destroy(mvg_comm* c);

/* ------------------------------------------------------------------ engine
 * The distributed multiplier: one object per (alg, R, C, comm). Holds, per local device,
 * the shard of A, the x segment, the partial y and (on rank 0) the full y.
 *   distribute : host A/x on the root (rank 0's process) -> device shards (H2D, the
 *                Scatter/Bcast/Pack+Send of the reference). A_host == NULL on non-root.
 *   fill_synth : device-resident inputs, generated on each device (no host copy).
 *   multiply   : local GEMV on every device + the exchange step
 *                (row: ncclGather of y; col: ncclReduce(SUM); block: ncclReduce(SUM) on each
 *                 grid-row communicator, then ncclGather of the row leaders' slices).
 *                Asynchronous on the engine's streams; mvg_engine_sync waits. The exchange
 *                runs on a second stream per device and overlaps the next multiply's GEMV
 *                (partial y double-buffered); collect and sync wait for it.
 *   collect    : y (R doubles) -> host on the root.  */
typedef struct mvg_engine mvg_engine;
int mvg_engine_create(mvg_engine** out, int alg, int64_t R, int64_t C, mvg_comm* comm);
int mvg_engine_shard(const mvg_engine* e, int local_index, mvg_shard* out);
int mvg_engine_distribute(mvg_engine* e, const double* A_host, const double* x_host);
/* One process per GPU on one node: the root's A, x live in host memory every rank maps
 * (shared memory); each GPU pulls its own shard over its own PCIe link, all in parallel (the
 * analog of MPICH's shared-memory MPI_Scatter on one host). Every rank passes the full A, x.
 * In single-process mode identical to mvg_engine_distribute. */
int mvg_engine_distribute_shared(mvg_engine* e, const double* A_shared, const double* x_shared);
int mvg_engine_fill_synth(mvg_engine* e, uint64_t seed_a, uint64_t seed_x);
int mvg_engine_multiply(mvg_engine* e);
int mvg_engine_sync(mvg_engine* e);
int mvg_engine_collect(mvg_engine* e, double* y_host);
/* per-local-device GEMV stream (hipStream_t as void*), e.g. for hipEvent timing of the GEMV by
 * the caller; y on the root is complete only after mvg_engine_sync / mvg_engine_collect */
int mvg_engine_stream(const mvg_engine* e, int local_index, void** stream);
/* Average GEMV kernel time (ms) over the multiply calls since the last reset, measured with
 * hipEvents bracketing the kernel on each local device's stream (max over local devices).
 * every = N > 0 brackets every Nth multiply call (1 = all); 0 turns timing off; -1 times spans:
 * one event before the first GEMV after a reset or a sync and one at the next mvg_engine_sync,
 * nothing between the GEMVs of the span (a bracketing marker stalls the stream around its
 * kernel), so the average is the span over its multiplies (the GEMVs back to back, with their
 * dispatch gaps; at more than one rank it also holds the GEMV stream's waits on the exchange).
 * A span that also holds other writes to the shard — a distribution, a synthetic fill, exact
 * mode's panel relayout after the span's first GEMV, a chunked distribution's copies — is
 * dropped: it adds no launches and no time to the average. */
int mvg_engine_kernel_timing(mvg_engine* e, int every);
int mvg_engine_kernel_ms(mvg_engine* e, double* avg_ms, int64_t* launches);
int mvg_engine_destroy(mvg_engine* e);
/* Bit-exact mode (off by default; MVG_EXACT=1 in the environment turns it on at creation):
 * local products by mvg_gemv_exact, and the exchange adds the partials in the reference's own
 * order — the column split's MPI_Reduce as MPICH 3.3.2 sums it (binomial tree, or reduce-scatter
 * + gather for buffers over 2 KiB, oracle/cpu_ref.c ref_mpich_reduce)
 * (colwise.c:124), the block split's partials into a zeroed y in rank order
 * (blockwise.c:150-207) — after an ncclGather of every partial to rank 0. y is then
 * bit-identical to the reference's (block split with > 2 grid columns: to the reference's
 * result for rank-order message arrival; its own order varies run to run). */
int mvg_engine_set_exact(mvg_engine* e, int on);
int mvg_engine_exact(const mvg_engine* e, int* on);
/* Exact mode keeps a column-panel copy of a tall long-row shard (mvg_exact_panel_width) and
 * multiplies it with mvg_gemv_exact_panels: the copy is allocated (if it fits in free HBM with
 * 8 GiB to spare) and rebuilt from the row-major shard by the second multiply after each
 * distribute / fill — a distribution multiplied once never pays for it — and released when exact
 * mode is switched off; MVG_NO_PANELS=1 turns it off. *P = the panel width of local shard i's
 * copy, 0 while it runs the row-major kernels: also after a distribute / fill has made a built
 * copy stale (its memory is kept), until the second multiply rebuilds it. */
int mvg_engine_exact_panels(const mvg_engine* e, int local_index, int64_t* P);
/* Chunked distribution (off by default; MVG_OVERLAP=n in the environment sets it at creation):
 * chunks > 1 makes distribute / distribute_shared move each shard's rows in that many chunks on
 * a copy stream, and the next multiply runs each chunk's GEMV as soon as its rows have landed,
 * so only the last chunk's GEMV follows the transfer (the root-send distribution of one process
 * per GPU is unchanged). 0 or 1 = one copy, then the GEMV. y is the same either way (row chunks
 * are independent products; bit for bit in exact mode). */
int mvg_engine_set_overlap(mvg_engine* e, int chunks);
/* A block of vectors on the distributed A (beyond the reference, whose drivers know one x):
 * Y = A X for X = [x_0 ... x_{nv-1}], 1 <= nv <= MVG_MAX_VECTORS, with one pass over each shard
 * and one exchange for the whole block. Per vector the result is what distribute's x gets from
 * multiply: multiply_std_rowwise on the shard (matr_utils.c:86-96), then the row split's gather
 * (rowwise.c:141), the column split's reduce (colwise.c:124) or the block split's row sums
 * (blockwise.c:144-210). In exact mode column v of Y is bit-identical to the exact single-vector
 * y for x_v (every vector combined as if alone: MPICH's algorithm switch looks at one y's
 * length); in tree mode it is within 1e-12 relative of it on non-negative data.
 *   set_vectors        : the root's host X (C x nv column-major, vector v at X_host + v*ldx,
 *                        ldx >= C; NULL off the root with one process per GPU) -> the whole X on
 *                        every device (H2D per device, or the root's H2D and an ncclBroadcast).
 *                        Touches neither A nor the single x, and needs no earlier distribute.
 *                        The block's device buffers are made here and remade when nv grows. Like
 *                        every write on the GEMV stream it drops an open kernel-timing span.
 *   fill_synth_vectors : X generated on each device, X[j, v] = mvg_synth_value(seed_x, v*C + j).
 *   multiply_multi     : mvg_gemv_multi (mvg_gemv_exact_multi in exact mode) on the row-major
 *                        shard, then the block's exchange; needs A (distribute / fill_synth) and
 *                        X, MVG_E_STATE otherwise. Asynchronous like multiply. It is never part
 *                        of kernel timing (an open span is dropped) and does not count as a
 *                        multiply for exact mode's panel copy.
 *   collect_multi      : Y (R x nv column-major, ldy >= R) -> host on the root.
 *   vectors            : nv of the block last set (0: none yet).
 * The block has its own device buffers: collect after a multiply_multi still returns the last
 * multiply's y, and collect_multi after a multiply the last multiply_multi's Y. */
#define MVG_MAX_VECTORS 16
int mvg_engine_set_vectors(mvg_engine* e, const double* X_host, int64_t ldx, int nv);
int mvg_engine_fill_synth_vectors(mvg_engine* e, uint64_t seed_x, int nv);
int mvg_engine_multiply_multi(mvg_engine* e);
int mvg_engine_collect_multi(mvg_engine* e, double* Y_host, int64_t ldy);
int mvg_engine_vectors(const mvg_engine* e, int* nv);
/* Test hooks of the root-send distribution (one process per GPU: rank 0 stages every peer's
 * shard through two device buffers and sends it, the reference's sequential root Send loop,
 * colwise.c:33-57; no device needed by either hook). A shard travels as its x segment, then its
 * rows in runs of whole rows of at most `stage` doubles, the same list on the sending and the
 * receiving side. mvg_debug_set_stage_elems: the staging size in doubles that engines created
 * afterwards use, read once at mvg_engine_create (0 = the default, 256 MiB; n < 0:
 * MVG_E_INVALID); a live engine keeps the value it was created with. mvg_debug_shard_pieces:
 * the pieces of rank `rank`'s shard at `stage_elems` doubles (0 = the default), in send order:
 * row0[i] = -1 for the x segment, else the piece's first shard row; rows[i] whole rows (1 for
 * the x segment); count[i] doubles. *n pieces are written (none for a shard without columns);
 * more than `max`, or a shard row longer than the staging, is MVG_E_INVALID. */
int mvg_debug_set_stage_elems(int64_t n);
int mvg_debug_shard_pieces(int alg, int64_t R, int64_t C, int nranks, int rank, int64_t stage_elems, int64_t* row0,
                           int64_t* rows, int64_t* count, int max, int* n);

/* ------------------------------------------------------------------ text I/O (src/matr_utils.c)
 * Same file names under the same directory convention: <dir>/matrix_<R>_<C>.txt,
 * <dir>/vector_<n>.txt (dir "./data" in the executables, matr_utils.c:45,68). Whitespace
 * separated "%lf" tokens, row-major. Parsing is strtod (== fscanf "%lf") on an mmap'd file,
 * split over threads; 64-bit indexing. Returns MVG_E_IO if the file is missing or short. */
int mvg_matrix_filename(int64_t R, int64_t C, char* buf, size_t buflen);
int mvg_vector_filename(int64_t n, char* buf, size_t buflen);
int mvg_load_matr(const char* dir, int64_t R, int64_t C, double* A);
/* Binary cache beside the text (<dir>/matrix_<R>_<C>.bin: "MVGBIN1\0", int64 R, int64 C, R*C
 * native fp64). mvg_load_matr reads it instead of the text when it exists, matches (R, C) and is
 * not older than the text; with MVG_BIN_CACHE=1 it also writes it after parsing the text;
 * MVG_BIN_CACHE=0 ignores it. Parsing a 30-120 GB text file once is then enough. */
int mvg_write_matr_bin(const char* path, const double* A, int64_t R, int64_t C);
int mvg_load_vec(const char* dir, int64_t n, double* x);
int mvg_write_vec(const char* path, const double* v, int64_t n);   /* "%.17g\n" per value */
int mvg_write_matr_synth(const char* path, int64_t R, int64_t C, uint64_t seed); /* "%.4f " */

#ifdef __cplusplus
}
#endif
#endif /* MATVEC_GPU_H */
