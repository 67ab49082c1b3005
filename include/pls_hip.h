/*
 * pls_hip.h -- C-ABI of the MI355X (gfx950) PLS fit / predict hot path.
 *
 * This is the drop-in boundary for the body of PLS::Model::plsr and the products
 * behind Model::scores / coefficients / fitted_values of tjhladish/PLS:
 *
 *   reference interface                                   replaced by
 *   ----------------------------------------------------  --------------------------
 *   void Model::plsr(const Mat2D&, const Mat2D&, METHOD)   pls_hip_fit
 *     include/PLS/pls.h:199, src/pls.cpp:390-437
 *   const Mat2Dc Model::coefficients(size_t)               pls_hip_coefficients
 *     include/PLS/pls.h:214, src/pls.cpp:444-447
 *   const Mat2D  Model::fitted_values(const Mat2D&,size_t) pls_hip_xb  (X_new * B)
 *     include/PLS/pls.h:218, src/pls.cpp:449-451
 *   const Mat2Dc Model::scores(const Mat2D&, size_t)       pls_hip_xb  (X_new * R[:, :c])
 *     include/PLS/pls.h:203, src/pls.cpp:439-442
 *
 * The reference has no FFI of its own (it is a C++ library on Eigen); the binding a
 * maintainer adds is the body of Model::plsr in src/pls.cpp -- shown in INTEGRATION.md and
 * shipped in pls_amd/host/pls.cpp.
 *
 * Conventions (the reference's, include/PLS/pls.h:22-27): every matrix is COLUMN-MAJOR
 * with an explicit leading dimension in elements (ld >= rows); dimensions are 64-bit.
 * X is N x K (samples x predictors), Y is N x M, A components.  W,P,R are K x A, Q is
 * M x A, B is K x M, T is N x A.  W,P,Q,R,B and every vector are always fp64; X, Y and T
 * use the storage dtype of the call (fp64, or fp32 storage with fp64 accumulation).
 * All results are real: the reference's std::complex containers (include/PLS/pls.h:26-27)
 * always hold zero imaginary parts and are rebuilt at the C++ boundary.
 *
 * A handle is not thread-safe: one caller at a time per handle (the reference's Model has no shared
 * state either; use one handle per host thread, handles are independent).
 *
 * History: the bits a call returns are a function of its arguments (values, shapes, leading dimensions and the
 * alignment of the pointers), of the handle's options at the time of the call and of the environment switches read by
 * pls_hip_create -- NOT of any earlier call on this handle or on another one: not of the workspaces earlier calls
 * sized and left behind, of calls that were refused or timed out, of options that were changed and set back, of a
 * graph captured under PLS_HIP_OPT_GRAPH, nor of the stream the handle used before.  "Two calls with the same arguments
 * return the same bits" below is meant in this sense.  What results may depend on besides is the device, not history:
 * its number of compute units (launch geometry, hence summation order) and, for the calls that work through their
 * items in rounds (fit_batch, cv_folds, fit_resampled, cv_press_batch), the free device memory where half of it is
 * less than a round of 4 GB would take.  tests/test_gpu_history.py holds every entry point to this on one GPU;
 * INTEGRATION.md section K lists the state a handle does keep.
 *
 * Stream order: every compute entry point works on the handle's stream (pls_hip_create, pls_hip_set_stream) and on nothing else
 * a caller can observe.  A call either ENQUEUES -- it returns once its work is queued, without waiting for the device -- or
 * COMPLETES -- it returns after its work has run, because the host has to read something back (a convergence word, the
 * results of a host-memory call) or hands the device host memory of its own per round.  For both kinds:
 *   1. no input is read before the work already queued on the handle's stream has run;
 *   2. every output is complete for whatever is queued behind the call on that stream;
 *   3. a call that enqueues does not wait for the device -- on a handle that has run the same call before: a first call
 *      allocates or grows workspaces, the allocation may wait for the device, and growing a workspace that is in use waits
 *      for the stream.
 * Host arrays passed to a device-memory call (test_idx) may be reused as soon as the call returns.
 *                                           PLS_HIP_MEM_DEVICE   PLS_HIP_MEM_HOST   ("-": the entry has device pointers only)
 *   pls_hip_fit                             enqueues             completes
 *   pls_hip_coefficients                    enqueues             completes
 *   pls_hip_xb                              enqueues             completes
 *   pls_hip_xty                             enqueues             -
 *   pls_hip_deflate                         enqueues             -
 *   pls_hip_colwise_z_scores                enqueues             -
 *   pls_hip_sse_by_components               enqueues             -
 *   pls_hip_model_sse                       enqueues             completes
 *   pls_hip_cv_folds                        completes            completes          (the index list is the caller's host memory)
 *   pls_hip_validation                      enqueues             completes
 *   pls_hip_x_diagnostics                   enqueues             completes
 *   pls_hip_var_diagnostics                 enqueues             -
 *   pls_hip_fit_batch                       enqueues             completes
 *   pls_hip_fit_resampled                   enqueues             completes
 *   pls_hip_cv_press_batch                  completes            completes          (the index list)
 *   pls_hip_fit_missing, M = 1              enqueues             completes
 *   pls_hip_fit_missing, M > 1              completes            completes          (the host reads the convergence word)
 *   pls_hip_cv_folds_missing                completes            completes          (the index list; the convergence word)
 *   pls_hip_scores_missing                  enqueues             completes
 *   pls_hip_x_diagnostics_missing           enqueues             completes
 *   pls_hip_colwise_z_scores_missing        enqueues             completes
 *   pls_hip_synth_x                         enqueues             -
 *   pls_hip_synth_y                         enqueues             -
 * pls_hip_set_stream and pls_hip_destroy wait for the work pending on the handle's stream first: a call left pending by either
 * still finishes with its outputs right.  A host-memory call may follow a pending device-memory call of the same handle
 * without a synchronisation in between.  A handle on a row-sharded group completes wherever a message's answer is read by the
 * host; pls_hip_group_* run member streams and host threads of their own and are not covered by this table.
 * tests/test_gpu_stream_order.py holds every row of the table, on every route of the entry, to all three points on one GPU;
 * INTEGRATION.md section K lists the state that crosses streams.
 *
 * No torch types, no C++ types, no exceptions cross this boundary; every entry point
 * returns a pls_hip_status and never calls exit().  There is NO CPU fallback: without a
 * gfx950 device every compute entry point fails with PLS_HIP_ERR_DEVICE.
 */
#ifndef PLS_HIP_H
#define PLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLS_HIP_ABI_VERSION 1

#if defined(PLS_HIP_BUILDING)
#define PLS_HIP_API __attribute__((visibility("default")))
#else
#define PLS_HIP_API
#endif

typedef struct pls_hip_context *pls_hip_handle;

typedef enum {
    PLS_HIP_OK = 0,
    PLS_HIP_ERR_INVALID = 1,     /* bad shape / pointer / enum (the reference only assert()s: src/pls.cpp:345-347) */
    PLS_HIP_ERR_DEVICE = 2,      /* HIP runtime error or no usable gfx950 device */
    PLS_HIP_ERR_ALLOC = 3,       /* device allocation failed */
    PLS_HIP_ERR_UNSUPPORTED = 4, /* valid request this build does not implement */
    PLS_HIP_ERR_REDUCER = 5      /* the injected all-reduce returned non-zero */
} pls_hip_status;

/* PLS::METHOD, include/PLS/pls.h:131 */
typedef enum { PLS_HIP_KERNEL_TYPE1 = 0, PLS_HIP_KERNEL_TYPE2 = 1 } pls_hip_method;

typedef enum { PLS_HIP_F64 = 0, PLS_HIP_F32 = 1 } pls_hip_dtype;

/* where the caller's X/Y/outputs live */
typedef enum { PLS_HIP_MEM_HOST = 0, PLS_HIP_MEM_DEVICE = 1 } pls_hip_mem;

/* How the score/loading passes treat X (identical W,P,Q,R,T,B up to rounding):
 *  KERNEL : the reference's operation sequence -- X is read-only, only the K x M matrix
 *           XY is deflated (src/pls.cpp:419-429).
 *  NIPALS : the north-star sequence -- t = X_a w, p = X_a^T t, then the rank-1 deflation
 *           X_{a+1} = X_a - t p^T on a library-owned working copy.
 *  GRAM   : XX = X^T X once on the matrix cores (v_mfma_f64_16x16x4_f64 SYRK), the component loop on
 *           K x K data as KERNEL_TYPE2 does (tt = r^T XX r, p = XX r / tt, src/pls.cpp:422-425), then
 *           T = X R in one pass.  2 + A*0 passes over X; pays off when A exceeds ~K/50.
 *  AUTO   : KERNEL or GRAM, whichever a bandwidth / matrix-core cost model predicts to be faster for
 *           the shape of the call (GRAM only for K <= 2048, single rank).  AUTO never picks DUAL.
 *  DUAL   : the sample-space plan for short, wide X (hundreds to a few thousand rows, any number of columns): G = X X^T
 *           (N x N) once on the matrix cores, the component loop on N-sized data only -- the scores are mutually
 *           orthogonal, so XY_a = X^T (Y - T_a Q_a^T) and everything :403-429 needs is a product with G -- then W and P
 *           from ONE product X^T [U | T diag(1/tt)] (one sweep per 64 columns of [U | T], i.e. one up to A = 32).  Two
 *           sweeps over X whatever A is, no K x K object, no limit on K.  Opt-in, PLS_HIP_KERNEL_TYPE1 only
 *           (PLS_HIP_KERNEL_TYPE2 ignores it as it ignores every plan).  Limits, refused with PLS_HIP_ERR_UNSUPPORTED
 *           before anything is written: N <= 8192 (G is N x N doubles: 512 MB there), M <= 32, no reducer / a group of
 *           one member (G needs every row).  For M > 1 the sign of a component may differ from the other plans' (the
 *           eigenvector is normalised in the response space from a differently rounded matrix); B does not depend on
 *           it.  PLS_HIP_OPT_FUSE, _DEFER and _WORK_LAYOUT do not apply; a DUAL fit is never captured by
 *           PLS_HIP_OPT_GRAPH, it simply runs.  Like GRAM it squares the singular values of X; unlike GRAM it
 *           orthogonalises every score against the earlier ones explicitly.
 *           pls_hip_cv_folds on a handle with this option runs every fold from the same G: one sweep over X for the whole
 *           call (see there).  pls_hip_fit_batch on such a handle runs every problem from the same G: one sweep over X for
 *           Q, tt and ssy, one wide product X^T [...] per round for R and for B, any K (see there).  pls_hip_fit_resampled on
 *           such a handle runs every row-weighted replicate (bootstrap, jack-knife) from the same G (see there).
 *           pls_hip_cv_press_batch on such a handle runs the cross-validation folds of every problem from the same G and
 *           reduces PRESS on the device: one sweep over X for a whole Q^2 permutation test (see there).
 *
 * Accuracy (measured: INTEGRATION.md section I, "Accuracy on hard data").  On column-centred data every plan returns B within
 * 1e-10 (relative Frobenius; 2e-5 with fp32 storage) of an extended-precision fit.  The forms that work from X^T X or X X^T
 * -- GRAM, KERNEL_TYPE2, the single-launch X^T X fit AUTO picks for mid-size data, the host-memory entry under AUTO / GRAM,
 * pls_hip_fit_batch, pls_hip_cv_folds on its batched route, everything under DUAL, which includes the sample-space routes
 * of pls_hip_fit_resampled and pls_hip_cv_press_batch, and the K-space route of pls_hip_cv_press_batch -- square the
 * condition number of X: on uncentred or nearly rank-deficient X they lose what that algebra loses in plain fp64 on a CPU
 * (B to 1e-7 .. 7e-6 with column means of 1e4 on unit-scale data, where KERNEL and NIPALS keep 1e-11; measured for the two
 * calls: B of a replicate 5e-11 .. 1e-7 and its standard error 7e-10 .. 4e-7 on the sample-space route, where the row-scaled
 * refits keep 1e-11 .. 3e-8; PRESS 2e-10 .. 3e-6 relative), and no more: every route stays within a factor 10 of the CPU
 * restatement of its own form (the two calls within 3.0).  pls_hip_fit_missing is NIPALS and keeps 1e-11 on such data.  The library centres nothing, and AUTO chooses by shape alone: it does
 * not look at the data.  Centre the columns, or ask for KERNEL / NIPALS, when the means are large against the spread. */
typedef enum {
    PLS_HIP_ALGO_KERNEL = 0,
    PLS_HIP_ALGO_NIPALS = 1,
    PLS_HIP_ALGO_GRAM = 2,
    PLS_HIP_ALGO_AUTO = 3,
    PLS_HIP_ALGO_DUAL = 4
} pls_hip_algo;

typedef enum {
    PLS_HIP_OPT_ALGO = 1,       /* pls_hip_algo; default PLS_HIP_ALGO_KERNEL */
    PLS_HIP_OPT_FUSE = 2,       /* 0: one kernel per product (Xv, X^T t, deflate); 1 (default): row-tile-resident fused pass when the shape allows */
    PLS_HIP_OPT_PROFILE = 3,    /* HIP events on the launch stream: 1 = around the streaming kernels over X, 2 = around every kernel */
    PLS_HIP_OPT_POWER_ITERS = 4, /* squarings of the S^T S power iteration (m > 1); default 48 */
    PLS_HIP_OPT_FUSED_GRID = 5,  /* workgroups of the fused pass; 0 (default) = 2 per CU */
    PLS_HIP_OPT_WORK_LAYOUT = 6, /* NIPALS work buffer (the deflated copy of X) of a fused fit: 1 (default) row-tile-major, 0 column-major.
                                    The buffer is scratch of the library, not an output: the last component's pass deflates in
                                    registers only, so after a fused fit of A components it holds X_{A-2} */
    PLS_HIP_OPT_DEFER = 7,       /* NIPALS plan, K <= 512: write the deflated matrix back every D-th component only (1..4); the
                                    D - 1 pending rank-1 updates are re-applied in registers.  1 (default) = explicit deflation:
                                    every X_a that a later pass reads is materialised (the last one, which none reads, is not) */
    PLS_HIP_OPT_GRAPH = 8,       /* 1: a device-memory pls_hip_fit that repeats an earlier call (same pointers, shapes, options) is
                                    captured into a hipGraph on its second occurrence and replayed as ONE graph launch from the
                                    third on.  Single rank, profiling off, a stream of its own (not the default stream).  0 (default): every
                                    call enqueues its kernels */
    PLS_HIP_OPT_VALIDATION_LDS_ROWS = 9, /* pls_hip_validation: the largest nobs whose signed-rank sums are formed by ONE workgroup per
                                    (response, alternative) pair, the column pair sorted in LDS; longer columns take the streaming
                                    radix sort.  Default (what pls_hip_get_option returns on a fresh handle): the most this device
                                    allows (16000 rows with 160 KiB of LDS per workgroup).  May be lowered, 0 = every column streams;
                                    a value above the device's own is PLS_HIP_ERR_INVALID */
    PLS_HIP_OPT_MISSING_ITERS = 10      /* pls_hip_fit_missing, M > 1: the most iterations of a component's inner loop.  Default 500
                                    (what pls_hip_get_option returns on a fresh handle); 1 .. 2^20, anything else is
                                    PLS_HIP_ERR_INVALID */
} pls_hip_option;

/*
 * In-place sum over ranks of `count` fp64 values at DEVICE address `buf`, ordered on
 * `stream` (a hipStream_t).  Must leave bit-identical results on every rank.
 * EVERY message is SLICED: `count` is a multiple of PLS_HIP_REDUCE_SLICES, the buffer is
 * PLS_HIP_REDUCE_SLICES slices of count / 8 values, and the library's consumers add the
 * slices of a value in index order.  A reducer may therefore either sum element by element
 * (RCCL, torch.distributed) or leave the total of the 8 slices in slice 0 and zeros in
 * slices 1..7 (the library's device-side exchanges); the library never calls it with an
 * unsliced count.
 * Calls per KERNEL_TYPE1 fit: once with count = 8*K*M (the X^T Y partial), once per
 * component with count = 8*(K+1) (the packed [X^T t, t^T t]), and -- on every fit of a
 * handle with nranks > 1 -- once more with count = 8*8 after the component loop: the
 * replica-divergence guard (checksums of W, P, Q, R, B; the environment switch
 * PLS_HIP_REPLICA_GUARD=0, which must be set identically on EVERY rank, removes it).
 * KERNEL_TYPE2 / GRAM add one message of 8*K*K (X^T X); pls_hip_colwise_z_scores sends two
 * of 8*K, pls_hip_sse_by_components one of 8*A*M per range of component counts,
 * pls_hip_x_diagnostics exactly one of 8*(2*A+1) per call ([ssx (A+1), sst (A)], whichever outputs were asked for).
 * pls_hip_var_diagnostics sends exactly one when it reads X (ssxk, sst, or VIP without tt is asked for) and none otherwise:
 * 8*(A + K*(A+1)) values, [sst (A) | ssxk (K x (A+1), ld K)], with ssxk asked for, 8*A values, [sst (A)], without.
 * pls_hip_cv_folds sends, in this order: the partition (8*nranks: each rank's row count in
 * its own slot); on its batched route X^T X (8*K*K) and X^T Y (8*K*M) of all rows; the
 * held-out rows (8*rows*(K+M) per message of whole folds, rows*(K+M) capped at 2^20 unless a
 * single fold is larger); then E (8*len per piece of at most 2^20 of its values) on the
 * batched route, or the messages of one KERNEL_TYPE1 fit per fold on the refit route.
 * pls_hip_fit_batch sends, in this order: X^T X (8*K*K); then, round by round, one message per piece of whole problems,
 * [XY_b (K*M), ssy_b (M)] per problem: 8*(K+1)*M*nb values, (K+1)*M*nb capped at 2^20 unless a single problem is larger
 * (a piece never spans two rounds).  On its per-problem route: the messages of one KERNEL_TYPE2 fit per problem, each followed
 * by one of 8*M (ssy) when ssy is asked for.
 * Return 0 on success.
 */
#define PLS_HIP_REDUCE_SLICES 8
typedef int (*pls_hip_allreduce_fn)(void *user, void *buf, int64_t count, void *stream);

/* Per-family device time of every launch since the previous pls_hip_get_timing call (recorded
 * only while PLS_HIP_OPT_PROFILE=1; ms from hipEventElapsedTime on the launch stream), launch
 * counts and algorithmic bytes.  pls_hip_get_timing synchronises the stream and resets. */
enum {
    PLS_HIP_FAM_XTY = 0,     /* X^T Y  and  X^T t   (column reductions)           */
    PLS_HIP_FAM_XB = 1,      /* t = X v, X B        (row products)                */
    PLS_HIP_FAM_DEFLATE = 2, /* X -= t p^T                                        */
    PLS_HIP_FAM_FUSED = 3,   /* tile-resident fused pass ([deflate +] score + loading) */
    PLS_HIP_FAM_SMALL = 4,   /* partial reduction + per-component K-sized bookkeeping */
    PLS_HIP_FAM_COUNT = 5
};
typedef struct {
    double fit_ms;                       /* summed over fits: first launch to last     */
    int64_t fits;                        /* number of pls_hip_fit calls covered        */
    double fam_ms[PLS_HIP_FAM_COUNT];    /* summed over launches of the family        */
    int64_t fam_launches[PLS_HIP_FAM_COUNT];
    int64_t fam_bytes[PLS_HIP_FAM_COUNT]; /* ALGORITHMIC bytes summed over those launches */
} pls_hip_timing;

/* ---- lifetime ------------------------------------------------------------------- */

PLS_HIP_API int pls_hip_abi_version(void);

/* device: HIP ordinal.  stream: the hipStream_t every kernel, copy and event of this handle is
 * issued on; NULL = the device's default (null) stream.  Fails with PLS_HIP_ERR_DEVICE if the
 * device is not gfx950. */
PLS_HIP_API int pls_hip_create(pls_hip_handle *out, int device, void *stream);
PLS_HIP_API int pls_hip_destroy(pls_hip_handle h);
PLS_HIP_API int pls_hip_set_stream(pls_hip_handle h, void *stream);
PLS_HIP_API int pls_hip_set_option(pls_hip_handle h, int option, int64_t value);
PLS_HIP_API int pls_hip_get_option(pls_hip_handle h, int option, int64_t *value);
/* Row-sharded fit over `nranks` processes (one per GPU): every rank passes its own row
 * block and the same K, M, A; fn sums the small partial products.  fn == NULL: single rank. */
PLS_HIP_API int pls_hip_set_reducer(pls_hip_handle h, pls_hip_allreduce_fn fn, void *user, int rank, int nranks);
/* What pls_hip_set_reducer left: *installed = 1 when a reducer function is set (the handle's calls are collectives), and the
 * handle's rank and nranks.  Any of the three pointers may be NULL. */
PLS_HIP_API int pls_hip_get_reducer(pls_hip_handle h, int *installed, int *rank, int *nranks);
/* Optional caller-owned DEVICE staging buffer for the reducer
 * (>= PLS_HIP_REDUCE_SLICES * max(K*M, K+1) fp64), so a
 * host runtime can hand its collective a buffer it allocated itself. */
PLS_HIP_API int pls_hip_set_reduce_buffer(pls_hip_handle h, void *buf, int64_t count);
PLS_HIP_API int pls_hip_synchronize(pls_hip_handle h);
PLS_HIP_API const char *pls_hip_last_error(pls_hip_handle h);
PLS_HIP_API int pls_hip_get_timing(pls_hip_handle h, pls_hip_timing *out);

/* ---- the hot path --------------------------------------------------------------- */

/*
 * Fit A components: the body of Model::plsr (src/pls.cpp:390-437).
 * X, Y are never written.  PLS_HIP_KERNEL_TYPE2 (XX = X^T X once, no pass over X per component,
 * src/pls.cpp:398,422-425) does not compute T: T may be NULL and is left untouched.  B (K x M, ld K)
 * may be NULL; otherwise it receives coefficients(A) = R Q^T (src/pls.cpp:444-447).
 * mem == DEVICE: all pointers are device pointers, the call only enqueues work on the
 * stream (pls_hip_synchronize or the caller's own stream sync completes it).
 * mem == HOST: pointers are host memory; the call copies in (pinned double-buffered staging pipeline), fits, copies
 * out and returns with the results in place.  Under PLS_HIP_ALGO_AUTO / _GRAM and for PLS_HIP_KERNEL_TYPE2 (single
 * rank) X^T X and X^T Y are accumulated on the matrix cores while X crosses PCIe and the component loop starts from them.
 * Shapes follow the reference's asserts (src/pls.cpp:345-347): 1 <= A <= K, N >= 1
 * (N may be 0 on a rank of a sharded fit), 1 <= M <= 1024 (beyond 32 responses the M-sized work of the component
 * update runs from global memory: correct, about a millisecond per component slower).  Single-response problems that fit
 * one workgroup's registers (N <= 1024, K <= 26 * floor(16 / ceil(N/64))) run as ONE launch under the KERNEL / AUTO plans.
 * A > rank(X) yields inf/NaN in the surplus columns, as in the reference (:427-428).
 * Under PLS_HIP_ALGO_DUAL (PLS_HIP_KERNEL_TYPE1): the same outputs from G = X X^T in two sweeps over X, any K, any
 * ld >= N, element-aligned pointers, either storage type, either memory kind; N > 8192, M > 32 or a handle with a reducer
 * return PLS_HIP_ERR_UNSUPPORTED with every output untouched.  Workspace: N^2 doubles for G, up to 4 GB of split partials.
 */
PLS_HIP_API int pls_hip_fit(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                int64_t N, int64_t K, int64_t M, int64_t A, int method, int dtype, int mem,
                double *W, double *P, double *Q, double *R, void *T, int64_t ldt, double *B);

/* B(K x M) = R[:, :c] Q[:, :c]^T.  Model::coefficients, src/pls.cpp:444-447. */
PLS_HIP_API int pls_hip_coefficients(pls_hip_handle h, const double *R, const double *Q, int64_t K,
                         int64_t M, int64_t A, int64_t c, int mem, double *B);

/* out(N x C) = X(N x K) * Bm(K x C); Bm fp64, X/out in `dtype`.
 * Model::fitted_values (Bm = B, src/pls.cpp:449-451), Model::scores (Bm = R[:, :c], :439-442). */
PLS_HIP_API int pls_hip_xb(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K,
               const double *Bm, int64_t ldb, int64_t C, int dtype, int mem, void *out,
               int64_t ldo);

/* ---- single steps of the path on DEVICE pointers (parity tests, bench, profiling) -- */

/* XY(K x M, ld K, fp64) = X^T Y   (src/pls.cpp:396; with Y = t, M = 1: src/pls.cpp:421) */
PLS_HIP_API int pls_hip_xty(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                int64_t N, int64_t K, int64_t M, int dtype, double *XY);
/* dst = src - t p^T  (N x K; dst may equal src).  The north-star rank-1 deflation. */
PLS_HIP_API int pls_hip_deflate(pls_hip_handle h, const void *src, int64_t lds, void *dst, int64_t ldd,
                    int64_t N, int64_t K, const void *t, const double *p, int dtype);

/* ---- callers either side of the path, on DEVICE pointers ---- */

/* Column z-scores as the reference's main applies them before the fit (src/pls.cpp:69-111,
 * src/main.cpp:24-25): mean[k], sd[k] = sqrt(SST/(n_total-1)), Z = (X - mean)/sd (Z may be NULL to get
 * the statistics only, or equal to X for an in-place transform).  A constant column yields NaN, as
 * upstream (:103).  n_total = rows over all ranks of a sharded matrix (= N on one GPU). */
PLS_HIP_API int pls_hip_colwise_z_scores(pls_hip_handle h, const void *X, int64_t ldx, int64_t N,
                                         int64_t n_total, int64_t K, int dtype, void *Z, int64_t ldz,
                                         double *mean, double *sd);
/* SSE(M x A, ld M)[m, c-1] = sum_i (Y[i,m] - (S[:, :c] Q[:, :c]^T)[i,m])^2 for c = 1..A in one sweep
 * over the scores S = X R (N x A): Model::SSE for every component count (src/pls.cpp:457-459) without the
 * A separate X*B passes of print_explained_variance (:551-562).  Any A (long component lists are swept in ranges of
 * 1024/M component counts); M <= 1024. */
PLS_HIP_API int pls_hip_sse_by_components(pls_hip_handle h, const void *S, int64_t lds, const void *Y,
                                          int64_t ldy, int64_t N, int64_t A, int64_t M, const double *Q,
                                          int dtype, double *SSE);

/* The same for a model (R: K x A, Q: M x A, ld = rows) and data (X, Y) in host or device memory:
 * S = X R (one pass over X, kept on the device) followed by the sweep above. */
PLS_HIP_API int pls_hip_model_sse(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                                  int64_t N, int64_t K, int64_t M, int64_t A, const double *R,
                                  const double *Q, int dtype, int mem, double *SSE);

/*
 * Cross-validation folds in one batched launch (Model::cv_LOO / cv_LSO,
 * src/pls.cpp:469-549).  Fold f refits A components on every row EXCEPT test_idx[f*test_size .. +test_size)
 * and records the residuals of those test rows:
 *     E[m*(nobs*A) + (f*test_size + i) + c*nobs] = Y[row, m] - x_row^T B_{c+1}^{(f)},   nobs = num_folds*test_size
 * i.e. M matrices of nobs x A, the layout of PLS::Residual::errors().  Leave-one-out = test_size 1,
 * num_folds N, test_idx = 0..N-1.  test_idx is HOST memory (distinct indices within a fold); X, Y, E follow
 * `mem`.  All folds share XX = X^T X and XY = X^T Y formed once; a fold works on
 * XX - X_test^T X_test applied on the fly (the KERNEL_TYPE2 recurrence, src/pls.cpp:422-425): no per-fold
 * pass over X.  Small single-response data (N <= 1024, K <= 26 * floor(16 / ceil(N/64)), M = 1) run as one single-launch fit per
 * fold on the masked X instead (no X^T X at all).  Shapes that launch declines (M > 32, A > 4096, K > 16384, workspaces that do not fit) run as one
 * device refit per fold instead -- same results, num_folds fits.  The call returns after the work
 * has completed.
 * Under PLS_HIP_ALGO_DUAL (no reducer, N <= 8192, M <= 32, PLS_HIP_CV_REFIT unset) the call is taken before all of these by
 * the sample-space route: G = X X^T once -- the only pass over X, whatever A and num_folds are -- then every fold runs the
 * plan's recursion on vectors of length N with its held-out rows masked (Y_0 = diag(mask) Y; the score of every row comes
 * from G, so a held-out row's score under the fold's model is free), in rounds of as many folds as 4 GB of workspace and
 * half of the free device memory hold (PLS_HIP_DUALCV_ROUND=n caps a round): per component one product G [Y_a of every
 * fold] and one workgroup per fold.  Same E, any K, either storage type (fp64 arithmetic), either memory kind; two calls
 * with the same arguments return the same bits.  A fold with fewer training rows than A has inf/NaN in its surplus columns,
 * the earlier ones intact.  A call outside those limits routes as under the other plans (per-fold refits that the
 * sample-space plan would refuse -- M > 32, more than 8192 training rows -- run under the default plan); a workspace that does not fit falls back to the routes above.
 * Row-sharded handle (a reducer installed, pls_hip_set_reducer): the call is a COLLECTIVE.  Every rank calls it
 * with the same K, M, A, test_idx, test_size, num_folds and dtype; X, Y are the rank's own block of N rows
 * (N may be 0), blocks contiguous in rank order (rank r owns global rows [sum_{s<r} N_s, + N_r), as
 * pls_amd.distributed.row_partition makes them), and test_idx holds GLOBAL row indices in [0, n_total).  The
 * library learns the partition from one message of the ranks' N; the checks on global data (an index out of
 * range, n_total < 2, test_size >= n_total: a fold leaving no training rows) run after it, so every rank returns
 * the same PLS_HIP_ERR_INVALID; checks on local data (pointers, ld) run before it, as in the sharded fit.  Every
 * rank receives the full E, bit-identical on all ranks.  The batched route (never the single-launch routes, which
 * read every row) sums X^T X and X^T Y over the ranks and runs a contiguous range of the folds on each rank; the
 * refit route runs one sharded fit per fold, every rank on its own training rows.  A workspace that does not fit
 * on any rank fails the call on every rank (PLS_HIP_ERR_ALLOC) instead of falling back to the refit route.
 * PLS_HIP_CV_REFIT must be set alike on every rank.
 */
PLS_HIP_API int pls_hip_cv_folds(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                                 int64_t N, int64_t K, int64_t M, int64_t A, const int64_t *test_idx,
                                 int64_t test_size, int64_t num_folds, int dtype, int mem, double *E);

/*
 * Validation summary of cross-validation residuals E (the layout pls_hip_cv_folds writes: M matrices of nobs x A, column
 * (m, c) at E + (m*A + c)*nobs; fp64; host or device memory, the outputs live where E lives).  Model::validation and
 * optimal_num_components (src/pls.cpp:235-289) without the host loops:
 *   PRESS (M x A, ld M)   PRESS[m + c*M] = sum_i E[m][i, c]^2.  Fixed summation order: two calls on the same E return the same
 *                         bits (a column is summed in runs of 4096 rows, the runs in index order).
 *   ref (M, int64)        0-based first column with the strictly smallest PRESS of the response (scan from column 0 with `<`: a
 *                         NaN PRESS never replaces the current minimum, a NaN in column 0 is never replaced).
 *   D (M x A, ld M)       for alt < ref[m]: the Wilcoxon signed-rank sum of del_i = |E[m][i, ref]| - |E[m][i, alt]|,
 *                         D = sum_i rank_i * sign(del_i), rank_i = 1-based position of |del_i| in ascending order; exact (it is
 *                         accumulated in 64-bit integers).  Entries with alt >= ref[m] are 0.
 *                         TIES in |del| rank in ROW ORDER (a stable sort).  The reference sorts with std::sort (src/pls.cpp:198),
 *                         which leaves the order of equal keys unspecified; this library defines it.  Rows with del == 0 or NaN
 *                         have sign 0; NaNs rank last.
 *   probw (M x A, ld M)   for alt < ref[m]: 1 - normalcdf((v - ev) / sv) with t = n(n+1)/2, v = (t - D)/2, ev = t/2,
 *                         sv = sqrt(n(n+1)(2n+1)/24) (src/pls.cpp:204-210; n(n+1)(2n+1) is formed in fp64 -- the reference's
 *                         size_t product wraps beyond n = 2.09e6).  Entries with alt >= ref[m] are NaN.
 * EVERY alt < ref[m] is evaluated (the reference stops at the first alt with probw > ALPHA, :281-286), so the result does not
 * depend on ALPHA; the pick is 1 + the first alt < ref[m] with probw > ALPHA, else ref[m] + 1.
 * Any of PRESS / D / probw / ref may be NULL.  nobs, A, M >= 1 and E non-NULL, else PLS_HIP_ERR_INVALID.
 * mem == DEVICE: the work is enqueued on the handle's stream, nothing returns to the host.  mem == HOST: E crosses through the
 * pinned staging pipeline -- in pieces of at most 64 MB through one buffer when neither D nor probw is asked for, as a whole
 * otherwise -- and the call returns with the results in place.
 * Columns of at most PLS_HIP_OPT_VALIDATION_LDS_ROWS rows: one launch for all pairs, one workgroup sorting each pair in LDS.
 * Longer columns: a stable least-significant-digit radix sort of the 63 magnitude bits (8 passes of 8 bits, the sign rides in
 * bit 63) in library workspace, the pairs batched per round as far as 4 GB (2 * nobs * 8 bytes and nobs / 2 bytes of counters per
 * pair) and the device's free memory allow.
 * On a handle with a reducer installed the call is LOCAL: no message is sent (every rank holds the same E).
 */
PLS_HIP_API int pls_hip_validation(pls_hip_handle h, const double *E, int64_t nobs, int64_t A, int64_t M, int mem,
                                   double *PRESS, double *D, double *probw, int64_t *ref);

/*
 * X-space diagnostics of a model (R, P: K x A, ld K, fp64) on data X (N x K, as given: no centring is done here) for every
 * component count c = 1..A in one call.  With S = X R and F_c = X - S[:, :c] P[:, :c]^T:
 *   Qres (N x A, ld ldq)   Qres[i, c-1] = sum_k F_c[i,k]^2          the Q residual (SPE) of row i
 *   T2   (N x A, ld ldt2)  T2[i, c-1]   = sum_{a<c} S[i,a]^2 / tvar[a]   Hotelling T^2; tvar[a] = t_a^T t_a / (n_train - 1)
 *   S    (N x A, ld lds)   the scores, in the storage dtype of the call
 *   ssx  (A + 1)           ssx[0] = sum X^2, ssx[c] = sum_i Qres[i, c-1]:  R^2 X_c = 1 - ssx[c] / ssx[0]
 *   sst  (A)               sst[a] = sum_i S[i,a]^2
 * F_c is formed explicitly, component by component in fp64, and then squared (no expansion of the square: it cancels).
 * The scores are fp64 inside the library for either storage dtype.  Any of Qres, T2, S, ssx, sst may be NULL and work
 * nobody asked for is not done: X is read once for the scores and, when Qres or ssx is wanted, once more per 24 component
 * counts by the residual sweep.  tvar == NULL: X is the training set, tvar[a] = sst[a] / (n_total - 1) from this call's own
 * scores (T2 then needs n_total >= 2).  A zero or non-finite tvar[a] gives inf/NaN in T2 from column a on.
 * mem says where X, R, P, tvar and every output live.  DEVICE: the work is enqueued on the handle's stream, nothing returns
 * to the host.  HOST: through the pinned staging pipeline, the call returns with the results in place.
 * N >= 1 (0 on a rank of a sharded handle), 1 <= A <= K, A <= 2^20, K <= 2^30.  Fixed summation order: two calls with the
 * same arguments return the same bits.
 * Row-sharded handle (a reducer installed): a COLLECTIVE.  Qres, T2, S are the rank's own rows, n_total = rows over all
 * ranks; ssx and sst are summed over the ranks in one message and every rank ends with identical bits.
 */
PLS_HIP_API int pls_hip_x_diagnostics(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t n_total,
                                      int64_t K, int64_t A, const double *R, const double *P, const double *tvar,
                                      int dtype, int mem, double *Qres, int64_t ldq, double *T2, int64_t ldt2, void *S,
                                      int64_t lds, double *ssx, double *sst);

/*
 * Variable-space diagnostics of a model on data X (N x K, as given: no centring) for every component count c = 1..A: which
 * predictors the model uses (VIP) and how much of each predictor it reproduces (the per-variable residual sums of squares).
 * DEVICE pointers only.  W, R, P are K x A with ld K, Q is M x A with ld M, tt has A entries; all fp64.  With S = X R (fp64 inside
 * the library for either storage dtype) and F_c = X - S[:, :c] P[:, :c]^T:
 *   ssxk (K x (A+1), ld ldk >= K)  ssxk[k, 0] = sum_i X[i,k]^2, ssxk[k, c] = sum_i F_c[i,k]^2:  R^2 X of variable k with c
 *                                  components = 1 - ssxk[k, c] / ssxk[k, 0]
 *   sst  (A)                       sst[a] = sum_i S[i,a]^2 from this call's scores
 *   VIP  (K x A, ld ldv >= K)      VIP[k, c-1] = sqrt(K * sum_{a<c} ssy_a W[k,a]^2 / ||w_a||^2 / sum_{a<c} ssy_a),
 *                                  ssy_a = tau_a * sum_m Q[m,a]^2, tau = tt when tt is non-NULL, this call's sst otherwise
 *                                  (tt = t_a^T t_a of the training scores, as pls_hip_fit returns them in T; a zero denominator
 *                                  gives the NaN the formula gives)
 * F_c is formed explicitly, component by component in fp64, and then squared (no expansion of the square: it cancels).
 * Any output may be NULL and work nobody asked for is not done: VIP with tt given reads nothing N-sized (X may be NULL, N is
 * ignored); sst alone, or VIP without tt, reads X once for the scores; ssxk reads X once for the scores and once more per 24
 * component counts by the column sweep.  Nothing N x K is written.
 * PLS_HIP_ERR_INVALID, before anything is written: an output asked for without the inputs its definition names (ssxk: X, R, P;
 * sst: X, R; VIP: W, Q, and tt or X and R); N < 1 where X is needed (0 on a rank of a sharded handle); A < 1, A > K, A > 2^20,
 * K > 2^30; M < 1 when VIP is asked for; ldx < N, ldk < K, ldv < K.
 * Any ld >= rows, element-aligned pointers, both storage dtypes, fixed summation order without atomics: the bits are a function
 * of the arguments, the alignment of X and the device's CU count.  The call only enqueues work on the handle's stream.
 * Row-sharded handle (a reducer installed): a COLLECTIVE whenever X is needed, which follows from the arguments every rank
 * shares.  [sst | ssxk] is summed over the ranks in one message (pls_hip_allreduce_fn), VIP is formed behind it, and every rank
 * ends with identical bits.  VIP with tt given is local.
 * Out of scope: pls_hip_group_* and the C++ PLS::Model; a host-memory form of this call (host callers upload; the Python layer
 * does); NaN cells in X (a NaN spreads through its column and every score); selectivity ratio; contribution plots; control limits.
 */
PLS_HIP_API int pls_hip_var_diagnostics(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t M, int64_t A,
                                        const double *W, const double *R, const double *P, const double *Q, const double *tt,
                                        int dtype, double *ssxk, int64_t ldk, double *VIP, int64_t ldv, double *sst);

/*
 * Many response sets against ONE X: for every problem b = 0..nprob-1 the model Model::plsr(X, Y_b, KERNEL_TYPE2)
 * (src/pls.cpp:390-437), Y_b = columns [b*M, (b+1)*M) of Ys (N x nprob*M, column-major, ld ldy).  All problems share
 * XX = X^T X, formed once; each starts from its own XY_b = X^T Y_b, all of them formed in one wide product on the matrix
 * cores.  This is the work behind a response-permutation (Y-randomisation) test, a scan of one model per phenotype, or any
 * loop of pls_hip_fit(..., KERNEL_TYPE2) over the same X.  X and Ys use the storage dtype of the call (fp64 accumulation
 * throughout) and are never written.  Outputs, all fp64, any may be NULL (work nobody asked for beyond the loop itself is not
 * done):
 *   R    R + b*K*A   K x A, ld K            Q    Q + b*M*A   M x A, ld M
 *   tt   tt + b*A    tt[a] = r_a^T XX r_a   B    B + b*K*M   K x M, ld K, = R Q^T
 *   ssy  ssy + b*M   sum_i Y_b[i,m]^2
 * so that ESS[m,c] = sum_{a<=c} Q[m,a]^2 tt[a] and R^2 Y = ESS / ssy are host arithmetic on M*A numbers.  W, P and T are NOT
 * returned: a caller who wants them for one problem calls pls_hip_fit on (X, Y_b).  Sign convention for M > 1: that of
 * pls_hip_fit.  The algebra on X^T X squares the condition number of X: the bars of INTEGRATION.md section H hold for
 * column-centred data; on uncentred or nearly rank-deficient X the call loses what KERNEL_TYPE2 loses (the Accuracy note above).
 * 1 <= A <= K, N >= 1 (0 on a rank of a sharded handle), M >= 1, nprob >= 1, ldx, ldy >= N, X and Ys non-NULL; anything else
 * is PLS_HIP_ERR_INVALID before anything is written.
 * mem == DEVICE: the call only enqueues work on the handle's stream.  mem == HOST: the inputs cross through the pinned staging
 * pipeline and the call returns with the results in place.  Fixed summation order: two calls with the same arguments return
 * the same bits.
 * Batched route (K <= 16384, M <= 32, A <= 4096): the problems run in rounds of as many as 4 GB of workspace and half the
 * free device memory hold (3 K A + K M + M A + K + 1 values per problem and the columns of the product); per component two
 * launches for ALL problems of a round -- V = XX [r_0 r_1 ...] as one matrix-core GEMM, then one workgroup per problem.
 * Per-problem route (every other shape, a workspace that does not fit, or PLS_HIP_BATCH_REFIT=1 in the environment): one
 * KERNEL_TYPE2 fit per problem under the handle's plan -- same results to rounding, nprob fits; shapes pls_hip_fit refuses
 * return its status.
 * Under PLS_HIP_ALGO_DUAL (no reducer, 1 <= N <= 8192, M <= 32, PLS_HIP_BATCH_REFIT unset) the call is taken before both by the
 * sample-space route: G = X X^T once -- with Q, tt and ssy asked for the only pass over X, whatever A and nprob are -- then
 * every problem runs the plan's recursion on vectors of length N from its own Y_b, in rounds of as many problems as 4 GB of
 * workspace and half of the free device memory hold (2 N M + 2 N A + A^2 + M A + 2 A + N values per problem;
 * PLS_HIP_DUALBATCH_ROUND=n caps a round): per component one product G [Y_a of every problem] and one workgroup per problem.
 * Q, tt (= t_a^T t_a) and ssy are written from N-sized work.  R and B come back through sample space: R_b = X^T S_b with
 * s_a = u_a - sum_{j<a} C[j,a] s_j, B_b = X^T (S_b Q_b^T), so R (and B) of all problems of a round is ONE product
 * X^T [S_0 | S_1 | ...] written straight into the caller's array: one launch per round and output (up to 64 columns the
 * back-projection kernel of the DUAL fit, beyond them 128 x 128 blocks on the matrix cores), nothing K-sized besides the
 * outputs.  Any K, any ld >= N, element-aligned pointers, either storage type (fp64 arithmetic), either memory kind; the
 * same values as the other routes to rounding (for M > 1 a component's sign may differ, as for the DUAL fit; B does not
 * depend on it); two calls with the same arguments return the same bits.  A call outside those limits routes exactly as
 * without the option, and so does one whose workspace does not fit even for one problem.  PLS_HIP_BATCH_REFIT=1 under the
 * option is the library's cross-check for K <= 32768.
 * Row-sharded handle (a reducer installed): a COLLECTIVE with the same K, M, A, nprob on every rank; Ys holds the rank's
 * own rows.  X^T X and the products of every piece of problems are summed over the ranks (pls_hip_allreduce_fn lists the
 * messages), the component loops then run replicated from identical bits: every rank ends with identical outputs.
 * PLS_HIP_BATCH_REFIT must be set alike on every rank.
 */
PLS_HIP_API int pls_hip_fit_batch(pls_hip_handle h, const void *X, int64_t ldx, const void *Ys, int64_t ldy,
                                  int64_t N, int64_t K, int64_t M, int64_t A, int64_t nprob, int dtype, int mem,
                                  double *R, double *Q, double *tt, double *B, double *ssy);

/* ---- row-weighted replicate fits: bootstrap and jack-knife of B ------------------------------
 * The same (X, Y) fitted under nrep sets of non-negative row weights.  Wt is N x nrep fp64, column-major with ldw >= N, and
 * lives where `mem` says.  Replicate b is the model Model::plsr(diag(s_b) X, diag(s_b) Y, KERNEL_TYPE1) with
 * s_b = sqrt(Wt[:, b]): a bootstrap draw is a column of integer counts, a jack-knife segment a 0/1 mask, a case-weighted fit
 * one replicate.  The data are used as given -- no centring, the convention of pls_hip_cv_folds.
 * Outputs, all fp64, any may be NULL (work nobody asked for beyond the component loop is not done):
 *   Q + b*M*A (M x A) and tt + b*A      of replicate b; tt[a] = t~_a^T t~_a, the WEIGHTED sum of squares of the score
 *   B + b*K*M (K x M, ld K)             the coefficients of replicate b, for UNSCALED rows: y^ = x^T B_b
 *   B0 (K x M)                          the fit with unit weights, computed by the same route as a replicate: a replicate whose
 *                                       weights are all 1 has B_b - B0 == 0 exactly
 *   Bmean, Bm2 (K x M)                  with d_b = B_b - B0 accumulated in replicate order, s1 = sum d_b and s2 = sum d_b^2
 *                                       (formed with fma): Bmean = B0 + s1 / nrep, Bm2 = s2 - s1^2 / nrep.
 * The caller scales: bootstrap se = sqrt(Bm2 / (nrep - 1)), delete-a-group jack-knife over g groups se = sqrt((g - 1) / g Bm2).
 * Rows of weight 0 drop out of the replicate.  The library does NOT inspect the weights: a negative or non-finite weight gives
 * NaN in that replicate and in the summaries.  A replicate with fewer positively weighted rows than A has inf / NaN in its
 * surplus columns, as a fold of pls_hip_cv_folds does.
 * 1 <= A <= K, N >= 1, M >= 1, nrep >= 1, ldx, ldy, ldw >= N, X, Y and Wt non-NULL; anything else is PLS_HIP_ERR_INVALID.  A
 * handle with a reducer installed returns PLS_HIP_ERR_UNSUPPORTED.  Both before anything is written.
 * mem == DEVICE: the call only enqueues work on the handle's stream.  mem == HOST: the inputs cross through the pinned staging
 * pipeline and the call returns with the results in place.  Fixed summation order: two calls with the same arguments return
 * the same bits.
 * Sample-space route (PLS_HIP_ALGO_DUAL set, N <= 8192, M <= 32, PLS_HIP_RESAMPLE_REFIT unset): G = X X^T once -- the only pass
 * over X unless B, B0, Bmean or Bm2 is asked for.  The Gram matrix of the scaled rows is diag(s) G diag(s), so per component a
 * round of replicates costs ONE product G [s o Y~_a of every replicate] and one workgroup per replicate that reads it back
 * through s; B of a round is one product X^T [s o S~_b Q_b^T of every replicate], straight into the caller's array (into
 * workspace when only a summary is wanted), and B0 one product of M columns.  Rounds hold as many replicates as 4 GB of workspace
 * and half of the free device memory allow (3 N M + 2 N A + A^2 + M A + 2 A + 2 N values per replicate, plus K M when a summary
 * is wanted without B; PLS_HIP_RESAMPLE_ROUND=n caps a round).  A workspace that does not fit even one replicate falls
 * through to the general route.
 * General route (every other handle or shape, PLS_HIP_RESAMPLE_REFIT=1): per replicate diag(s) X and diag(s) Y are written into
 * fp64 work copies (N x K, N x M) and fitted by the handle's KERNEL_TYPE1 plan (a handle under PLS_HIP_ALGO_DUAL refits under
 * PLS_HIP_ALGO_KERNEL: the route is the cross-check of the sample-space one and does not share its algebra); tt comes from
 * that fit's scores.  Shapes
 * pls_hip_fit refuses return its status; a work copy that does not fit returns PLS_HIP_ERR_ALLOC.
 */
PLS_HIP_API int pls_hip_fit_resampled(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                                      int64_t N, int64_t K, int64_t M, int64_t A, const double *Wt, int64_t ldw,
                                      int64_t nrep, int dtype, int mem, double *Q, double *tt, double *B, double *B0,
                                      double *Bmean, double *Bm2);

/* ---- cross-validated fits of many response sets: PRESS per problem, the Q^2 permutation test ----
 * The cross-validation of pls_hip_cv_folds for nprob response sets against one X, reduced to what a Q^2 needs.  Ys is as in
 * pls_hip_fit_batch (N x nprob*M, problem b owns the columns [b*M, (b+1)*M)); test_idx (HOST memory), test_size and num_folds
 * are as in pls_hip_cv_folds, nobs = num_folds * test_size, and the same folds apply to every problem.  The data are used as
 * given -- no centring.
 * Outputs, all fp64, living where `mem` says, any may be NULL:
 *   PRESS + b*M*A (M x A, ld M)   PRESS[m + c*M] = sum over o < nobs of E_b[m][o, c]^2
 *   ssy + b*M (M)                 ssy[m] = sum over o < nobs of Y_b[row(o), m]^2: the PRESS of the zero-component model over the
 *                                 same observations (a row held out twice counts twice), so Q^2[m, c] = 1 - PRESS / ssy
 *   E + b*M*nobs*A                exactly what pls_hip_cv_folds(X, Y_b, ...) documents, for problem b.  Normally NULL: nothing
 *                                 nobs x A-sized per problem then exists anywhere.
 * The checks of pls_hip_cv_folds, nprob >= 1 and Ys non-NULL; anything else is PLS_HIP_ERR_INVALID.  A handle with a reducer
 * installed returns PLS_HIP_ERR_UNSUPPORTED.  Both before anything is written.  The call returns after the work has completed.
 * Fixed summation order, no atomics: two calls with the same arguments return the same bits, and PRESS and ssy have the same
 * bits whether or not E is asked for.
 * Sample-space route (the conditions of pls_hip_cv_folds under PLS_HIP_ALGO_DUAL, and PLS_HIP_CVBATCH_REFIT unset): G = X X^T
 * once -- the only pass over X whatever A, nprob and num_folds are.  The work items are the pairs item = b*num_folds + f, in
 * that order, in rounds of as many as 4 GB of workspace and half of the free device memory hold (2 N M + N A + N + 2 A +
 * 3 test_size M + M A + M values per item, fewer than 2^30 / (N M) items; PLS_HIP_DUALCVB_ROUND=n caps a round); a problem's
 * folds may straddle two rounds.  The training-row masks exist once per fold (N ints each), shared by the problems.  Per
 * component a round costs one product G [Y_a of every item] and one workgroup per item, which leaves the item's partial PRESS
 * summed over its held-out rows by test position; after the round the partials are added to PRESS_b in item order, so every
 * (b, m, c) adds its folds in fold order wherever the round boundaries fall.  ssy likewise.  The columns of Ys are converted to
 * fp64 round by round.  A workspace that does not fit even one item falls through to the general route.
 * General route (every other handle or shape, PLS_HIP_CVBATCH_REFIT=1): per problem pls_hip_cv_folds on (X, Y_b) -- into the
 * caller's slice of E or a workspace of M nobs A doubles -- then the PRESS kernels of pls_hip_validation; a small kernel for
 * ssy.  The same results to rounding at the cost of nprob cross-validations; statuses of pls_hip_cv_folds are passed on, and
 * PRESS there needs nobs < 2^31, M A <= 2^24 (PLS_HIP_ERR_UNSUPPORTED otherwise).
 */
PLS_HIP_API int pls_hip_cv_press_batch(pls_hip_handle h, const void *X, int64_t ldx, const void *Ys, int64_t ldy,
                                       int64_t N, int64_t K, int64_t M, int64_t A, int64_t nprob,
                                       const int64_t *test_idx, int64_t test_size, int64_t num_folds, int dtype, int mem,
                                       double *PRESS, double *ssy, double *E);

/* ---- X with missing values: NIPALS with the missing cells skipped --------------------------------
 * NaN in X marks a missing cell (any payload, either sign, quiet or signalling: the result does not depend on it); obs(i,k) =
 * X[i,k] is no NaN.  Y must be complete: it is not inspected, a NaN in Y propagates.  Every inner product over a column or a
 * row of X runs over the observed cells only and is divided by the sum of squares of the other factor over the same cells
 * (Wold's NIPALS, as ropls and mixOmics implement it).  For component a = 0 .. A-1 on the work copies X_a, Y_a:
 *   u = the column of Y_a with the largest sum of squares (lowest index on ties); M = 1: u = y_a
 *   repeat, it = 1, 2, ...
 *     w_k = sum_{i: obs(i,k)} X_a[i,k] u_i / sum_{i: obs(i,k)} u_i^2;   w = w / |w|_2
 *     t_i = sum_{k: obs(i,k)} X_a[i,k] w_k / sum_{k: obs(i,k)} w_k^2;   q = Y_a^T t / t^T t
 *     M = 1: stop after it = 1.  M > 1: stop when it >= 2 and |t - t_prev|^2 <= 1e-20 |t|^2, or at it =
 *     PLS_HIP_OPT_MISSING_ITERS; else u = Y_a q / q^T q
 *   p_k = sum_{i: obs(i,k)} X_a[i,k] t_i / sum_{i: obs(i,k)} t_i^2
 *   X_{a+1} = X_a - t p^T on the observed cells (a NaN stays a NaN);  Y_{a+1} = Y_a - t q^T
 *   r_a = w_a - sum_{j<a} r_j (p_j^T w_a);   B = R Q^T
 * All sums fp64 in a fixed order, no atomics; a quotient whose denominator is exactly 0 (no observed cell) is 0, so a row or a
 * column without an observed cell gets zeros in T[i,:] and in W/P/R/B[k,:] and leaves everything else finite.
 * R is DEFINED by the recursion above, not as W (P^T W)^-1: with missing cells P^T W is not triangular and the two differ (ropls
 * and mixOmics report W (P^T W)^-1).  The recursion is the matrix for which x^T R equals the scores that sequential deflation
 * gives a complete row x, so B is self-consistent with T.  On data without NaN this is ordinary NIPALS PLS: the outputs equal
 * the NIPALS plan of pls_hip_fit to rounding, up to the sign of a component for M > 1.
 * Conventions of pls_hip_fit: column-major, any ld >= rows, element-aligned pointers, both storage types (fp64 arithmetic;
 * the work copy of X is in the storage type), both memory kinds (host through the pinned staging pipeline).  X and Y are never
 * written.  T in the storage type.  B and iters may be NULL; iters (A values, where `mem` says): the iterations each component
 * took (all 1 for M = 1).  1 <= A <= K, N >= 1, M >= 1, ldx, ldy, ldt >= N, X, Y, W, P, Q, R, T non-NULL; anything else is
 * PLS_HIP_ERR_INVALID.  M > 32, or a handle with a reducer installed, returns PLS_HIP_ERR_UNSUPPORTED.  Both before anything is
 * written.  M = 1 and PLS_HIP_MEM_DEVICE: the call only enqueues.  M > 1: the call returns after the work has completed -- the
 * iterations are enqueued in batches of 8, every kernel of an iteration returns at once when the device convergence word is
 * set, and the host reads that word through pinned memory after each batch.  PLS_HIP_OPT_ALGO, _FUSE, _DEFER and _GRAPH do not
 * apply: there is one route.  Two calls with the same arguments return the same bits.
 * Per component the work copy is read three times and written once for M = 1 (deflate + w, t, p), read 2 iters + 1 times and
 * written once for M > 1; the first sweep reads the caller's matrix instead.  Workspace: the N x K work copy and, for short
 * wide X, up to 1024 partial score vectors.
 * Out of scope: row-sharded handles and groups, missing values in Y, resampling on data with NaN, a sample-space form.
 * Cross-validation: pls_hip_cv_folds_missing below; Q residuals, T^2 and R^2 X: pls_hip_x_diagnostics_missing below.
 */
PLS_HIP_API int pls_hip_fit_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                                    int64_t N, int64_t K, int64_t M, int64_t A, int dtype, int mem, double *W, double *P,
                                    double *Q, double *R, void *T, int64_t ldt, double *B, int64_t *iters);

/* Scores of rows, new or training, that may have missing cells: the sequential deflation above with the model's W and P (K x A,
 * ld K): t_a = sum_obs x_k w_ka / sum_obs w_ka^2, then x <- x - t_a p_a, on a work copy with the fit's own sweeps.  S: N x A in
 * the storage type.  On the training X it reproduces T; on complete rows it equals pls_hip_xb(X, R).  Fitted values are
 * S[:, :c] Q[:, :c]^T (pls_hip_xb on S).  N >= 1, 1 <= A <= K, ldx, lds >= N, non-NULL pointers, else PLS_HIP_ERR_INVALID; a
 * handle with a reducer installed: PLS_HIP_ERR_UNSUPPORTED.  PLS_HIP_MEM_DEVICE: the call only enqueues. */
PLS_HIP_API int pls_hip_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t A,
                                       const double *W, const double *P, int dtype, int mem, void *S, int64_t lds);

/* X-space diagnostics of rows, new or training, that may have missing cells: what pls_hip_x_diagnostics is to complete data, for
 * the models of pls_hip_fit_missing.  NaN in X marks a missing cell exactly as for pls_hip_fit_missing: any payload, either sign,
 * and the bits of the result do not depend on it.  W and P are the model's own W and P (K x A, ld K, fp64) -- NOT R: the
 * convention of pls_hip_scores_missing.  For row i let x be the row and O the set of its observed columns:
 *   q_0 = sum_{k in O} x_k^2
 *   for a = 0 .. A-1:
 *     t_a = sum_{k in O} x_k W[k,a] / sum_{k in O} W[k,a]^2        (a denominator of exactly 0 gives 0)
 *     x_k <- x_k - t_a P[k,a]  for k in O                          (a NaN stays a NaN)
 *     q_{a+1} = sum_{k in O} x_k^2
 * Outputs; any of them may be NULL, and work nobody asked for is not done:
 *   S     N x A, ld lds, storage dtype   S[i,a] = t_a: the definition of pls_hip_scores_missing
 *   Qres  N x A, ld ldq, fp64            Qres[i,c-1] = q_c: the Q residual over the observed cells after c components
 *   T2    N x A, ld ldt2, fp64           T2[i,c-1] = sum_{a<c} t_a^2 / tvar[a]
 *   ssx   A + 1, fp64                    ssx[0] = sum_i q_0, ssx[c] = sum_i Qres[i,c-1]; R^2 X_c = 1 - ssx[c] / ssx[0], over the
 *                                        observed cells
 *   sst   A, fp64                        sst[a] = sum_i t_a^2
 *   nobs  N, int64                       the observed cells of row i, so that a caller can scale Q by K / nobs
 * tvar == NULL means X is the training set: tvar[a] = sst[a] / (N - 1) from this call's own scores.  A zero or non-finite tvar[a]
 * gives inf / NaN in T2 from column a on, as in pls_hip_x_diagnostics.  A row without an observed cell has S = Qres = T2 = 0 and
 * nobs = 0.
 * All arithmetic is fp64.  The row is NEVER rounded to the storage type between components, and T2, Qres, ssx and sst use the
 * unrounded t_a.  This differs from pls_hip_scores_missing, which keeps its work copy in the storage type: with fp32 storage the
 * two calls' S agree to fp32 rounding, with fp64 storage to 1e-10.
 * Sums run in a fixed order with no atomics.  An output has the same bits whichever other outputs are asked for.  Two calls with
 * the same arguments return the same bits, from host or device memory (a host-memory call is the device-memory call on the
 * staged layout), whatever the handle ran before ("History" at the top of this file).  As for every entry point, the bits may
 * differ with the alignment of X: 16-byte loads are used when the pointer and ldx allow them, element loads otherwise.
 * Two routes, chosen by shape (xdiagmiss_layout.hpp), both reading the caller's X directly, neither with a work copy.  Tall X
 * (K <= 1024, N >= 8 rows per compute unit): a workgroup holds a tile of rows on chip across all components, X is read ONCE.
 * Everything else: one read-only sweep per component plus one for q_A (A + 1 reads of X; A when neither Qres nor ssx is asked
 * for), every cell rebuilt in registers from the scores so far, K split over workgroups where the rows alone do not fill the
 * chip.  PLS_HIP_XDIAGMISS_ROUTE=stream in the environment of pls_hip_create forces the second route (the cross-check; the two
 * agree to rounding, not in bits).  Workspace: N x A scores, up to N x (A + 1) Q columns, and on the streaming route 32 bytes per
 * row and K range -- nothing N x K.
 * `mem` says where X, W, P, tvar and every output live.  PLS_HIP_MEM_DEVICE: the call only enqueues.
 * PLS_HIP_ERR_INVALID, before anything is written: N < 1; A < 1 or A > K; ldx < N, or the ld of an output that was asked for < N;
 * X, W or P NULL; T2 asked for with tvar == NULL and N < 2.  PLS_HIP_ERR_UNSUPPORTED, before anything is written: a handle with a
 * reducer installed (and K >= 2^31, A > 2^20).  PLS_HIP_OPT_ALGO, _FUSE, _DEFER and _GRAPH do not apply.
 * Out of scope: row-sharded handles and groups, NaN in W, P or tvar, a per-column R^2 X. */
PLS_HIP_API int pls_hip_x_diagnostics_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K, int64_t A,
                                              const double *W, const double *P, const double *tvar, int dtype, int mem,
                                              double *Qres, int64_t ldq, double *T2, int64_t ldt2, void *S, int64_t lds,
                                              double *ssx, double *sst, int64_t *nobs);

/* Cross-validation folds of X with missing values: what pls_hip_cv_folds is to pls_hip_fit, for pls_hip_fit_missing.
 * Fold f holds out the rows test_idx[f * test_size .. + test_size) (host memory, as in pls_hip_cv_folds).  Its result is BY
 * DEFINITION what the entry points above give: pls_hip_fit_missing on the training rows -> W, P, Q;
 * S = pls_hip_scores_missing(X_test, W, P); E_c = Y_test - S[:, :c] Q[:, :c]^T for c = 1 .. A.  The data are used as given, no
 * centring (the convention of pls_hip_cv_folds).  E has exactly the layout pls_hip_cv_folds documents:
 * E[m * (nobs * A) + a * nobs + f * test_size + i], nobs = num_folds * test_size; pls_hip_validation takes it unchanged.
 * iters may be NULL; else num_folds x A values, iters[f * A + a] (all 1 for M = 1).  X, Y, E and iters follow `mem`.
 * No rows are gathered: with m the 0/1 training mask of the fold, the algorithm of pls_hip_fit_missing runs on work copies of
 * ALL rows, the mask entering through N-sized vectors only -- w and p accumulate against m o u and m o t, q and the stop rule
 * see m o t, u starts from the column of Y_a with the largest sum of squares over the training rows; t is computed for every
 * row and every row of X_a and Y_a is deflated with its own t.  A held-out row adds exact zeros to every column sum and goes
 * through the sequential deflation of pls_hip_scores_missing; after component a its row of Y_{a+1} is E's column a.  This equals
 * the definition to rounding (at most 8e-15 measured, relative Frobenius on E).  A column with no observed training cell in a fold has
 * w_k = p_k = 0 there, a row with no observed cell t = 0.
 * The folds run in rounds: as many at a time as 4 GB of workspace and half the free device memory hold (each fold has its own
 * work copy of X), at least one; PLS_HIP_ERR_ALLOC when not even one fits.  Every kernel of the component loop is launched once
 * per round with the fold as a grid dimension, so the launches per component do not grow with the number of folds.  M > 1: every
 * fold has its own convergence word; the host reads "every fold of the round has stopped" through pinned memory after each 8
 * iterations.  The masked form reads the held-out rows in the w and p sweeps too: 1 / num_folds more bytes than gathered refits.
 * All sums fp64 in a fixed order, no atomics, the sweep geometry from (N, K, type, CU count) alone: the bits of a fold's slice
 * of E and iters depend on X, Y, A, that fold's indices, dtype, the leading dimensions, the pointer alignment and the device --
 * not on num_folds, the round, the other folds or the handle's history.
 * Checks, all before anything is written.  PLS_HIP_ERR_INVALID: those of pls_hip_fit_missing, N < 2, an index out of range, an
 * index twice within a fold, test_size < 1 or >= N, num_folds < 1 (limits: 2^22 folds of 2^20 rows).  PLS_HIP_ERR_UNSUPPORTED:
 * M > 32, a handle with a reducer installed.  The call returns after the work has completed.  PLS_HIP_OPT_ALGO, _FUSE, _DEFER
 * and _GRAPH do not apply; PLS_HIP_OPT_MISSING_ITERS does.  R, B and T are not produced.
 * Out of scope: row-sharded handles and groups, NaN in Y, a PRESS-only batched form. */
PLS_HIP_API int pls_hip_cv_folds_missing(pls_hip_handle h, const void *X, int64_t ldx, const void *Y, int64_t ldy,
                                         int64_t N, int64_t K, int64_t M, int64_t A, const int64_t *test_idx,
                                         int64_t test_size, int64_t num_folds, int dtype, int mem, double *E,
                                         int64_t *iters);

/* pls_hip_colwise_z_scores over the observed cells: nobs[k] = observed cells of column k, mean and sd = sqrt(SST / (nobs - 1))
 * over them (one sweep), Z = (X - mean) / sd with NaN kept.  Z may be NULL or equal to X; nobs may be NULL.  A column with fewer
 * than two observed cells (sd = NaN; none: mean = NaN too) or with zero spread (sd = 0) gets NaN throughout, as the complete-data
 * call does for a constant column; pls_hip_fit_missing then treats it as entirely missing and it drops out of the model with
 * w_k = p_k = B_k = 0.  Single rank only: a handle with a reducer installed returns PLS_HIP_ERR_UNSUPPORTED. */
PLS_HIP_API int pls_hip_colwise_z_scores_missing(pls_hip_handle h, const void *X, int64_t ldx, int64_t N, int64_t K,
                                                 int dtype, int mem, void *Z, int64_t ldz, double *mean, double *sd,
                                                 int64_t *nobs);

/* ---- synthetic inputs, generated on the device (DESIGN.md "Synthetic inputs") ------ */

/* rows [row0, row0+nrows) of the global matrix -> X (nrows x K, ld ldx) / Y (nrows x M) */
PLS_HIP_API int pls_hip_synth_x(pls_hip_handle h, void *X, int64_t ldx, int64_t row0, int64_t nrows,
                    int64_t K, uint64_t seed, int dtype);
PLS_HIP_API int pls_hip_synth_y(pls_hip_handle h, void *Y, int64_t ldy, int64_t row0, int64_t nrows,
                    int64_t M, uint64_t seed, int dtype);

/* ---- one process per GPU without RCCL: the device-side exchange across processes ---------------------------------
 *
 * The reducer of a row-sharded fit (pls_hip_set_reducer) as a direct exchange between the ranks' GPUs: every rank owns an
 * inbox in fine-grained device memory, exported with hipIpcGetMemHandle; a collective is two small launches per rank --
 * the rank WRITES its partial sums into every peer's inbox over xGMI and raises a sequence flag there, then spins on its
 * own flags and adds the inboxes in rank order (exchange_kernels.hpp; the same kernels the in-process group uses).  These
 * messages are a few KB and latency-bound, which is what this form is for; RCCL (include/pls_hip_rccl.h) or any other
 * pls_hip_allreduce_fn remain alternatives.  Set-up, on every rank:
 *     pls_hip_xchg_create(h, rank, nranks, mine)         -> `mine`: PLS_HIP_XCHG_HANDLE_BYTES to publish
 *     (all-gather the blobs in rank order with whatever the application has: MPI, torch.distributed, a file)
 *     pls_hip_xchg_connect(h, all)                        opens the peers' inboxes, installs the reducer
 *     pls_hip_xchg_selftest(h)                            COLLECTIVE: one round on known values with a 5 s limit;
 *                                                         PLS_HIP_ERR_REDUCER if this system cannot do it -- then every
 *                                                         rank should pls_hip_xchg_destroy and take another reducer
 * A rank that waits longer than 30 s (PLS_HIP_XCHG_TIMEOUT_S) for a peer -- a rank failed or fell out of step -- gives up:
 * pls_hip_synchronize returns PLS_HIP_ERR_REDUCER from then on.  2 <= nranks <= 16.
 */
#define PLS_HIP_XCHG_HANDLE_BYTES 160
PLS_HIP_API int pls_hip_xchg_create(pls_hip_handle h, int rank, int nranks, void *mine);
PLS_HIP_API int pls_hip_xchg_connect(pls_hip_handle h, const void *all);
PLS_HIP_API int pls_hip_xchg_selftest(pls_hip_handle h);
PLS_HIP_API int pls_hip_xchg_destroy(pls_hip_handle h);

/* ---- one process, several GPUs: a group of handles behind one call ------------------
 *
 * The reference's Model is one object driven by one host thread (include/PLS/pls.h:187-199, src/pls.cpp:340-353).
 * A group keeps that shape while the rows of X and Y are spread over the GPUs of the node: it owns one handle and
 * one stream per member and runs every call with one host thread per member inside the library.  The members'
 * partial products are summed by a reducer the group installs itself -- a fixed-order all-reduce with no RCCL and,
 * when every member has a GPU of its own, nothing on the host at all: each member WRITES its partial sums into an
 * inbox on every peer over xGMI and raises a sequence flag there, and the consumer's kernel spins on its flags and adds
 * the inboxes in rank order ("device-side exchange": two small launches per member and collective, a one-hop direct
 * write as SURVEY.md 8(e) recommends for these latency-bound messages; a member that waits longer than 30 s -- a peer
 * failed or fell out of step -- makes the call return PLS_HIP_ERR_REDUCER).  The exchange is tried once on known
 * values when the group is created.  Where it is not available (members that share a GPU -- see below -- or no peer
 * writes into fine-grained memory), and for messages beyond 512 KB, the members instead READ each other's buffers
 * behind two host-thread barriers per collective ("host-synchronised exchange").  Either way all members end up with
 * identical bits.  PLS_HIP_GROUP_EXCHANGE = device | host overrides the choice.
 * `devices[r]` is the HIP ordinal of member r; an ordinal may repeat ("virtual shards" sharing one GPU: the way the
 * sharded path is exercised on a one-GPU machine).  A group of one member is a plain single-GPU fit.
 *
 * Matrices live on the device(s) between calls (288 GB of HBM per GPU: the training data of a Model stays resident
 * instead of being copied on the host as src/pls.cpp:344 does): pls_hip_group_upload spreads a HOST matrix over the
 * members by rows -- member r owns a contiguous block, the same partition for every matrix of the same row
 * count -- through a double-buffered pinned staging pipeline (host threads repack a tile while the DMA engine
 * transfers the previous one).
 */
typedef struct pls_hip_group_s *pls_hip_group;
typedef struct pls_hip_matrix_s *pls_hip_matrix;

PLS_HIP_API int pls_hip_group_create(pls_hip_group *out, int n, const int *devices);
PLS_HIP_API int pls_hip_group_destroy(pls_hip_group g);
PLS_HIP_API int pls_hip_group_size(pls_hip_group g);
/* 1 = the device-side exchange carries the group's collectives, 0 = the host-synchronised one (or one member) */
PLS_HIP_API int pls_hip_group_exchange(pls_hip_group g);
/* member r's handle (options, timing); it stays owned by the group */
PLS_HIP_API int pls_hip_group_handle(pls_hip_group g, int rank, pls_hip_handle *out);
PLS_HIP_API int pls_hip_group_set_option(pls_hip_group g, int option, int64_t value);
PLS_HIP_API const char *pls_hip_group_last_error(pls_hip_group g);

/* N x K host matrix (column-major, ld) -> resident, row-sharded.  Returns when the data has left `host`. */
PLS_HIP_API int pls_hip_group_upload(pls_hip_group g, const void *host, int64_t ld, int64_t N, int64_t K,
                                     int dtype, pls_hip_matrix *out);
/* X (N x K) and Y (N x M) of one data set together.  While the rows of X stream in over PCIe, every member
 * accumulates X^T X and X^T Y of its rows block by block on the matrix cores (a block's SYRK takes a fraction of
 * its transfer time), and the pair keeps them: a later pls_hip_group_fit(X, Y) under PLS_HIP_ALGO_AUTO or _GRAM (and
 * KERNEL_TYPE2) starts its component loop at once -- no pass over X before it, one (T = X R) after it -- and
 * pls_hip_group_cv_folds skips its own X^T X.  Layouts the matrix-core kernel declines (K > 4096, unaligned)
 * simply upload; the fit then forms the products itself. */
PLS_HIP_API int pls_hip_group_upload_xy(pls_hip_group g, const void *hostX, int64_t ldx, const void *hostY,
                                        int64_t ldy, int64_t N, int64_t K, int64_t M, int dtype,
                                        pls_hip_matrix *X, pls_hip_matrix *Y);
/* uninitialised resident N x K matrix (e.g. the scores T of a fit) */
PLS_HIP_API int pls_hip_group_alloc(pls_hip_group g, int64_t N, int64_t K, int dtype, pls_hip_matrix *out);
/* columns [col0, col0 + ncols) of a resident matrix -> host (N x ncols, ld) */
PLS_HIP_API int pls_hip_group_download(pls_hip_group g, pls_hip_matrix m, int64_t col0, int64_t ncols, void *host,
                                       int64_t ld);
PLS_HIP_API int pls_hip_group_free(pls_hip_group g, pls_hip_matrix m);
PLS_HIP_API int pls_hip_matrix_shape(pls_hip_matrix m, int64_t *N, int64_t *K, int *dtype);
/* member r's block of a resident matrix: device pointer, leading dimension, first row, row count */
PLS_HIP_API int pls_hip_matrix_block(pls_hip_matrix m, int rank, void **data, int64_t *ld, int64_t *row0,
                                     int64_t *nrows);

/* pls_hip_fit on resident X (N x K), Y (N x M); T: resident N x A (scores stay on the devices; NULL for
 * PLS_HIP_KERNEL_TYPE2).  W, P, R (K x A), Q (M x A), B (K x M, may be NULL) are HOST memory, ld = rows.  Every
 * member derives the same W, P, Q, R, B bit for bit; the call checks that before it returns
 * (PLS_HIP_ERR_REDUCER otherwise). */
PLS_HIP_API int pls_hip_group_fit(pls_hip_group g, pls_hip_matrix X, pls_hip_matrix Y, int64_t A, int method,
                                  double *W, double *P, double *Q, double *R, pls_hip_matrix T, double *B);
/* out (resident N x C) = X * Bm, Bm HOST K x C fp64 (Model::scores / fitted_values, src/pls.cpp:439-451) */
PLS_HIP_API int pls_hip_group_xb(pls_hip_group g, pls_hip_matrix X, const double *Bm, int64_t ldb, int64_t C,
                                 pls_hip_matrix out);
/* pls_hip_model_sse on resident data; R, Q, SSE (M x A) HOST */
PLS_HIP_API int pls_hip_group_model_sse(pls_hip_group g, pls_hip_matrix X, pls_hip_matrix Y, int64_t A,
                                        const double *R, const double *Q, double *SSE);
/* pls_hip_x_diagnostics on a resident X; R, P (K x A), tvar (A, or NULL: X is the training set), ssx (A + 1), sst (A) HOST;
 * Qres, T2 (fp64) and S (dtype of X) resident N x A matrices.  Any output may be NULL. */
PLS_HIP_API int pls_hip_group_x_diagnostics(pls_hip_group g, pls_hip_matrix X, int64_t A, const double *R, const double *P,
                                            const double *tvar, pls_hip_matrix Qres, pls_hip_matrix T2, pls_hip_matrix S,
                                            double *ssx, double *sst);
/* pls_hip_fit_batch on resident X (N x K) and Ys (N x nprob*M, the storage type of X); R, Q, tt, B, ssy HOST, any may be NULL.
 * The members run as for pls_hip_group_fit; an X^T X that came with pls_hip_group_upload_xy is used.  A one-member group
 * whose member has PLS_HIP_ALGO_DUAL set reaches the sample-space route of pls_hip_fit_batch through the member's handle. */
PLS_HIP_API int pls_hip_group_fit_batch(pls_hip_group g, pls_hip_matrix X, pls_hip_matrix Ys, int64_t M, int64_t A,
                                        double *R, double *Q, double *tt, double *B, double *ssy);
/* pls_hip_cv_folds on resident data, E (M x nobs x A) HOST.  Groups of one member only (the fold kernel works on
 * K-sized data of ONE device); PLS_HIP_ERR_UNSUPPORTED otherwise. */
PLS_HIP_API int pls_hip_group_cv_folds(pls_hip_group g, pls_hip_matrix X, pls_hip_matrix Y, int64_t A,
                                       const int64_t *test_idx, int64_t test_size, int64_t num_folds, double *E);

#ifdef __cplusplus
}
#endif
#endif /* PLS_HIP_H */
