/*
 * dlsa_hip.h -- C-ABI of libdlsa_hip.so, the MI355X (gfx950) DLSA estimator.
 *
 * This is the drop-in boundary for the reference's map/combine/select path
 * (Vicky-Lamperouge/dlsa).  The reference has no FFI: its map stage is a
 * Spark GROUPED_MAP pandas_udf around dlsa/models.py:logistic_model, its
 * combine is dlsa/dlsa.py:dlsa_mapred and its selection step is
 * dlsa/lsa.py:lars_lsa (or R lars.lsa via rpy2, dlsa/dlsa.py:64-81).  Each
 * entry point below names the reference interface it replaces.  The Python
 * binding (ctypes) lives in dlsa_amd/_hip.py; INTEGRATION.md shows the stub a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - Plain C types only.  Pointers named X/y/theta/... are DEVICE pointers
 *     (hipMalloc'd or torch tensor data_ptr()), except where "host" is noted.
 *   - The caller owns every buffer.  Scratch comes from the caller's
 *     workspace (dlsa_fit_options.workspace) or, when that is NULL, is
 *     hipMallocAsync'd on the stream and freed before return.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, NULL = default
 *     stream).  dlsa_logistic_fit_batched* reads a 16-byte device counter
 *     back once per Newton iteration (a stream synchronisation); the other
 *     device entry points are fully asynchronous.
 *   - Return 0 on success, a negative DLSA_E_* code on failure; the message
 *     is in dlsa_last_error() (thread-local).
 *   - Row-major fp64.  Partition k owns rows offsets[k] .. offsets[k+1]-1 of X
 *     (partitions contiguous: the layout Spark's repartition(K,
 *     "partition_id") + groupby produce per task, projects/logistic_dlsa.py:
 *     303-325).  X must be readable up to the next 16-byte boundary past its
 *     last element (true for any torch/hipMalloc allocation that starts at
 *     the tensor); what those bytes hold does not matter.
 *   - P = p + fit_intercept is the parameter count; with an intercept the
 *     intercept is parameter 0 (dlsa/models.py:116-122).
 */
#ifndef DLSA_HIP_H
#define DLSA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define DLSA_OK 0
#define DLSA_E_INVALID (-1)
#define DLSA_E_HIP (-2)
#define DLSA_E_UNSUPPORTED (-3)
#define DLSA_E_WORKSPACE (-4)

/* per-partition status (status[] output) -- SURVEY.md section 5: the
 * reference only warns (models.py:84-91,144-145); here every partition
 * reports what happened. */
#define DLSA_STATUS_OK 0          /* converged */
#define DLSA_STATUS_MAXITER 1     /* max_iter reached; the last iterate is returned
                                     with Sig_inv = X^T W X evaluated at it (one
                                     extra exact pass, as sklearn's model is used at
                                     whatever coef it stopped at, models.py:114-130) */
#define DLSA_STATUS_SINGULAR 2    /* X^T W X not positive definite */
#define DLSA_STATUS_EMPTY 3       /* no rows: zero block, like models.py:84-91 */
#define DLSA_STATUS_NONFINITE 4   /* NaN/Inf in the data or the iterates */
#define DLSA_STATUS_MISSING_LEVEL 5  /* categorical fit: a selected dummy level has no
                                        rows in the partition -> the reference's
                                        all-zero frame (models.py:84-91) */

/* Hessian arithmetic of the Newton passes.  The gradient, eta, the weights
 * and the returned log-likelihood are fp64 in every mode; the approximate
 * Hessians only steer Newton (the fp64 gradient fixes the solution).  The
 * Hessian returned as Sig_inv comes from the EXACT pass(es) that end the fit,
 * whose arithmetic dlsa_fit_options.exact_pass selects (DLSA_EXACT_*). */
#define DLSA_HESSIAN_MIXED 0      /* bf16 MFMA Hessian until the step is below
                                     switch_tol, then exact pass(es); a partition
                                     whose step stops shrinking (two iterations
                                     in a row without halving, or backtracking)
                                     moves to fp32 MFMA, then to exact passes */
#define DLSA_HESSIAN_FP64 1       /* fp64 MFMA Hessian on every pass (exact_pass is
                                     ignored) */
#define DLSA_HESSIAN_MIXED_F32 2  /* as MIXED with fp32 MFMA approximate passes
                                     (for ill-conditioned designs) */

/* Arithmetic of the exact pass in the MIXED modes.
 * DLSA_EXACT_AUTO: X^T W X from int8 digit slices on the int8 matrix cores
 *   (the Ozaki scheme) wherever it applies -- P <= 112 with chunks of at most
 *   32767 rows, every partition of the pass carrying a max |z| record from
 *   its last approximate pass (a partition stopped by max_iter in an
 *   approximate phase does not), and P > DLSA_MAX_P_FUSED when the workspace
 *   holds the digit records -- otherwise fp64 MFMA.  A chunk whose bound on
 *   |z| passes 2^1009 fails its partition (non-finite) instead of wrapping
 *   its digits.  z = sqrt(w) x is rounded to a 38-bit
 *   fixed-point grid below 2^E_f per chunk (or row group) and feature, the
 *   digit products are summed exactly in int32 and the levels below 2^-40 of
 *   the leading product are dropped: every entry of Sig_inv is within about
 *   1e-12 sqrt(H_ii H_jj) of the fp64 sum (tests/test_gpu_ozaki.py pins
 *   < 1e-10 on heavy-tailed designs), and the result is bit-identical run to
 *   run.  The logistic weights, gradient, log-likelihood and theta stay fp64.
 * DLSA_EXACT_FP64: every exact pass on the fp64 MFMA (v_mfma_f64_16x16x4). */
#define DLSA_EXACT_AUTO 0
#define DLSA_EXACT_FP64 1

#define DLSA_MAX_P_FUSED 192  /* largest P handled by the fused pass + LDS Newton solve */
#define DLSA_MAX_P 512        /* largest P overall: above DLSA_MAX_P_FUSED a row pass, a
                                 128x128-tiled Gram pass and a blocked Cholesky in HBM
                                 take over (BASELINE config 5, p = 500) */

/* The families the entries that take one as an argument know (dlsa_glm_gof_*). */
#define DLSA_FAMILY_LOGISTIC 0
#define DLSA_FAMILY_POISSON 2
/* Candidates of one goodness-of-fit pass: the most at which none of its
   kernels spills (two sums per candidate). */
#define DLSA_MAX_GOF_CANDIDATES 16
/* The row weight d_i of dlsa_glm_gram_batched's sum_i d_i x_i x_i^T. */
#define DLSA_GRAM_SCORE 0        /* d = s^2, s = omega (y - mu): the sandwich's meat */
#define DLSA_GRAM_INFORMATION 1  /* d = omega w: the information matrix at beta */

typedef struct dlsa_fit_options {
  int32_t hessian_mode;     /* DLSA_HESSIAN_MIXED (default) or _FP64 */
  int32_t record_timing;    /* 1: time every launch with hipEvents, see
                               dlsa_last_fit_stats() */
  double switch_tol;        /* MIXED: relative step size that triggers the fp64
                               pass (<= 0: default 1e-6) */
  void* workspace;          /* device scratch, NULL: allocate per call */
  int64_t workspace_bytes;  /* size of `workspace` */
  int32_t rows_per_chunk;   /* <= 0: automatic (rows one workgroup streams).
                               A tuning hint, here and in every entry that takes
                               one: a chunk holds at most (2^31 - 2^20) / (8 p)
                               rows, so that its X (p columns, 8 p bytes per
                               row) stays inside one 2 GiB buffer range with
                               32-bit offsets.  A partition asked for in longer
                               chunks is split evenly into ceil(n_k / that
                               limit) or more of them
                               (dlsa_fit_stats.n_chunks,
                               dlsa_logistic_workspace_bytes count these).
                               Sums depend on the chunking in their last bits,
                               as for any other rows_per_chunk; the per-row
                               outputs of dlsa_glm_rows_batched do not */
  int32_t warm_start;       /* 1 (default): the first Newton iterations run on
                               row prefixes of each partition (1/16, then 1/4
                               of the rows, never fewer than max(2048, 64 P))
                               to a 0.1-relative step, then on all rows to tol -- the
                               fixed point is unchanged; 0: all rows from the
                               start.  Prefix iterations count against max_iter
                               (a level takes at most half of what is left), so
                               iters[k] <= max_iter and max_iter = 1 is one
                               full-data Newton step from 0 */
  int32_t exact_pass;       /* DLSA_EXACT_AUTO (default) or DLSA_EXACT_FP64 */
  int32_t exact_waves;      /* geometry of the fp64 exact pass for P <= 128: 0 =
                               automatic, 1 = all tiles in one wave, 2 = two waves
                               (P 17..112); the result does not depend on it */
  int64_t oz_max_bytes;     /* P > DLSA_MAX_P_FUSED, mixed mode: at most this many
                               bytes of int8 digit records (<= 0: no cap); more
                               runs the fp64 Gram (dlsa_fit_stats.oz_fallbacks) */
  int32_t reserved[2];
} dlsa_fit_options;
/* The library reads no environment variable that changes a result: the
 * output of every entry point depends only on its arguments.  (DLSA_TRACE
 * prints per-iteration steps to stderr; profiling builds compiled with
 * -DDLSA_ENV_KNOBS=1 also read the A/B knobs named in csrc/fit_plan.hpp and the fit_*.hip files.) */

typedef struct dlsa_fit_stats {
  int32_t iterations;       /* Newton iterations run (max over partitions) */
  int32_t passes_fp32;      /* approximate-Hessian (bf16/fp32 MFMA) pass launches */
  int32_t passes_fp64;      /* fp64-Hessian pass launches */
  int32_t n_chunks;         /* waves per pass launch */
  double ms_pass_fp32;      /* summed kernel time (record_timing only) */
  double ms_pass_fp64;
  double ms_solve;          /* per-partition Cholesky/Newton update kernels */
  double ms_total;          /* whole call, host wall clock */
  int64_t rows_fp32;        /* rows streamed by approximate-Hessian passes (sum
                               over launches, warm-start levels included) */
  int64_t rows_fp64;        /* rows streamed by fp64 passes (sum) */
  double ms_wide_row;       /* P > DLSA_MAX_P_FUSED: row-pass kernel time (there
                               ms_pass_fp32/fp64 hold the bf16 / fp64 Gram-pass time) */
  double ms_wide_gram;      /* P > DLSA_MAX_P_FUSED: Gram-pass kernel time */
  double ms_wide_assemble;  /* P > DLSA_MAX_P_FUSED: partial-tile assembly time */
  int32_t passes_f32x;      /* of passes_fp32: fp32-MFMA passes of partitions that
                               escalated from bf16 (stall / lost definiteness) */
  int32_t polish_partitions; /* partitions left running by max_iter that got the
                               exact pass publishing Sig_inv at their theta */
  int32_t passes_oz;        /* of passes_fp64: on the int8 matrix cores (Ozaki
                               digit slices) */
  int32_t oz_fallbacks;     /* P > DLSA_MAX_P_FUSED, mixed mode: fits whose exact
                               Gram took the fp64 MFMA path because the int8
                               digit records had no room (a workspace of at least
                               the size without them but smaller than
                               dlsa_logistic_workspace_bytes, a failed
                               allocation, or dlsa_fit_options.oz_max_bytes) */
  int32_t oz_stale_partitions; /* P <= 112, mixed mode: partition passes of an
                               exact pass that ran on the fp64 MFMA beside the
                               int8 launch of the others, for lack of a fresh
                               max |sqrt(w) x| record */
} dlsa_fit_stats;

/* Default options (mixed Hessian, automatic chunking, no timing). */
void dlsa_fit_options_default(dlsa_fit_options* opt);

/* Device scratch needed by a fit with these partitions (offsets: HOST array of
 * K+1 int64).  Pass at least this many bytes in dlsa_fit_options.workspace.
 * The plan does not depend on the family: the same size serves
 * dlsa_poisson_fit_batched_ex (whose K start values and constant-term partials
 * live in a small allocation of the fit's own, on the stream).
 * For P > DLSA_MAX_P_FUSED this includes the int8 digit records of the
 * mixed-mode exact Gram (n * PP * 5 bytes, PP = P rounded up to 128; DESIGN.md
 * 4.4b): a smaller workspace that still holds everything else runs the fp64
 * Gram instead (dlsa_fit_stats.oz_fallbacks).  The library keeps no device
 * memory between calls: a NULL workspace is allocated on the stream and
 * freed before return. */
int64_t dlsa_logistic_workspace_bytes(const int64_t* offsets, int32_t K,
                                      int32_t p, int32_t fit_intercept,
                                      int32_t rows_per_chunk);

/*
 * Batched local logistic fit -- replaces the body of the map-stage UDF,
 * dlsa/models.py:42-147 logistic_model(), for K partitions at once:
 *   standardise (models.py:99-101; center/scale may be NULL),
 *   unpenalised logistic MLE (sklearn newton-cg, models.py:110-113),
 *   theta = [b0, b] with the intercept first (models.py:116-122),
 *   Sig_inv = X^T diag(p(1-p)) X at theta (models.py:130),
 *   Sig_invMcoef = Sig_inv theta (models.py:131).
 * Newton/IRLS from theta = 0; converged when max|step| <= tol*(1+max|theta|).
 *
 *  X        [n_total, p] fp64 row-major, device
 *  y        [n_total] fp64 0/1 labels, device
 *  offsets  [K+1] int64, HOST, offsets[0] = 0, non-decreasing
 *  center, scale  [p] fp64 device or NULL (both or neither)
 *  theta          [K, P] out     sig_inv       [K, P, P] out
 *  sig_inv_theta  [K, P] out     loglik        [K] out (at theta)
 *  iters          [K] int32 out  status        [K] int32 out (DLSA_STATUS_*)
 * 1 <= P <= DLSA_MAX_P.
 */
int dlsa_logistic_fit_batched(const double* X, const double* y,
                              const int64_t* offsets, int32_t K, int32_t p,
                              int32_t fit_intercept, const double* center,
                              const double* scale, int32_t max_iter,
                              double tol, double* theta, double* sig_inv,
                              double* sig_inv_theta, double* loglik,
                              int32_t* iters, int32_t* status, void* stream);

/* Same, with options (Hessian mode, caller workspace, timing). */
int dlsa_logistic_fit_batched_ex(const double* X, const double* y,
                                 const int64_t* offsets, int32_t K, int32_t p,
                                 int32_t fit_intercept, const double* center,
                                 const double* scale, int32_t max_iter,
                                 double tol, double* theta, double* sig_inv,
                                 double* sig_inv_theta, double* loglik,
                                 int32_t* iters, int32_t* status,
                                 const dlsa_fit_options* opt, void* stream);

/*
 * Batched local Poisson regression (log link) -- a third family of the
 * batched fit; the reference has no counterpart.  Arguments and outputs
 * exactly as dlsa_logistic_fit_batched_ex.  Per partition:
 *   eta = x . theta, mu = exp(eta) (intercept first, center/scale as there),
 *   theta         the unpenalised Poisson MLE,
 *   sig_inv       X^T diag(mu) X at the returned theta,
 *   sig_inv_theta sig_inv theta,
 *   loglik        sum_i y_i eta_i - mu_i - lgamma(y_i + 1), the full
 *                 log-likelihood (the step control compares the constant-free
 *                 sum; the constant is added where loglik is returned).
 * y is real, finite and >= 0 (non-integer y allowed: quasi-likelihood use).
 * Start point: with an intercept theta = (log mean y_k, 0, ..., 0), the MLE of
 * the intercept-only model; without one theta = 0.  A partition restarted by
 * a failed warm-start level goes back to this point.  Two statuses are
 * decided before any pass, with all-zero outputs: a negative or non-finite y
 * gives DLSA_STATUS_NONFINITE, sum y = 0 (the MLE does not exist)
 * DLSA_STATUS_SINGULAR.  A step after which the log-likelihood is not finite
 * (exp overflow) is halved like one after which it fell.
 * opt may be NULL.  hessian_mode, exact_waves, warm_start, switch_tol and the
 * workspace keep their meaning; exact_pass: DLSA_EXACT_AUTO resolves to the
 * fp64 MFMA (the weights exp(eta) are unbounded: the int8 exact pass does not
 * apply).  Limit: P <= DLSA_MAX_P_FUSED (192), else DLSA_E_UNSUPPORTED before
 * any launch.  Workspace: dlsa_logistic_workspace_bytes.
 */
int dlsa_poisson_fit_batched_ex(const double* X, const double* y,
                                const int64_t* offsets, int32_t K, int32_t p,
                                int32_t fit_intercept, const double* center,
                                const double* scale, int32_t max_iter,
                                double tol, double* theta, double* sig_inv,
                                double* sig_inv_theta, double* loglik,
                                int32_t* iters, int32_t* status,
                                const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_poisson_fit_batched_ex with a per-row offset of the linear predictor
 * (rate models: eta_offset = log exposure, R's glm(offset=)):
 *   eta_i = x_i . theta + eta_offset_i,  mu_i = exp(eta_i).
 *  eta_offset  [n_total] fp64, device, finite; row i belongs to row i of X.
 *              NULL: exactly dlsa_poisson_fit_batched_ex (the same kernels,
 *              bit-identical outputs).
 * (`offsets` stays the partition boundaries; the two are unrelated.)
 * All other arguments and the outputs as there; sig_inv = X^T diag(mu) X and
 * loglik are taken at the mu above.  The offset is one more 8 B/row stream of
 * the passes; nothing per row is stored and the workspace is unchanged.
 * Start point: with an intercept theta = (log(sum y_k / sum exp(eta_offset_k)),
 * 0, ..., 0), the MLE of the intercept-only rate model; without one theta = 0.
 * Restarts go back to it.  Beside the rules of dlsa_poisson_fit_batched_ex, a
 * partition with a non-finite eta_offset, or whose sum exp(eta_offset) is not
 * finite and positive, ends DLSA_STATUS_NONFINITE before any pass with
 * all-zero outputs; the other partitions are not affected.  A zero exposure
 * (eta_offset = -inf) is the caller's row to drop.
 * Limit: P <= DLSA_MAX_P_FUSED (192), else DLSA_E_UNSUPPORTED before any launch.
 */
int dlsa_poisson_fit_batched_offset(const double* X, const double* y,
                                    const double* eta_offset,
                                    const int64_t* offsets, int32_t K, int32_t p,
                                    int32_t fit_intercept, const double* center,
                                    const double* scale, int32_t max_iter,
                                    double tol, double* theta, double* sig_inv,
                                    double* sig_inv_theta, double* loglik,
                                    int32_t* iters, int32_t* status,
                                    const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_logistic_loglik_batched_sum for the Poisson family:
 *   loglik[k * n_beta + b] = sum_i y_i eta_i - exp(eta_i) - lgamma(y_i + 1),
 * eta_i = x_i . beta_b.  Same arguments, limits (P <= 512, 1 <= n_beta <= 16)
 * and fixed summation order.
 */
int dlsa_poisson_loglik_batched_sum(const double* X, const double* y,
                                    const int64_t* offsets, int32_t K, int32_t p,
                                    int32_t fit_intercept, const double* center,
                                    const double* scale, const double* betas,
                                    int32_t n_beta, double* loglik, double* loglik_sum,
                                    void* stream);

/*
 * dlsa_poisson_loglik_batched_sum with the per-row offset of
 * dlsa_poisson_fit_batched_offset: eta_i = x_i . beta_b + eta_offset_i for every
 * candidate (the constant lgamma(y + 1) is unchanged).  eta_offset [n_total]
 * fp64, device; NULL: exactly dlsa_poisson_loglik_batched_sum.
 */
int dlsa_poisson_loglik_batched_sum_offset(const double* X, const double* y,
                                           const double* eta_offset,
                                           const int64_t* offsets, int32_t K,
                                           int32_t p, int32_t fit_intercept,
                                           const double* center, const double* scale,
                                           const double* betas, int32_t n_beta,
                                           double* loglik, double* loglik_sum,
                                           void* stream);

/*
 * Per-row prior weights omega (R's glm(weights=), sample_weight /
 * freq_weights elsewhere) for the logistic and Poisson fits, per partition:
 *   eta and mu are unchanged; the IRLS weight is omega_i w_i, the score
 *   sum_i omega_i (y_i - mu_i) x_i, sig_inv = X^T diag(omega w) X at the
 *   returned theta, loglik = sum_i omega_i l_i with l_i the unweighted entry's
 *   per-row term (Poisson: including -omega_i lgamma(y_i + 1)).
 *  row_weight  [n_total] fp64, device, finite and >= 0; row i belongs to row i
 *              of X.  NULL: exactly the unweighted entry
 *              (dlsa_logistic_fit_batched_ex, dlsa_poisson_fit_batched_offset):
 *              the same kernels, bit-identical outputs.
 * omega_i = 0 drops the row from the fit, but its x and y must still be
 * finite: 0 * NaN is NaN, so a non-finite x ends the partition
 * DLSA_STATUS_NONFINITE as in the unweighted fit.
 * Logistic y is used as given: with y_i = s_i / m_i and omega_i = m_i this is
 * the grouped-binomial fit (s_i successes of m_i trials per row) without the
 * binomial-coefficient constant sum_i log C(m_i, s_i) in loglik.
 * All other arguments and the outputs as in the unweighted entries; eta_offset
 * of the Poisson entry may be NULL.  The weights are one more 8 B/row stream
 * of the passes; nothing per row is stored and the workspace
 * (dlsa_logistic_workspace_bytes) is unchanged.
 * Statuses, decided by one pass over omega before any Newton pass: a partition
 * with a negative or non-finite omega ends DLSA_STATUS_NONFINITE, one with
 * sum omega = 0 (Poisson: or sum omega y = 0) DLSA_STATUS_SINGULAR, both with
 * all-zero outputs; the other partitions are not affected.
 * Start point: logistic theta = 0; Poisson with an intercept theta =
 * (log(sum omega y / sum omega exp(eta_offset)), 0, ..., 0), the MLE of the
 * weighted intercept-only model, to which restarts go back.
 * Limits (each a follow-up):
 *   - the fused path only: P = p + intercept <= DLSA_MAX_P_FUSED (192), else
 *     DLSA_E_UNSUPPORTED before any launch (no weighted wide path);
 *   - the categorical-code layout takes weights through entries of its own,
 *     dlsa_logistic_fit_categorical_weighted and
 *     dlsa_logistic_loglik_categorical_weighted below (logistic only);
 *   - no weights for OLS (dlsa_ols_fit_batched);
 *   - no int8 exact pass: the exact passes of a weighted fit run on the fp64
 *     MFMA whatever opt->exact_pass says (the digit-grid bound of the int8
 *     pass relies on sqrt(w) <= 1/2, which omega breaks); dlsa_fit_stats
 *     passes_oz stays 0.
 */
int dlsa_logistic_fit_batched_weighted(const double* X, const double* y,
                                       const double* row_weight,
                                       const int64_t* offsets, int32_t K, int32_t p,
                                       int32_t fit_intercept, const double* center,
                                       const double* scale, int32_t max_iter,
                                       double tol, double* theta, double* sig_inv,
                                       double* sig_inv_theta, double* loglik,
                                       int32_t* iters, int32_t* status,
                                       const dlsa_fit_options* opt, void* stream);
int dlsa_poisson_fit_batched_weighted(const double* X, const double* y,
                                      const double* eta_offset,
                                      const double* row_weight,
                                      const int64_t* offsets, int32_t K, int32_t p,
                                      int32_t fit_intercept, const double* center,
                                      const double* scale, int32_t max_iter,
                                      double tol, double* theta, double* sig_inv,
                                      double* sig_inv_theta, double* loglik,
                                      int32_t* iters, int32_t* status,
                                      const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_logistic_loglik_batched_sum / dlsa_poisson_loglik_batched_sum_offset
 * with the prior weights of the weighted fits:
 *   loglik[k * n_beta + b] = sum_i omega_i l_ib
 * (Poisson: l_ib includes -lgamma(y_i + 1); eta_offset may be NULL).
 * row_weight [n_total] fp64, device; NULL: exactly the unweighted entry,
 * bit-identical.  The weights are not checked here: a non-finite omega makes
 * its partition's sums non-finite.  Same limits (P <= 512, 1 <= n_beta <= 16)
 * and fixed summation order; dense layout only.
 */
int dlsa_logistic_loglik_batched_sum_weighted(const double* X, const double* y,
                                              const double* row_weight,
                                              const int64_t* offsets, int32_t K,
                                              int32_t p, int32_t fit_intercept,
                                              const double* center, const double* scale,
                                              const double* betas, int32_t n_beta,
                                              double* loglik, double* loglik_sum,
                                              void* stream);
int dlsa_poisson_loglik_batched_sum_weighted(const double* X, const double* y,
                                             const double* eta_offset,
                                             const double* row_weight,
                                             const int64_t* offsets, int32_t K,
                                             int32_t p, int32_t fit_intercept,
                                             const double* center, const double* scale,
                                             const double* betas, int32_t n_beta,
                                             double* loglik, double* loglik_sum,
                                             void* stream);

/*
 * Batched local OLS fit (the linear DLSA path; the
 * reference only has a statsmodels per-group demo,
 * projects/results/linear_regression_dc.py:27-37):
 *   theta_k = (X_k^T X_k)^-1 X_k^T y_k,  Sig_inv_k = X_k^T X_k,
 *   sig_inv_theta_k = Sig_inv_k theta_k (= X_k^T y_k),
 *   rss_k = sum (y - X theta_k)^2.
 * One fp64 pass over X at theta = 0 (w = 1; P <= 64: X streamed straight
 * into the fp64-MFMA operands, ols_stream.hip; larger P: the logistic pass's
 * kernels with w = 1) plus one per-partition Cholesky solve.  opt may be
 * NULL; its hessian_mode is ignored (always fp64).
 */
int dlsa_ols_fit_batched(const double* X, const double* y, const int64_t* offsets,
                         int32_t K, int32_t p, int32_t fit_intercept,
                         const double* center, const double* scale, double* theta,
                         double* sig_inv, double* sig_inv_theta, double* rss,
                         int32_t* status, const dlsa_fit_options* opt,
                         void* stream);

/*
 * Log-likelihood evaluation pass -- replaces the per-partition body of
 * dlsa/models.py:151-225 logistic_model_eval (driven by dlsa/model_eval.py:
 * 10-42): for every partition k and candidate vector b (intercept first when
 * fit_intercept, standardised like the fit),
 *   loglik[k * n_beta + b] = sum_i y_i x_i.beta_b - log(1 + exp(x_i.beta_b)).
 * betas [n_beta, P] device, 1 <= n_beta <= 16, P <= 512; loglik [K, n_beta]
 * device.  One pass over X for all candidates; synchronises the stream.
 */
int dlsa_logistic_loglik_batched(const double* X, const double* y,
                                 const int64_t* offsets, int32_t K, int32_t p,
                                 int32_t fit_intercept, const double* center,
                                 const double* scale, const double* betas,
                                 int32_t n_beta, double* loglik, void* stream);

/*
 * Batched local logistic fit on a categorical-code layout -- the dummy branch
 * of dlsa/models.py:56-91 logistic_model() (airline design, BASELINE config
 * 3) without materialising the dummy matrix.  Row i of partition k holds
 *   Xn[i, 0:q]     q numeric columns (fp64, standardised by center/scale
 *                  [q] like models.py:99-101 -- dummies are never standardised)
 *   codes[i, 0:F]  one uint8 level code per factor f: 0 = the baseline level
 *                  (dropped, models.py:67/77), c in 1..levels[f]-1 = dummy
 *                  column c of factor f
 *   y[i]           0/1 label.
 * Parameters (P = fit_intercept + q + sum_f (levels[f] - 1) <= DLSA_MAX_P_FUSED):
 *   [intercept] [numeric 0..q-1] [factor 0 dummies 1..L0-1] [factor 1 ...] ...
 * The one-hot blocks of X^T W X are computed as weighted histograms in LDS
 * with int64 fixed-point bins: each term w, w x_i, y - mu is rounded once to
 * a power-of-two grid chosen per partition and column from the partition's
 * own max |x_i| (so that no bin can overflow), then summed exactly --
 * bit-identical run to run and within ~1e-13 of an fp64 sum relative to the
 * column's scale; the numeric x numeric block is fp64.  Outputs are as in
 * dlsa_logistic_fit_batched (theta,
 * Sig_inv = X^T W X of the dummy-expanded design at theta, ...).  A partition
 * in which some dummy column has no rows gets DLSA_STATUS_MISSING_LEVEL and
 * all-zero outputs, the reference's "fake zero matrix".  Codes >= levels[f]
 * fail the call with DLSA_E_INVALID.  Limits: F <= 16, levels[f] in 1..256,
 * fit_intercept + q <= 16.  Before any launch, F > 16 or a levels[f] outside
 * 1..256 is DLSA_E_INVALID, and P > DLSA_MAX_P_FUSED, fit_intercept + q > 16
 * or histograms that do not fit the LDS DLSA_E_UNSUPPORTED (no shape inside
 * the limits overflows the LDS: with one replica per histogram the largest,
 * 16 factors beside 13 numeric columns without an intercept, takes 153 240 of
 * the 163 840 bytes).
 * levels is a HOST array [F]; opt may be NULL
 * (hessian_mode is ignored: every pass is exact; warm_start runs a 1/16-prefix
 * level first only when the partitions average >= 2^19 rows).  Workspace:
 * there is no size query for this layout; opt->workspace is used when it is
 * large enough, and when it is NULL or too small the call allocates its own
 * (stream-ordered) instead of returning DLSA_E_WORKSPACE.
 */
int dlsa_logistic_fit_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                  const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                  const int32_t* levels, int32_t fit_intercept,
                                  const double* center, const double* scale,
                                  int32_t max_iter, double tol, double* theta,
                                  double* sig_inv, double* sig_inv_theta, double* loglik,
                                  int32_t* iters, int32_t* status,
                                  const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_logistic_fit_categorical with per-row prior weights omega, with the
 * semantics of dlsa_logistic_fit_batched_weighted per partition: the IRLS
 * weight is omega_i w_i, the score sum_i omega_i (y_i - mu_i) x_i, sig_inv =
 * X^T diag(omega w) X of the dummy-expanded design at the returned theta,
 * loglik = sum_i omega_i l_i.  A design made of factors collapses to its
 * distinct cells: rows (cell, s successes, m trials) with y = s / m and omega
 * = m give the MLE and sig_inv of the m-times replicated 0/1 rows.
 *  row_weight  [n_total] fp64, device, finite and >= 0.  NULL: exactly
 *              dlsa_logistic_fit_categorical, the same kernels and bits.
 * omega_i = 0 drops row i (its x and y must still be finite).
 * Statuses, decided before any Newton pass, each with all-zero outputs and
 * no effect on another partition: (1) a negative or non-finite omega ends the
 * partition DLSA_STATUS_NONFINITE; (2) sum omega = 0 DLSA_STATUS_SINGULAR;
 * (3) a partition still running gets DLSA_STATUS_MISSING_LEVEL when some dummy
 * column has no row with omega > 0 (rows with omega = 0 count as absent).  A
 * code >= levels[f] fails the call with DLSA_E_INVALID whatever its row's
 * weight.
 * Fixed-point bins: every bin term carries omega, so the partition's grids are
 * those of the unweighted fit divided by omega_max,k, its largest finite
 * weight (omega == 1: the unweighted grids).  The result stays bit-identical
 * run to run; a bin's rounding error relative to the column's scale is
 * ~1e-13 x omega_max / mean omega, and a huge weight coarsens only its own
 * partition's bins.  The weights are one more 8 B/row stream of every pass
 * (93 instead of 85 B/row at the airline shape).
 */
int dlsa_logistic_fit_categorical_weighted(const double* Xn, const uint8_t* codes,
                                           const double* y, const double* row_weight,
                                           const int64_t* offsets, int32_t K, int32_t q,
                                           int32_t F, const int32_t* levels,
                                           int32_t fit_intercept, const double* center,
                                           const double* scale, int32_t max_iter,
                                           double tol, double* theta, double* sig_inv,
                                           double* sig_inv_theta, double* loglik,
                                           int32_t* iters, int32_t* status,
                                           const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_logistic_loglik_batched with the job-level total of the reference's
 * second pass (the group-by sum of dlsa/model_eval.py:38):
 *   loglik_sum[b] = sum_k loglik[k * n_beta + b], k ascending, from one small
 * kernel (bit-identical run to run).  loglik_sum [n_beta] device or NULL.
 */
int dlsa_logistic_loglik_batched_sum(const double* X, const double* y,
                                     const int64_t* offsets, int32_t K, int32_t p,
                                     int32_t fit_intercept, const double* center,
                                     const double* scale, const double* betas,
                                     int32_t n_beta, double* loglik, double* loglik_sum,
                                     void* stream);

/*
 * Log-likelihood evaluation pass on the categorical-code layout of
 * dlsa_logistic_fit_categorical (Xn, codes, levels, center / scale of the
 * numeric columns, parameter order as there): for every partition k and
 * candidate b
 *   eta_i = beta_b[0] (intercept) + sum_j (x_ij - c_j) / s_j beta_b[ic + j]
 *           + sum_f (code_if > 0 ? beta_b[dummy column code_if of factor f] : 0)
 *   loglik[k * n_beta + b] = sum_i y_i eta_i - log(1 + exp(eta_i)),
 * the value dlsa_logistic_loglik_batched gives on the dummy-expanded design,
 * from 8 q + F + 8 bytes per row instead of 8 P + 8.  The dummy coefficients
 * are a table in LDS; no atomics: bit-identical run to run.  loglik_sum
 * [n_beta] (device or NULL) = sum_k loglik[k, .] in k order.  An empty
 * partition gives 0.  rows_per_chunk = 0: the plan's default.  Codes >=
 * levels[f] fail the call with DLSA_E_INVALID (they are never used as an
 * index).  Limits: F <= 16, levels[f] in 1..256, fit_intercept + q <= 16,
 * P <= DLSA_MAX_P, 1 <= n_beta <= 16.  levels is a HOST array [F]; betas
 * [n_beta, P] device.  Synchronises the stream.
 */
int dlsa_logistic_loglik_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                     const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                     const int32_t* levels, int32_t fit_intercept,
                                     const double* center, const double* scale,
                                     const double* betas, int32_t n_beta,
                                     int32_t rows_per_chunk, double* loglik,
                                     double* loglik_sum, void* stream);

/*
 * dlsa_logistic_loglik_categorical with the prior weights of
 * dlsa_logistic_fit_categorical_weighted:
 *   loglik[k * n_beta + b] = sum_i omega_i (y_i eta_i - log(1 + exp(eta_i))).
 * row_weight [n_total] fp64, device; NULL: exactly the unweighted entry,
 * bit-identical.  The weights are not checked here: a non-finite omega makes
 * its own partition's sums non-finite.  8 q + F + 16 bytes per row; same
 * limits and fixed summation order.
 */
int dlsa_logistic_loglik_categorical_weighted(const double* Xn, const uint8_t* codes,
                                              const double* y, const double* row_weight,
                                              const int64_t* offsets, int32_t K, int32_t q,
                                              int32_t F, const int32_t* levels,
                                              int32_t fit_intercept, const double* center,
                                              const double* scale, const double* betas,
                                              int32_t n_beta, int32_t rows_per_chunk,
                                              double* loglik, double* loglik_sum,
                                              void* stream);

/*
 * Poisson regression (log link) on the categorical-code layout of
 * dlsa_logistic_fit_categorical (Xn, codes, levels, parameter order, limits
 * and the missing-level rule as there): count data with an exposure on a
 * design made of factors -- a claim table -- from 8 q + F + 8 (+ 8 per row
 * extra) bytes per row.  Per partition exactly
 * dlsa_poisson_fit_batched_weighted on the dummy-expanded design: eta = x .
 * theta + eta_offset, mu = exp(eta), IRLS weight omega mu, sig_inv = X^T
 * diag(omega mu) X at the returned theta, loglik = sum omega (y eta - mu -
 * lgamma(y + 1)); the start point log(sum omega y / sum omega e^o) on the
 * intercept; a step that overshoots is halved.
 *  eta_offset  [n_total] fp64, device, finite; NULL: none.
 *  row_weight  [n_total] fp64, device, finite and >= 0 (0 drops the row);
 *              NULL: none.
 * Statuses, decided before any Newton pass, each with all-zero outputs: a
 * negative or non-finite y, eta_offset or omega DLSA_STATUS_NONFINITE; sum
 * omega = 0 or sum omega y = 0 DLSA_STATUS_SINGULAR; then, among the
 * partitions still running, a dummy column with no row of omega > 0
 * DLSA_STATUS_MISSING_LEVEL.  A code >= levels[f] fails the call.
 * Fixed-point bins: mu has no bound, so the partition's grids are sized on
 * the device before every pass from an upper bound on its rows' eta at that
 * pass's theta -- the smaller of an analytic bound (from theta, the columns'
 * ranges, the largest offset and omega_max) and one measured by the previous
 * pass (its largest omega mu, moved by the step); the residual's also covers
 * omega_max y_max: no term can overflow, the result is bit-identical run to run, and the pass
 * whose Hessian is returned follows a small step, so its grid is tight (bins
 * within ~1e-13 of an fp64 sum).  A pass for which no grid exists counts as an
 * overshoot.  opt->warm_start does not apply (a single plan level).
 */
int dlsa_poisson_fit_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                 const double* eta_offset, const double* row_weight,
                                 const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                 const int32_t* levels, int32_t fit_intercept,
                                 const double* center, const double* scale,
                                 int32_t max_iter, double tol, double* theta,
                                 double* sig_inv, double* sig_inv_theta, double* loglik,
                                 int32_t* iters, int32_t* status,
                                 const dlsa_fit_options* opt, void* stream);

/*
 * dlsa_logistic_loglik_categorical for the Poisson family:
 *   loglik[k * n_beta + b] = sum_i omega_i (y_i eta_i - exp(eta_i) - lgamma(y_i + 1)),
 * eta_i as there plus eta_offset_i; the value
 * dlsa_poisson_loglik_batched_sum_weighted gives on the dummy-expanded
 * design.  eta_offset, row_weight: [n_total] fp64, device, or NULL (o = 0,
 * omega = 1); neither is checked here.  Same limits and fixed summation order.
 */
int dlsa_poisson_loglik_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                    const double* eta_offset, const double* row_weight,
                                    const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                    const int32_t* levels, int32_t fit_intercept,
                                    const double* center, const double* scale,
                                    const double* betas, int32_t n_beta,
                                    int32_t rows_per_chunk, double* loglik,
                                    double* loglik_sum, void* stream);

/*
 * Goodness of fit of candidate coefficient vectors, one more evaluation pass
 * (the bytes per row, limits and scratch handling of the log-likelihood entry
 * of the same layout and row extras).  family: DLSA_FAMILY_LOGISTIC or
 * DLSA_FAMILY_POISSON, any other DLSA_E_UNSUPPORTED.  With mu_i the mean at
 * eta_i = x_i . beta (+ eta_offset_i) and omega_i the prior weight:
 *   deviance[k * n_beta + b] = sum_i d_i,   pearson[k * n_beta + b] = sum_i chi_i
 *   n_pos[k] = the rows of partition k with omega_i > 0 (all of them without
 *              weights), an exact integer in fp64
 *   Poisson:  d = 2 omega (y log(y / mu) - (y - mu)) (2 omega mu at y = 0),
 *             chi = omega (y - mu)^2 / mu
 *   logistic: d = 2 omega (y log y + (1 - y) log(1 - y) - (y eta - log(1 + exp(eta)))),
 *             0 log 0 = 0 (-2 omega l for 0/1 data),
 *             chi = omega (y - mu)^2 / (mu (1 - mu));
 *             y is taken as given in [0, 1] (a grouped row: y = s / m, omega =
 *             m) and not checked: outside it the sums are NaN.
 *   At a saturated eta each term takes its limit; for y in [0, 1] (logistic)
 *   and y >= 0 (Poisson) with omega > 0 no term is NaN.  Logistic, ea =
 *   exp(-|eta|): a row on its own side (y = 1 at eta >= 0, y = 0 below) has
 *   chi = omega ea, which is 0 once ea has underflowed (|eta| > 745.13); any
 *   other row's chi grows like 1 / ea and is +inf from there.  Poisson: at
 *   y = 0 chi = omega mu (0 once mu has underflowed, eta < -745.13), at y > 0
 *   over such a mu chi = +inf; from eta > 709.78, where mu overflows, chi and d
 *   are +inf.  (omega = 0 times such an infinity is NaN.)
 * eta_offset, row_weight: [n_total] fp64, device, or NULL; an offset with the
 * logistic family is DLSA_E_INVALID.  Neither is checked here.
 * betas, beta_part_stride: partition k is evaluated at the [n_beta, P] matrix
 * at betas + k * beta_part_stride -- 0: the same candidates for every
 * partition; P with n_beta = 1: betas is [K, P], each partition at its own
 * row (its own estimate).  Any other stride is DLSA_E_INVALID.
 * 1 <= n_beta <= DLSA_MAX_GOF_CANDIDATES.
 * sums: NULL, or [2 n_beta + 1] device: the sums over k of deviance, of
 * pearson and of n_pos, in that order.  Fixed summation order throughout: two
 * calls give the same bits.
 */
int dlsa_glm_gof_batched(int32_t family, const double* X, const double* y,
                         const double* eta_offset, const double* row_weight,
                         const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                         const double* center, const double* scale, const double* betas,
                         int32_t n_beta, int64_t beta_part_stride, double* deviance,
                         double* pearson, double* n_pos, double* sums, void* stream);

/*
 * Score outer products: one more pass over the dense layout (8 (p + 1) bytes
 * per row plus 8 per row extra, each streamed once) that gives, per partition
 * k at its coefficient vector beta_k, with eta_i = x_i . beta_k (+
 * eta_offset_i), mu_i the family's mean, omega_i the prior weight and
 * s_i = omega_i (y_i - mu_i):
 *   gram[k]  = sum_i d_i x_i x_i^T   [K, P, P], both triangles, exactly symmetric
 *   score[k] = sum_i s_i x_i         [K, P]
 *   kind DLSA_GRAM_SCORE:        d_i = s_i^2 -- the meat M_k of the sandwich
 *       (Huber-White, HC0) covariance A^-1 (sum_k M_k) A^-1; omega enters
 *       squared: precision / survey weights, not replicated rows
 *   kind DLSA_GRAM_INFORMATION:  d_i = omega_i w_i, w = mu (1 - mu) (logistic)
 *       or mu (Poisson) -- the information matrix (a fit's Sig_inv) at beta_k.
 * x_i is the standardised row ((x - center) / scale when both are given) with
 * the implicit intercept column first when fit_intercept is set.
 * family: DLSA_FAMILY_LOGISTIC or DLSA_FAMILY_POISSON, any other
 * DLSA_E_UNSUPPORTED; any other kind DLSA_E_INVALID.  eta_offset, row_weight:
 * [n_total] fp64, device, or NULL; an offset with the logistic family is
 * DLSA_E_INVALID.  Neither is checked here.
 * betas, beta_part_stride: partition k is evaluated at betas + k *
 * beta_part_stride -- 0: one [P] vector for every partition; P: betas is
 * [K, P], each partition at its own row.  Any other stride is DLSA_E_INVALID.
 * Limit: P = p + fit_intercept <= DLSA_MAX_P_FUSED (192), else
 * DLSA_E_UNSUPPORTED before any launch.  An empty partition gets zero blocks.
 * gram_sum [P, P], score_sum [P]: NULL, or the sums over k ascending.  The
 * chunk partials go to a stream-ordered scratch and are summed in chunk
 * order: two calls give the same bits.  fp64 throughout (v_mfma_f64_16x16x4).
 */
int dlsa_glm_gram_batched(int32_t family, int32_t kind, const double* X, const double* y,
                          const double* eta_offset, const double* row_weight,
                          const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                          const double* center, const double* scale, const double* betas,
                          int64_t beta_part_stride, double* gram, double* score,
                          double* gram_sum, double* score_sum, void* stream);
/* ... with the rows of a chunk (one workgroup's share of a partition) chosen
 * by the caller; rows_per_chunk = 0: automatic, as above.  The sums are taken
 * in chunk order, so their last bits depend on it. */
int dlsa_glm_gram_batched_chunked(int32_t family, int32_t kind, const double* X, const double* y,
                                  const double* eta_offset, const double* row_weight,
                                  const int64_t* offsets, int32_t K, int32_t p,
                                  int32_t fit_intercept, const double* center,
                                  const double* scale, const double* betas,
                                  int64_t beta_part_stride, int32_t rows_per_chunk, double* gram,
                                  double* score, double* gram_sum, double* score_sum,
                                  void* stream);

/*
 * Score outer products on the categorical-code layout (Xn [n, q] fp64, codes
 * [n, F] uint8, levels [F] on the host, as dlsa_logistic_fit_categorical
 * takes them): dlsa_glm_gram_batched_chunked's semantics on the dummy-expanded
 * design -- parameter order [intercept][q numeric][factor 0: levels 1..]...,
 * gram [K, P, P] both triangles and exactly symmetric, score [K, P], an empty
 * partition exact zeros, beta_part_stride 0 or P, gram_sum / score_sum NULL or
 * the sums over k ascending -- at 8 q + F + 8 bytes per row (plus 8 per row
 * extra), each streamed twice: a measuring sweep that sizes the fixed-point
 * grids of the histograms from the terms themselves, then the categorical
 * pass with the row weights (d_i, s_i) in place of the Newton pass's.
 * Limits and errors are the categorical fit's: P <= DLSA_MAX_P_FUSED,
 * intercept + q <= 16 and histograms that fit the LDS, else
 * DLSA_E_UNSUPPORTED; F <= 16 and levels[f] in 1..256, else DLSA_E_INVALID;
 * an offset with the logistic family, a kind or a stride
 * out of range DLSA_E_INVALID; a code >= levels[f] DLSA_E_INVALID, found by
 * the sweep before the gram pass is launched (the outputs are then not
 * written).  rows_per_chunk = 0: the categorical fit's chunk plan.
 * Each dummy row or column entry is a fixed-point sum: within n_k R 2^-60 B
 * of the fp64-exact sum in the worst case (n_k the partition's rows, R the
 * rows of its largest chunk, at least 1024, B the partition's largest term
 * of that entry's kind: |d|, |s| or |d x_j|); the numeric block is summed in
 * fp64.  Two calls give the same bits.  A partition with a term that is not
 * finite (a NaN weight, offset, y or x) gets an all-NaN gram and score; no
 * other partition is touched.
 */
int dlsa_glm_gram_categorical(int32_t family, int32_t kind, const double* Xn,
                              const uint8_t* codes, const double* y, const double* eta_offset,
                              const double* row_weight, const int64_t* offsets, int32_t K,
                              int32_t q, int32_t F, const int32_t* levels, int32_t fit_intercept,
                              const double* center, const double* scale, const double* betas,
                              int64_t beta_part_stride, int32_t rows_per_chunk, double* gram,
                              double* score, double* gram_sum, double* score_sum, void* stream);

/*
 * Row diagnostics: one more pass over the dense layout (8 (p + 1) bytes per
 * row plus 8 per row extra read, each once; 8 per requested output written)
 * that gives, per row i of partition k at its coefficient vector beta_k:
 *   eta[i]         x_i . beta_k (+ eta_offset_i)
 *   mu[i]          the family's mean
 *   dev_res[i]     sign(y_i - mu_i) sqrt(max(d_i, 0)), d_i the row's deviance
 *   pearson_res[i] sign(y_i - mu_i) sqrt(chi_i), chi_i the row's Pearson term
 *                  (the row terms of dlsa_glm_gof_batched, omega included)
 *   leverage[i]    h_i = omega_i w_i |R_k x_i|^2 = omega_i w_i x_i^T S_k^-1 x_i
 * with x_i, omega_i, w_i as in dlsa_glm_gram_batched.  rfac: the factor R_k,
 * [P, P] row-major, lower triangular (the upper triangle is read and must be
 * 0), R_k^T R_k = S_k^-1 -- the inverse of the Cholesky factor of S_k.
 * rfac_part_stride: 0 (one R for every partition) or P P (rfac is [K, P, P]);
 * betas, beta_part_stride as in dlsa_glm_gram_batched.  Any other stride is
 * DLSA_E_INVALID.  Each of the five outputs is [n_total] fp64, device, or
 * NULL (not computed); rfac may be NULL only if leverage is.  A non-finite
 * R_k gives NaN leverages in partition k alone.
 * family, eta_offset, row_weight, center / scale, the limit P <=
 * DLSA_MAX_P_FUSED and the error cases are dlsa_glm_gram_batched's, checked
 * before any launch.  An empty partition writes nothing.  Every value of a row
 * depends on that row, beta_k and R_k alone, in one summation order: the bits
 * are the same from call to call and for every rows_per_chunk.
 */
int dlsa_glm_rows_batched(int32_t family, const double* X, const double* y,
                          const double* eta_offset, const double* row_weight,
                          const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                          const double* center, const double* scale, const double* betas,
                          int64_t beta_part_stride, const double* rfac,
                          int64_t rfac_part_stride, double* eta, double* mu, double* dev_res,
                          double* pearson_res, double* leverage, void* stream);
/* ... with the rows of a chunk chosen by the caller; rows_per_chunk = 0:
 * automatic, as above. */
int dlsa_glm_rows_batched_chunked(int32_t family, const double* X, const double* y,
                                  const double* eta_offset, const double* row_weight,
                                  const int64_t* offsets, int32_t K, int32_t p,
                                  int32_t fit_intercept, const double* center,
                                  const double* scale, const double* betas,
                                  int64_t beta_part_stride, const double* rfac,
                                  int64_t rfac_part_stride, int32_t rows_per_chunk, double* eta,
                                  double* mu, double* dev_res, double* pearson_res,
                                  double* leverage, void* stream);

/*
 * dlsa_glm_gof_batched on the categorical-code layout of
 * dlsa_logistic_loglik_categorical (its arguments, limits and error cases: a
 * code >= levels[f] fails the call with DLSA_E_INVALID): the values the dense
 * entry gives on the dummy-expanded design.
 */
int dlsa_glm_gof_categorical(int32_t family, const double* Xn, const uint8_t* codes,
                             const double* y, const double* eta_offset,
                             const double* row_weight, const int64_t* offsets, int32_t K,
                             int32_t q, int32_t F, const int32_t* levels,
                             int32_t fit_intercept, const double* center, const double* scale,
                             const double* betas, int32_t n_beta, int64_t beta_part_stride,
                             int32_t rows_per_chunk, double* deviance, double* pearson,
                             double* n_pos, double* sums, void* stream);

/* Timing/iteration record of the calling thread's last fit. */
int dlsa_last_fit_stats(dlsa_fit_stats* out);

/*
 * Local pre-reduction of this device's partitions -- the group-sum of
 * dlsa/dlsa.py:30-34 (groupby('par_id').sum), done in HBM before the one
 * RCCL all-reduce that replaces the Spark shuffle + collect:
 *   out[0 : P*P]          = sum_k sig_inv[k]
 *   out[P*P : P*P+P]      = sum_k sig_inv_theta[k]
 *   out[P*P+P : P*P+2P]   = sum_k theta[k]
 *   out[P*P+2P]           = K   (partition count, for ONESHOT, dlsa.py:51-52)
 * Deterministic (fixed summation order over k).
 */
int dlsa_reduce_partitions(const double* sig_inv, const double* sig_inv_theta,
                           const double* theta, int32_t K, int32_t p,
                           double* out, void* stream);

/*
 * Row repartitioning in HBM -- replaces the Spark shuffle that groups rows by
 * partition before the map stage: `repartition(K, "partition_id")` + the
 * `groupby("partition_id").apply(udf)` of projects/logistic_dlsa.py:303-325,
 * with ids from monotonically_increasing_id() % K (:243-245) or a column.
 * A stable counting sort: rows of partition k land in output rows
 * offsets[k] .. offsets[k+1]-1 in their input order.
 *  part_id   [n] int32 device, every id in [0, K) (else DLSA_E_INVALID)
 *  src, dst, row_bytes  HOST arrays of n_arrays (<= 4) entries: device
 *            pointers of row-major arrays with row_bytes bytes per row (e.g.
 *            X [n, p] fp64 -> 8p, y -> 8, uint8 codes [n, F] -> F); dst must
 *            not overlap src
 *  offsets   [K+1] int64 HOST out (the layout every fit entry point takes)
 *  order     [n] int64 device out or NULL: input row of each output row
 * 1 <= K <= 16000.  Synchronises the stream (offsets are read back).
 */
int dlsa_partition_rows(const int32_t* part_id, int64_t n, int32_t K, int32_t n_arrays,
                        const void* const* src, void* const* dst, const int64_t* row_bytes,
                        int64_t* offsets, int64_t* order, void* stream);

/*
 * Column moments in HBM -- the device half of Spark's describe(), which the
 * reference runs over the whole data set to standardise every partition
 * with the global mean and stddev (projects/logistic_dlsa.py:287-298, read
 * by dlsa/models.py:99-101):
 *   out[0 p + j] = count, out[1 p + j] = mean, out[2 p + j] = M2 = sum (x - mean)^2,
 *   out[3 p + j] = min,   out[4 p + j] = max    of column j of X [n, p] (fp64,
 * row-major, device; out device [5 p]).  NaN entries are skipped (describe
 * ignores nulls); a column without values gets count 0 and NaN elsewhere.
 * Two passes over X (mean, then the squared deviations, compensated sums in
 * a fixed order: bit-identical run to run); stddev = sqrt(M2 / (count - 1)).
 * Partial moments of several shards combine exactly by Chan's formula
 * (dlsa_amd.ingest.merge_moments).  Scratch is allocated on the stream and
 * freed before return.
 */
int dlsa_column_moments(const double* X, int64_t n, int32_t p, double* out, void* stream);

/*
 * Synthetic logistic data in HBM (the input generator of SURVEY 8(d) for
 * configs too large for the host): X[i, j] = u(seed, row0 + i, j) - 0.5 with
 * u a counter-based (splitmix64) U[0,1) double; beta* = 1 on the first
 * floor(0.4 p) columns (dlsa/models.py:12-19); y ~ Bernoulli(sigmoid(X beta*))
 * drawn from an independent counter stream (models.py:23-30).  Rows are
 * written partition-contiguous; row0 offsets the counter so shards on
 * different GPUs draw disjoint rows.  Bit-exact with the numpy restatement
 * in oracle/ (simulate_counter).
 */
int dlsa_simulate_logistic(double* X, double* y, int64_t n, int32_t p,
                           uint64_t seed, int64_t row0, void* stream);

/*
 * LARS / adaptive-lasso path on the LSA quadratic form, HOST code --
 * replaces dlsa/lsa.py:90-212 lars_lsa (and R lars.lsa called from
 * dlsa/dlsa.py:77-80).  Sigma0 [P*P] row-major and b0 [P] are HOST arrays.
 * type: 0 = "lar", 1 = "lasso".  max_steps <= 0 means 8*m (lsa.py:116-117)
 * with m = P - intercept.  Outputs (HOST, caller-allocated for
 * max_steps+1 rows): beta [(max_steps+1) * m] row-major, beta0, aic, bic
 * [max_steps+1]; *n_steps = number of rows written (k+1).
 * Reference defects fixed: lsa.py:100 (intercept indexes range(1, n) with the
 * sample size), lsa.py:141-142 (singular back-out).
 */
int dlsa_lars_lsa(const double* Sigma0, const double* b0, int32_t P,
                  int32_t intercept, double n, int32_t type, double eps,
                  int32_t max_steps, double* beta, double* beta0, double* aic,
                  double* bic, int32_t* n_steps);

/* Thread-local message of the last failing call ("" if none). */
const char* dlsa_last_error(void);

/* Library build identification (gfx target, git-independent version). */
const char* dlsa_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* DLSA_HIP_H */
