// extern "C" entry points of libdlsa_hip.so (declared in include/dlsa_hip.h)
// and the short ones' host code.  The three batched fits are fit_fused.hip,
// fit_wide.hip and fit_cat.hip; their planning is fit_plan.hpp, what they
// share fit_driver.hpp.
#include <map>
#include <mutex>

#include "fit_driver.hpp"

namespace dlsa {

thread_local std::string g_last_error;
thread_local dlsa_fit_stats g_stats;

void set_error(const std::string& msg) { g_last_error = msg; }

hipError_t ensure_max_lds(const void* kernel, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> done;  // (kernel, device) -> bytes set
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find({kernel, dev});
  if (it != done.end() && it->second >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done[{kernel, dev}] = bytes;
  return e;
}

// A fit on dense X: the checks, then the fused or the wide path by P.
static int fit_dense(int family, const double* X, const double* y, const int64_t* offsets,
                     int32_t K, int32_t p, int32_t fit_intercept, const double* center,
                     const double* scale, int32_t max_iter, double tol, const FitOutputs& out,
                     const dlsa_fit_options* opt_in, void* stream,
                     const double* eta_offset = nullptr, const double* row_weight = nullptr) {
  DenseFit f{family, X, y, offsets, K, p, fit_intercept, center, scale, max_iter, tol, out,
             fit_begin(opt_in, stream), eta_offset, row_weight};
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  if (p < 0 || (p == 0 && !fit_intercept)) {
    set_error("p must be >= 1 (or 0 with an intercept)");
    return DLSA_E_INVALID;
  }
  const int P = p + (fit_intercept ? 1 : 0);
  const FamilyRules rules = family_rules(family);
  if (P > DLSA_MAX_P) {
    set_error("P = p + intercept > " + std::to_string(DLSA_MAX_P) + " is not supported");
    return DLSA_E_UNSUPPORTED;
  }
  if (P > rules.max_p) {  // (the Poisson family: fused path only)
    set_error("Poisson fit: P = p + intercept > DLSA_MAX_P_FUSED = " +
              std::to_string(DLSA_MAX_P_FUSED) + " is not supported");
    return DLSA_E_UNSUPPORTED;
  }
  if (row_weight && (!rules.weights || P > DLSA_MAX_P_FUSED)) {  // before any launch
    set_error("weighted fit: P = p + intercept > DLSA_MAX_P_FUSED = " +
              std::to_string(DLSA_MAX_P_FUSED) + " (the wide path) is not supported");
    return DLSA_E_UNSUPPORTED;
  }
  rc = check_fit_args(center, scale, out, f.max_iter, f.tol);
  if (rc != DLSA_OK) return rc;
  if (offsets[K] > 0 && (!X || !y)) {
    set_error("null X or y");
    return DLSA_E_INVALID;
  }
  if (!rules.iterates) f.max_iter = 1;  // closed form: one exact fp64 pass
  return P > DLSA_MAX_P_FUSED ? fit_wide(f) : fit_fused(f);
}

// The chunk tables of an evaluation pass, copied from the pageable plan
// (part: null when the pass does not read the chunks' partitions).
static hipError_t upload_eval_plan(const Plan& pl, int K, int64_t* d_row0, int32_t* d_rows,
                                   int32_t* d_part, int32_t* d_pcb, hipStream_t s) {
  hipError_t e = hipSuccess;
  auto up = [&](void* dst, const void* src, int64_t bytes) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  };
  if (pl.n_chunks > 0) {
    up(d_row0, pl.chunk_row0.data(), 8LL * pl.n_chunks);
    up(d_rows, pl.chunk_rows.data(), 4LL * pl.n_chunks);
    if (d_part) up(d_part, pl.chunk_part.data(), 4LL * pl.n_chunks);
  }
  up(d_pcb, pl.part_chunk_begin.data(), 4LL * (K + 1));
  return e;
}

}  // namespace dlsa

using namespace dlsa;

extern "C" {

void dlsa_fit_options_default(dlsa_fit_options* opt) {
  if (!opt) return;
  memset(opt, 0, sizeof(*opt));
  opt->hessian_mode = DLSA_HESSIAN_MIXED;
  opt->switch_tol = 1e-6;
  opt->warm_start = 1;
}

const char* dlsa_last_error(void) { return g_last_error.c_str(); }

const char* dlsa_build_info(void) {
  return "libdlsa_hip gfx950 (CDNA4): fused IRLS passes over an LDS-DMA ring (bf16 16x16x32 "
         "approximate Hessians; exact Hessians as int8 16x16x64 digit-slice sums or f64 "
         "16x16x4 MFMA), wide 128x128 Gram tiles, LDS Cholesky Newton update, host LARS";
}

int64_t dlsa_logistic_workspace_bytes(const int64_t* offsets, int32_t K, int32_t p,
                                      int32_t fit_intercept, int32_t rows_per_chunk) {
  if (check_offsets(offsets, K) != DLSA_OK) return -1;
  const int P = p + (fit_intercept ? 1 : 0);
  if (P > DLSA_MAX_P_FUSED)  // sized for the warm-start levels too (an upper bound)
    return make_wide_layout(wide_level_plans(offsets, K, p, fit_intercept, rows_per_chunk, true),
                            K, offsets[K], P)
        .total;
  Plan pl;
  make_plan(offsets, K, p, fit_intercept, rows_per_chunk, pl);
  return make_layout(pl, K).total;
}

int dlsa_last_fit_stats(dlsa_fit_stats* out) {
  if (!out) return DLSA_E_INVALID;
  *out = g_stats;
  return DLSA_OK;
}

int dlsa_logistic_fit_batched_ex(const double* X, const double* y, const int64_t* offsets,
                                 int32_t K, int32_t p, int32_t fit_intercept,
                                 const double* center, const double* scale, int32_t max_iter,
                                 double tol, double* theta, double* sig_inv,
                                 double* sig_inv_theta, double* loglik, int32_t* iters,
                                 int32_t* status, const dlsa_fit_options* opt, void* stream) {
  return fit_dense(FAMILY_LOGISTIC, X, y, offsets, K, p, fit_intercept, center, scale, max_iter,
                   tol, {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream);
}

int dlsa_poisson_fit_batched_ex(const double* X, const double* y, const int64_t* offsets,
                                int32_t K, int32_t p, int32_t fit_intercept,
                                const double* center, const double* scale, int32_t max_iter,
                                double tol, double* theta, double* sig_inv,
                                double* sig_inv_theta, double* loglik, int32_t* iters,
                                int32_t* status, const dlsa_fit_options* opt, void* stream) {
  return fit_dense(FAMILY_POISSON, X, y, offsets, K, p, fit_intercept, center, scale, max_iter,
                   tol, {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream);
}

int dlsa_poisson_fit_batched_offset(const double* X, const double* y, const double* eta_offset,
                                    const int64_t* offsets, int32_t K, int32_t p,
                                    int32_t fit_intercept, const double* center,
                                    const double* scale, int32_t max_iter, double tol,
                                    double* theta, double* sig_inv, double* sig_inv_theta,
                                    double* loglik, int32_t* iters, int32_t* status,
                                    const dlsa_fit_options* opt, void* stream) {
  return fit_dense(FAMILY_POISSON, X, y, offsets, K, p, fit_intercept, center, scale, max_iter,
                   tol, {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream,
                   eta_offset);
}

int dlsa_logistic_fit_batched_weighted(const double* X, const double* y, const double* row_weight,
                                       const int64_t* offsets, int32_t K, int32_t p,
                                       int32_t fit_intercept, const double* center,
                                       const double* scale, int32_t max_iter, double tol,
                                       double* theta, double* sig_inv, double* sig_inv_theta,
                                       double* loglik, int32_t* iters, int32_t* status,
                                       const dlsa_fit_options* opt, void* stream) {
  return fit_dense(FAMILY_LOGISTIC, X, y, offsets, K, p, fit_intercept, center, scale, max_iter,
                   tol, {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream,
                   nullptr, row_weight);
}

int dlsa_poisson_fit_batched_weighted(const double* X, const double* y, const double* eta_offset,
                                      const double* row_weight, const int64_t* offsets, int32_t K,
                                      int32_t p, int32_t fit_intercept, const double* center,
                                      const double* scale, int32_t max_iter, double tol,
                                      double* theta, double* sig_inv, double* sig_inv_theta,
                                      double* loglik, int32_t* iters, int32_t* status,
                                      const dlsa_fit_options* opt, void* stream) {
  return fit_dense(FAMILY_POISSON, X, y, offsets, K, p, fit_intercept, center, scale, max_iter,
                   tol, {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream,
                   eta_offset, row_weight);
}

int dlsa_logistic_fit_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                  const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                  const int32_t* levels, int32_t fit_intercept,
                                  const double* center, const double* scale, int32_t max_iter,
                                  double tol, double* theta, double* sig_inv,
                                  double* sig_inv_theta, double* loglik, int32_t* iters,
                                  int32_t* status, const dlsa_fit_options* opt, void* stream) {
  return fit_categorical(FAMILY_LOGISTIC, Xn, codes, y, nullptr, nullptr, offsets, K, q, F, levels,
                         fit_intercept, center, scale, max_iter, tol,
                         {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream);
}

int dlsa_logistic_fit_categorical_weighted(const double* Xn, const uint8_t* codes, const double* y,
                                           const double* row_weight, const int64_t* offsets,
                                           int32_t K, int32_t q, int32_t F, const int32_t* levels,
                                           int32_t fit_intercept, const double* center,
                                           const double* scale, int32_t max_iter, double tol,
                                           double* theta, double* sig_inv, double* sig_inv_theta,
                                           double* loglik, int32_t* iters, int32_t* status,
                                           const dlsa_fit_options* opt, void* stream) {
  return fit_categorical(FAMILY_LOGISTIC, Xn, codes, y, nullptr, row_weight, offsets, K, q, F,
                         levels, fit_intercept, center, scale, max_iter, tol,
                         {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream);
}

int dlsa_poisson_fit_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                 const double* eta_offset, const double* row_weight,
                                 const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                 const int32_t* levels, int32_t fit_intercept,
                                 const double* center, const double* scale, int32_t max_iter,
                                 double tol, double* theta, double* sig_inv,
                                 double* sig_inv_theta, double* loglik, int32_t* iters,
                                 int32_t* status, const dlsa_fit_options* opt, void* stream) {
  return fit_categorical(FAMILY_POISSON, Xn, codes, y, eta_offset, row_weight, offsets, K, q, F,
                         levels, fit_intercept, center, scale, max_iter, tol,
                         {theta, sig_inv, sig_inv_theta, loglik, iters, status}, opt, stream);
}

int dlsa_ols_fit_batched(const double* X, const double* y, const int64_t* offsets, int32_t K,
                         int32_t p, int32_t fit_intercept, const double* center,
                         const double* scale, double* theta, double* sig_inv,
                         double* sig_inv_theta, double* rss, int32_t* status,
                         const dlsa_fit_options* opt, void* stream) {
  dlsa_fit_options o;
  if (opt)
    o = *opt;
  else
    dlsa_fit_options_default(&o);
  o.hessian_mode = DLSA_HESSIAN_FP64;
  // the iteration count is always 1 for OLS and not part of this ABI: give
  // the driver a throw-away device array for it
  Workspace iters((hipStream_t)stream);
  if (K > 0)
    if (int rc = iters.alloc(sizeof(int32_t) * K)) return rc;
  return fit_dense(FAMILY_GAUSSIAN, X, y, offsets, K, p, fit_intercept, center, scale, 1, 1.0,
                   {theta, sig_inv, sig_inv_theta, rss, K > 0 ? (int32_t*)iters.at(0) : nullptr,
                    status},
                   &o, stream);
}

int dlsa_logistic_fit_batched(const double* X, const double* y, const int64_t* offsets,
                              int32_t K, int32_t p, int32_t fit_intercept, const double* center,
                              const double* scale, int32_t max_iter, double tol, double* theta,
                              double* sig_inv, double* sig_inv_theta, double* loglik,
                              int32_t* iters, int32_t* status, void* stream) {
  return dlsa_logistic_fit_batched_ex(X, y, offsets, K, p, fit_intercept, center, scale,
                                      max_iter, tol, theta, sig_inv, sig_inv_theta, loglik,
                                      iters, status, nullptr, stream);
}

// What a goodness-of-fit call has beside a log-likelihood call's arguments
// (whose `loglik` is then the deviance and whose `loglik_sum` is null).
struct GofCall {
  int64_t beta_part_stride;
  double* pearson;  // [K, n_beta]
  double* n_pos;    // [K]
  double* sums;     // null, or [2 n_beta + 1]: the sums over k of deviance, pearson, n_pos
};
// the family, stride and outputs of a goodness-of-fit entry
static int check_gof(const char* entry, int family, const double* eta_offset, int n_beta, int P,
                     double* deviance, const GofCall& g) {
  if (family != FAMILY_LOGISTIC && family != FAMILY_POISSON) {
    set_error(std::string(entry) + ": family must be DLSA_FAMILY_LOGISTIC or DLSA_FAMILY_POISSON");
    return DLSA_E_UNSUPPORTED;
  }
  if (eta_offset && family != FAMILY_POISSON) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  if (n_beta < 1 || n_beta > kGofMaxB || !deviance || !g.pearson || !g.n_pos ||
      !(g.beta_part_stride == 0 || (g.beta_part_stride == P && n_beta == 1))) {
    set_error(std::string(entry) + ": invalid arguments (1 <= n_beta <= " +
              std::to_string(kGofMaxB) + ", beta_part_stride 0, or P with n_beta = 1)");
    return DLSA_E_INVALID;
  }
  return DLSA_OK;
}
// the three reductions of a goodness-of-fit pass's chunk partials, fixed order
static hipError_t gof_reduce(const double* d_partial, const GofOut& go, const int32_t* d_pcb, int K,
                             int B, double* deviance, const GofCall& g, hipStream_t s) {
  hipError_t e = launch_loglik_reduce(d_partial, d_pcb, K, B, deviance, s);
  if (e == hipSuccess) e = launch_loglik_reduce(go.partial_chi, d_pcb, K, B, g.pearson, s);
  if (e == hipSuccess) e = launch_loglik_reduce(go.partial_npos, d_pcb, K, 1, g.n_pos, s);
  if (e != hipSuccess || !g.sums) return e;
  e = launch_loglik_total(deviance, K, B, g.sums, s);
  if (e == hipSuccess) e = launch_loglik_total(g.pearson, K, B, g.sums + B, s);
  if (e == hipSuccess) e = launch_loglik_total(g.n_pos, K, 1, g.sums + 2 * B, s);
  return e;
}

// (entry: the name the argument check reports; gof: the goodness-of-fit pass)
static int loglik_dense(int family, const char* entry, const double* X, const double* y,
                        const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                        const double* center,
                        const double* scale, const double* betas, int32_t n_beta,
                        double* loglik, double* loglik_sum, void* stream_,
                        const double* eta_offset = nullptr, const double* row_weight = nullptr,
                        const GofCall* gof = nullptr) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  const int P = p + (fit_intercept ? 1 : 0);
  if (p < 0 || P < 1 || P > 512 || n_beta < 1 || n_beta > 16 || !betas || !loglik ||
      (center == nullptr) != (scale == nullptr)) {
    set_error(std::string(entry) + ": invalid arguments (1 <= P <= 512, 1 <= n_beta <= 16)");
    return DLSA_E_INVALID;
  }
  if (gof) {
    rc = check_gof(entry, family, eta_offset, n_beta, P, loglik, *gof);
    if (rc != DLSA_OK) return rc;
  }
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!X || !y)) {
    set_error("null X or y");
    return DLSA_E_INVALID;
  }
  Plan pl;
  make_plan(offsets, K, p, fit_intercept, 0, pl);
  const int64_t nc = std::max(pl.n_chunks, 1);
  Bump b;
  const int64_t off_row0 = b.take(8 * nc), off_rows = b.take(4 * nc), off_part = b.take(4 * nc);
  const int64_t off_pcb = b.take(4LL * (K + 1)), off_partial = b.take(8 * nc * n_beta);
  const int64_t off_chi = gof ? b.take(8 * nc * n_beta) : 0, off_npos = gof ? b.take(8 * nc) : 0;
  Workspace ws(stream);
  rc = ws.alloc(b.o);
  if (rc != DLSA_OK) return rc;
  int64_t* d_row0 = (int64_t*)ws.at(off_row0);
  int32_t* d_rows = (int32_t*)ws.at(off_rows);
  int32_t* d_part = (int32_t*)ws.at(off_part);
  int32_t* d_pcb = (int32_t*)ws.at(off_pcb);
  double* d_partial = (double*)ws.at(off_partial);
  GofArgs ea;  // (each kernel takes its slice, launch_loglik_eval; launch_gof_eval all of it)
  memset(&ea, 0, sizeof(ea));
  if (gof) ea.gof = {(double*)ws.at(off_chi), (double*)ws.at(off_npos), gof->beta_part_stride};
  DLSA_HIP_TRY(upload_eval_plan(pl, K, d_row0, d_rows, d_part, d_pcb, stream));
  if (pl.n_chunks > 0) {
    ea.X = X;
    ea.y = y;
    ea.chunk_row0 = d_row0;
    ea.chunk_rows = d_rows;
    ea.chunk_part = d_part;
    ea.center = center;
    ea.scale = scale;
    ea.betas = betas;
    ea.partial = d_partial;
    ea.eta_offset = eta_offset;
    ea.row_weight = row_weight;
    ea.p = p;
    set_stream_bounds(ea, n_total);
    ea.P = P;
    ea.intercept = fit_intercept ? 1 : 0;
    ea.nbeta = n_beta;
    ea.slot_bytes = eval_slot_bytes(p, ex_count(pass_extras(ea)));
    const int PM = ((P + 7) / 8) * 8;
    const int budget = 160 * 1024 - (n_beta * PM + 2 * PM + 64) * 8;
    ea.nslot = std::max(2, std::min(budget / ea.slot_bytes, 6));
    DLSA_HIP_TRY(gof ? launch_gof_eval(ea, family, pl.n_chunks, stream)
                     : launch_loglik_eval(ea, family, pl.n_chunks, stream));
  }
  if (gof) {
    DLSA_HIP_TRY(gof_reduce(d_partial, ea.gof, d_pcb, K, n_beta, loglik, *gof, stream));
  } else {
    DLSA_HIP_TRY(launch_loglik_reduce(d_partial, d_pcb, K, n_beta, loglik, stream));
    if (loglik_sum) DLSA_HIP_TRY(launch_loglik_total(loglik, K, n_beta, loglik_sum, stream));
  }
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  return DLSA_OK;
}

int dlsa_logistic_loglik_batched(const double* X, const double* y, const int64_t* offsets,
                                 int32_t K, int32_t p, int32_t fit_intercept,
                                 const double* center, const double* scale,
                                 const double* betas, int32_t n_beta, double* loglik,
                                 void* stream) {
  return loglik_dense(FAMILY_LOGISTIC, "dlsa_logistic_loglik_batched", X, y, offsets, K, p,
                      fit_intercept, center, scale, betas,
                      n_beta, loglik, nullptr, stream);
}

int dlsa_logistic_loglik_batched_sum(const double* X, const double* y, const int64_t* offsets,
                                     int32_t K, int32_t p, int32_t fit_intercept,
                                     const double* center, const double* scale,
                                     const double* betas, int32_t n_beta, double* loglik,
                                     double* loglik_sum, void* stream) {
  return loglik_dense(FAMILY_LOGISTIC, "dlsa_logistic_loglik_batched", X, y, offsets, K, p,
                      fit_intercept, center, scale, betas,
                      n_beta, loglik, loglik_sum, stream);
}

int dlsa_poisson_loglik_batched_sum(const double* X, const double* y, const int64_t* offsets,
                                    int32_t K, int32_t p, int32_t fit_intercept,
                                    const double* center, const double* scale,
                                    const double* betas, int32_t n_beta, double* loglik,
                                    double* loglik_sum, void* stream) {
  return loglik_dense(FAMILY_POISSON, "dlsa_poisson_loglik_batched_sum", X, y, offsets, K, p,
                      fit_intercept, center, scale, betas,
                      n_beta, loglik, loglik_sum, stream);
}

int dlsa_poisson_loglik_batched_sum_offset(const double* X, const double* y,
                                           const double* eta_offset, const int64_t* offsets,
                                           int32_t K, int32_t p, int32_t fit_intercept,
                                           const double* center, const double* scale,
                                           const double* betas, int32_t n_beta, double* loglik,
                                           double* loglik_sum, void* stream) {
  return loglik_dense(FAMILY_POISSON, "dlsa_poisson_loglik_batched_sum", X, y, offsets, K, p,
                      fit_intercept, center, scale, betas,
                      n_beta, loglik, loglik_sum, stream, eta_offset);
}

int dlsa_logistic_loglik_batched_sum_weighted(const double* X, const double* y,
                                              const double* row_weight, const int64_t* offsets,
                                              int32_t K, int32_t p, int32_t fit_intercept,
                                              const double* center, const double* scale,
                                              const double* betas, int32_t n_beta, double* loglik,
                                              double* loglik_sum, void* stream) {
  return loglik_dense(FAMILY_LOGISTIC, "dlsa_logistic_loglik_batched_sum_weighted", X, y, offsets,
                      K, p, fit_intercept, center, scale, betas, n_beta, loglik, loglik_sum,
                      stream, nullptr, row_weight);
}

int dlsa_poisson_loglik_batched_sum_weighted(const double* X, const double* y,
                                             const double* eta_offset, const double* row_weight,
                                             const int64_t* offsets, int32_t K, int32_t p,
                                             int32_t fit_intercept, const double* center,
                                             const double* scale, const double* betas,
                                             int32_t n_beta, double* loglik, double* loglik_sum,
                                             void* stream) {
  return loglik_dense(FAMILY_POISSON, "dlsa_poisson_loglik_batched_sum_weighted", X, y, offsets, K,
                      p, fit_intercept, center, scale, betas, n_beta, loglik, loglik_sum, stream,
                      eta_offset, row_weight);
}

// (eta_offset: FAMILY_POISSON's per-row offset or null; row_weight: prior
// weights or null)
static int loglik_categorical(int family, const double* Xn, const uint8_t* codes, const double* y,
                              const double* eta_offset, const double* row_weight,
                              const int64_t* offsets, int32_t K,
                              int32_t q, int32_t F, const int32_t* levels, int32_t fit_intercept,
                              const double* center, const double* scale, const double* betas,
                              int32_t n_beta, int32_t rows_per_chunk, double* loglik,
                              double* loglik_sum, void* stream_, const GofCall* gof = nullptr) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  const int ic = fit_intercept ? 1 : 0;
  int D = 0, P = 0;
  rc = check_cat_shape(q, F, levels, ic, DLSA_MAX_P, "evaluation", &D, &P);
  if (rc != DLSA_OK) return rc;
  if (n_beta < 1 || n_beta > kEvalCatMaxB || rows_per_chunk < 0 || !betas || !loglik ||
      (center == nullptr) != (scale == nullptr)) {
    set_error(std::string(family == FAMILY_POISSON ? "dlsa_poisson_loglik_categorical"
                                                   : "dlsa_logistic_loglik_categorical") +
              ": invalid arguments (1 <= n_beta <= 16, "
              "rows_per_chunk >= 0, center and scale both or neither)");
    return DLSA_E_INVALID;
  }
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!y || (q > 0 && !Xn) || (F > 0 && !codes))) {
    set_error("null Xn, codes or y");
    return DLSA_E_INVALID;
  }
  const bool pois = family == FAMILY_POISSON;
  if (eta_offset && !pois) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  if (gof) {
    rc = check_gof("dlsa_glm_gof_categorical", family, eta_offset, n_beta, P, loglik, *gof);
    if (rc != DLSA_OK) return rc;
  }
  // (every kernel takes its slice: EvalCatArgs, EvalCatArgsWgt, EvalCatArgsPois or all)
  GofCatArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.q = q;
  ea.F = F;
  ea.P = P;
  ea.intercept = ic;
  ea.nbeta = n_beta;
  for (int f = 0, o = 0; f < F; ++f) {
    ea.levels[f] = levels[f];
    ea.toff[f] = o;
    o += levels[f];
  }
  if (!eval_cat_plan(ea, (eta_offset ? EX_OFS : 0) | (row_weight ? EX_WGT : 0))) {
    set_error("categorical evaluation: the coefficient table does not fit the LDS");
    return DLSA_E_UNSUPPORTED;
  }
  Plan pl;
  make_plan(offsets, K, q, ic, rows_per_chunk, pl);
  const int64_t nc = std::max(pl.n_chunks, 1);
  Bump b;
  const int64_t off_row0 = b.take(8 * nc), off_rows = b.take(4 * nc), off_bad = b.take(4 * nc);
  const int64_t off_pcb = b.take(4LL * (K + 1)), off_partial = b.take(8 * nc * n_beta);
  const int64_t off_part = gof ? b.take(4 * nc) : 0;  // (only the goodness-of-fit kernels read it)
  const int64_t off_chi = gof ? b.take(8 * nc * n_beta) : 0, off_npos = gof ? b.take(8 * nc) : 0;
  Workspace ws(stream);
  rc = ws.alloc(b.o);
  if (rc != DLSA_OK) return rc;
  int64_t* d_row0 = (int64_t*)ws.at(off_row0);
  int32_t* d_rows = (int32_t*)ws.at(off_rows);
  int32_t* d_bad = (int32_t*)ws.at(off_bad);
  int32_t* d_pcb = (int32_t*)ws.at(off_pcb);
  double* d_partial = (double*)ws.at(off_partial);
  int32_t* d_part = gof ? (int32_t*)ws.at(off_part) : nullptr;
  if (gof) ea.gof = {(double*)ws.at(off_chi), (double*)ws.at(off_npos), gof->beta_part_stride};
  DLSA_HIP_TRY(upload_eval_plan(pl, K, d_row0, d_rows, d_part, d_pcb, stream));
  std::vector<int32_t> h_bad(pl.n_chunks, 0);
  if (pl.n_chunks > 0) {
    ea.Xn = Xn;
    ea.codes = codes;
    ea.y = y;
    ea.chunk_row0 = d_row0;
    ea.chunk_rows = d_rows;
    ea.chunk_part = d_part;
    ea.center = center;
    ea.scale = scale;
    ea.betas = betas;
    ea.partial = d_partial;
    ea.bad = d_bad;
    if (q > 0) {
      ea.x_lo = ((uintptr_t)Xn + 15) & ~(uintptr_t)15;
      ea.x_hi = (uintptr_t)(Xn + n_total * (int64_t)q) & ~(uintptr_t)15;
    }
    if (F > 0) {
      ea.c_lo = ((uintptr_t)codes + 15) & ~(uintptr_t)15;
      ea.c_hi = (uintptr_t)(codes + n_total * (int64_t)F) & ~(uintptr_t)15;
    }
    ea.y_last4 = (uintptr_t)(y + n_total) - 4;
    ea.row_weight = row_weight;
    if (row_weight) ea.w_last4 = (uintptr_t)(row_weight + n_total) - 4;
    ea.eta_offset = eta_offset;
    if (eta_offset) ea.o_last4 = (uintptr_t)(eta_offset + n_total) - 4;
    if (gof)
      DLSA_HIP_TRY(pois ? launch_gof_cat_pois(ea, pl.n_chunks, stream)
                        : launch_gof_cat(ea, pl.n_chunks, stream));
    else
      DLSA_HIP_TRY(pois ? launch_loglik_cat_pois(ea, pl.n_chunks, stream)
                        : launch_loglik_cat(ea, pl.n_chunks, stream));
    DLSA_HIP_TRY(hipMemcpyAsync(h_bad.data(), d_bad, 4LL * pl.n_chunks, hipMemcpyDeviceToHost,
                                stream));
  }
  if (gof) {
    DLSA_HIP_TRY(gof_reduce(d_partial, ea.gof, d_pcb, K, n_beta, loglik, *gof, stream));
  } else {
    DLSA_HIP_TRY(launch_loglik_reduce(d_partial, d_pcb, K, n_beta, loglik, stream));
    if (loglik_sum) DLSA_HIP_TRY(launch_loglik_total(loglik, K, n_beta, loglik_sum, stream));
  }
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  for (int k = 0; k < K; ++k) {
    int64_t nbad = 0;
    for (int c = pl.part_chunk_begin[k]; c < pl.part_chunk_begin[k + 1]; ++c) nbad += h_bad[c];
    if (nbad) {
      set_error("partition " + std::to_string(k) + ": " + std::to_string(nbad) +
                " level codes >= levels[f]");
      return DLSA_E_INVALID;
    }
  }
  return DLSA_OK;
}

int dlsa_logistic_loglik_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                     const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                     const int32_t* levels, int32_t fit_intercept,
                                     const double* center, const double* scale,
                                     const double* betas, int32_t n_beta, int32_t rows_per_chunk,
                                     double* loglik, double* loglik_sum, void* stream) {
  return loglik_categorical(FAMILY_LOGISTIC, Xn, codes, y, nullptr, nullptr, offsets, K, q, F,
                            levels, fit_intercept,
                            center, scale, betas, n_beta, rows_per_chunk, loglik, loglik_sum,
                            stream);
}

int dlsa_logistic_loglik_categorical_weighted(const double* Xn, const uint8_t* codes,
                                              const double* y, const double* row_weight,
                                              const int64_t* offsets, int32_t K, int32_t q,
                                              int32_t F, const int32_t* levels,
                                              int32_t fit_intercept, const double* center,
                                              const double* scale, const double* betas,
                                              int32_t n_beta, int32_t rows_per_chunk,
                                              double* loglik, double* loglik_sum, void* stream) {
  return loglik_categorical(FAMILY_LOGISTIC, Xn, codes, y, nullptr, row_weight, offsets, K, q, F,
                            levels, fit_intercept, center, scale, betas, n_beta, rows_per_chunk,
                            loglik, loglik_sum, stream);
}

int dlsa_poisson_loglik_categorical(const double* Xn, const uint8_t* codes, const double* y,
                                    const double* eta_offset, const double* row_weight,
                                    const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                    const int32_t* levels, int32_t fit_intercept,
                                    const double* center, const double* scale,
                                    const double* betas, int32_t n_beta, int32_t rows_per_chunk,
                                    double* loglik, double* loglik_sum, void* stream) {
  return loglik_categorical(FAMILY_POISSON, Xn, codes, y, eta_offset, row_weight, offsets, K, q,
                            F, levels, fit_intercept, center, scale, betas, n_beta,
                            rows_per_chunk, loglik, loglik_sum, stream);
}

int dlsa_glm_gof_batched(int32_t family, const double* X, const double* y,
                         const double* eta_offset, const double* row_weight,
                         const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                         const double* center, const double* scale, const double* betas,
                         int32_t n_beta, int64_t beta_part_stride, double* deviance,
                         double* pearson, double* n_pos, double* sums, void* stream) {
  const GofCall gof{beta_part_stride, pearson, n_pos, sums};
  return loglik_dense(family, "dlsa_glm_gof_batched", X, y, offsets, K, p, fit_intercept, center,
                      scale, betas, n_beta, deviance, nullptr, stream, eta_offset, row_weight,
                      &gof);
}

static int gram_dense(int32_t family, int32_t kind, const double* X, const double* y,
                      const double* eta_offset, const double* row_weight, const int64_t* offsets,
                      int32_t K, int32_t p, int32_t fit_intercept, const double* center,
                      const double* scale, const double* betas, int64_t beta_part_stride,
                      int32_t rows_per_chunk, double* gram, double* score, double* gram_sum,
                      double* score_sum, void* stream_) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  if (family != FAMILY_LOGISTIC && family != FAMILY_POISSON) {
    set_error("dlsa_glm_gram_batched: family must be DLSA_FAMILY_LOGISTIC or DLSA_FAMILY_POISSON");
    return DLSA_E_UNSUPPORTED;
  }
  const int P = p + (fit_intercept ? 1 : 0);
  if (p < 0 || P < 1 || rows_per_chunk < 0 || !betas || !gram || !score ||
      (kind != GRAM_SCORE && kind != GRAM_INFORMATION) ||
      (center == nullptr) != (scale == nullptr)) {
    set_error("dlsa_glm_gram_batched: invalid arguments (P >= 1, kind DLSA_GRAM_SCORE or "
              "DLSA_GRAM_INFORMATION, center and scale both or neither)");
    return DLSA_E_INVALID;
  }
  if (P > DLSA_MAX_P_FUSED) {  // before any launch
    set_error("dlsa_glm_gram_batched: P = p + intercept > DLSA_MAX_P_FUSED = " +
              std::to_string(DLSA_MAX_P_FUSED) + " is not supported");
    return DLSA_E_UNSUPPORTED;
  }
  if (eta_offset && family != FAMILY_POISSON) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  if (beta_part_stride != 0 && beta_part_stride != P) {
    set_error("dlsa_glm_gram_batched: beta_part_stride must be 0 or P");
    return DLSA_E_INVALID;
  }
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!X || !y)) {
    set_error("null X or y");
    return DLSA_E_INVALID;
  }
  Plan pl;
  make_plan(offsets, K, p, fit_intercept, rows_per_chunk, pl);
  const int64_t nc = std::max(pl.n_chunks, 1);
  Bump b;
  const int64_t off_row0 = b.take(8 * nc), off_rows = b.take(4 * nc), off_part = b.take(4 * nc);
  const int64_t off_pcb = b.take(4LL * (K + 1));
  const int64_t off_G = b.take(8 * nc * pl.T * 256), off_s = b.take(8 * nc * pl.PP);
  Workspace ws(stream);
  rc = ws.alloc(b.o);
  if (rc != DLSA_OK) return rc;
  int64_t* d_row0 = (int64_t*)ws.at(off_row0);
  int32_t* d_rows = (int32_t*)ws.at(off_rows);
  int32_t* d_part = (int32_t*)ws.at(off_part);
  int32_t* d_pcb = (int32_t*)ws.at(off_pcb);
  GramArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.P = P;
  ga.slab_G = (double*)ws.at(off_G);
  ga.slab_s = (double*)ws.at(off_s);
  DLSA_HIP_TRY(upload_eval_plan(pl, K, d_row0, d_rows, d_part, d_pcb, stream));
  if (pl.n_chunks > 0) {
    ga.X = X;
    ga.y = y;
    ga.chunk_row0 = d_row0;
    ga.chunk_rows = d_rows;
    ga.chunk_part = d_part;
    ga.center = center;
    ga.scale = scale;
    ga.betas = betas;
    ga.eta_offset = eta_offset;
    ga.row_weight = row_weight;
    ga.p = p;
    set_stream_bounds(ga, n_total);
    ga.intercept = fit_intercept ? 1 : 0;
    ga.nbeta = 1;
    ga.beta_part_stride = beta_part_stride;
    ga.kind = kind;
    DLSA_HIP_TRY(launch_score_pass(ga, family, pl.n_chunks, stream));
  }
  DLSA_HIP_TRY(launch_gram_reduce(ga, d_pcb, K, gram, score, gram_sum, score_sum, stream));
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  return DLSA_OK;
}

int dlsa_glm_gram_batched(int32_t family, int32_t kind, const double* X, const double* y,
                          const double* eta_offset, const double* row_weight,
                          const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                          const double* center, const double* scale, const double* betas,
                          int64_t beta_part_stride, double* gram, double* score,
                          double* gram_sum, double* score_sum, void* stream) {
  return gram_dense(family, kind, X, y, eta_offset, row_weight, offsets, K, p, fit_intercept,
                    center, scale, betas, beta_part_stride, 0, gram, score, gram_sum, score_sum,
                    stream);
}

int dlsa_glm_gram_batched_chunked(int32_t family, int32_t kind, const double* X, const double* y,
                                  const double* eta_offset, const double* row_weight,
                                  const int64_t* offsets, int32_t K, int32_t p,
                                  int32_t fit_intercept, const double* center,
                                  const double* scale, const double* betas,
                                  int64_t beta_part_stride, int32_t rows_per_chunk, double* gram,
                                  double* score, double* gram_sum, double* score_sum,
                                  void* stream) {
  return gram_dense(family, kind, X, y, eta_offset, row_weight, offsets, K, p, fit_intercept,
                    center, scale, betas, beta_part_stride, rows_per_chunk, gram, score, gram_sum,
                    score_sum, stream);
}

static int rows_dense(int32_t family, const double* X, const double* y, const double* eta_offset,
                      const double* row_weight, const int64_t* offsets, int32_t K, int32_t p,
                      int32_t fit_intercept, const double* center, const double* scale,
                      const double* betas, int64_t beta_part_stride, const double* rfac,
                      int64_t rfac_part_stride, int32_t rows_per_chunk, double* eta, double* mu,
                      double* dev_res, double* pearson_res, double* leverage, void* stream_) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  if (family != FAMILY_LOGISTIC && family != FAMILY_POISSON) {
    set_error("dlsa_glm_rows_batched: family must be DLSA_FAMILY_LOGISTIC or DLSA_FAMILY_POISSON");
    return DLSA_E_UNSUPPORTED;
  }
  const int P = p + (fit_intercept ? 1 : 0);
  if (p < 0 || P < 1 || rows_per_chunk < 0 || !betas ||
      (center == nullptr) != (scale == nullptr)) {
    set_error("dlsa_glm_rows_batched: invalid arguments (P >= 1, rows_per_chunk >= 0, center "
              "and scale both or neither)");
    return DLSA_E_INVALID;
  }
  if (P > DLSA_MAX_P_FUSED) {  // before any launch
    set_error("dlsa_glm_rows_batched: P = p + intercept > DLSA_MAX_P_FUSED = " +
              std::to_string(DLSA_MAX_P_FUSED) + " is not supported");
    return DLSA_E_UNSUPPORTED;
  }
  if (eta_offset && family != FAMILY_POISSON) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  if (beta_part_stride != 0 && beta_part_stride != P) {
    set_error("dlsa_glm_rows_batched: beta_part_stride must be 0 or P");
    return DLSA_E_INVALID;
  }
  if (rfac_part_stride != 0 && rfac_part_stride != (int64_t)P * P) {
    set_error("dlsa_glm_rows_batched: rfac_part_stride must be 0 or P * P");
    return DLSA_E_INVALID;
  }
  if (leverage && !rfac) {
    set_error("dlsa_glm_rows_batched: leverage needs rfac");
    return DLSA_E_INVALID;
  }
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!X || !y)) {
    set_error("null X or y");
    return DLSA_E_INVALID;
  }
  Plan pl;
  make_plan(offsets, K, p, fit_intercept, rows_per_chunk, pl);
  if (pl.n_chunks == 0) return DLSA_OK;  // nothing to write
  const int64_t nc = pl.n_chunks;
  Bump b;
  const int64_t off_row0 = b.take(8 * nc), off_rows = b.take(4 * nc), off_part = b.take(4 * nc);
  const int64_t off_pcb = b.take(4LL * (K + 1));
  Workspace ws(stream);
  rc = ws.alloc(b.o);
  if (rc != DLSA_OK) return rc;
  int64_t* d_row0 = (int64_t*)ws.at(off_row0);
  int32_t* d_rows = (int32_t*)ws.at(off_rows);
  int32_t* d_part = (int32_t*)ws.at(off_part);
  int32_t* d_pcb = (int32_t*)ws.at(off_pcb);
  DLSA_HIP_TRY(upload_eval_plan(pl, K, d_row0, d_rows, d_part, d_pcb, stream));
  RowsArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.P = P;
  ra.X = X;
  ra.y = y;
  ra.chunk_row0 = d_row0;
  ra.chunk_rows = d_rows;
  ra.chunk_part = d_part;
  ra.center = center;
  ra.scale = scale;
  ra.betas = betas;
  ra.eta_offset = eta_offset;
  ra.row_weight = row_weight;
  ra.p = p;
  set_stream_bounds(ra, n_total);
  ra.intercept = fit_intercept ? 1 : 0;
  ra.nbeta = 1;
  ra.beta_part_stride = beta_part_stride;
  ra.rfac = rfac;
  ra.rfac_part_stride = rfac_part_stride;
  ra.eta = eta;
  ra.mu = mu;
  ra.dev_res = dev_res;
  ra.pearson_res = pearson_res;
  ra.leverage = leverage;
  DLSA_HIP_TRY(launch_rows_pass(ra, family, pl.n_chunks, stream));
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  return DLSA_OK;
}

int dlsa_glm_rows_batched(int32_t family, const double* X, const double* y,
                          const double* eta_offset, const double* row_weight,
                          const int64_t* offsets, int32_t K, int32_t p, int32_t fit_intercept,
                          const double* center, const double* scale, const double* betas,
                          int64_t beta_part_stride, const double* rfac,
                          int64_t rfac_part_stride, double* eta, double* mu, double* dev_res,
                          double* pearson_res, double* leverage, void* stream) {
  return rows_dense(family, X, y, eta_offset, row_weight, offsets, K, p, fit_intercept, center,
                    scale, betas, beta_part_stride, rfac, rfac_part_stride, 0, eta, mu, dev_res,
                    pearson_res, leverage, stream);
}

int dlsa_glm_rows_batched_chunked(int32_t family, const double* X, const double* y,
                                  const double* eta_offset, const double* row_weight,
                                  const int64_t* offsets, int32_t K, int32_t p,
                                  int32_t fit_intercept, const double* center,
                                  const double* scale, const double* betas,
                                  int64_t beta_part_stride, const double* rfac,
                                  int64_t rfac_part_stride, int32_t rows_per_chunk, double* eta,
                                  double* mu, double* dev_res, double* pearson_res,
                                  double* leverage, void* stream) {
  return rows_dense(family, X, y, eta_offset, row_weight, offsets, K, p, fit_intercept, center,
                    scale, betas, beta_part_stride, rfac, rfac_part_stride, rows_per_chunk, eta,
                    mu, dev_res, pearson_res, leverage, stream);
}

int dlsa_glm_gof_categorical(int32_t family, const double* Xn, const uint8_t* codes,
                             const double* y, const double* eta_offset,
                             const double* row_weight, const int64_t* offsets, int32_t K,
                             int32_t q, int32_t F, const int32_t* levels,
                             int32_t fit_intercept, const double* center, const double* scale,
                             const double* betas, int32_t n_beta, int64_t beta_part_stride,
                             int32_t rows_per_chunk, double* deviance, double* pearson,
                             double* n_pos, double* sums, void* stream) {
  const GofCall gof{beta_part_stride, pearson, n_pos, sums};
  return loglik_categorical(family, Xn, codes, y, eta_offset, row_weight, offsets, K, q, F, levels,
                            fit_intercept, center, scale, betas, n_beta, rows_per_chunk, deviance,
                            nullptr, stream, &gof);
}

int dlsa_partition_rows(const int32_t* part_id, int64_t n, int32_t K, int32_t n_arrays,
                        const void* const* src, void* const* dst, const int64_t* row_bytes,
                        int64_t* offsets, int64_t* order, void* stream_) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  if (K < 1 || K > kPartMaxK || n < 0 || n_arrays < 0 || n_arrays > kPartMaxArrays ||
      !offsets || (n_arrays > 0 && (!src || !dst || !row_bytes))) {
    set_error("dlsa_partition_rows: need 1 <= K <= " + std::to_string(kPartMaxK) +
              ", 0 <= n_arrays <= " + std::to_string(kPartMaxArrays) +
              ", host src/dst/row_bytes arrays and a host offsets[K+1]");
    return DLSA_E_INVALID;
  }
  for (int a = 0; a < n_arrays; ++a)
    if (row_bytes[a] < 1 || (n > 0 && (!src[a] || !dst[a]))) {
      set_error("dlsa_partition_rows: array " + std::to_string(a) + " has no rows or pointers");
      return DLSA_E_INVALID;
    }
  if (n == 0) {
    for (int k = 0; k <= K; ++k) offsets[k] = 0;
    return DLSA_OK;
  }
  if (!part_id) {
    set_error("dlsa_partition_rows: null part_id");
    return DLSA_E_INVALID;
  }
  // ~2048 blocks of input rows (block order = input order: stable)
  const int64_t rpb = std::max<int64_t>(kPartSubRows, (n + 2047) / 2048);
  const int nb = (int)((n + rpb - 1) / rpb);
  Bump b;
  const int64_t off_counts = b.take(4LL * nb * K), off_bad = b.take(4LL * nb);
  const int64_t off_tot = b.take(8LL * K), off_offs = b.take(8LL * (K + 1));
  Workspace ws(stream);
  if (int rc = ws.alloc(b.o)) return rc;
  int32_t* counts = (int32_t*)ws.at(off_counts);
  int32_t* bad = (int32_t*)ws.at(off_bad);
  int64_t* totals = (int64_t*)ws.at(off_tot);
  int64_t* offs_dev = (int64_t*)ws.at(off_offs);
  DLSA_HIP_TRY(launch_partition_rows(part_id, n, K, rpb, nb, counts, bad, totals, offs_dev,
                                     stream));
  std::vector<int32_t> h_bad(nb);
  DLSA_HIP_TRY(hipMemcpyAsync(h_bad.data(), bad, 4LL * nb, hipMemcpyDeviceToHost, stream));
  DLSA_HIP_TRY(hipMemcpyAsync(offsets, offs_dev, 8LL * (K + 1), hipMemcpyDeviceToHost, stream));
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  int64_t nbad = 0;
  for (int b = 0; b < nb; ++b) nbad += h_bad[b];
  if (nbad) {
    set_error("dlsa_partition_rows: " + std::to_string(nbad) + " partition ids outside [0, K)");
    return DLSA_E_INVALID;
  }
  for (int k = 0; k < K; ++k)
    if (offsets[k + 1] - offsets[k] > INT32_MAX) {
      set_error("dlsa_partition_rows: a partition has more than 2^31 - 1 rows");
      return DLSA_E_UNSUPPORTED;
    }
  DLSA_HIP_TRY(launch_partition_scatter(part_id, n, K, rpb, nb, counts, offs_dev, src, dst,
                                        row_bytes, n_arrays, order, stream));
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  return DLSA_OK;
}

int dlsa_reduce_partitions(const double* sig_inv, const double* sig_inv_theta,
                           const double* theta, int32_t K, int32_t p, double* out,
                           void* stream) {
  g_last_error.clear();
  if (K < 1 || p < 1 || !sig_inv || !sig_inv_theta || !theta || !out) {
    set_error("dlsa_reduce_partitions: invalid arguments");
    return DLSA_E_INVALID;
  }
  DLSA_HIP_TRY(launch_reduce_partitions(sig_inv, sig_inv_theta, theta, K, p, out,
                                        (hipStream_t)stream));
  return DLSA_OK;
}

int dlsa_column_moments(const double* X, int64_t n, int32_t p, double* out, void* stream_) {
  g_last_error.clear();
  if (n < 0 || p < 1 || (n > 0 && !X) || !out) {
    set_error("dlsa_column_moments: invalid arguments");
    return DLSA_E_INVALID;
  }
  hipStream_t stream = (hipStream_t)stream_;
  int G = 1;
  int64_t rpr = 1;
  column_moments_plan(n, p, &G, &rpr);
  double* ws = nullptr;
  DLSA_HIP_TRY(hipMallocAsync((void**)&ws, sizeof(double) * (5LL * G + 5) * p, stream));
  const hipError_t e = launch_column_moments(X, n, p, out, ws, G, rpr, stream);
  const hipError_t f = hipFreeAsync(ws, stream);
  DLSA_HIP_TRY(e);
  DLSA_HIP_TRY(f);
  return DLSA_OK;
}

int dlsa_simulate_logistic(double* X, double* y, int64_t n, int32_t p, uint64_t seed,
                           int64_t row0, void* stream) {
  g_last_error.clear();
  if (n < 0 || p < 1 || (n > 0 && (!X || !y))) {
    set_error("dlsa_simulate_logistic: invalid arguments");
    return DLSA_E_INVALID;
  }
  DLSA_HIP_TRY(launch_simulate(X, y, n, p, seed, row0, (hipStream_t)stream));
  return DLSA_OK;
}

}  // extern "C"
