// Internal declarations shared by the HIP translation units of libdlsa_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <utility>

#include "../../include/dlsa_hip.h"

namespace dlsa {

// Per-partition Newton phase.  MIXED fits start in PHASE_F32 (approximate
// Hessian at the fit's approximate precision: bf16 MFMA in MIXED, fp32 in
// MIXED_F32; fp64 gradient) and switch to PHASE_F64 for the pass whose
// Hessian is returned as Sig_inv; FP64 fits start in PHASE_F64.  A partition
// whose bf16-steered Newton stalls (or whose bf16 Hessian is not positive
// definite) escalates to PHASE_F32X (fp32-MFMA Hessian), then to PHASE_F64.
// PHASE_LEVEL_DONE: finished the current warm-start subsample level.
// counters[PHASE_F32 .. PHASE_F32X] count the partitions running per phase.
enum : int32_t {
  PHASE_F32 = 0,
  PHASE_F64 = 1,
  PHASE_F32X = 2,
  PHASE_DONE = 3,
  PHASE_LEVEL_DONE = 4,
  // host-set for one launch only: a PHASE_F64 partition whose max |z| record
  // is stale, routed to the fp64-MFMA exact pass beside an int8 pass of the
  // fresh ones (fit_fused.hip FusedFit::pass); restored to PHASE_F64 before the solve
  PHASE_F64_STALE = 5
};
constexpr int kRunPhases = 3;
enum : int32_t { STATUS_RUNNING = -1 };
// FAMILY_POISSON (log link): iterative like the logistic family; fused path only
enum : int32_t { FAMILY_LOGISTIC = 0, FAMILY_GAUSSIAN = 1, FAMILY_POISSON = 2 };

// What a family may launch: the one place the fits (capi.hip, fit_fused.hip,
// fit_wide.hip) and the pass launchers read it from, at run time or in
// `if constexpr`.
struct FamilyRules {
  // Newton to tol at the fit's Hessian mode; else one exact pass: PREC_F64
  // only, max_iter = 1, no warm-start levels, no polish
  bool iterates;
  // may record the digit scales (colmax / zcolmax) and take the int8 exact pass
  bool digit_scales;
  // fp64 passes sum the log-likelihood's constant term into slab_llc
  bool sums_ll_const;
  // starts from a device-computed point (launch_fit_prepass), which may end partitions
  bool device_start;
  // may carry a per-row eta_offset (the EX_OFS kernels, PassArgsOfs)
  bool offset;
  // may carry per-row prior weights (the EX_WGT kernels, PassArgsWgt): fused
  // path only, exact passes on the fp64 MFMA
  bool weights;
  int max_p;  // largest P = p + intercept
};
constexpr FamilyRules kLogisticRules = {true, true, false, false, false, true, DLSA_MAX_P};
constexpr FamilyRules kGaussianRules = {false, false, false, false, false, false, DLSA_MAX_P};
constexpr FamilyRules kPoissonRules = {true, false, true, true, true, true, DLSA_MAX_P_FUSED};
constexpr FamilyRules family_rules(int family) {
  return family == FAMILY_GAUSSIAN ? kGaussianRules
         : family == FAMILY_POISSON ? kPoissonRules
                                    : kLogisticRules;
}

// A compilation unit of a pass (irls_coop*.hip, irls_wave*.hip, irls_oz*.hip)
// instantiates the launchers of one set of families and one list of NT.
template <int... V>
struct IntList {
  static constexpr unsigned mask = ((1u << V) | ...);
};
typedef IntList<FAMILY_LOGISTIC> FamLogistic;
typedef IntList<FAMILY_LOGISTIC, FAMILY_GAUSSIAN> FamLogisticGaussian;
typedef IntList<FAMILY_POISSON> FamPoisson;
// f(integral_constant FAM, integral_constant NT) of the run-time (family, NT);
// hipErrorInvalidValue for a pair the unit does not hold
template <int... FAMS, int... NTS, typename F>
inline hipError_t unit_dispatch(IntList<FAMS...>, IntList<NTS...>, int family, int NT, F&& f) {
  hipError_t e = hipErrorInvalidValue;
  auto by_nt = [&](auto fam) {
    (void)((NT == NTS && ((e = f(fam, std::integral_constant<int, NTS>{})), true)) || ...);
  };
  (void)((family == FAMS && (by_nt(std::integral_constant<int, FAMS>{}), true)) || ...);
  return e;
}
// Row extras: the per-row 8-byte streams a pass reads beside X and y, a
// compile-time mask of its kernels.  Each extra streams like y: a
// bounds-checked buffer resource of its own over the chunk, one more LDS-DMA
// load of 256 B per 32-row block, placed behind y in the ring slot in bit
// order (the offset, then the weight).
enum : int { EX_NONE = 0, EX_OFS = 1, EX_WGT = 2 };
constexpr int ex_count(int ex) { return (ex & 1) + ((ex >> 1) & 1); }
// Row of a pass's routing table: the unit entry point that holds the
// instantiations of these families and this row-extras mask for NT in
// [nt_lo, nt_hi]
template <typename Fn>
struct UnitRow {
  unsigned families;  // IntList::mask
  int extras;         // EX_* mask
  int nt_lo, nt_hi;
  Fn* launch;
};
template <typename Fn, size_t N>
inline Fn* find_unit(const UnitRow<Fn> (&table)[N], int family, int extras, int NT) {
  for (const UnitRow<Fn>& r : table)
    if (((r.families >> family) & 1u) && r.extras == extras && NT >= r.nt_lo && NT <= r.nt_hi)
      return r.launch;
  return nullptr;
}

// Cache policy of the LDS-DMA loads that stream X (the aux / cpol operand of
// buffer_load ... lds; profiling builds override it, tools/build_variants.sh).
// The cooperative (but see DLSA_COOP_NT7_DMA_AUX) and per-wave passes keep
// the default policy: with nt (2) the lines their consecutive blocks share
// are fetched twice (PMC, run r04g:
// 842.6 vs 812.4 B/row for the config-2 bf16 pass, 624 vs 523 B/row for the
// config-4 OLS pass, whose blocks are 8 rows); the Ozaki exact pass streams
// non-temporally (813.6 vs 812.4 B/row, 17.6-18.0 vs 17.9-18.1 ms at config
// 2 in two A/B runs, profiles/r04g_dma_policy_ab.txt).
#ifndef DLSA_X_DMA_AUX
#define DLSA_X_DMA_AUX 0
#endif
#ifndef DLSA_OZ_DMA_AUX
#define DLSA_OZ_DMA_AUX 2
#endif
// The bf16 cooperative pass at NT = 7 (96 < P <= 112, the flagship's shape: a
// two-slot ring, one block in flight per workgroup) streams non-temporally as
// well: the re-fetched shared lines cost less than the policy gains there,
// 13.21-13.22 -> 12.91-12.93 ms per full config-2 pass in interleaved rounds.
// At the other shapes measured (p = 16, 50, 120, 140: deeper rings, one
// workgroup per CU or eight waves) nt is level or slower, up to +0.6 ms at
// p = 140, so they keep the default (profiles/r08a_coop_pipeline_ab.txt).
#ifndef DLSA_COOP_NT7_DMA_AUX
#define DLSA_COOP_NT7_DMA_AUX 2
#endif
// Cooperative pass: 4 (8) waves per workgroup, 32-row blocks.
constexpr int kCoopRows = 32;
// MFMA arithmetic of a pass's Hessian.
enum : int32_t { PREC_BF16 = 0, PREC_F32 = 1, PREC_F64 = 2 };

// Arguments of the fused IRLS pass (one workgroup = one chunk of one partition).
struct PassArgs {
  const double* X;            // [n_total, p]
  const double* y;            // [n_total]
  const int64_t* chunk_row0;  // [n_chunks] first global row of the chunk
  const int32_t* chunk_rows;  // [n_chunks]
  const int32_t* chunk_part;  // [n_chunks]
  const int32_t* phase;       // [K]
  const double* theta;        // [K, P] current iterate
  const double* center;       // [p] or null
  const double* scale;        // [p] or null
  double* slab_H;             // [n_chunks, T, 16, 16] partial X^T W X tiles
  double* slab_g;             // [n_chunks, 16*NT] partial X^T (y - mu)
  double* slab_ll;            // [n_chunks] partial log-likelihood
  uintptr_t x_last16;         // last 16-B aligned address whose 16 B are readable
  uintptr_t y_last4;          // last 4-B address inside y
  int32_t p;                  // columns of X
  int32_t P;                  // p + intercept
  int32_t intercept;
  int32_t want_phase;
  int32_t nslot;              // cooperative pass: LDS ring depth (32-row slots)
  int32_t slot_bytes;
  // Digit scales of the Ozaki exact pass (irls_oz_impl.hpp), written by the
  // bf16 passes of the final level when set:
  //   colmax  [n_chunks, 16*NT] per chunk and feature max |x| (the fp64 high
  //           dword, after standardisation)
  //   zcolmax [n_chunks, 16*NT] max |z|, z = sqrt(w) x at the pass's theta
  //           (fp32 bits)
  //   theta_rec [K, P] the theta of the partition's last recording pass
  uint32_t* colmax;
  uint32_t* zcolmax;
  const double* theta_rec;
  // null, or zcolmax is written only if zrec_gate[0] > 0: the near-switch
  // count of the solve before, for a pass enqueued before the host read it
  const int32_t* zrec_gate;
  int32_t waves;  // fp64 per-wave pass geometry (dlsa_fit_options.exact_waves; 0 = auto)
  // FAMILY_POISSON, fp64 passes: [n_chunks] partial sums of -lgamma(y + 1), the
  // log-likelihood's constant term.  slab_ll is the constant-free sum
  // y eta - mu in every pass (what the step halving compares); the constant
  // is added where loglik is published (newton_solve.hip)
  double* slab_llc;
};
// PassArgs of the cooperative and per-wave passes with the Poisson family's
// per-row offset: eta = x . theta + eta_offset.  The offset streams like y (a
// bounds-checked buffer resource of its own over the chunk, placed behind y
// in the ring slot).  Only the OFS instantiations take this struct as their
// kernel argument: growing PassArgs itself moved the register allocation of
// a dozen offset-free cooperative kernels (NT = 4, 9: up to +20 VGPRs), so
// every other kernel keeps the PassArgs it had.  The dispatchers
// (launch_irls_coop, launch_irls_wave) route on eta_offset != nullptr.
struct PassArgsOfs : PassArgs {
  const double* eta_offset;  // [n_total] or null (none)
  uintptr_t o_last4;         // last 4-B address inside eta_offset
};
// ... and with per-row prior weights omega (EX_WGT): IRLS weight omega w,
// score residual omega (y - mu), log-likelihood terms omega l_i.  Only the
// weighted instantiations take this struct, for the same reason; PassArgs
// and PassArgsOfs keep their size.  It is what the dispatchers are handed
// (every other kernel takes its slice).
struct PassArgsWgt : PassArgsOfs {
  const double* row_weight;  // [n_total] or null (none)
  uintptr_t w_last4;         // last 4-B address inside row_weight
};
template <int EX>
struct pass_args_of {
  typedef PassArgsWgt type;
};
template <>
struct pass_args_of<EX_NONE> {
  typedef PassArgs type;
};
template <>
struct pass_args_of<EX_OFS> {
  typedef PassArgsOfs type;
};
// the row-extras mask the dispatchers route on (A: PassArgsWgt or EvalArgsWgt)
template <typename A>
inline int pass_extras(const A& a) {
  return (a.eta_offset ? EX_OFS : 0) | (a.row_weight ? EX_WGT : 0);
}
// The bounds the LDS-DMA loads of a pass clamp their tail pieces to, so that
// none reads past an array: the last readable 16 B of X and the last 4 B of y
// and of each row extra the pass has (A: PassArgsWgt or EvalArgsWgt with X,
// y, eta_offset, row_weight and p set; zeros stand for n_total = 0).
template <typename A>
inline void set_stream_bounds(A& a, int64_t n_total) {
  if (n_total <= 0) return;
  const uintptr_t xend = (uintptr_t)(a.X + n_total * (int64_t)a.p);
  a.x_last16 = ((xend + 15) & ~(uintptr_t)15) - 16;
  a.y_last4 = (uintptr_t)(a.y + n_total) - 4;
  if (a.eta_offset) a.o_last4 = (uintptr_t)(a.eta_offset + n_total) - 4;
  if (a.row_weight) a.w_last4 = (uintptr_t)(a.row_weight + n_total) - 4;
}

// A/B knobs of profiling builds.  The product library reads no environment
// variable that changes a result (include/dlsa_hip.h): env_knob() is getenv
// only in builds compiled with -DDLSA_ENV_KNOBS=1 (tools/build_variants.sh).
#ifndef DLSA_ENV_KNOBS
#define DLSA_ENV_KNOBS 0
#endif
inline const char* env_knob(const char* name) {
#if DLSA_ENV_KNOBS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// ---- device helpers shared by the pass kernels --------------------------------
// Workgroup barrier for a block loop over an LDS-DMA ring: this wave's LDS
// reads/writes are complete (lgkmcnt(0)), then s_barrier.  Unlike
// __syncthreads() it carries no memory fence, whose lowering drains vmcnt to
// 0 -- that would wait for the LDS-DMA of the blocks still streaming in, i.e.
// empty the ring at every barrier.  The "memory" clobber keeps the compiler
// from moving LDS accesses across it; the DMA'd slot of a block is waited for
// by each wave's counted vmcnt before the first barrier that publishes it.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Buffer resource with every word made wave-uniform (readfirstlane), so the
// LDS-DMA loads take it in SGPRs: without this the compiler may keep it in
// VGPRs and wrap every buffer_load ... lds in a waterfall loop.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(uintptr_t base, uintptr_t bytes) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)base >> 32));
  const uint32_t nr = __builtin_amdgcn_readfirstlane(
      (uint32_t)(bytes < 0x7FFFFFF0u ? bytes : 0x7FFFFFF0u));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0, (int)nr,
                                           0x00020000);
}

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

// s_waitcnt vmcnt(N); wait_vmcnt_le<N>(n): vmcnt(min(n, N)) for a run-time n
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits on gfx950");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt_le(int n) {
  if constexpr (N <= 0) {
    wait_vmcnt<0>();
  } else {
    if (n >= N)
      wait_vmcnt<N>();
    else
      wait_vmcnt_le<N - 1>(n);
  }
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// chunk_row0[chunk] with both dwords wave-uniform (SGPRs)
__device__ __forceinline__ int64_t uniform_row0(const int64_t* chunk_row0, int chunk) {
  return ((int64_t)__builtin_amdgcn_readfirstlane((int)(chunk_row0[chunk] >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_row0[chunk]);
}

// (The ring zeroing and the center / 1/scale fill of the pass kernels are not
// helpers: as inlined functions they changed the register allocation of the
// standardising cooperative and per-wave kernels, tools/kernel_diff.py.)

// v of the lane that DPP control CTRL selects, both dwords
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// lgamma(y + 1) for y >= 0, the constant term of the Poisson log-likelihood.
// x = y + 1 is shifted up to z >= 8 by lgamma(x) = lgamma(x + n) - log(x (x + 1)
// ... (x + n - 1)) (n <= 7, the product <= 8!), then Stirling's series to
// z^-13 (the next term is < 1e-15 at z = 8).  Two logs, one division, no
// branches: about a fifth of the library lgamma's instructions and none of
// its registers (in the per-wave fp64 pass, whose accumulators fill the
// register file, the library call spilled ~100 VGPRs).  Absolute error
// ~1e-15 + a few ulps of the value (tests/test_cpu_poisson.py restates it);
// the terms are summed over rows, so that is what counts.
__host__ __device__ __forceinline__ double lgamma1p(double y) {
  double z = y + 1.0, pr = 1.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const bool up = z < 8.0;
    pr = up ? pr * z : pr;
    z = up ? z + 1.0 : z;
  }
  const double r = 1.0 / z, r2 = r * r;
  double s = 1.0 / 156.0;
  s = fma(s, r2, -691.0 / 360360.0);
  s = fma(s, r2, 1.0 / 1188.0);
  s = fma(s, r2, -1.0 / 1680.0);
  s = fma(s, r2, 1.0 / 1260.0);
  s = fma(s, r2, -1.0 / 360.0);
  s = fma(s, r2, 1.0 / 12.0);
  return fma(z - 0.5, log(z), -z) + 0.91893853320467274178 + s * r - log(pr);
}

// Arguments of the per-partition Newton update.
struct SolveArgs {
  const int32_t* part_chunk_begin;  // [K+1]
  const double* slab_H;
  const double* slab_g;
  const double* slab_ll;
  double* theta;        // [K, P] (in/out: the iterate, returned as coef)
  double* theta_prev;   // [K, P]
  double* delta_prev;   // [K, P]
  double* ll_prev;      // [K]
  int32_t* phase;       // [K]
  int32_t* backtracks;  // [K]
  int32_t* iters;       // [K]
  int32_t* status;      // [K]
  int32_t* counters;    // [4]: [kRunPhases] partitions still running per phase, [3] of the
                        // PHASE_F32 ones, those whose step was <= kOzNearTol (1 + max|theta|)
  double* dm_prev;      // [K] max |step| of the last approximate iteration (0: none)
  int32_t* stall;       // [K] consecutive stalled approximate iterations
  double* sig_inv;      // [K, P, P] out
  double* loglik;       // [K] out
  int32_t P;
  int32_t NT;
  int32_t family;  // FAMILY_LOGISTIC / FAMILY_POISSON: Newton to tol; FAMILY_GAUSSIAN: one exact step
  int32_t subsample;  // 1 on a warm-start level (row prefix of each partition)
  double tol;
  double switch_tol;
  double level_tol;   // warm-start level: stop when max|step| <= level_tol (1+max|theta|)
  int32_t escalate_to;  // next phase of a stalled PHASE_F32 partition (PHASE_F32X / PHASE_F64)
  int32_t eval_only;    // polish: publish Sig_inv / loglik at the current theta, no step
  // FAMILY_POISSON (null otherwise): slab_llc of the pass (PassArgs), and
  // theta0 [K], the start value of parameter 0 (log of the partition's mean y
  // with an intercept, else 0) a restarted partition goes back to
  double* slab_llc;
  const double* theta0;
};

// Step control of the Newton update (stall escalation, step halving,
// convergence): newton_step.hpp.
// An approximate iteration whose max |step| is below kOzNearTol (1 + max|theta|)
// is one or two iterations from the exact pass: the next bf16 pass records
// max |sqrt(w) x| for the Ozaki digit scales (fit_fused.hip, irls_oz_impl.hpp)
constexpr double kOzNearTol = 1e-2;

// Arguments of the log-likelihood evaluation pass.
struct EvalArgs {
  const double* X;
  const double* y;
  const int64_t* chunk_row0;
  const int32_t* chunk_rows;
  const int32_t* chunk_part;
  const double* center;  // [p] or null
  const double* scale;
  const double* betas;   // [nbeta, P]
  double* partial;       // [n_chunks, nbeta]
  uintptr_t x_last16;
  uintptr_t y_last4;
  int32_t p, P, intercept, nbeta;
  int32_t nslot, slot_bytes;
  // FAMILY_POISSON: per-row offset added to every candidate's eta (null: none)
  const double* eta_offset;
  uintptr_t o_last4;
};
// EvalArgs of the weighted instantiations (eval_pass_wgt.hip): every row's
// terms are multiplied by row_weight.  The unweighted kernels keep EvalArgs.
struct EvalArgsWgt : EvalArgs {
  const double* row_weight;  // [n_total]
  uintptr_t w_last4;
};
template <int EX>
struct eval_args_of {
  typedef typename std::conditional<(EX & EX_WGT) != 0, EvalArgsWgt, EvalArgs>::type type;
};
// Goodness-of-fit pass (gof_pass.hip, gof_cat_pass*.hip): the evaluation pass
// with two sums per candidate, the deviance (in `partial`) and the Pearson
// chi-square, and per chunk the count of rows with omega > 0.  Its kernels
// take these structs of their own, every row-extras mask alike; the
// log-likelihood kernels keep theirs.  Partition k reads its candidates at
// betas + k * beta_part_stride: 0, every partition the same [nbeta, P], or P
// with nbeta = 1, partition k at its own row of a [K, P] matrix.
constexpr int kGofMaxB = DLSA_MAX_GOF_CANDIDATES;
struct GofOut {
  double* partial_chi;   // [n_chunks, nbeta]
  double* partial_npos;  // [n_chunks]
  int64_t beta_part_stride;
};
struct GofArgs : EvalArgsWgt {
  GofOut gof;
};

// Score outer-product pass (score_pass_impl.hpp): per partition the weighted
// Gram sum_i d_i x_i x_i^T and the score sum_i s_i x_i at one coefficient
// vector per partition (betas + k * beta_part_stride, stride 0 or P; nbeta is
// 1 and `partial` unused).  Its kernels take this struct of their own; the
// row extras are run-time nullable pointers.
enum : int32_t { GRAM_SCORE = DLSA_GRAM_SCORE, GRAM_INFORMATION = DLSA_GRAM_INFORMATION };
struct GramArgs : EvalArgsWgt {
  int64_t beta_part_stride;
  int32_t kind;    // GRAM_SCORE: d = s^2; GRAM_INFORMATION: d = omega w
  double* slab_G;  // [n_chunks, T, 16, 16] partial lower-triangle tiles (the fit's slab layout)
  double* slab_s;  // [n_chunks, 16 NT] partial scores
};
// (sets nslot and slot_bytes itself)
hipError_t launch_score_pass(const GramArgs& a, int family, int n_chunks, hipStream_t s);
// gram[k] (both triangles) and score[k]: the sums of partition k's chunk
// partials in chunk order; then, where set, their sums over k ascending
hipError_t launch_gram_reduce(const GramArgs& a, const int32_t* pcb, int K, double* gram,
                              double* score, double* gram_sum, double* score_sum, hipStream_t s);

// Row diagnostics pass (rows_pass_impl.hpp): per row eta, mu, the signed
// deviance and Pearson residuals and the leverage omega w |R_k x|^2, at one
// coefficient vector (betas + k * beta_part_stride, stride 0 or P) and one
// lower-triangular factor R_k, R_k^T R_k = S_k^-1 (rfac + k * rfac_part_stride,
// stride 0 or P P), per partition.  Each output is [n_total] or null; rfac may
// be null only if leverage is.  No chunk partials: `partial` is unused.
struct RowsArgs : EvalArgsWgt {
  int64_t beta_part_stride;
  const double* rfac;
  int64_t rfac_part_stride;
  double *eta, *mu, *dev_res, *pearson_res, *leverage;
};
// (sets nslot and slot_bytes itself)
hipError_t launch_rows_pass(const RowsArgs& a, int family, int n_chunks, hipStream_t s);

// Wide-P path (DLSA_MAX_P_FUSED < P <= DLSA_MAX_P, wide_exact.hip): a row
// pass (eta, weights, gradient, log-lik) and a separate Gram pass over
// 128x128 output tiles of the padded PP = 128 * NB Hessian.
constexpr int kWideTile = 128;
struct WideArgs {
  const double* X;
  const double* y;
  const int64_t* rc_row0;  // row-pass chunks
  const int32_t* rc_rows;
  const int32_t* rc_part;
  const int64_t* gc_row0;  // Gram-pass row groups
  const int32_t* gc_rows;
  const int32_t* gc_part;
  const int32_t* phase;    // [K]
  const double* theta;     // [K, P]
  const double* center;    // [p] or null
  const double* scale;
  double* w;               // [n_total] IRLS weight of each row (row pass -> Gram pass)
  double* slab_g;          // [n_rchunks, PP] partial gradients
  double* slab_ll;         // [n_rchunks] partial log-likelihoods
  double* slab_G;          // [n_gchunks, TB, 128 * 128] partial Gram tiles
  double* slab_gz;         // [n_gchunks, PP] fused pass: partial gradients
  double* slab_llz;        // [n_gchunks] fused pass: partial log-likelihoods
  int32_t p, P, intercept;
  int32_t NB;              // 128-wide column blocks, PP = 128 NB
  int32_t n_gchunks;
  // int8 exact Gram (wide_oz.hip): the row pass's per-chunk max |sqrt(w) x|
  // (high dwords, [n_rchunks, PP]) when set
  uint32_t* slab_zmax;
};

// int8 exact Gram of the wide path (wide_oz.hip)
struct WideOzArgs {
  const int32_t* rcb;      // [K+1] row-pass chunks of each partition
  const uint32_t* zmax;    // [n_rchunks, PP] the row pass's max |sqrt(w) x| high dwords
  int32_t* E;              // [n_gchunks, PP] digit exponents of each Gram row group
  // digit records, part of the fit's workspace (WideLayout::off_digits):
  // [n_gchunks][maxblk][4 rowblocks][slice 0: PP x 16 B | slice 1: PP x 16 B |
  // slice 2: PP x 8 B] -- kWideOzRec bytes per (8 rows, feature)
  int8_t* D;
  int32_t maxblk;          // 32-row blocks of the largest Gram row group
};
hipError_t launch_wide_oz_scale(const WideArgs& a, const WideOzArgs& o, hipStream_t s);
hipError_t launch_wide_oz_digits(const WideArgs& a, const WideOzArgs& o, bool standardize,
                                 hipStream_t s);
hipError_t launch_wide_oz_gram(const WideArgs& a, const WideOzArgs& o, hipStream_t s);
constexpr int kWideOzMaxRows = 32767;  // int32 level sums of one row group
constexpr int kWideOzRec = 40;         // digit bytes per (8 rows, feature): 5 planes
// bytes of the digit records of a Gram plan with n_gchunks row groups of at
// most max_rows rows and PP padded features
inline int64_t wide_oz_digit_bytes(int n_gchunks, int max_rows, int PP) {
  const int64_t maxblk = (max_rows + 31) / 32;
  return (int64_t)(n_gchunks > 1 ? n_gchunks : 1) * maxblk * 4 * PP * kWideOzRec;
}

// Categorical-code pass (cat_pass.hip): q numeric fp64 columns + F uint8
// level codes per row; the one-hot blocks of X^T W X are LDS histograms.
constexpr int kCatMaxFactors = 16;
constexpr int kCatMaxPairs = kCatMaxFactors * (kCatMaxFactors - 1) / 2;
constexpr int kCatPMax = 192;  // P <= DLSA_MAX_P_FUSED (the Newton solve's limit)
constexpr int kCatQMax = 16;   // intercept + numeric columns
struct CatArgs {
  const double* Xn;           // [n_total, q] numeric columns
  const uint8_t* codes;       // [n_total, F] level codes (0 = baseline: no column)
  const double* y;            // [n_total]
  const int64_t* chunk_row0;
  const int32_t* chunk_rows;
  const int32_t* chunk_part;
  const int32_t* phase;
  const double* theta;        // [K, P]
  const double* center;       // [q] or null
  const double* scale;
  double* slab_H;             // same partial slab layout as PassArgs
  double* slab_g;
  double* slab_ll;
  int32_t q, F, P, intercept, NT, want_phase;
  int32_t hist_doubles;       // LDS histogram doubles
  int32_t nd_stride;          // 8-byte words per (replica, level) row of an nd histogram: q + 1
                              // rounded up to odd (the lanes' rows then fall on distinct banks)
  int32_t nlev[kCatMaxFactors];    // dummy columns of factor f (L_f - 1)
  int32_t nd_lev[kCatMaxFactors];  // level slots per replica of f's nd / gradient histograms:
                                   // nlev, + 1 for the fold factor (its baseline level)
  int32_t fold;                    // the exact-bucket kernel's fold factor, else -1: its
                                   // histograms also take the baseline level, so the
                                   // intercept row of X^T W X and gradient are the sums of
                                   // its levels (no register accumulators for them)
  int32_t doff[kCatMaxFactors];    // parameter index of factor f's first dummy
  int32_t nd_off[kCatMaxFactors];  // LDS: [rep][level slot][q + 1] (w, w x_0 ..; cat_slot)
  int32_t nd_rep[kCatMaxFactors];  // replicas (power of two)
  int32_t g_off[kCatMaxFactors];   // LDS: [rep][level slot] gradient
  int32_t pr_off[kCatMaxPairs];    // LDS: pair (f < g) [rep][nlev_f][nlev_g]
  int32_t pr_rep[kCatMaxPairs];
  // fixed-point scales of the int64 histograms per partition, device
  // [K][kCatQMax + 2] (powers of two: [0] w and the pair cells, [1] the
  // gradient residuals, [2 + i] w x_i of numeric column i)
  const double* hscale;
};
// CatArgs of the weighted instantiations (cat_pass_wgt.hip): every row's w,
// residual and log-likelihood term are multiplied by row_weight.  The
// unweighted kernels keep CatArgs (and its size: DESIGN 4.5e).
struct CatArgsWgt : CatArgs {
  const double* row_weight;  // [n_total] prior weights omega
  double* wmax;              // [n_chunks] the presence pass's max finite omega per chunk
};
template <bool WGT>
struct cat_args_of {
  typedef typename std::conditional<WGT, CatArgsWgt, CatArgs>::type type;
};
// CatArgs of the Poisson instantiations (cat_pass_pois*.hip), every row-extras
// mask alike: mu = exp(eta + eta_offset) is unbounded, so each pass also
// measures its largest mu per partition, from which the grids of the next pass
// are sized on the device (launch_cat_pois_grid).  CatArgs and CatArgsWgt keep
// their sizes.
struct CatArgsPois : CatArgsWgt {
  const double* eta_offset;   // [n_total] or null (the kernels without EX_OFS)
  double* slab_llc;           // [n_chunks] partial sums of -omega lgamma(y + 1)
  unsigned long long* mumax;  // [K] the pass's largest omega mu as bits (>= 0: ordered like its bits)
  double* ymax;               // [n_chunks] the presence pass's largest finite y
  double* omax;               // [n_chunks] ... and largest finite eta_offset (> 0, else 0)
};
// the kernel argument of a family's pass with row-extras mask RX
template <int FAM, int RX>
struct cat_pass_args_of {
  typedef typename std::conditional<FAM == FAMILY_POISSON, CatArgsPois,
                                    typename cat_args_of<(RX & EX_WGT) != 0>::type>::type type;
};

// Log-likelihood evaluation pass on the categorical-code layout
// (eval_cat_pass.hip): P <= DLSA_MAX_P, the other limits are the fit's.
constexpr int kEvalCatMaxB = 16;
struct EvalCatArgs {
  const double* Xn;           // [n_total, q]
  const uint8_t* codes;       // [n_total, F]
  const double* y;            // [n_total]
  const int64_t* chunk_row0;
  const int32_t* chunk_rows;
  const double* center;       // [q] or null
  const double* scale;
  const double* betas;        // [nbeta, P]
  double* partial;            // [n_chunks, nbeta]
  int32_t* bad;               // [n_chunks] codes >= levels[f] met in the chunk
  // LDS-DMA source windows: the whole 16-byte granules inside Xn / codes
  // ([lo, hi), both multiples of 16; empty: lo >= hi) and the last 4 bytes of y
  uintptr_t x_lo, x_hi, c_lo, c_hi, y_last4;
  int32_t q, F, P, intercept, nbeta;
  int32_t rb, nslot;          // rows per block, ring depth (eval_cat_plan)
  int32_t levels[kCatMaxFactors];
  int32_t toff[kCatMaxFactors];  // first table entry of factor f: sum of levels[0..f)
};
// EvalCatArgs of the weighted kernels: every row's term is multiplied by
// row_weight, one more 256-byte-piece stream behind y in the ring slot
struct EvalCatArgsWgt : EvalCatArgs {
  const double* row_weight;  // [n_total] or null (the unweighted kernels, which take EvalCatArgs)
  uintptr_t w_last4;         // last 4-B address inside row_weight
};
// ... of the Poisson kernels (eval_cat_pass_pois.hip), every mask alike: the
// per-row offset is one more 256-byte-piece stream, behind y and before omega
struct EvalCatArgsPois : EvalCatArgsWgt {
  const double* eta_offset;  // [n_total] or null
  uintptr_t o_last4;         // last 4-B address inside eta_offset
};
// sets rb and nslot (extras: the EX_* mask of the row extras the ring slot
// also holds); false: does not fit the LDS
bool eval_cat_plan(EvalCatArgs& a, int extras = EX_NONE);
// routes on a.row_weight; the unweighted kernels are handed the EvalCatArgs slice
hipError_t launch_loglik_cat(const EvalCatArgsWgt& a, int n_chunks, hipStream_t s);
// FAMILY_POISSON: routes on a.eta_offset and a.row_weight
hipError_t launch_loglik_cat_pois(const EvalCatArgsPois& a, int n_chunks, hipStream_t s);
hipError_t launch_loglik_total(const double* ll, int K, int B, double* out, hipStream_t s);
// ... of the goodness-of-fit kernels on this layout (GofArgs above), which
// also read their chunk's partition
struct GofCatArgs : EvalCatArgsPois {
  const int32_t* chunk_part;  // [n_chunks]
  GofOut gof;
};
// route on the family, a.eta_offset and a.row_weight (gof_cat_pass.hip the
// logistic kernels, gof_cat_pass_pois.hip the Poisson ones)
hipError_t launch_gof_cat(const GofCatArgs& a, int n_chunks, hipStream_t s);
hipError_t launch_gof_cat_pois(const GofCatArgs& a, int n_chunks, hipStream_t s);

// Row repartitioning (partition_rows.hip): stable counting sort by partition id.
constexpr int kPartMaxArrays = 4;
constexpr int kPartMaxK = 16000;    // LDS histogram / cursors
constexpr int kPartSubRows = 4096;  // rows ranked per scatter sub-block
hipError_t launch_partition_rows(const int32_t* pid, int64_t n, int K, int64_t rows_per_block,
                                 int nb, int32_t* counts, int32_t* bad, int64_t* totals,
                                 int64_t* offsets_dev, hipStream_t s);
hipError_t launch_partition_scatter(const int32_t* pid, int64_t n, int K, int64_t rows_per_block,
                                    int nb, const int32_t* base, const int64_t* offsets_dev,
                                    const void* const* src, void* const* dst,
                                    const int64_t* row_bytes, int n_arrays, int64_t* order,
                                    hipStream_t s);

// Launchers (defined in the .hip files).
hipError_t launch_cat_pass(const CatArgs& a, bool standardize, int n_chunks, hipStream_t s);
size_t cat_lds_bytes(const CatArgs& a);  // dynamic LDS of the pass
bool cat_exact_bucket(const CatArgs& a);  // the pass's exact-bucket kernel applies (fold factor)
constexpr int kCatStaticLds =  // its tables: factor and pair records, dummy offsets
    16 * (kCatMaxFactors + 1) + 16 * (kCatMaxPairs + 1) + 4 * kCatMaxFactors;
hipError_t launch_cat_presence(const CatArgs& a, int n_chunks, int32_t* counts, int32_t* bad,
                               double* colmax,
                               hipStream_t s);
hipError_t launch_cat_mark(const CatArgs& a, const int32_t* pcb, const int32_t* counts,
                           const int32_t* bad, int K, int32_t* phase, int32_t* status,
                           int32_t* bad_part, hipStream_t s);
// with prior weights (cat_pass_wgt.hip): the pass, and the presence pass whose
// level flags count rows with omega > 0 only and which also clears and fills
// a.wmax [n_chunks]
hipError_t launch_cat_pass_wgt(const CatArgsWgt& a, bool standardize, int n_chunks,
                               hipStream_t s);
hipError_t launch_cat_presence_wgt(const CatArgsWgt& a, int n_chunks, int32_t* counts,
                                   int32_t* bad, double* colmax, hipStream_t s);
// FAMILY_POISSON on the code layout (cat_pass_pois*.hip): one unit per
// row-extras mask RX holds its pass kernels and its presence kernel (row
// oriented like the weighted one; it also clears and fills a.ymax and, by RX,
// a.omax and a.wmax); the two launchers below route on a.eta_offset and
// a.row_weight.
template <int RX>
hipError_t launch_cat_pass_pois_unit(const CatArgsPois& a, bool standardize, int n_chunks,
                                     hipStream_t s);
template <int RX>
hipError_t launch_cat_presence_pois_unit(const CatArgsPois& a, int n_chunks, int32_t* counts,
                                         int32_t* bad, double* colmax, hipStream_t s);
hipError_t launch_cat_pass_pois(const CatArgsPois& a, bool standardize, int n_chunks,
                                hipStream_t s);
hipError_t launch_cat_presence_pois(const CatArgsPois& a, int n_chunks, int32_t* counts,
                                    int32_t* bad, double* colmax, hipStream_t s);
// The per-partition bounds the Poisson grids are sized from, fixed after the
// presence pass: bounds [K][kCatPoisBounds] = m~_j (the bound on the
// standardised column j) for j < kCatQMax, then o_max, omega_max, y_max.  Also
// puts theta[k][0] of a MISSING_LEVEL partition back to 0 (the pre-pass wrote
// the start point there before the mark kernel ended the partition).
constexpr int kCatPoisBounds = kCatQMax + 3;
hipError_t launch_cat_pois_bounds(const CatArgsPois& a, const int32_t* pcb, int K,
                                  const double* colmax, double* bounds, double* theta,
                                  const int32_t* status, hipStream_t s);
// Before every Poisson pass: the hscale row of each running partition from an
// upper bound on its rows' eta at the pass's theta, theta
// snapshotted into theta_snap [K, P] and a.mumax cleared for the pass.  rmax:
// the most rows of a chunk, at least 1024.  A partition no grid can serve
// gets hscale[0] = NaN: its pass publishes a non-finite log-likelihood.
hipError_t launch_cat_pois_grid(const CatArgsPois& a, int K, const double* bounds,
                                double* theta_snap, double* hscale, double rmax, hipStream_t s);
hipError_t launch_wide_row(const WideArgs& a, bool standardize, int family, int n_chunks,
                           hipStream_t s);
hipError_t launch_wide_gram(const WideArgs& a, bool standardize, hipStream_t s);
hipError_t launch_wide_fused(const WideArgs& a, bool standardize, hipStream_t s);
hipError_t launch_wide_assemble(const WideArgs& a, const int32_t* gcb, double* Hfull, int K,
                                hipStream_t s);
hipError_t launch_wide_newton(const SolveArgs& sa, const WideArgs& wa, const int32_t* rcb,
                              const int32_t* gcb, double* Hfull, int K, hipStream_t s);
int wide_newton_lds_bytes(int NB);
// routes on the row extras; each kernel is handed the slice of EvalArgsWgt it takes
hipError_t launch_loglik_eval(const EvalArgsWgt& a, int family, int n_chunks, hipStream_t s);
// the goodness-of-fit pass (gof_pass.hip): the same rules and routing
hipError_t launch_gof_eval(const GofArgs& a, int family, int n_chunks, hipStream_t s);
hipError_t launch_loglik_reduce(const double* partial, const int32_t* pcb, int K, int B,
                                double* out, hipStream_t s);
int eval_slot_bytes(int p, int n_extras = 0);  // + 256 B per row extra behind y
// per-wave fp64 pass (irls_wave_impl.hpp): P <= 128
hipError_t launch_irls_wave(const PassArgsWgt& a, int NT, bool standardize, int family,
                            int n_chunks, hipStream_t s);
int wave_lds_bytes(int NT, int p);
constexpr int kWaveMaxNT = 8;
// Ozaki-scheme exact pass (irls_oz_impl.hpp): NT <= kOzMaxNT, chunks <= kOzMaxRows rows;
// a.nslot = oz_nslot(NT, p) ring slots
hipError_t launch_irls_oz(const PassArgs& a, int NT, bool standardize, int family, int n_chunks,
                          hipStream_t s);
bool oz_applies(int NT, int p);  // NT <= kOzMaxNT, image and 6-slot ring fit
constexpr int kOzMaxRows = 32767;
constexpr int kOzMaxNT = 7;
// OLS pass at theta = 0 streaming X into the MFMA operand registers
// (ols_stream.hip), P <= 64
bool ols_stream_applies(int NT);
hipError_t launch_ols_stream(const PassArgs& a, int NT, bool standardize, int n_chunks,
                             hipStream_t s);
hipError_t launch_irls_coop(const PassArgsWgt& a, int NT, int prec, bool standardize, int family,
                            int n_chunks, hipStream_t s);
// the ring slot of a launch over X (coop_slot, irls_coop_impl.hpp: a KiB less
// where every block starts 16-byte aligned and p % 4 == 0); + 256 B per row
// extra behind y
int coop_slot_bytes(int NT, const double* X, int p, int n_extras = 0);
int coop_extra_bytes(int NT);  // LDS beyond the ring
hipError_t launch_newton_solve(const SolveArgs& a, int K, hipStream_t s);
hipError_t launch_fit_init(const int64_t* offsets_dev, int K, int P, int start_phase,
                           double* theta, int32_t* phase, int32_t* backtracks,
                           int32_t* iters, int32_t* status, double* ll_prev,
                           double* sig_inv, double* loglik, hipStream_t s);
hipError_t launch_level_reset(int K, int P, int start_phase, int32_t* phase, int32_t* status,
                              double* ll_prev, int32_t* backtracks, double* theta,
                              int32_t* counters, hipStream_t s, const double* theta0 = nullptr);
// Pre-pass of a fit (aux_kernels.hip), after fit_init, for a family with a
// device start (Poisson) or a fit with prior weights omega: per partition one
// fixed-order pass over y, eta_offset and row_weight (either may be null:
// o = 0, omega = 1).  A negative or non-finite y, o or omega ends the
// partition NONFINITE, sum omega = 0 or (Poisson) sum omega y = 0 SINGULAR, a
// sum omega exp(o) that is not finite and positive NONFINITE (phase
// PHASE_DONE, outputs left zeroed by fit_init); nothing per row is stored.
// Poisson: theta0[k] = log(sum omega y / sum omega exp(o)) with an intercept,
// else 0, written to theta[k][0] too.  Logistic: statuses only (the weight
// check); theta and theta0 are not touched.  A no-op for any other fit
hipError_t launch_fit_prepass(int family, const double* y, const double* eta_offset,
                              const double* row_weight, const int64_t* offsets_dev, int K, int P,
                              int intercept, double* theta, double* theta0, int32_t* phase,
                              int32_t* status, hipStream_t s);
hipError_t launch_polish_mark(int K, int32_t* phase, const int32_t* status, int32_t* counters,
                              hipStream_t s);
// theta_rec[k] = theta[k] for the partitions in phase `ph` (before a pass
// that records the Ozaki digit scales)
hipError_t launch_theta_snapshot(int K, int P, const int32_t* phase, int ph, const double* theta,
                                 double* theta_rec, hipStream_t s, const int32_t* gate = nullptr);
hipError_t launch_fit_finalize(int K, int P, const double* theta, const double* sig_inv,
                               double* sig_inv_theta, int32_t* status, hipStream_t s);
hipError_t launch_reduce_partitions(const double* sig_inv, const double* sig_inv_theta,
                                    const double* theta, int K, int P, double* out,
                                    hipStream_t s);
hipError_t launch_simulate(double* X, double* y, int64_t n, int p, uint64_t seed,
                           int64_t row0, hipStream_t s);

// Column moments (moments.hip): out [5, p] = count, mean, M2, min, max; ws
// holds (5 G + 5) p doubles.
hipError_t launch_column_moments(const double* X, int64_t n, int p, double* out, double* ws,
                                 int G, int64_t rows_per_range, hipStream_t s);
void column_moments_plan(int64_t n, int p, int* G, int64_t* rows_per_range);

// The calling thread's last error text and last fit's statistics (capi.hip).
extern thread_local std::string g_last_error;
extern thread_local dlsa_fit_stats g_stats;
void set_error(const std::string& msg);

// Raise a kernel's dynamic-LDS limit to `bytes` once per (kernel, device):
// thread-safe (one process may drive several GPUs from several threads).
hipError_t ensure_max_lds(const void* kernel, int bytes);

}  // namespace dlsa
