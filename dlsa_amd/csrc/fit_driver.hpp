// Scaffolding shared by the three batched Newton fits (fit_fused.hip,
// fit_wide.hip, fit_cat.hip) and the short entry points of capi.hip: the
// device workspace, the pinned staging, the event timer and the steps every
// fit takes around its own passes (prologue, Newton-state arguments, level
// entry, counter readback, epilogue).
#pragma once

#include <stdio.h>
#include <string.h>

#include <chrono>

#include "fit_plan.hpp"

namespace dlsa {

#define DLSA_HIP_TRY(expr)                                                            \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
      return DLSA_E_HIP;                                                              \
    }                                                                                 \
  } while (0)

// What a Workspace does with a caller's buffer that is missing or too small.
enum class WsPolicy {
  kCallerMustFit,  // missing: allocate; too small: DLSA_E_WORKSPACE
  kOwnIfSmall      // missing or too small: allocate
};

// The device buffer of one call: the caller's or one from hipMallocAsync on
// the call's stream, which the destructor hands back (hipFreeAsync) on every
// return path.
class Workspace {
 public:
  explicit Workspace(hipStream_t s) : s_(s) {}
  Workspace(const Workspace&) = delete;
  Workspace& operator=(const Workspace&) = delete;
  ~Workspace() {
    if (owned_ && p_) (void)hipFreeAsync(p_, s_);
  }
  // `need` bytes by `policy`; a too-small caller buffer is reported as
  // needing `report` bytes (the wide fit asks for more than it requires)
  int acquire(void* caller, int64_t caller_bytes, int64_t need, WsPolicy policy,
              int64_t report = -1) {
    if (caller && caller_bytes >= need) {
      p_ = (char*)caller;
      return DLSA_OK;
    }
    if (caller && policy == WsPolicy::kCallerMustFit) {
      set_error("workspace too small: need " + std::to_string(report < 0 ? need : report) +
                " bytes");
      return DLSA_E_WORKSPACE;
    }
    const hipError_t e = hipMallocAsync((void**)&p_, need, s_);
    if (e != hipSuccess) {
      p_ = nullptr;
      set_error(std::string("hipMallocAsync: ") + hipGetErrorString(e));
      return DLSA_E_HIP;
    }
    owned_ = true;
    return DLSA_OK;
  }
  int alloc(int64_t bytes) { return acquire(nullptr, 0, bytes, WsPolicy::kOwnIfSmall); }
  // `need` bytes if they can be had: false (and no error) when the caller's
  // buffer is smaller or the allocation fails
  bool try_acquire(void* caller, int64_t caller_bytes, int64_t need) {
    if (caller) {
      if (caller_bytes >= need) p_ = (char*)caller;
      return p_ != nullptr;
    }
    if (hipMallocAsync((void**)&p_, need, s_) != hipSuccess) {
      (void)hipGetLastError();  // out of memory: not this call's error
      p_ = nullptr;
      return false;
    }
    owned_ = true;
    return true;
  }
  explicit operator bool() const { return p_ != nullptr; }
  void* at(int64_t off) const { return (void*)(p_ + off); }

 private:
  char* p_ = nullptr;
  bool owned_ = false;
  hipStream_t s_;
};

// Pinned host staging of the per-iteration readbacks (running counters +
// phases), grown on demand and kept for the thread's lifetime: a
// hipHostMalloc / hipHostFree pair per fit costs a pinning call (and the free
// an implicit synchronisation) on every call.  Never freed: the process exit
// reclaims it (a thread_local destructor could run after the HIP runtime's).
inline int32_t* pinned_staging(size_t n_i32) {
  thread_local int32_t* buf = nullptr;
  thread_local size_t cap = 0;
  if (cap < n_i32) {
    int32_t* nb = nullptr;
    if (hipHostMalloc((void**)&nb, n_i32 * 4, hipHostMallocDefault) != hipSuccess) return nullptr;
    if (buf) (void)hipHostFree(buf);
    buf = nb;
    cap = n_i32;
  }
  return buf;
}

// Pinned host staging of the chunk tables a fit uploads at its start and at
// every warm-start level change.  From pageable vectors hipMemcpyAsync copies
// through the runtime's own staging and returns when the copy is done: the
// first such copy of a process took 16.7 ms at config 2's level change
// (profiles/r06d_first_fit_trace.txt), with the GPU idle behind it.  From
// here the copies are asynchronous.  Thread-local, grown on demand at a fit's
// start (reserve: every plan of the fit), never shrunk; an event after the
// last staged copy guards the reuse by the next fit (a fit that fails early
// returns without its final synchronisation).
struct PinnedArena {
  char* buf = nullptr;
  size_t cap = 0, used = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
};
inline PinnedArena& pinned_arena() {
  thread_local PinnedArena a;
  return a;
}
inline hipError_t pinned_arena_reserve(size_t bytes) {
  PinnedArena& a = pinned_arena();
  if (a.pending) {
    hipError_t e = hipEventSynchronize(a.done);
    if (e != hipSuccess) return e;
    a.pending = false;
  }
  a.used = 0;
  if (!a.done) {
    hipError_t e = hipEventCreateWithFlags(&a.done, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  if (a.cap >= bytes) return hipSuccess;
  char* nb = nullptr;
  hipError_t e = hipHostMalloc((void**)&nb, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return e;
  if (a.buf) (void)hipHostFree(a.buf);
  a.buf = nb;
  a.cap = bytes;
  return hipSuccess;
}
// bytes one call of staged_upload takes from the arena
inline size_t staged_bytes(size_t bytes) { return (size_t)align_up((int64_t)bytes, 64); }
// H2D copy of host data through the arena (pageable copy if it is full)
inline hipError_t staged_upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  PinnedArena& a = pinned_arena();
  if (!a.buf || a.used + staged_bytes(bytes) > a.cap)
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
  char* p = a.buf + a.used;
  a.used += staged_bytes(bytes);
  memcpy(p, src, bytes);
  hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(a.done, s);
  if (e == hipSuccess) a.pending = true;
  return e;
}
// arena bytes of one plan's chunk tables (row0, rows, part, partition chunk begins)
inline size_t plan_staged_bytes(const Plan& q, int K) {
  return staged_bytes(8 * (size_t)q.n_chunks) + 2 * staged_bytes(4 * (size_t)q.n_chunks) +
         staged_bytes(4 * ((size_t)K + 1));
}
inline hipError_t upload_plan_tables(const Plan& q, int K, void* d_row0, void* d_rows,
                                     void* d_part, void* d_pcb, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (q.n_chunks > 0) {
    e = staged_upload(d_row0, q.chunk_row0.data(), 8LL * q.n_chunks, s);
    if (e == hipSuccess) e = staged_upload(d_rows, q.chunk_rows.data(), 4LL * q.n_chunks, s);
    if (e == hipSuccess) e = staged_upload(d_part, q.chunk_part.data(), 4LL * q.n_chunks, s);
  }
  if (e == hipSuccess) e = staged_upload(d_pcb, q.part_chunk_begin.data(), 4LL * (K + 1), s);
  return e;
}

// Event timer of the fit's stream (record_timing only).  A pair of events
// brackets every launch; the elapsed times are read after the fit's final
// stream synchronisation (flush), so timing adds no host round trip per
// launch and the launches stay queued back to back.
struct StreamTimer {
  hipStream_t stream;
  bool on;
  std::vector<hipEvent_t> ev;        // 2 per recorded launch, reused across calls
  std::vector<double*> dst_a, dst_b; // accumulators of each recorded launch
  size_t used = 0;
  ~StreamTimer() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  template <typename F>
  hipError_t operator()(double* acc, F&& launch, double* acc2 = nullptr) {
    if (!on) return launch();
    if (2 * used + 2 > ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
      }
    }
    hipError_t e = hipEventRecord(ev[2 * used], stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipEventRecord(ev[2 * used + 1], stream);
    if (e != hipSuccess) return e;
    dst_a.push_back(acc);
    dst_b.push_back(acc2);
    ++used;
    return hipSuccess;
  }
  // after the stream has been synchronised
  hipError_t flush() {
    for (size_t i = 0; i < used; ++i) {
      float ms = 0.f;
      hipError_t e = hipEventSynchronize(ev[2 * i + 1]);
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
      if (e != hipSuccess) return e;
      *dst_a[i] += ms;
      if (dst_b[i]) *dst_b[i] += ms;
    }
    used = 0;
    dst_a.clear();
    dst_b.clear();
    return hipSuccess;
  }
};

// ---- the steps every fit shares ------------------------------------------

struct FitOutputs {  // device arrays, one entry (row, matrix) per partition
  double *theta, *sig_inv, *sig_inv_theta, *loglik;
  int32_t *iters, *status;
};

// Start of every fit: the clock of ms_total, a clean error and stats, the
// caller's options or the defaults.
struct FitStart {
  std::chrono::steady_clock::time_point t_start;
  hipStream_t stream;
  dlsa_fit_options opt;
};
inline FitStart fit_begin(const dlsa_fit_options* opt_in, void* stream) {
  FitStart f;
  f.t_start = std::chrono::steady_clock::now();
  g_last_error.clear();
  memset(&g_stats, 0, sizeof(g_stats));
  f.stream = (hipStream_t)stream;
  if (opt_in)
    f.opt = *opt_in;
  else
    dlsa_fit_options_default(&f.opt);
  if (f.opt.switch_tol <= 0) f.opt.switch_tol = 1e-6;
  return f;
}
// The argument checks of every fit (after the path's own shape checks) and
// the defaults of max_iter and tol.
inline int check_fit_args(const double* center, const double* scale, const FitOutputs& out,
                          int32_t& max_iter, double& tol) {
  if ((center == nullptr) != (scale == nullptr)) {
    set_error("center and scale must both be given or both be NULL");
    return DLSA_E_INVALID;
  }
  if (!out.theta || !out.sig_inv || !out.sig_inv_theta || !out.loglik || !out.iters ||
      !out.status) {
    set_error("null output pointer");
    return DLSA_E_INVALID;
  }
  if (max_iter < 1) max_iter = 1;
  if (!(tol > 0)) tol = 1e-10;
  return DLSA_OK;
}

// A dense fit after fit_dense's checks (capi.hip), as fit_fused and fit_wide take it.
struct DenseFit {
  int family;
  const double *X, *y;
  const int64_t* offsets;
  int32_t K, p, fit_intercept;
  const double *center, *scale;
  int32_t max_iter;
  double tol;
  FitOutputs out;
  FitStart start;
  // FAMILY_POISSON: per-row offset of eta [n_total], device, or null (fused path only)
  const double* eta_offset = nullptr;
  // per-row prior weights omega [n_total], device, or null (logistic and
  // Poisson, fused path only)
  const double* row_weight = nullptr;
};
int fit_fused(const DenseFit& f);  // P <= DLSA_MAX_P_FUSED (fit_fused.hip)
int fit_wide(const DenseFit& f);   // P > DLSA_MAX_P_FUSED (fit_wide.hip)
// (family: FAMILY_LOGISTIC or FAMILY_POISSON; eta_offset: Poisson's per-row
// offset or null; row_weight: prior weights or null)
int fit_categorical(int family, const double* Xn, const uint8_t* codes, const double* y,
                    const double* eta_offset, const double* row_weight, const int64_t* offsets,
                    int32_t K, int32_t q, int32_t F,
                    const int32_t* levels, int32_t fit_intercept, const double* center,
                    const double* scale, int32_t max_iter, double tol, const FitOutputs& out,
                    const dlsa_fit_options* opt_in, void* stream);  // fit_cat.hip

// The SolveArgs fields every path fills alike: the Newton state carved from
// the workspace and the output arrays.  The path adds its slabs, NT,
// switch_tol and escalate_to.
inline SolveArgs newton_solve_args(const Workspace& ws, const NewtonState& ns,
                                   const FitOutputs& out, int P, int family, double tol) {
  SolveArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.theta = out.theta;
  sa.theta_prev = (double*)ws.at(ns.off_thprev);
  sa.delta_prev = (double*)ws.at(ns.off_dprev);
  sa.ll_prev = (double*)ws.at(ns.off_llprev);
  sa.phase = (int32_t*)ws.at(ns.off_phase);
  sa.backtracks = (int32_t*)ws.at(ns.off_bt);
  sa.iters = out.iters;
  sa.status = out.status;
  sa.counters = (int32_t*)ws.at(ns.off_counters);
  sa.dm_prev = (double*)ws.at(ns.off_dmprev);
  sa.stall = (int32_t*)ws.at(ns.off_stall);
  sa.sig_inv = out.sig_inv;
  sa.loglik = out.loglik;
  sa.P = P;
  sa.family = family;
  sa.tol = tol;
  return sa;
}
inline hipError_t fit_init(const SolveArgs& sa, const int64_t* d_offsets, int K, int start_phase,
                           hipStream_t s) {
  return launch_fit_init(d_offsets, K, sa.P, start_phase, sa.theta, sa.phase, sa.backtracks,
                         sa.iters, sa.status, sa.ll_prev, sa.sig_inv, sa.loglik, s);
}

// The host's copy of the running counters and the phases: pinned, adjacent
// like the device's (counters[4] then phase[K]), so one copy reads both.
// `extra` more ints follow the phases.
struct Readback {
  int32_t* cnt = nullptr;
  int32_t* phase = nullptr;
  bool init(int K, size_t extra = 0) {
    cnt = pinned_staging(4 + (size_t)K + extra);
    if (!cnt) set_error("pinned host staging allocation failed");
    phase = cnt ? cnt + 4 : nullptr;
    return cnt != nullptr;
  }
  void running(int* n_running) const {
    for (int ph = 0; ph < kRunPhases; ++ph) n_running[ph] = cnt[ph];
  }
};
inline int running_total(const int* n_running) {
  int n = 0;
  for (int ph = 0; ph < kRunPhases; ++ph) n += n_running[ph];
  return n;
}
// counters + phases in one copy (adjacent on both sides)
inline hipError_t enqueue_readback(const SolveArgs& sa, int K, const Readback& h, hipStream_t s) {
  return hipMemcpyAsync(h.cnt, sa.counters, 16 + 4LL * K, hipMemcpyDeviceToHost, s);
}
inline hipError_t read_counters(const SolveArgs& sa, int K, const Readback& h, int* n_running,
                                hipStream_t s) {
  hipError_t e = enqueue_readback(sa, K, h, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) h.running(n_running);
  return e;
}
inline hipError_t read_phases(const SolveArgs& sa, int K, const Readback& h, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(h.phase, sa.phase, 4LL * K, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e;
}
// Entry of a level after the first: every running partition re-enters at
// start_phase; the counters and phases are read back.
inline hipError_t reenter_level(const SolveArgs& sa, int K, int start_phase, const Readback& h,
                                int* n_running, hipStream_t s) {
  hipError_t e = hipMemsetAsync(sa.counters, 0, 16, s);
  if (e == hipSuccess)
    e = launch_level_reset(K, sa.P, start_phase, sa.phase, sa.status, sa.ll_prev, sa.backtracks,
                           sa.theta, sa.counters, s, sa.theta0);
  if (e == hipSuccess) e = read_counters(sa, K, h, n_running, s);
  return e;
}
// The level's solve settings; returns the iteration at which the level ends
// (<= it: no budget left for this warm-start level).
inline int begin_level(SolveArgs& sa, bool final_level, bool fused_tol, double switch_tol, int it,
                       int max_iter) {
  sa.subsample = final_level ? 0 : 1;
  sa.level_tol = warm_level_tol(fused_tol);
  sa.switch_tol = final_level ? switch_tol : 0.0;
  return it + iter_budget(final_level, it, max_iter);
}
inline hipError_t clear_stall_state(const SolveArgs& sa, int K, hipStream_t s) {
  hipError_t e = hipMemsetAsync(sa.dm_prev, 0, 8LL * K, s);
  if (e == hipSuccess) e = hipMemsetAsync(sa.stall, 0, 4LL * K, s);
  return e;
}
// Polish of the dense paths: the partitions the budget left running (any
// phase) are marked PHASE_F64 for one exact pass; the phases are read back.
inline hipError_t mark_polish(const SolveArgs& sa, int K, const Readback& h, hipStream_t s) {
  hipError_t e = hipMemsetAsync(sa.counters, 0, 16, s);
  if (e == hipSuccess) e = launch_polish_mark(K, sa.phase, sa.status, sa.counters, s);
  if (e == hipSuccess) e = read_phases(sa, K, h, s);
  return e;
}

// DLSA_TRACE=1: per-iteration max |step| over all partitions (diagnostics;
// copies theta and the last step to the host, so only for investigation)
inline bool trace_enabled() { return getenv("DLSA_TRACE") != nullptr; }
inline hipError_t trace_iteration(int K, const SolveArgs& sa, size_t lvl, int it,
                                  const int* n_running) {
  const int P = sa.P;
  std::vector<double> th((size_t)K * P), dp((size_t)K * P);
  hipError_t e = hipMemcpy(th.data(), sa.theta, 8LL * K * P, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(dp.data(), sa.delta_prev, 8LL * K * P, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  double dmax = 0.0, tmax = 0.0;
  for (size_t i = 0; i < th.size(); ++i) {
    dmax = std::max(dmax, std::fabs(dp[i]));
    tmax = std::max(tmax, std::fabs(th[i]));
  }
  fprintf(stderr,
          "[dlsa trace] level %zu iter %d: max|step| %.3e max|theta| %.3e running approx %d "
          "f32x %d f64 %d\n",
          lvl, it, dmax, tmax, n_running[PHASE_F32], n_running[PHASE_F32X], n_running[PHASE_F64]);
  return hipSuccess;
}

// End of every fit: Sig_inv theta and the final statuses, the stream drained,
// ms_total and the event timer's launches.
inline int fit_end(const FitStart& f, const SolveArgs& sa, int K, double* sig_inv_theta,
                   StreamTimer& timed) {
  DLSA_HIP_TRY(launch_fit_finalize(K, sa.P, sa.theta, sa.sig_inv, sig_inv_theta, sa.status,
                                   f.stream));
  DLSA_HIP_TRY(hipStreamSynchronize(f.stream));
  g_stats.ms_total =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f.t_start)
          .count();
  DLSA_HIP_TRY(timed.flush());
  return DLSA_OK;
}

}  // namespace dlsa
