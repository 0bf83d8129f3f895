// The wide fit (P > DLSA_MAX_P_FUSED, wide_common.hpp): per Newton iteration the
// fused bf16 pass (PHASE_F32 partitions) and/or the row + exact Gram passes
// (PHASE_F64), the deterministic partial-tile assembly and the per-partition
// blocked-Cholesky update.  Same warm-start levels, phases, state machine and
// outputs as the fused path.
#include "fit_driver.hpp"

namespace dlsa {

int fit_wide(const DenseFit& f) {
  const dlsa_fit_options& opt = f.start.opt;
  hipStream_t stream = f.start.stream;
  const int family = f.family, K = f.K, p = f.p;
  const FamilyRules rules = family_rules(family);
  const int64_t* offsets = f.offsets;
  const int P = p + (f.fit_intercept ? 1 : 0);
  const int NB = (P + kWideTile - 1) / kWideTile;
  const std::vector<WidePlans> plans = wide_level_plans(
      offsets, K, p, f.fit_intercept, opt.rows_per_chunk,
      rules.iterates && opt.warm_start);
  const WideLayout L = make_wide_layout(plans, K, offsets[K], P);
  g_stats.n_chunks = plans.back().gram.n_chunks;

  // The exact Gram pass runs on the int8 matrix cores (wide_oz.hip) in mixed
  // mode when the final plan's row groups are <= kWideOzMaxRows rows and its
  // digit records fit the workspace: the caller's (dlsa_logistic_workspace_bytes
  // counts them) or the one allocated here.  Without room for them -- a
  // caller workspace of at least base_total but less than total bytes, a
  // failed allocation, or opt.oz_max_bytes below the records' size -- the
  // fp64 Gram runs (stats.oz_fallbacks).  DLSA_EXACT_FP64: always the fp64 Gram.
  bool use_wide_oz = opt.exact_pass != DLSA_EXACT_FP64 && rules.digit_scales &&
                     opt.hessian_mode == DLSA_HESSIAN_MIXED && L.digit_bytes > 0;
  if (use_wide_oz && opt.oz_max_bytes > 0 && L.digit_bytes > opt.oz_max_bytes) {
    use_wide_oz = false;
    g_stats.oz_fallbacks++;
  }
  Workspace ws(stream);
  const bool holds_base = !opt.workspace || opt.workspace_bytes >= L.base_total;
  if (use_wide_oz && holds_base && !ws.try_acquire(opt.workspace, opt.workspace_bytes, L.total)) {
    use_wide_oz = false;
    g_stats.oz_fallbacks++;
  }
  if (!ws)
    if (int rc = ws.acquire(opt.workspace, opt.workspace_bytes, L.base_total,
                            WsPolicy::kCallerMustFit, L.total))
      return rc;
  int64_t* d_offsets = (int64_t*)ws.at(L.off_offsets);
  int32_t* d_rcb = (int32_t*)ws.at(L.off_rcb);
  int32_t* d_gcb = (int32_t*)ws.at(L.off_gcb);
  double* d_H = (double*)ws.at(L.off_H);

  SolveArgs sa = newton_solve_args(ws, L.ns, f.out, P, family, f.tol);
  sa.escalate_to = PHASE_F64;  // no fp32 fused wide pass: bf16 -> fp64
  sa.switch_tol = opt.switch_tol;

  WideArgs wa;
  memset(&wa, 0, sizeof(wa));
  wa.X = f.X;
  wa.y = f.y;
  wa.rc_row0 = (const int64_t*)ws.at(L.off_r_row0);
  wa.rc_rows = (const int32_t*)ws.at(L.off_r_rows);
  wa.rc_part = (const int32_t*)ws.at(L.off_r_part);
  wa.gc_row0 = (const int64_t*)ws.at(L.off_g_row0);
  wa.gc_rows = (const int32_t*)ws.at(L.off_g_rows);
  wa.gc_part = (const int32_t*)ws.at(L.off_g_part);
  wa.phase = sa.phase;
  wa.theta = f.out.theta;
  wa.center = f.center;
  wa.scale = f.scale;
  wa.w = (double*)ws.at(L.off_w);
  wa.slab_g = (double*)ws.at(L.off_slabg);
  wa.slab_ll = (double*)ws.at(L.off_slabll);
  wa.slab_G = (double*)ws.at(L.off_slabG);
  wa.slab_gz = (double*)ws.at(L.off_slabgz);
  wa.slab_llz = (double*)ws.at(L.off_slabllz);
  wa.p = p;
  wa.P = P;
  wa.intercept = f.fit_intercept ? 1 : 0;
  wa.NB = NB;

  {
    size_t need = staged_bytes(8 * ((size_t)K + 1));
    for (const WidePlans& q : plans) need += plan_staged_bytes(q.rows, K) + plan_staged_bytes(q.gram, K);
    DLSA_HIP_TRY(pinned_arena_reserve(need));
  }
  DLSA_HIP_TRY(staged_upload(d_offsets, offsets, 8LL * (K + 1), stream));

  // MIXED / MIXED_F32: bf16-MFMA Gram passes until the step is below
  // switch_tol, then fp64 Gram passes (the fused path's phase machine)
  const int start_phase =
      (opt.hessian_mode == DLSA_HESSIAN_FP64 || !rules.iterates) ? PHASE_F64 : PHASE_F32;
  DLSA_HIP_TRY(fit_init(sa, d_offsets, K, start_phase, stream));
  int n_running[kRunPhases] = {0, 0, 0};
  for (int k = 0; k < K; ++k)
    if (offsets[k + 1] > offsets[k]) n_running[start_phase]++;

  const bool standardize = f.center != nullptr;
  StreamTimer timed{stream, opt.record_timing != 0};
  Readback h;
  if (!h.init(K)) return DLSA_E_HIP;
  const bool trace = trace_enabled();

  // The row pass of an int8 exact Gram also records each row chunk's max
  // |sqrt(w) x|, from which the scale kernel takes the digit exponents of
  // every Gram row group.
  WideOzArgs woz;
  memset(&woz, 0, sizeof(woz));
  woz.rcb = d_rcb;
  woz.zmax = (const uint32_t*)ws.at(L.off_zmax);
  woz.E = (int32_t*)ws.at(L.off_ozE);
  woz.maxblk = (plans.back().gram.max_chunk_rows + 31) / 32;
  woz.D = use_wide_oz ? (int8_t*)ws.at(L.off_digits) : nullptr;
  auto exact_gram = [&](const WidePlans& q, bool final_level) -> hipError_t {
    const bool oz = use_wide_oz && final_level;
    wa.slab_zmax = oz ? (uint32_t*)ws.at(L.off_zmax) : nullptr;
    hipError_t e = timed(&g_stats.ms_wide_row, [&] {
      return launch_wide_row(wa, standardize, family, q.rows.n_chunks, stream);
    });
    wa.slab_zmax = nullptr;
    if (e != hipSuccess) return e;
    if (!oz)
      return timed(
          &g_stats.ms_wide_gram, [&] { return launch_wide_gram(wa, standardize, stream); },
          &g_stats.ms_pass_fp64);
    g_stats.passes_oz++;
    return timed(
        &g_stats.ms_wide_gram,
        [&] {
          hipError_t e2 = launch_wide_oz_scale(wa, woz, stream);
          if (e2 == hipSuccess) e2 = launch_wide_oz_digits(wa, woz, standardize, stream);
          if (e2 == hipSuccess) e2 = launch_wide_oz_gram(wa, woz, stream);
          return e2;
        },
        &g_stats.ms_pass_fp64);
  };
  // partial tiles -> H, then the Newton update (eval_only: the polish)
  auto assemble_and_solve = [&](bool clear_counters) -> hipError_t {
    hipError_t e = timed(&g_stats.ms_wide_assemble,
                         [&] { return launch_wide_assemble(wa, d_gcb, d_H, K, stream); });
    if (e == hipSuccess && clear_counters) e = hipMemsetAsync(sa.counters, 0, 16, stream);
    if (e == hipSuccess)
      e = timed(&g_stats.ms_solve,
                [&] { return launch_wide_newton(sa, wa, d_rcb, d_gcb, d_H, K, stream); });
    return e;
  };

  int it = 0;
  for (size_t lvl = 0; lvl < plans.size(); ++lvl) {
    const WidePlans& q = plans[lvl];
    const bool final_level = lvl + 1 == plans.size();
    if (q.rows.n_chunks > L.cap_rows || q.gram.n_chunks > L.cap_gram) {
      set_error("internal: wide plan exceeds its workspace layout");
      return DLSA_E_INVALID;
    }
    DLSA_HIP_TRY(upload_plan_tables(q.rows, K, ws.at(L.off_r_row0), ws.at(L.off_r_rows),
                                    ws.at(L.off_r_part), d_rcb, stream));
    DLSA_HIP_TRY(upload_plan_tables(q.gram, K, ws.at(L.off_g_row0), ws.at(L.off_g_rows),
                                    ws.at(L.off_g_part), d_gcb, stream));
    wa.n_gchunks = q.gram.n_chunks;
    const std::vector<int64_t> part_rows = plan_part_rows(q.rows, K);
    if (lvl > 0)
      DLSA_HIP_TRY(reenter_level(sa, K, start_phase, h, n_running, stream));
    else
      DLSA_HIP_TRY(read_phases(sa, K, h, stream));
    const int it_end = begin_level(sa, final_level, false, opt.switch_tol, it, f.max_iter);
    if (it_end <= it) continue;  // no budget left for this warm-start level
    DLSA_HIP_TRY(clear_stall_state(sa, K, stream));
    for (; it < it_end && running_total(n_running) > 0 && q.rows.n_chunks > 0; ++it) {
      // approximate partitions: one fused pass (gradient + bf16 Hessian)
      if (n_running[PHASE_F32] > 0) {
        DLSA_HIP_TRY(timed(
            &g_stats.ms_wide_gram, [&] { return launch_wide_fused(wa, standardize, stream); },
            &g_stats.ms_pass_fp32));
        g_stats.passes_fp32++;
        g_stats.rows_fp32 += phase_rows(part_rows, h.phase, PHASE_F32);
      }
      // exact partitions: row pass (gradient, w) + the exact Gram pass
      if (n_running[PHASE_F64] > 0) {
        DLSA_HIP_TRY(exact_gram(q, final_level));
        g_stats.passes_fp64++;
        g_stats.rows_fp64 += phase_rows(part_rows, h.phase, PHASE_F64);
      }
      DLSA_HIP_TRY(assemble_and_solve(true));
      DLSA_HIP_TRY(read_counters(sa, K, h, n_running, stream));
      if (trace) DLSA_HIP_TRY(trace_iteration(K, sa, lvl, it, n_running));
    }
  }
  g_stats.iterations = it;
  // polish: partitions the budget left running get Sig_inv = X^T W X at the
  // theta they return (row pass + exact Gram pass, no step)
  if (rules.iterates && running_total(n_running) > 0 && plans.back().rows.n_chunks > 0) {
    const WidePlans& q = plans.back();
    DLSA_HIP_TRY(mark_polish(sa, K, h, stream));
    DLSA_HIP_TRY(exact_gram(q, true));
    g_stats.passes_fp64++;
    g_stats.rows_fp64 += phase_rows(plan_part_rows(q.rows, K), h.phase, PHASE_F64);
    g_stats.polish_partitions = running_total(n_running);
    sa.eval_only = 1;
    sa.subsample = 0;
    DLSA_HIP_TRY(assemble_and_solve(false));
    sa.eval_only = 0;
  }
  return fit_end(f.start, sa, K, f.out.sig_inv_theta, timed);
}

}  // namespace dlsa
