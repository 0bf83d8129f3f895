// The fused-pass fit (P <= DLSA_MAX_P_FUSED): per Newton iteration one pass
// per running phase over the row chunks (gradient + Hessian tiles in one
// sweep of X) and the per-partition LDS Cholesky update.
#include "fit_driver.hpp"

namespace dlsa {

namespace {

struct ReadEvent {  // the counters' copy of an iteration (destroyed on every return)
  hipEvent_t ev = nullptr;
  ~ReadEvent() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

// The passes of one fused fit and the host's record of what they saw.
struct FusedFit {
  const DenseFit& f;
  const int K, P;
  hipStream_t stream;
  StreamTimer timed;
  Readback h;
  int32_t* h_route = nullptr;  // [K] phases with stale partitions marked (one launch)
  PassArgsWgt pa;  // (eta_offset / row_weight null unless the fit has that row extra)
  SolveArgs sa;
  int approx_prec = PREC_BF16;
  bool standardize = false;
  // exact passes on the int8 matrix cores (irls_oz_impl.hpp) unless DLSA_EXACT_FP64:
  // the first full-data bf16 pass records, per chunk and feature, max |x|; the
  // bf16 passes that follow an iteration with a partition near the switch
  // (counters[3], kOzNearTol) record max |sqrt(w) x| at the theta they saw
  // (snapshotted into theta_rec first); the exact passes of the final plan
  // take their digit scales from the partition's last records (a chunk with
  // no max |z| record -- zcolmax = +inf, theta_rec = 0 -- gets max |x| / 2)
  bool use_oz = false;
  uint32_t *d_colmax = nullptr, *d_zcolmax = nullptr;
  double* d_threc = nullptr;
  bool colmax_ready = false;
  bool near_switch = false;  // counters[3] of the last solve
  // per partition: the last approximate pass that processed it recorded max |z|
  // (so its exact pass starts from a record one small step away); a partition
  // lacking one runs its exact pass on the fp64 MFMA instead (a second launch
  // beside the int8 one, PHASE_F64_STALE): without a fresh record the digit
  // exponents fall back to max |x| / 2, which a column with large |x| at w ~ 0
  // (an outlier row) turns into ~1e-5 per-entry errors
  // (tests/test_gpu_ozaki.py::test_ozaki_polish_pass_per_entry)
  std::vector<char> zfresh;
  // DLSA_OZ_ZREC=0 (knob builds, A/B only): no max |z| records, so no partition
  // is ever fresh and every exact pass runs on the fp64 MFMA (it no longer
  // measures round 3's "every exponent from max |x| / 2" int8 pass)
  const bool zrec = !(env_knob("DLSA_OZ_ZREC") && atoi(env_knob("DLSA_OZ_ZREC")) == 0);

  explicit FusedFit(const DenseFit& fit)
      : f(fit), K(fit.K), P(fit.p + (fit.fit_intercept ? 1 : 0)), stream(fit.start.stream),
        timed{fit.start.stream, fit.start.opt.record_timing != 0}, zfresh((size_t)fit.K, 0) {}

  int run();
  void set_pass_args(const Plan& pl, const Workspace& ws, const Layout& L);
  hipError_t pass(int ph, const Plan& q, bool full, const std::vector<int64_t>& part_rows,
                  const int32_t* hph);
  hipError_t spec_pass(const Plan& q, bool full);
  void count_spec_pass(bool final_level, const std::vector<int64_t>& part_rows);
};

void FusedFit::set_pass_args(const Plan& pl, const Workspace& ws, const Layout& L) {
  memset(&pa, 0, sizeof(pa));
  pa.X = f.X;
  pa.y = f.y;
  pa.chunk_row0 = (const int64_t*)ws.at(L.off_row0);
  pa.chunk_rows = (const int32_t*)ws.at(L.off_rows);
  pa.chunk_part = (const int32_t*)ws.at(L.off_part);
  pa.phase = sa.phase;
  pa.theta = f.out.theta;
  pa.center = f.center;
  pa.scale = f.scale;
  pa.slab_H = (double*)ws.at(L.off_slabH);
  pa.slab_g = (double*)ws.at(L.off_slabg);
  pa.slab_ll = (double*)ws.at(L.off_slabll);
  pa.slab_llc = sa.slab_llc;
  pa.eta_offset = f.eta_offset;
  pa.row_weight = f.row_weight;
  pa.p = f.p;
  set_stream_bounds(pa, f.offsets[K]);
  pa.P = P;
  pa.intercept = f.fit_intercept ? 1 : 0;
  pa.waves = f.start.opt.exact_waves;
  // cooperative-pass LDS ring: two workgroups per CU (P <= 112) so that one's
  // row phase and barrier waits overlap the other's tile phase (measured
  // 27.4 -> 21.8 ms per bf16 pass at config 2 against one workgroup with a
  // deeper ring)
  pa.slot_bytes = coop_slot_bytes(pl.NT, pa.X, f.p, ex_count(pass_extras(pa)));
  const int wg_per_cu = pl.NT < 8 ? 2 : 1;
  const int budget = 160 * 1024 / wg_per_cu - coop_extra_bytes(pl.NT);
  pa.nslot = std::max(2, std::min(budget / pa.slot_bytes, 6));
}

// one pass over the chunks of plan q whose partition is in phase ph:
// exact (fp64 Hessian) passes by the per-wave kernel up to P = 128 and the
// cooperative one above; approximate passes (PHASE_F32 at the fit's
// approximate precision, PHASE_F32X at fp32) by the cooperative kernel
// (full: q is the all-rows plan, whose chunks the digit scales describe)
hipError_t FusedFit::pass(int ph, const Plan& q, bool full, const std::vector<int64_t>& part_rows,
                          const int32_t* hph) {
  const int family = f.family;
  const FamilyRules rules = family_rules(family);
  const bool f64 = ph == PHASE_F64;
  const int prec = f64 ? PREC_F64 : (ph == PHASE_F32X ? PREC_F32 : approx_prec);
  pa.want_phase = ph;
  const bool wave = f64 && q.NT <= kWaveMaxNT;
  int n_fresh = 0, n_stale = 0;
  if (f64)
    for (int k = 0; k < K; ++k)
      if (hph[k] == PHASE_F64) (zfresh[k] ? n_fresh : n_stale)++;
  const bool oz = wave && use_oz && colmax_ready && full && n_fresh > 0;
  // int8 for the fresh partitions, fp64 MFMA for the stale ones: the stale
  // ones are marked PHASE_F64_STALE on the device for the int8 launch (which
  // skips them), then passed by the per-wave fp64 kernel, then restored
  const bool split = oz && n_stale > 0;
  if (split) {
    for (int k = 0; k < K; ++k)
      h_route[k] = (hph[k] == PHASE_F64 && !zfresh[k]) ? PHASE_F64_STALE : hph[k];
    hipError_t e = hipMemcpyAsync(sa.phase, h_route, 4LL * K, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    g_stats.oz_stale_partitions += n_stale;
  }
  // digit-scale records of a full-data bf16 pass: max |x| on the first,
  // max |z| near the switch
  const bool rec_x = use_oz && full && ph == PHASE_F32 && !colmax_ready;
  const bool rec_z = use_oz && full && ph == PHASE_F32 && near_switch && zrec;
  if (rec_z) {
    hipError_t e = launch_theta_snapshot(K, P, sa.phase, PHASE_F32, sa.theta, d_threc, stream);
    if (e != hipSuccess) return e;
  }
  hipError_t e = timed(f64 ? &g_stats.ms_pass_fp64 : &g_stats.ms_pass_fp32, [&] {
    PassArgsWgt pc = pa;
    pc.colmax = (oz || rec_x) ? d_colmax : nullptr;
    pc.zcolmax = (oz || rec_z) ? d_zcolmax : nullptr;
    pc.theta_rec = d_threc;
    if (oz) {
      hipError_t eo = launch_irls_oz(pc, q.NT, standardize, family, q.n_chunks, stream);
      if (eo != hipSuccess || !split) return eo;
      PassArgsWgt ps = pa;  // the stale partitions on the fp64 MFMA
      ps.want_phase = PHASE_F64_STALE;
      return launch_irls_wave(ps, q.NT, standardize, family, q.n_chunks, stream);
    }
    // OLS (one pass at theta = 0): X streamed into registers, no LDS ring.
    // Its buffer range and row offsets are 32-bit, like those of the kernels
    // below (there is no kernel to fall back to for a longer chunk): make_plan
    // keeps every chunk's X within kMaxChunkBytes, which this restates
    if (f64 && !rules.iterates && ols_stream_applies(q.NT) &&
        (int64_t)q.max_chunk_rows * f.p * 8 <= kMaxChunkBytes)
      return launch_ols_stream(pc, q.NT, standardize, q.n_chunks, stream);
    if (wave) return launch_irls_wave(pc, q.NT, standardize, family, q.n_chunks, stream);
    return launch_irls_coop(pc, q.NT, prec, standardize, family, q.n_chunks, stream);
  });
  if (split && e == hipSuccess)  // hph is the pinned readback, unchanged until the next sync
    e = hipMemcpyAsync(sa.phase, hph, 4LL * K, hipMemcpyHostToDevice, stream);
  if (rec_x) colmax_ready = true;
  if (!f64)  // this pass's partitions moved on from their records unless it took one
    for (int k = 0; k < K; ++k)
      if (hph[k] == ph) zfresh[k] = rec_z;
  if (oz) g_stats.passes_oz++;
  if (f64) {
    g_stats.passes_fp64++;
    g_stats.rows_fp64 += phase_rows(part_rows, hph, ph);
  } else {
    g_stats.passes_fp32++;
    g_stats.rows_fp32 += phase_rows(part_rows, hph, ph);
    if (ph == PHASE_F32X) g_stats.passes_f32x++;
  }
  return e;
}

// The next iteration's approximate pass is enqueued before the host reads
// this iteration's counters: a pass checks its partitions'
// phases on the device, so one enqueued for partitions that have since
// switched or finished runs as a no-op, and the GPU no longer idles through
// every hand-back (hipStreamSynchronize's return, the host's decisions and
// the next launch: 25-45 us per iteration).  The one decision
// such a pass needs from those counters -- whether to record max |z| (a
// partition near the switch, counters[3]) -- is taken on the device
// (PassArgs::zrec_gate, the gated theta snapshot), and the host's
// bookkeeping of the pass (count_spec_pass: zfresh, stats) runs after the
// read, from the phases the pass saw.
hipError_t FusedFit::spec_pass(const Plan& q, bool full) {
  pa.want_phase = PHASE_F32;
  const bool zg = use_oz && full && zrec;
  int32_t* gate = sa.counters + 3;
  if (zg) {
    hipError_t e = launch_theta_snapshot(K, P, sa.phase, PHASE_F32, sa.theta, d_threc, stream, gate);
    if (e != hipSuccess) return e;
  }
  return timed(&g_stats.ms_pass_fp32, [&] {
    PassArgsWgt pc = pa;
    pc.colmax = nullptr;
    pc.zcolmax = zg ? d_zcolmax : nullptr;
    pc.theta_rec = d_threc;
    pc.zrec_gate = zg ? gate : nullptr;
    return launch_irls_coop(pc, q.NT, approx_prec, standardize, f.family, q.n_chunks, stream);
  });
}
// the bookkeeping of a pass enqueued before the last read, from the phases it saw
void FusedFit::count_spec_pass(bool final_level, const std::vector<int64_t>& part_rows) {
  const bool rz = use_oz && final_level && zrec && near_switch;  // the device's decision
  for (int k = 0; k < K; ++k)
    if (h.phase[k] == PHASE_F32) zfresh[k] = rz;
  g_stats.passes_fp32++;
  g_stats.rows_fp32 += phase_rows(part_rows, h.phase, PHASE_F32);
}

int FusedFit::run() {
  const dlsa_fit_options& opt = f.start.opt;
  const int family = f.family;
  const FamilyRules rules = family_rules(family);
  const int64_t* offsets = f.offsets;
  // warm-start levels: Newton on row prefixes (1/16) before all rows
  const std::vector<Plan> plans =
      level_plans(offsets, K, f.p, f.fit_intercept, rules.iterates && opt.warm_start,
                  [&](double, int64_t) { return opt.rows_per_chunk; });
  const Plan& pl = plans.back();
  const Layout L = make_layout(pl, K);
  g_stats.n_chunks = pl.n_chunks;

  Workspace ws(stream);
  if (int rc = ws.acquire(opt.workspace, opt.workspace_bytes, L.total, WsPolicy::kCallerMustFit))
    return rc;
  int64_t* d_offsets = (int64_t*)ws.at(L.off_offsets);
  int32_t* d_pcb = (int32_t*)ws.at(L.off_pcb);
  auto upload = [&](const Plan& q) -> hipError_t {
    return upload_plan_tables(q, K, ws.at(L.off_row0), ws.at(L.off_rows), ws.at(L.off_part), d_pcb,
                              stream);
  };
  {
    size_t need = staged_bytes(8 * ((size_t)K + 1));
    for (const Plan& q : plans) need += plan_staged_bytes(q, K);
    DLSA_HIP_TRY(pinned_arena_reserve(need));
  }
  DLSA_HIP_TRY(staged_upload(d_offsets, offsets, 8LL * (K + 1), stream));

  approx_prec = opt.hessian_mode == DLSA_HESSIAN_MIXED_F32 ? PREC_F32 : PREC_BF16;
  standardize = f.center != nullptr;
  sa = newton_solve_args(ws, L.ns, f.out, P, family, f.tol);
  sa.part_chunk_begin = d_pcb;
  sa.slab_H = (double*)ws.at(L.off_slabH);
  sa.slab_g = (double*)ws.at(L.off_slabg);
  sa.slab_ll = (double*)ws.at(L.off_slabll);
  sa.NT = pl.NT;
  sa.switch_tol = opt.switch_tol;
  // a stalled bf16-steered partition goes on with fp32-MFMA Hessians first
  sa.escalate_to = approx_prec == PREC_BF16 ? PHASE_F32X : PHASE_F64;
  // Poisson: the K start values and the per-chunk constant-term partials live
  // in an allocation of the fit's own (the workspace layout is the logistic one)
  Workspace pws(stream);
  if (rules.device_start || rules.sums_ll_const) {
    Bump pb;
    const int64_t off_t0 = pb.take(8LL * std::max(K, 1));
    const int64_t off_llc = pb.take(8LL * std::max(pl.n_chunks, 1));
    if (int rc = pws.alloc(pb.o)) return rc;
    DLSA_HIP_TRY(hipMemsetAsync(pws.at(0), 0, pb.o, stream));
    sa.theta0 = (const double*)pws.at(off_t0);
    sa.slab_llc = (double*)pws.at(off_llc);
  }
  set_pass_args(pl, ws, L);

  const int start_phase =
      (opt.hessian_mode == DLSA_HESSIAN_FP64 || !rules.iterates) ? PHASE_F64 : PHASE_F32;
  DLSA_HIP_TRY(fit_init(sa, d_offsets, K, start_phase, stream));
  // the start point of a family that has one and the weight check; may end partitions
  const bool pre_pass = rules.device_start || f.row_weight != nullptr;
  if (pre_pass)
    DLSA_HIP_TRY(launch_fit_prepass(family, f.y, f.eta_offset, f.row_weight, d_offsets, K, P,
                                    f.fit_intercept ? 1 : 0, sa.theta,
                                    const_cast<double*>(sa.theta0), sa.phase, sa.status, stream));
  int n_running[kRunPhases] = {0, 0, 0};
  for (int k = 0; k < K; ++k)
    if (offsets[k + 1] > offsets[k]) n_running[start_phase]++;

  if (!h.init(K, (size_t)K)) return DLSA_E_HIP;
  h_route = h.phase + K;
  const bool trace = trace_enabled();

  // (Poisson weights are unbounded: no int8 exact pass, DLSA_EXACT_AUTO is fp64 MFMA;
  // so are prior weights: the digit-grid fallback bound relies on sqrt(w) <= 1/2)
  use_oz = rules.digit_scales && !f.row_weight && opt.exact_pass != DLSA_EXACT_FP64 &&
           approx_prec == PREC_BF16 && oz_applies(pl.NT, f.p) && pl.max_chunk_rows <= kOzMaxRows;
  d_colmax = (uint32_t*)ws.at(L.off_colmax);
  d_zcolmax = (uint32_t*)ws.at(L.off_zcolmax);
  d_threc = (double*)ws.at(L.off_threc);
  if (use_oz) {
    DLSA_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_zcolmax, 0x7F800000u,
                                   (size_t)std::max(pl.n_chunks, 1) * pl.PP, stream));
    DLSA_HIP_TRY(hipMemsetAsync(d_threc, 0, 8LL * K * P, stream));
  }
  ReadEvent read_ev;
  DLSA_HIP_TRY(hipEventCreateWithFlags(&read_ev.ev, hipEventDisableTiming));

  int it = 0;
  for (size_t lvl = 0; lvl < plans.size(); ++lvl) {
    const Plan& q = plans[lvl];
    const bool final_level = lvl + 1 == plans.size();
    const std::vector<int64_t> part_rows = plan_part_rows(q, K);
    bool spec = false;  // this iteration's PHASE_F32 pass was enqueued before the last read
    DLSA_HIP_TRY(upload(q));
    if (lvl > 0)  // re-enter every running partition
      DLSA_HIP_TRY(reenter_level(sa, K, start_phase, h, n_running, stream));
    else
      DLSA_HIP_TRY(read_phases(sa, K, h, stream));
    if (lvl == 0 && pre_pass) {  // less the partitions the start point / weight check ended
      n_running[start_phase] = 0;
      for (int k = 0; k < K; ++k)
        if (h.phase[k] == start_phase) n_running[start_phase]++;
    }
    // the prefix MLE is ~sqrt(P/n) from the full one (max step ~0.35 entering
    // the full level at config 2), so a level need not converge: it stops at
    // a 0.2-relative step (warm_level_tol)
    const int it_end = begin_level(sa, final_level, true, opt.switch_tol, it, f.max_iter);
    if (it_end <= it) continue;  // no budget left for this warm-start level
    DLSA_HIP_TRY(clear_stall_state(sa, K, stream));
    for (; it < it_end && running_total(n_running) > 0 && q.n_chunks > 0; ++it) {
      // approximate (bf16 or fp32), escalated fp32, then exact passes
      for (int ph : {PHASE_F32, PHASE_F32X, PHASE_F64}) {
        if (n_running[ph] == 0) continue;
        if (ph == PHASE_F32 && spec)
          count_spec_pass(final_level, part_rows);
        else
          DLSA_HIP_TRY(pass(ph, q, final_level, part_rows, h.phase));
      }
      DLSA_HIP_TRY(hipMemsetAsync(sa.counters, 0, 16, stream));
      DLSA_HIP_TRY(timed(&g_stats.ms_solve, [&] { return launch_newton_solve(sa, K, stream); }));
      DLSA_HIP_TRY(enqueue_readback(sa, K, h, stream));
      // the next iteration's approximate pass, if this one had approximate
      // partitions and the next needs no first max |x| record (rec_x)
      spec = n_running[PHASE_F32] > 0 && it + 1 < it_end &&
             !(use_oz && final_level && !colmax_ready);
      if (spec) {
        // wait for the copy only: the pass runs on while the host decides
        DLSA_HIP_TRY(hipEventRecord(read_ev.ev, stream));
        DLSA_HIP_TRY(spec_pass(q, final_level));
        DLSA_HIP_TRY(hipEventSynchronize(read_ev.ev));
      } else {
        DLSA_HIP_TRY(hipStreamSynchronize(stream));
      }
      h.running(n_running);
      near_switch = final_level && h.cnt[3] > 0;
      if (trace) DLSA_HIP_TRY(trace_iteration(K, sa, lvl, it, n_running));
    }
  }
  g_stats.iterations = it;
  // polish: partitions the budget left running (any phase) get one exact pass
  // at the theta they return; its X^T W X is published as Sig_inv, no step
  // (models.py:114,130 evaluate the weights at the coef sklearn stopped at)
  if (rules.iterates && running_total(n_running) > 0 && pl.n_chunks > 0) {
    // (the final level's plan, pl, is on the device: it was the last uploaded)
    // a partition stopped in an approximate phase took a full step after its
    // last record: its polish pass cannot use that record
    for (int k = 0; k < K; ++k)
      if (h.phase[k] != PHASE_F64) zfresh[k] = 0;
    DLSA_HIP_TRY(mark_polish(sa, K, h, stream));
    g_stats.polish_partitions = running_total(n_running);
    DLSA_HIP_TRY(pass(PHASE_F64, pl, true, plan_part_rows(pl, K), h.phase));
    sa.eval_only = 1;
    sa.subsample = 0;
    DLSA_HIP_TRY(timed(&g_stats.ms_solve, [&] { return launch_newton_solve(sa, K, stream); }));
    sa.eval_only = 0;
  }
  return fit_end(f.start, sa, K, f.out.sig_inv_theta, timed);
}

}  // namespace

int fit_fused(const DenseFit& f) { return FusedFit(f).run(); }

}  // namespace dlsa
