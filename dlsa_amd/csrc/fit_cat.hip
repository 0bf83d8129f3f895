// The categorical-code fit (cat_pass.hip): q numeric columns + F uint8 level
// codes per row.  Every pass is exact (PHASE_F64); a presence pass over all
// rows comes first (missing levels, invalid codes, the fixed-point grids of
// the histograms).  The Newton solve, the warm-start levels and the phases are
// the fused path's.  With prior weights (row_weight) the pre-pass of the dense
// weighted fits decides NONFINITE / SINGULAR first, the presence pass counts a
// level only in rows with omega > 0 and takes the partition's omega_max, which
// scales the grids, and the passes are cat_pass_wgt.hip's.
// FAMILY_POISSON (cat_pass_pois*.hip), with an optional per-row offset and
// optional prior weights: the dense Poisson fit's start point, pre-pass
// statuses and constant term (fit_fused.hip), a single plan level, and grids
// written on the device before every pass instead of cat_grids' (DESIGN 4.5h).
#include "fit_driver.hpp"

namespace dlsa {

namespace {

// Fixed-point grids of the int64 histograms, [K][kCatQMax + 2]: 2^E with
// |term| * 2^E * max(rows of a chunk, 1024) <= 2^60, so a bin's sum stays in
// int64 and every term below 2^50 (the kernel's 1.5 * 2^52 rounding needs
// |term| < 2^51).  Per partition (its chunks of the full plan `pl` cover all
// its rows, so the bound holds for every warm-start level's chunks too): an
// outlier row coarsens only its own partition's grid.  colmax
// [n_chunks][kCatQMax] is the presence pass's max |x_i| per chunk and column;
// hc / hs are the host's center and scale (0 / 1 without standardisation).
// Prior weights: every term carries omega, so each bound is multiplied by the
// partition's omega_max = the max over its chunks of wmax [n_chunks] (the
// presence pass's largest finite omega; empty without weights, and 0 -- a
// partition the pre-pass has ended -- counts as 1).  The residual bound then
// assumes 0 <= y <= 1, as the unweighted grid does.  omega == 1 gives the
// unweighted grids; a huge weight coarsens only its own partition's bins,
// which are then resolved omega_max / mean omega times coarser relative to
// their own sums than the unweighted ~1e-13.
std::vector<double> cat_grids(const std::vector<Plan>& plans, int K, int q, bool standardize,
                              const std::vector<double>& colmax, const std::vector<double>& wmax,
                              const std::vector<double>& hc, const std::vector<double>& hs) {
  const Plan& pl = plans.back();
  int64_t rmax = 1024;
  for (const Plan& qn : plans) rmax = std::max<int64_t>(rmax, qn.max_chunk_rows);
  auto grid = [&](double bound) {  // bound: max |term|
    if (!(bound > 0) || !std::isfinite(bound)) bound = 1.0;
    const int e = (int)std::floor(60.0 - std::log2(bound * (double)rmax));
    return std::ldexp(1.0, std::max(-900, std::min(900, e)));
  };
  std::vector<double> grids((size_t)K * (kCatQMax + 2), 1.0);
  for (int k = 0; k < K; ++k) {
    double* o = grids.data() + (size_t)k * (kCatQMax + 2);
    double om = 0.0;
    if (!wmax.empty())
      for (int c = pl.part_chunk_begin[k]; c < pl.part_chunk_begin[k + 1]; ++c)
        om = std::max(om, wmax[c]);
    if (!(om > 0) || !std::isfinite(om)) om = 1.0;
    o[0] = grid(0.25 * om);  // omega w, w = mu (1 - mu) <= 1/4; pair cells
    o[1] = grid(om);         // omega |y - mu| <= omega
    for (int j = 0; j < q; ++j) {
      double m = 0.0;
      for (int c = pl.part_chunk_begin[k]; c < pl.part_chunk_begin[k + 1]; ++c)
        m = std::max(m, colmax[(size_t)c * kCatQMax + j]);
      if (standardize) m = (m + std::fabs(hc[j])) / std::fabs(hs[j]);  // the kernel sums w (x - c) / s
      o[2 + j] = grid(0.25 * om * m);
    }
  }
  return grids;
}

}  // namespace

int fit_categorical(int family, const double* Xn, const uint8_t* codes, const double* y,
                    const double* eta_offset, const double* row_weight, const int64_t* offsets,
                    int32_t K, int32_t q,
                    int32_t F, const int32_t* levels, int32_t fit_intercept, const double* center,
                    const double* scale, int32_t max_iter, double tol, const FitOutputs& out,
                    const dlsa_fit_options* opt_in, void* stream_) {
  const FitStart start = fit_begin(opt_in, stream_);
  dlsa_fit_options opt = start.opt;
  hipStream_t stream = start.stream;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  const int ic = fit_intercept ? 1 : 0;
  int D = 0, P = 0;
  rc = check_cat_shape(q, F, levels, ic, DLSA_MAX_P_FUSED, "fit", &D, &P);
  if (rc == DLSA_OK) rc = check_fit_args(center, scale, out, max_iter, tol);
  if (rc != DLSA_OK) return rc;
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!y || (q > 0 && !Xn) || (F > 0 && !codes))) {
    set_error("null Xn, codes or y");
    return DLSA_E_INVALID;
  }

  const bool pois = family == FAMILY_POISSON;
  if (family != FAMILY_LOGISTIC && !pois) {
    set_error("the categorical fit runs the logistic and Poisson families");
    return DLSA_E_INVALID;
  }
  if (eta_offset && !family_rules(family).offset) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  CatArgsPois ca;  // (every kernel takes its slice: CatArgs, CatArgsWgt or all of it)
  memset(&ca, 0, sizeof(ca));
  ca.q = q;
  ca.F = F;
  ca.P = P;
  ca.intercept = ic;
  int d = ic + q;
  for (int f = 0; f < F; ++f) {
    ca.doff[f] = d;
    d += levels[f] - 1;
  }
  if (!cat_layout(ca, levels)) {
    set_error("categorical histograms do not fit the 160 KB LDS of a workgroup (P = " +
              std::to_string(P) + ")");
    return DLSA_E_UNSUPPORTED;
  }

  // chunks: one workgroup per CU at this LDS size, so a launch should be
  // whole rounds of 256 workgroups: ~512 chunks, split evenly per partition
  // (a ceil-rounded n/512 gave 5 chunks per config-3 partition -> 640 chunks,
  // 3 rounds of which the last is half empty)
  auto cat_rpc = [&](double frac, int64_t min_rows) {
    if (opt.rows_per_chunk > 0) return (int)opt.rows_per_chunk;
    int64_t nmax = 0;
    for (int k = 0; k < K; ++k)
      nmax = std::max(nmax, rows_used(offsets[k + 1] - offsets[k], frac, min_rows));
    const int64_t per = std::max<int64_t>(1, 512 / std::max(K, 1));
    return (int)std::max<int64_t>(1024, std::min<int64_t>((nmax + per - 1) / per, 1 << 24));
  };
  // warm-start level (a 1/16 prefix of every partition, to a 0.2-relative
  // step) only for partitions of >= 2^19 rows on average: every categorical
  // pass is exact, so on small partitions the prefix passes' launches and host
  // round trips cost more than the full pass they save (1.5e7 rows in 128
  // partitions: 11.2 ms per fit without, 14.9 with, profiles r02), on large
  // ones they save a full pass (config 3, 1.2e8 rows in 120 partitions: 37.2
  // vs 38.7 ms per step, 7 vs 5 passes of which 4 vs 5 full,
  // profiles/r04n_cat_warm_start_ab.txt).  DLSA_WARM_START overrides.
  opt.warm_start = opt.warm_start && K > 0 && n_total / K >= (int64_t(1) << 19);
  if (const char* e = env_knob("DLSA_WARM_START")) opt.warm_start = atoi(e);
  // Poisson: no warm-start level.  A prefix pass measures mu_max on a prefix
  // only, so the first full pass after it would take the analytic bound's
  // coarse grid and could be the published one
  if (pois) opt.warm_start = 0;
  const std::vector<Plan> plans =
      level_plans(offsets, K, P - ic, ic, opt.warm_start != 0, cat_rpc, /*x_cols=*/q);
  const Plan& pl = plans.back();
  const int64_t nc = std::max(pl.n_chunks, 1);
  // the fused layout for the most chunks of any level, then the presence
  // pass's counts and the grids
  Plan sizing = pl;
  for (const Plan& qn : plans) sizing.n_chunks = std::max(sizing.n_chunks, qn.n_chunks);
  const Layout L = make_layout(sizing, K);
  Bump b{L.total};
  const int64_t off_counts = b.take(4 * nc * std::max(D, 1));
  const int64_t off_bad = b.take(4 * nc);
  const int64_t off_badp = b.take(4LL * K);
  const int64_t off_colmax = b.take(8LL * kCatQMax * nc);
  const int64_t off_hs = b.take(8LL * (kCatQMax + 2) * K);
  const int64_t off_wmax = row_weight ? b.take(8 * nc) : 0;  // weighted fits only
  g_stats.n_chunks = pl.n_chunks;

  Workspace ws(stream);
  rc = ws.acquire(opt.workspace, opt.workspace_bytes, b.o, WsPolicy::kOwnIfSmall);
  if (rc != DLSA_OK) return rc;
  int64_t* d_offsets = (int64_t*)ws.at(L.off_offsets);
  int32_t* d_pcb = (int32_t*)ws.at(L.off_pcb);
  int32_t* d_counts = (int32_t*)ws.at(off_counts);
  int32_t* d_bad = (int32_t*)ws.at(off_bad);
  int32_t* d_badp = (int32_t*)ws.at(off_badp);
  double* d_colmax = (double*)ws.at(off_colmax);
  double* d_hs = (double*)ws.at(off_hs);

  auto upload = [&](const Plan& qn) -> hipError_t {
    return upload_plan_tables(qn, K, ws.at(L.off_row0), ws.at(L.off_rows), ws.at(L.off_part),
                              d_pcb, stream);
  };
  {
    // the final plan is uploaded for the presence pass and again as the last
    // level, every other level once
    size_t need = staged_bytes(8 * ((size_t)K + 1)) + plan_staged_bytes(pl, K) +
                  staged_bytes(8 * ((size_t)kCatQMax + 2) * K);  // + the grids
    for (const Plan& qn : plans) need += plan_staged_bytes(qn, K);
    DLSA_HIP_TRY(pinned_arena_reserve(need));
  }
  DLSA_HIP_TRY(staged_upload(d_offsets, offsets, 8LL * (K + 1), stream));

  SolveArgs sa = newton_solve_args(ws, L.ns, out, P, family, tol);
  sa.part_chunk_begin = d_pcb;
  sa.slab_H = (double*)ws.at(L.off_slabH);
  sa.slab_g = (double*)ws.at(L.off_slabg);
  sa.slab_ll = (double*)ws.at(L.off_slabll);
  sa.NT = pl.NT;
  sa.escalate_to = PHASE_F64;  // every categorical pass is exact
  // Poisson: the start values, the constant-term partials and the state of
  // the grids live in an allocation of the fit's own, as in fit_fused.hip (the
  // workspace layout is the logistic one)
  Workspace pws(stream);
  double *d_bounds = nullptr, *d_thsnap = nullptr;
  if (pois) {
    Bump pb;
    const int64_t off_t0 = pb.take(8LL * std::max(K, 1));
    const int64_t off_llc = pb.take(8 * nc);
    const int64_t off_mumax = pb.take(8LL * std::max(K, 1));
    const int64_t off_snap = pb.take(8LL * std::max(K, 1) * P);
    const int64_t off_bounds = pb.take(8LL * std::max(K, 1) * kCatPoisBounds);
    const int64_t off_ymax = pb.take(8 * nc), off_omax = pb.take(8 * nc);
    const int64_t off_pwmax = pb.take(8 * nc);
    if (int prc = pws.alloc(pb.o)) return prc;
    DLSA_HIP_TRY(hipMemsetAsync(pws.at(0), 0, pb.o, stream));
    sa.theta0 = (const double*)pws.at(off_t0);
    sa.slab_llc = (double*)pws.at(off_llc);
    ca.slab_llc = sa.slab_llc;
    ca.mumax = (unsigned long long*)pws.at(off_mumax);
    ca.ymax = (double*)pws.at(off_ymax);
    ca.omax = (double*)pws.at(off_omax);
    ca.wmax = (double*)pws.at(off_pwmax);
    d_thsnap = (double*)pws.at(off_snap);
    d_bounds = (double*)pws.at(off_bounds);
  }
  DLSA_HIP_TRY(fit_init(sa, d_offsets, K, PHASE_F64, stream));
  // prior weights: a negative or non-finite omega ends its partition
  // NONFINITE, sum omega = 0 SINGULAR, before the presence pass marks missing
  // levels among the partitions still running
  // (Poisson: also a negative or non-finite y or offset, sum omega y = 0
  // SINGULAR, and the start point log(sum omega y / sum omega e^o))
  if (row_weight || pois)
    DLSA_HIP_TRY(launch_fit_prepass(family, y, eta_offset, row_weight, d_offsets, K, P, ic,
                                    out.theta, const_cast<double*>(sa.theta0), sa.phase,
                                    out.status, stream));

  ca.Xn = Xn;
  ca.codes = codes;
  ca.y = y;
  ca.row_weight = row_weight;
  ca.eta_offset = eta_offset;
  if (!pois) ca.wmax = row_weight ? (double*)ws.at(off_wmax) : nullptr;
  ca.chunk_row0 = (const int64_t*)ws.at(L.off_row0);
  ca.chunk_rows = (const int32_t*)ws.at(L.off_rows);
  ca.chunk_part = (const int32_t*)ws.at(L.off_part);
  ca.phase = sa.phase;
  ca.theta = out.theta;
  ca.center = center;
  ca.scale = scale;
  ca.slab_H = (double*)ws.at(L.off_slabH);
  ca.slab_g = (double*)ws.at(L.off_slabg);
  ca.slab_ll = (double*)ws.at(L.off_slabll);
  ca.NT = pl.NT;
  ca.want_phase = PHASE_F64;

  // level presence over all rows: partitions missing a level -> zero frame;
  // invalid codes fail the call.  The same pass takes max |x_i| per column for
  // the fixed-point grids of the histograms (cat_pass.hip).
  Readback h;
  if (!h.init(K)) return DLSA_E_HIP;
  std::vector<int32_t> h_badp(K, 0);
  std::vector<double> h_colmax((size_t)kCatQMax * nc, 0.0);
  std::vector<double> h_wmax(row_weight ? (size_t)nc : 0, 0.0);
  DLSA_HIP_TRY(upload(pl));
  if (pois) {
    DLSA_HIP_TRY(launch_cat_presence_pois(ca, pl.n_chunks, d_counts, d_bad, d_colmax, stream));
  } else if (row_weight) {
    DLSA_HIP_TRY(launch_cat_presence_wgt(ca, pl.n_chunks, d_counts, d_bad, d_colmax, stream));
    if (pl.n_chunks > 0)
      DLSA_HIP_TRY(hipMemcpyAsync(h_wmax.data(), ca.wmax, 8LL * pl.n_chunks,
                                  hipMemcpyDeviceToHost, stream));
  } else {
    DLSA_HIP_TRY(launch_cat_presence(ca, pl.n_chunks, d_counts, d_bad, d_colmax, stream));
  }
  if (pl.n_chunks > 0)
    DLSA_HIP_TRY(hipMemcpyAsync(h_colmax.data(), d_colmax, 8LL * kCatQMax * pl.n_chunks,
                                hipMemcpyDeviceToHost, stream));
  if (D > 0) {
    DLSA_HIP_TRY(launch_cat_mark(ca, d_pcb, d_counts, d_bad, K, sa.phase, out.status, d_badp,
                                 stream));
    DLSA_HIP_TRY(hipMemcpyAsync(h_badp.data(), d_badp, 4LL * K, hipMemcpyDeviceToHost, stream));
  }
  DLSA_HIP_TRY(read_phases(sa, K, h, stream));
  std::vector<double> hc(q, 0.0), hs(q, 1.0);
  if (center && q > 0) {
    DLSA_HIP_TRY(hipMemcpy(hc.data(), center, 8LL * q, hipMemcpyDeviceToHost));
    DLSA_HIP_TRY(hipMemcpy(hs.data(), scale, 8LL * q, hipMemcpyDeviceToHost));
  }
  if (pois) {
    // the grids are written before every pass; here only what they are sized
    // from, per partition, on the device
    DLSA_HIP_TRY(launch_cat_pois_bounds(ca, d_pcb, K, d_colmax, d_bounds, out.theta,
                                        out.status, stream));
  } else {
    // (staged into the pinned arena on upload)
    const std::vector<double> h_hs =
        cat_grids(plans, K, q, center != nullptr, h_colmax, h_wmax, hc, hs);
    DLSA_HIP_TRY(staged_upload(d_hs, h_hs.data(), 8LL * (kCatQMax + 2) * K, stream));
  }
  ca.hscale = d_hs;
  for (int k = 0; k < K; ++k)
    if (h_badp[k]) {
      set_error("partition " + std::to_string(k) + ": " + std::to_string(h_badp[k]) +
                " level codes >= levels[f]");
      return DLSA_E_INVALID;
    }
  int n_running[kRunPhases] = {0, 0, 0};
  for (int k = 0; k < K; ++k) n_running[PHASE_F64] += h.phase[k] == PHASE_F64;

  const bool standardize = center != nullptr;
  StreamTimer timed{stream, opt.record_timing != 0};
  const bool trace = trace_enabled();
  const double rmax = (double)std::max(1024, pl.max_chunk_rows);
  auto pass_and_solve = [&](const Plan& qn, const std::vector<int64_t>& part_rows,
                            bool clear_counters) -> hipError_t {
    if (pois) {  // this pass's grids, from theta and the last pass's largest mu
      hipError_t eg = launch_cat_pois_grid(ca, K, d_bounds, d_thsnap, d_hs, rmax, stream);
      if (eg != hipSuccess) return eg;
    }
    hipError_t e = timed(&g_stats.ms_pass_fp64, [&] {
      return pois         ? launch_cat_pass_pois(ca, standardize, qn.n_chunks, stream)
             : row_weight ? launch_cat_pass_wgt(ca, standardize, qn.n_chunks, stream)
                          : launch_cat_pass(ca, standardize, qn.n_chunks, stream);
    });
    g_stats.passes_fp64++;
    g_stats.rows_fp64 += phase_rows(part_rows, h.phase, PHASE_F64);
    if (e == hipSuccess && clear_counters) e = hipMemsetAsync(sa.counters, 0, 16, stream);
    if (e == hipSuccess)
      e = timed(&g_stats.ms_solve, [&] { return launch_newton_solve(sa, K, stream); });
    return e;
  };

  // (the phases of level 0 are the presence pass's; a level neither clears
  // dm_prev / stall nor has a switch: there is no approximate phase)
  int it = 0;
  for (size_t lvl = 0; lvl < plans.size(); ++lvl) {
    const Plan& qn = plans[lvl];
    const bool final_level = lvl + 1 == plans.size();
    const std::vector<int64_t> part_rows = plan_part_rows(qn, K);
    DLSA_HIP_TRY(upload(qn));
    if (lvl > 0) DLSA_HIP_TRY(reenter_level(sa, K, PHASE_F64, h, n_running, stream));
    const int it_end = begin_level(sa, final_level, true, 0.0, it, max_iter);
    if (it_end <= it) continue;  // no budget left for this warm-start level
    for (; it < it_end && running_total(n_running) > 0 && qn.n_chunks > 0; ++it) {
      DLSA_HIP_TRY(pass_and_solve(qn, part_rows, true));
      DLSA_HIP_TRY(read_counters(sa, K, h, n_running, stream));
      if (trace) DLSA_HIP_TRY(trace_iteration(K, sa, lvl, it, n_running));
    }
  }
  g_stats.iterations = it;
  // polish: Sig_inv of a partition the budget left running at the theta it
  // returns (one more exact pass, no step; see fit_fused.hip).  The final
  // level's plan, pl, is on the device: it was the last uploaded.
  if (running_total(n_running) > 0 && pl.n_chunks > 0) {
    g_stats.polish_partitions = running_total(n_running);
    sa.eval_only = 1;
    sa.subsample = 0;
    DLSA_HIP_TRY(pass_and_solve(pl, plan_part_rows(pl, K), false));
    sa.eval_only = 0;
  }
  return fit_end(start, sa, K, out.sig_inv_theta, timed);
}

}  // namespace dlsa
