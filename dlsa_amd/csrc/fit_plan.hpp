// Host-side planning of the batched fits: row chunks, warm-start levels,
// workspace layouts and the categorical LDS layout.  Everything here turns
// (offsets, K, p, intercept, rows_per_chunk, options) into plans and byte
// offsets and calls no HIP runtime function, so it runs (and is tested,
// through dlsa_logistic_workspace_bytes) on a machine without a GPU.
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "dlsa_internal.hpp"

namespace dlsa {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Bump allocation of a device buffer's regions: every region starts on a
// multiple of 256 bytes; `o` is the size of the buffer so far.
struct Bump {
  int64_t o = 0;
  int64_t take(int64_t bytes) {
    const int64_t r = o;
    o = align_up(o + bytes, 256);
    return r;
  }
};

struct Plan {
  int P = 0, NT = 0, T = 0, PP = 0;
  int n_chunks = 0;
  int max_chunk_rows = 0;
  std::vector<int64_t> chunk_row0;
  std::vector<int32_t> chunk_rows, chunk_part, part_chunk_begin;
};

// Chunking: ~8192 chunks, each a run of consecutive rows of one partition.  The
// cooperative pass runs one 4-wave workgroup per chunk (2 per CU: 512 in
// flight), the per-wave fp64 pass one wave per chunk (4 per CU: 1024 in
// flight), so a launch is whole rounds of either; the partial tiles
// (T * 2 KiB per chunk) stay ~1 % of the X traffic.  Measured at config 2
// (cooperative bf16 / fp64 pass ms): 1024 chunks 22.0 / 42.5, 2048 19.4 /
// 36.6, 4096 18.2 / 34.7, 8192 17.4 / 33.2, 16384 17.0 / 32.8 (but the Newton
// solve reads every chunk's partial tiles: 0.65 -> 0.74 ms per iteration).
// Round 2 (current kernels): ~6144 chunks of at least 4096 rows.  Config 2
// at 16384 rows per chunk (6144 chunks) against the old 8448: 82.8-84.1 vs
// 84.6-91.0 ms alternated on one box, 86.2-86.6 vs 86.3-86.6 on another
// (profiles/r02ap_c2_chunk_ab.txt, r02ar_c2_chunk_ab.txt); at the
// strong-scaling share of config 2 (n = 1.25e7 per GPU, 1525 rows per chunk
// by the old rule) 3072 / 6144-row chunks fit 12.8 / 12.7 ms against 13.5 ms
// (fewer per-chunk prologues and partial tiles; r02am).  Round 5 (current
// kernels, r05j, alternated): at that share 4096 / 6144 / 8192 / 12288 rows
// per chunk fit 11.10-11.28 / 10.70-10.73 / 10.85-10.97 / 10.71-10.81 ms, so the
// floor is 6144 rows (2048 chunks there; config 2 itself is unchanged).
inline int auto_rows_per_chunk(int64_t n_total) {
  if (const char* e = env_knob("DLSA_ROWS_PER_CHUNK")) return std::max(64, atoi(e));
  // rounded up to a multiple of 1024: equal partitions then split into whole
  // chunks (config 2: 16384 rows, 6 per partition) instead of a ragged extra one
  int64_t r = (n_total / 6144 + 1023) / 1024 * 1024;
  r = std::max<int64_t>(6144, std::min<int64_t>(r, 131072));
  return (int)r;
}

// rows_used(k) = clamp(ceil(frac * n_k), min_rows, n_k): a prefix of each
// partition (frac = 1: all rows).
inline int64_t rows_used(int64_t nk, double frac, int64_t min_rows) {
  if (frac >= 1.0) return nk;
  return std::min(nk, std::max(min_rows, (int64_t)std::ceil(frac * (double)nk)));
}
// warm-start row-prefix fractions (ascending, each < 1); DLSA_LEVELS="a,b,..."
// overrides (schedule sweeps, tools/level_sweep.sh), DLSA_LEVELS="" disables.
// A level using more than half of all rows is skipped, so "x,0.5" runs as
// "x" alone at config 2 (odd n_k round up).  Fused pass (config 2,
// profiles/r01m_level_sweep.jsonl, 6-step means): one 1/16 level at a
// 0.2-relative step 101 ms per fit vs 110 ms for 1/16, 1/4 at 0.1 (6 bf16 +
// 1 fp64 launches instead of 9 + 1: the 1/4 level's passes cost more than
// the one full pass they save).  Wide path: 1/16, 1/4 at 0.1, with a level
// dropped when the next has under twice its rows (wide_level_plans; config 5
// runs 1/4 alone) -- other schedules were within noise, slower (1/4 at a
// 0.15 tolerance: 56.4 ms fit, r06h) or triggered a second fp64 Gram pass.
inline std::vector<double> warm_level_fracs(bool fused) {
  std::vector<double> f = fused ? std::vector<double>{1.0 / 16.0}
                                : std::vector<double>{1.0 / 16.0, 1.0 / 4.0};
  if (const char* e = env_knob("DLSA_LEVELS")) {
    f.clear();
    for (const char* s = e; *s;) {
      char* end = nullptr;
      const double v = strtod(s, &end);
      if (end == s) break;
      if (v > 0.0 && v < 1.0) f.push_back(v);
      s = (*end == ',') ? end + 1 : end;
    }
  }
  return f;
}
// iteration budget of one warm-start level: at most kLevelIters and at most
// half of what is left of max_iter, so the levels and the full-data level
// together run at most max_iter iterations (sklearn's n_iter_ <= max_iter)
// and the full-data level always gets at least one; max_iter = 1 runs no
// level at all.
constexpr int kLevelIters = 10;
inline int iter_budget(bool final_level, int it, int max_iter) {
  if (final_level) return std::max(1, max_iter - it);
  return std::min(kLevelIters, (max_iter - it) / 2);
}

// fewest rows of a warm-start level per parameter (DLSA_LEVEL_ROWS_PER_P
// overrides in knob builds, schedule sweeps)
inline int64_t level_rows_per_param() {
  if (const char* e = env_knob("DLSA_LEVEL_ROWS_PER_P")) return std::max<int64_t>(1, atoll(e));
  return 64;
}

// a level stops once its max relative step is below this; DLSA_LEVEL_TOL overrides
inline double warm_level_tol(bool fused) {
  if (const char* e = env_knob("DLSA_LEVEL_TOL")) return atof(e);
  return fused ? 0.2 : 0.1;
}

inline int64_t level_rows(const int64_t* offsets, int K, double frac, int64_t min_rows) {
  int64_t n = 0;
  for (int k = 0; k < K; ++k) n += std::max<int64_t>(0, rows_used(offsets[k + 1] - offsets[k], frac, min_rows));
  return n;
}

// The longest chunk any plan holds.  The fused passes (irls_coop_impl.hpp,
// irls_wave_impl.hpp, irls_oz_impl.hpp, ols_stream.hip) read a chunk's X
// through one raw buffer resource of at most 0x7FFFFFF0 bytes (uniform_rsrc)
// with 32-bit offsets from the chunk's first 16-byte boundary, and a load past
// the resource's end returns zeros instead of faulting: a longer chunk would
// be fitted with its later rows read as zero rows.  So a chunk's X stays under
// 2^31 bytes less 1 MiB: the room holds the 15 bytes of alignment slack in
// front and what the last block's pieces read behind the chunk's last row
// (less than one LDS slot, 160 KiB), so that every offset a block forms stays a
// positive int inside the resource.  The automatic sizes (at most 131072 rows
// of DLSA_MAX_P columns: 2^29 bytes) never get here; a caller's rows_per_chunk
// can, and is then a hint: make_plan splits evenly into more chunks.
constexpr int64_t kMaxChunkBytes = (int64_t(1) << 31) - (int64_t(1) << 20);
inline int64_t max_chunk_rows(int p) {
  return std::max<int64_t>(1, kMaxChunkBytes / (8LL * std::max(p, 1)));
}

// x_cols: the doubles of a row in memory, which the cap on a chunk's bytes
// counts (-1: p, the dense layout; the categorical-code layout holds its q
// numeric columns, not the P - intercept columns of the expanded design).
inline bool make_plan(const int64_t* offsets, int K, int p, int intercept, int rows_per_chunk,
                      Plan& pl, double frac = 1.0, int64_t min_rows = 0, int x_cols = -1) {
  pl.P = p + (intercept ? 1 : 0);
  pl.NT = (pl.P + 15) / 16;
  pl.T = pl.NT * (pl.NT + 1) / 2;
  pl.PP = 16 * pl.NT;
  // fused pass: chunk size from all rows (a warm-start level keeps the full
  // pass's chunk size: fewer, equally long chunks -- measured as fast)
  const int64_t n_total = offsets[K];
  const int64_t rpc = std::min<int64_t>(
      rows_per_chunk > 0 ? rows_per_chunk : auto_rows_per_chunk(n_total),
      max_chunk_rows(x_cols >= 0 ? x_cols : p));
  pl.part_chunk_begin.assign(K + 1, 0);
  pl.chunk_row0.clear();
  pl.chunk_rows.clear();
  pl.chunk_part.clear();
  for (int k = 0; k < K; ++k) {
    pl.part_chunk_begin[k] = (int32_t)pl.chunk_row0.size();
    const int64_t a = offsets[k];
    const int64_t nk = offsets[k + 1] - a;
    const int64_t n = rows_used(nk, frac, min_rows);
    if (n <= 0) continue;
    const int64_t nc = (n + rpc - 1) / rpc;
    for (int64_t c = 0; c < nc; ++c) {
      const int64_t r0 = a + n * c / nc, r1 = a + n * (c + 1) / nc;
      pl.chunk_row0.push_back(r0);
      pl.chunk_rows.push_back((int32_t)(r1 - r0));
      pl.chunk_part.push_back(k);
    }
  }
  pl.part_chunk_begin[K] = (int32_t)pl.chunk_row0.size();
  pl.n_chunks = (int)pl.chunk_row0.size();
  pl.max_chunk_rows = 0;
  for (int32_t r : pl.chunk_rows) pl.max_chunk_rows = std::max<int>(pl.max_chunk_rows, r);
  return true;
}

// The plans of a fused or categorical fit: the warm-start levels (`levels`:
// Newton on a row prefix of every partition) then all rows.  A level that
// would stream more than half of the rows, or none, is skipped.
// rows_per_chunk(frac, min_rows) is make_plan's rows_per_chunk for that level.
template <typename RowsPerChunk>
std::vector<Plan> level_plans(const int64_t* offsets, int K, int p, int intercept, bool levels,
                              RowsPerChunk rows_per_chunk, int x_cols = -1) {
  std::vector<Plan> plans;
  if (levels) {
    const int P = p + (intercept ? 1 : 0);
    const int64_t min_rows = std::max<int64_t>(2048, level_rows_per_param() * P);
    for (double frac : warm_level_fracs(true)) {
      Plan q;
      make_plan(offsets, K, p, intercept, rows_per_chunk(frac, min_rows), q, frac, min_rows,
                x_cols);
      if (level_rows(offsets, K, frac, min_rows) <= offsets[K] / 2 && q.n_chunks > 0)
        plans.push_back(std::move(q));
    }
  }
  Plan full;
  make_plan(offsets, K, p, intercept, rows_per_chunk(1.0, 0), full, 1.0, 0, x_cols);
  plans.push_back(std::move(full));
  return plans;
}

// The per-partition Newton state every fit carves from its workspace.  The
// counters and the phases are adjacent (counters first, as in the pinned
// staging): one readback per iteration.
struct NewtonState {
  int64_t off_counters, off_phase, off_bt, off_llprev, off_thprev, off_dprev;
  int64_t off_dmprev, off_stall;
};
inline NewtonState take_newton_state(Bump& b, int K, int P) {
  NewtonState s;
  s.off_counters = b.take(16 + 4LL * K);
  s.off_phase = s.off_counters + 16;
  s.off_bt = b.take(4LL * K);
  s.off_llprev = b.take(8LL * K);
  s.off_thprev = b.take(8LL * K * P);
  s.off_dprev = b.take(8LL * K * P);
  s.off_dmprev = b.take(8LL * K);
  s.off_stall = b.take(4LL * K);
  return s;
}

struct Layout {
  int64_t off_row0, off_rows, off_part, off_pcb, off_offsets;
  int64_t off_slabH, off_slabg, off_slabll;
  NewtonState ns;
  int64_t off_colmax, off_zcolmax, off_threc;  // Ozaki digit scales (PassArgs)
  int64_t total;
};

inline Layout make_layout(const Plan& pl, int K) {
  Layout L;
  Bump b;
  const int64_t nc = std::max(pl.n_chunks, 1);
  L.off_row0 = b.take(8 * nc);
  L.off_rows = b.take(4 * nc);
  L.off_part = b.take(4 * nc);
  L.off_pcb = b.take(4LL * (K + 1));
  L.off_offsets = b.take(8LL * (K + 1));
  L.off_slabH = b.take(8 * nc * pl.T * 256);
  L.off_slabg = b.take(8 * nc * pl.PP);
  L.off_slabll = b.take(8 * nc);
  L.ns = take_newton_state(b, K, pl.P);
  L.off_colmax = b.take(4 * nc * pl.PP);
  L.off_zcolmax = b.take(4 * nc * pl.PP);
  L.off_threc = b.take(8LL * K * pl.P);
  L.total = b.o;
  return L;
}

// ---- wide-P path (P > DLSA_MAX_P_FUSED): row chunks + Gram row groups ------
struct WidePlans {
  Plan rows, gram;
};

// Row pass (exact partitions): ~2048 chunks (one 256-thread workgroup each,
// HBM-bound).  Gram row groups (fused bf16 pass and fp64 Gram pass): >= 256,
// a multiple of 8 so the XCD-aware mappings fill every XCD.
inline void make_wide_plans(const int64_t* offsets, int K, int p, int intercept,
                            int rows_per_chunk, WidePlans& wp, double frac = 1.0,
                            int64_t min_rows = 0) {
  // wide path: row-group sizes from the rows this level streams, so a
  // warm-start level fills the chip like a full pass
  const int64_t n_total = level_rows(offsets, K, frac, min_rows);
  const int P = p + (intercept ? 1 : 0);
  const int NB = (P + kWideTile - 1) / kWideTile;
  const int TB = NB * (NB + 1) / 2;
  int rpc_row = (int)std::max<int64_t>(256, std::min<int64_t>(n_total / 2048, 16384));
  // >= 256 row groups: the fused pass runs 2 workgroups per row group above
  // PP = 256 (512 in all, 1 per CU), the fp64 Gram pass TB per row group;
  // measured at config 5 (p = 500), fp64 pass: 64 / 128 / 256 row groups ->
  // 43.8 / 36.8 / 36.1 ms
  const int64_t groups = (std::max<int64_t>(256, (1024 + TB - 1) / TB) + 7) / 8 * 8;
  int rpc_gram = (int)std::max<int64_t>(1024, std::min<int64_t>((n_total + groups - 1) / groups,
                                                                int64_t(1) << 24));
  if (rows_per_chunk > 0) rpc_row = rpc_gram = rows_per_chunk;
  if (const char* e = env_knob("DLSA_WIDE_GRAM_ROWS")) rpc_gram = std::max(64, atoi(e));
  // the Gram kernels address a row group's X with 32-bit buffer offsets: half
  // of what make_plan allows every chunk (kMaxChunkBytes), which the row plan gets
  rpc_gram = (int)std::min<int64_t>(rpc_gram, (int64_t(1) << 30) / (8LL * std::max(p, 1)));
  make_plan(offsets, K, p, intercept, rpc_row, wp.rows, frac, min_rows);
  make_plan(offsets, K, p, intercept, rpc_gram, wp.gram, frac, min_rows);
}

struct WideLayout {
  int64_t off_r_row0, off_r_rows, off_r_part, off_rcb;
  int64_t off_g_row0, off_g_rows, off_g_part, off_gcb;
  int64_t off_offsets, off_w, off_slabg, off_slabll, off_slabG, off_slabgz, off_slabllz, off_H;
  NewtonState ns;
  int64_t off_zmax, off_ozE;  // int8 exact Gram: row-chunk max |z|, digit exponents
  // int8 exact Gram digit records (wide_oz.hip): the last region, so that
  // base_total bytes hold everything else; digit_bytes = 0 when the final
  // plan's row groups are too long (> kWideOzMaxRows) or the records would
  // exceed kWideOzMaxDigitBytes (the fp64 Gram runs then)
  int64_t off_digits, digit_bytes, base_total;
  int64_t total;
  int64_t cap_rows, cap_gram;  // row-chunk / Gram-row-group capacity of the tables and slabs
};

// Largest digit-record region a wide fit asks for (above it: fp64 Gram).
constexpr int64_t kWideOzMaxDigitBytes = int64_t(32) << 30;

// Sized for the largest chunk counts over ALL level plans: a warm-start
// level's row groups are sized from its own (smaller) row count, so with
// uneven partitions it can have more row chunks / Gram row groups than the
// final plan (e.g. P = 512, n_k = [1e7, 1e5, 1e5]: 258 vs 257 Gram groups).
inline WideLayout make_wide_layout(const std::vector<WidePlans>& plans, int K, int64_t n_total,
                                   int P) {
  const int NB = (P + kWideTile - 1) / kWideTile;
  const int64_t PP = (int64_t)kWideTile * NB;
  const int64_t TB = NB * (NB + 1) / 2;
  int64_t nr = 1, ng = 1;
  for (const WidePlans& wp : plans) {
    nr = std::max<int64_t>(nr, wp.rows.n_chunks);
    ng = std::max<int64_t>(ng, wp.gram.n_chunks);
  }
  WideLayout L;
  Bump b;
  L.off_r_row0 = b.take(8 * nr);
  L.off_r_rows = b.take(4 * nr);
  L.off_r_part = b.take(4 * nr);
  L.off_rcb = b.take(4LL * (K + 1));
  L.off_g_row0 = b.take(8 * ng);
  L.off_g_rows = b.take(4 * ng);
  L.off_g_part = b.take(4 * ng);
  L.off_gcb = b.take(4LL * (K + 1));
  L.off_offsets = b.take(8LL * (K + 1));
  L.off_w = b.take(8 * std::max<int64_t>(n_total, 1));
  L.off_slabg = b.take(8 * nr * PP);
  L.off_slabll = b.take(8 * nr);
  L.off_slabG = b.take(8 * ng * TB * kWideTile * kWideTile);
  L.off_slabgz = b.take(8 * ng * PP);
  L.off_slabllz = b.take(8 * ng);
  L.off_H = b.take(8LL * K * PP * PP);
  L.ns = take_newton_state(b, K, P);
  L.off_zmax = b.take(4 * nr * PP);
  L.off_ozE = b.take(4 * ng * PP);
  L.base_total = b.o;
  const Plan& fg = plans.back().gram;
  const int64_t db = wide_oz_digit_bytes(fg.n_chunks, fg.max_chunk_rows, (int)PP);
  L.digit_bytes = (fg.max_chunk_rows <= kWideOzMaxRows && db <= kWideOzMaxDigitBytes) ? db : 0;
  L.off_digits = b.take(L.digit_bytes);
  L.total = b.o;
  L.cap_rows = nr;
  L.cap_gram = ng;
  return L;
}

// The wide path's plans: the warm-start levels (logistic, warm_start) then
// all rows.  A level that would stream more than half of the rows is
// skipped (it would cost more than the full passes it saves).  A level
// whose row count is less than twice the previous level's replaces it: the
// min_rows floor can lift a small fraction to nearly the next one (config 5:
// 1/16 of n_k = 156250 is raised to 64 x 500 = 32000 rows, the 1/4 level has
// 39063), and two levels that close cost a level's iterations twice for the
// same start.  Config 5, one box, 4 A/B pairs (profiles/r06h_level_ab.txt):
// 1/16 + 1/4 10 iterations, fit 54.1-54.2 ms; 1/4 alone 9, 52.7-52.8 ms.
inline std::vector<WidePlans> wide_level_plans(const int64_t* offsets, int K, int p, int intercept,
                                               int rows_per_chunk, bool levels) {
  std::vector<WidePlans> plans;
  const int P = p + (intercept ? 1 : 0);
  if (levels) {
    const int64_t min_rows = std::max<int64_t>(2048, level_rows_per_param() * P);
    int64_t prev_rows = 0;
    for (double frac : warm_level_fracs(false)) {
      WidePlans q;
      make_wide_plans(offsets, K, p, intercept, rows_per_chunk, q, frac, min_rows);
      const int64_t rows = level_rows(offsets, K, frac, min_rows);
      if (rows > offsets[K] / 2 || q.rows.n_chunks == 0) continue;
      if (!plans.empty() && rows < 2 * prev_rows) plans.pop_back();
      plans.push_back(std::move(q));
      prev_rows = rows;
    }
  }
  WidePlans fin;
  make_wide_plans(offsets, K, p, intercept, rows_per_chunk, fin);
  plans.push_back(std::move(fin));
  return plans;
}

inline int check_offsets(const int64_t* offsets, int K) {
  if (!offsets || K < 1) {
    set_error("offsets must be a host array of K+1 >= 2 entries");
    return DLSA_E_INVALID;
  }
  if (offsets[0] != 0) {
    set_error("offsets[0] must be 0");
    return DLSA_E_INVALID;
  }
  for (int k = 0; k < K; ++k)
    if (offsets[k + 1] < offsets[k]) {
      set_error("offsets must be non-decreasing");
      return DLSA_E_INVALID;
    }
  for (int k = 0; k < K; ++k)
    if (offsets[k + 1] - offsets[k] > (int64_t)INT32_MAX) {
      set_error("a partition holds more than 2^31-1 rows");
      return DLSA_E_INVALID;
    }
  return DLSA_OK;
}

// Shape of a categorical-code problem: q numeric columns and F factors of
// levels[f] levels give D = sum(levels - 1) dummy columns and
// P = intercept + q + D parameters, P <= max_P (`what` names the caller in the
// error text: "fit" or "evaluation").
inline int check_cat_shape(int q, int F, const int32_t* levels, int intercept, int max_P,
                           const char* what, int* D_out, int* P_out) {
  if (q < 0 || F < 0 || F > kCatMaxFactors || (F > 0 && !levels)) {
    set_error("need 0 <= q, 0 <= F <= 16 and a host levels[F] array");
    return DLSA_E_INVALID;
  }
  int D = 0;
  for (int f = 0; f < F; ++f) {
    if (levels[f] < 1 || levels[f] > 256) {
      set_error("levels[" + std::to_string(f) + "] must be in 1..256 (uint8 codes)");
      return DLSA_E_INVALID;
    }
    D += levels[f] - 1;
  }
  const int P = intercept + q + D;
  if (P < 1 || P > max_P || intercept + q > kCatQMax) {
    set_error(std::string("categorical ") + what +
              " needs 1 <= P = intercept + q + sum(levels - 1) <= " + std::to_string(max_P) +
              " and intercept + q <= " + std::to_string(kCatQMax) + " (got P = " +
              std::to_string(P) + ")");
    return DLSA_E_UNSUPPORTED;
  }
  *D_out = D;
  *P_out = P;
  return DLSA_OK;
}

// level slots x replicas per factor of the numeric x dummy histograms before
// the LDS budget shrinks them
constexpr int kCatNdCap = 256;
// LDS layout of the categorical pass's histograms (cat_pass.hip): replicas so
// that a frequent level does not serialise the lanes of a wave on one address
// (nd: <= 128 slots per factor, pairs: <= 512 cells), shrunk until the
// workgroup fits 160 KB.
inline bool cat_layout(CatArgs& a, const int32_t* levels) {
  const int Qw = (a.q + 1) | 1;
  a.nd_stride = Qw;
  // the exact-bucket kernel folds the intercept row into the histograms of the
  // factor with the most levels (its baseline is the rarest: fewest extra adds)
  a.fold = -1;
  if (cat_exact_bucket(a))
    for (int f = 0; f < a.F; ++f)
      if (a.fold < 0 || levels[f] > levels[a.fold]) a.fold = f;
  int nd_cap = kCatNdCap, pr_cap = 512;
  for (int attempt = 0; attempt < 12; ++attempt) {
    int64_t o = 0;
    for (int f = 0; f < a.F; ++f) {
      const int nl = levels[f] - 1;
      const int ns = nl + (f == a.fold ? 1 : 0);  // level slots per replica
      int R = 1;
      while (R < 16 && ns * R * 2 <= nd_cap) R *= 2;
      a.nlev[f] = nl;
      a.nd_lev[f] = ns;
      a.nd_rep[f] = R;
      a.nd_off[f] = (int32_t)o;
      o += (int64_t)R * ns * Qw;
    }
    for (int f = 0; f < a.F; ++f) {
      a.g_off[f] = (int32_t)o;
      o += (int64_t)a.nd_rep[f] * a.nd_lev[f];
    }
    for (int f = 0; f < a.F; ++f)
      for (int g = f + 1; g < a.F; ++g) {
        const int pi = f * a.F - f * (f + 1) / 2 + (g - f - 1);
        const int cells = a.nlev[f] * a.nlev[g];
        int R = 1;
        while (R < 8 && cells * R * 2 <= pr_cap) R *= 2;
        a.pr_rep[pi] = R;
        a.pr_off[pi] = (int32_t)o;
        o += (int64_t)R * cells;
      }
    a.hist_doubles = (int32_t)std::min<int64_t>(o, INT32_MAX);
    if (cat_lds_bytes(a) + kCatStaticLds <= 160 * 1024) return true;
    if (nd_cap == 1 && pr_cap == 1) break;
    nd_cap = std::max(1, nd_cap / 2);
    pr_cap = std::max(1, pr_cap / 2);
  }
  return false;
}

// Rows a pass of phase `ph` streams: the rows (in this level's plan) of the
// partitions whose phase is ph.  The partition phases are read back with the
// per-iteration counters (stats only: rows_fp32 / rows_fp64).
inline std::vector<int64_t> plan_part_rows(const Plan& q, int K) {
  std::vector<int64_t> r(K, 0);
  for (int k = 0; k < K; ++k)
    for (int c = q.part_chunk_begin[k]; c < q.part_chunk_begin[k + 1]; ++c) r[k] += q.chunk_rows[c];
  return r;
}
inline int64_t phase_rows(const std::vector<int64_t>& part_rows, const int32_t* phase, int ph) {
  int64_t n = 0;
  for (size_t k = 0; k < part_rows.size(); ++k)
    if (phase[k] == ph) n += part_rows[k];
  return n;
}

}  // namespace dlsa
