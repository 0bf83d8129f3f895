// Per-wave fp64 IRLS pass (gfx950 / CDNA4): one 64-lane workgroup streams a
// chunk of rows of one partition through its OWN LDS-DMA ring and owns every
// lower-triangle 16x16 tile of X^T W X in registers.  Instantiated by
// irls_wave.hip.
//
// Replaces, per Newton iteration, the per-partition work of the reference map
// stage (sklearn newton-cg Hessian products, predict_proba and
// Sig_inv = X^T diag(p(1-p)) X, dlsa/models.py:110-131) with ONE pass over X;
// this is the exact (fp64-MFMA) pass whose Hessian is returned as Sig_inv
// (models.py:130) and the single pass of the OLS path.
//
// Why a wave-private design for fp64: on gfx950 fp64 VALU
// work and v_mfma_f64_16x16x4 never execute together on a SIMD
// (SQ_VALU_MFMA_COEXEC_CYCLES = 0 in profiles/r01f_pmc.csv), so the pass time
// is MFMA cycles + VALU cycles + stalls, and everything that is not an MFMA
// must be cut rather than overlapped:
//   * no barriers: a wave reads only the rows it DMA'd itself, so the row
//     phase (eta, w, r, log-lik, gradient) and the tile phase need no
//     workgroup synchronisation and the next block's DMA stays in flight
//     across both phases (s_waitcnt vmcnt counted, never drained);
//   * the row phase runs R = 64 / LPR rows at once (16 at LPR = 4), so the fp64
//     exp / division / log1p sequences cost one instruction stream per 16
//     rows instead of per 8 (the cooperative kernel) or per 4 (a k-step);
//   * the tile phase loads each column tile's operand once per k-step (NT
//     ds_read_b64), forms w*x with NT multiplies and issues all T MFMAs --
//     the same static code in every wave (no per-wave tile assignment whose
//     branch merges copy accumulators).
// T accumulators of 8 registers (224 at NT = 7) force one wave per SIMD;
// LPR = 8 (R = 8) above NT = 7 keeps the row-phase registers in budget.
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <array>
#include <type_traits>
#include <utility>

#include "dlsa_internal.hpp"
#include "glm_row.hpp"

namespace dlsa {

typedef double wd4 __attribute__((ext_vector_type(4)));

// Ring slots per workgroup: one block in flight while the current one is
// computed.  Three slots (two blocks in flight) for the OLS pass (8-row, 4 KiB
// blocks at P = 64) measured slower (config-4 pass 16.7-17.1 vs 14.9-15.2 ms,
// profiles/r04h_ols_ab.txt).
constexpr int kWaveSlots = 2;
// Ring slot: [16 B pad][npieces KiB of X rows][the row streams: y, the row
// extras (glm_row.hpp)]
__host__ __device__ __forceinline__ int wave_npieces(int RB, int p) {
  return (RB * p * 8 + 16 + 1023) / 1024;
}
__host__ __device__ __forceinline__ int wave_slot_bytes_impl(int RB, int p, int n_extras = 0) {
  return 16 + wave_npieces(RB, p) * 1024 + row_streams_bytes(n_extras);
}
// LDS of one workgroup: 2 ring slots + w of a block [RB] + theta [PMAX] +
// center / 1/scale [2][PMAX]
__host__ __device__ __forceinline__ int wave_lds_bytes_impl(int NT, int RB, int p,
                                                            int n_extras = 0) {
  return kWaveSlots * wave_slot_bytes_impl(RB, p, n_extras) + RB * 8 + 3 * 16 * NT * 8;
}

// Waves per workgroup.  W = 2 (P <= 112): the T tiles are split over two
// waves by whole tile rows (each holds ~T/2 accumulators, <= 256 registers),
// so two workgroups' waves share every SIMD and one wave's LDS / DMA /
// dependency waits are covered by the other's MFMAs; the rows of a block are
// split between the waves in the row phase (P >= 17).  W = 1 (P <= 128): all T tiles
// in one wave, one wave per SIMD.
constexpr int wave_w_default(int NT) { return (NT >= 2 && NT <= 7) ? 2 : 1; }
// Lanes per row in the row phase: 4 (16 rows per wave) at W = 1, P <= 112; 16 (4
// rows per wave, 8-row blocks) for OLS at W = 2, P <= 64; else 8.  The OLS
// setting halves the ring (12 vs 21 KB per workgroup at P = 64: LDS allowed only
// 3.5 waves per SIMD) and runs 5 waves per SIMD (wave_min_waves): config-4 pass
// 16.2 vs 17.4 ms (profiles/r02at_lpr_ab.txt).  Logistic keeps 8: its exp / rcp /
// log sequence runs once per RW rows, and 4-row (or 16-row, RB = 32: 3.5 -> 2
// waves per SIMD by LDS) blocks measured slower at P = 64 (4.3 / 4.8 vs 3.4 ms,
// r02at / r02as).
constexpr int wave_lpr(int NT, int W, int FAM) {
  return (W > 1 && NT <= 4 && FAM == FAMILY_GAUSSIAN) ? 16 : (W == 1 && NT <= 7) ? 4 : 8;
}
constexpr int wave_rb(int NT, int W, int FAM) { return W * (64 / wave_lpr(NT, W, FAM)); }

// Edge strip.  The last tile row holds only
// s = P - 16 (NT - 1) parameter rows (4 at P = 100).  On the MI355X a
// v_mfma_f64_4x4x4_4b issues every ~7 ns per SIMD (75 TF/s chip-wide;
// tools/mfma4_probe.hip, profiles/r02_mfma4_probe.txt) -- a quarter of a
// 16x16x4's flops in a fraction of its issue time -- so with NS > 0 the
// strip's tiles are NS 4x4x4_4b sub-blocks each instead of one 16x16x4
// (NS = 1 for s <= 4, 2 for s <= 8).  4x4x4_4b maps (probe): A lane
// i + 4 b + 16 k, B lane j + 4 b + 16 k, D lane j + 4 b + 16 i, block b
// independent (CBSZ / ABID broadcasts have no effect on it), so the A operand
// of sub-block r is feature 16 (NT - 1) + 4 r + (l & 3) of row k in every
// block -- read from LDS -- and B is the 16x16x4 column operand unchanged:
// D lane j + 4 b + 16 i = H[16 (NT - 1) + 4 r + i][16 J + 4 b + j].
// (Computing every tile as 4x4x4_4b sub-blocks against DPP-rotated B -- the
// probe's 75 TF/s shape -- measured slower in this kernel: 31.0 vs 29.3 ms per
// config-2 exact pass, profiles/r02w_mf4_ab.txt.)
// OLS: the tile phase takes x itself as the A operand (no w * x multiplies;
// padded rows are zeroed in the ring by the row phase): 16.2-16.4 vs
// 16.4-16.5 ms per config-4 pass (profiles/r02av_ols_nomul_ab.txt)
constexpr int wave_strip_ns(int NT, int P) {
  return (NT < 2)                     ? 0
         : (P - 16 * (NT - 1) <= 4)   ? 1
         : (P - 16 * (NT - 1) <= 8)   ? 2
                                      : 0;
}

// MFMA time of tile row I in quarter tiles (a 4x4x4_4b ~ 1/4 of a 16x16x4
// issue slot, conservatively)
constexpr int wave_row_cost(int NT, int NS, int I) {
  return (NS > 0 && I == NT - 1) ? NT * NS : 4 * (I + 1);
}

// tile rows of wave `wid`: rows are dealt most expensive first to the lighter
// wave (NT = 7, no strip: {6, 3, 2} and {5, 4, 1, 0}, 14 tiles each; NS = 1:
// {5, 2, 1} and {4, 3, 6, 0}, 44 / 47 quarter tiles)
constexpr unsigned wave_rows_mask(int NT, int NS, int W, int wid) {
  if (W == 1) return (1u << NT) - 1;
  int load0 = 0, load1 = 0;
  unsigned m0 = 0, m1 = 0, done = 0;
  for (int n = 0; n < NT; ++n) {
    int best = -1;
    for (int I = NT - 1; I >= 0; --I)
      if (!((done >> I) & 1u) &&
          (best < 0 || wave_row_cost(NT, NS, I) > wave_row_cost(NT, NS, best)))
        best = I;
    done |= 1u << best;
    if (load0 <= load1) {
      load0 += wave_row_cost(NT, NS, best);
      m0 |= 1u << best;
    } else {
      load1 += wave_row_cost(NT, NS, best);
      m1 |= 1u << best;
    }
  }
  return wid == 0 ? m0 : m1;
}

template <int NT, int NS, int W, int WID>
struct WaveTiles {
  static constexpr unsigned RM = wave_rows_mask(NT, NS, W, WID);
  static constexpr int count() {
    int c = 0;
    for (int I = 0; I < NT; ++I)
      if ((RM >> I) & 1u) c += I + 1;
    return c;
  }
  static constexpr int TW = count();
  static constexpr int ncols() {  // B operands needed: columns 0 .. max I
    int c = 0;
    for (int I = 0; I < NT; ++I)
      if ((RM >> I) & 1u) c = I + 1;
    return c;
  }
  static constexpr int NC = ncols();
  static constexpr int I_of(int i) {  // tile i of this wave: rows ascending, J ascending
    for (int I = 0; I < NT; ++I)
      if ((RM >> I) & 1u) {
        if (i <= I) return I;
        i -= I + 1;
      }
    return -1;
  }
  static constexpr int J_of(int i) {
    for (int I = 0; I < NT; ++I)
      if ((RM >> I) & 1u) {
        if (i <= I) return i;
        i -= I + 1;
      }
    return -1;
  }
};

// workgroup sync of the block loop: this wave's LDS ops done, then (W > 1) a
// barrier without the vmcnt drain of __syncthreads (the next block's DMA
// stays in flight; lds_barrier)
template <int W>
__device__ __forceinline__ void wv_sync() {
  if constexpr (W > 1)
    lds_barrier();
  else
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

struct WaveCtx {
  int64_t row0;
  int nrows, nb, npieces, slot_bytes, slot_y, part, chunk;
  __amdgpu_buffer_rsrc_t xr, yr;
  uintptr_t xcb;
  __amdgpu_buffer_rsrc_t orr;  // EX_OFS: the chunk's rows of a.eta_offset
  __amdgpu_buffer_rsrc_t wrr;  // EX_WGT: the chunk's rows of a.row_weight
};

// The block loop + epilogue of wave WID (a separate code path per wave: no
// branch merges of the accumulator arrays).
// EX (row extras, EX_* mask), each streamed like y behind it (RowStreams,
// glm_row.hpp): EX_OFS (FAMILY_POISSON only) eta = x . theta +
// a.eta_offset[row]; EX_WGT prior weights omega = a.row_weight[row], which
// multiply w, r and the row's log-likelihood terms once, after mu.
template <int NT, int NS, int W, int WID, bool STD, int FAM, int EX = EX_NONE>
__device__ __forceinline__ void wave_body(const PassArgs& a, const WaveCtx& cx, char* smem) {
  using TL = WaveTiles<NT, NS, W, WID>;
  using RS = RowStreams<EX>;
  // strip tiles (the last tile row as NS 4x4x4_4b sub-blocks)
  constexpr auto strip = [](int I) { return NS > 0 && I == NT - 1; };
  constexpr bool HAS_STRIP = NS > 0 && ((TL::RM >> (NT - 1)) & 1u);
  constexpr int NSA = NS > 0 ? NS : 1;
  constexpr int LPR = wave_lpr(NT, W, FAM);
  constexpr int RW = 64 / LPR;   // rows of a block in this wave's row phase
  constexpr int RB = W * RW;     // rows per block
  constexpr int KS = RB / 4;     // MFMA k-steps per block
  constexpr int PMAX = 16 * NT;
  constexpr int M = PMAX / LPR;  // features per lane in the row phase
  constexpr int TW = TL::TW, NC = TL::NC;
  // OLS (w in {0, 1}): A operands are x itself (padded rows zeroed in the ring,
  // the intercept column = w)
  constexpr bool OLS_NOMUL = FAM == FAMILY_GAUSSIAN;
  // OLS is one pass at theta = 0 (fit_dense: fit_init zeroes theta, max_iter =
  // 1, no warm-start levels, no polish): eta = 0 and r = y, so the row phase
  // skips the x . theta dot products and their row reductions -- fp64 VALU
  // work that never co-executes with the fp64 MFMAs of the tile phase
  constexpr bool ETA0 = FAM == FAMILY_GAUSSIAN;

  const int lane = threadIdx.x & 63;
  const int p = a.p, P = a.P, ic = a.intercept;
  double* wv = (double*)(smem + kWaveSlots * cx.slot_bytes);  // [RB] w of the block's rows
  double* bet = wv + RB;                             // [PMAX] theta of the partition
  double* stdv = bet + PMAX;                         // [2][PMAX] center, 1/scale (STD)

  // row-phase lane map: row = WID * RW + lane % RW, feature group sl = lane / RW;
  // the lane handles parameters f = sl + LPR m (m < M)
  const int rl = lane % RW, sl = lane / RW;
  const int row = WID * RW + rl;
  double gacc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) gacc[m] = 0.0;
  double llacc = 0.0;
  [[maybe_unused]] double llcacc = 0.0;  // Poisson: -sum lgamma(y + 1)
  wd4 acc[TW];           // 16x16x4 tiles (AGPRs)
  double sacc[TW][NSA];  // strip sub-blocks (the unused entries of either are dead)
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    acc[i] = wd4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < NSA; ++r) sacc[i][r] = 0.0;
  }

  // DMA: wave WID issues pieces j = WID, WID + W, ...; the last wave also the
  // row streams (the wait below is for all of a wave's loads)
  auto issue = [&](int blk) {
    char* sbase = smem + (blk % kWaveSlots) * cx.slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (cx.row0 + (int64_t)blk * RB) * p);
    const int so = __builtin_amdgcn_readfirstlane((int)((start & ~(uintptr_t)15) - cx.xcb));
    for (int j = WID; j < cx.npieces; j += W)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(cx.xr, (lds_void_t*)(sbase + 16 + j * 1024), 16,
                                               lane * 16, so + j * 1024, 0, DLSA_X_DMA_AUX);
    if (WID == W - 1)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(cx.yr, (lds_void_t*)(sbase + cx.slot_y), 4,
                                               lane * 4, blk * RB * 8, 0, 0);
    if constexpr (RS::OFS)
      if (WID == W - 1)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(cx.orr,
                                                 (lds_void_t*)(sbase + cx.slot_y + RS::OFS_OFF),
                                                 4, lane * 4, blk * RB * 8, 0, 0);
    if constexpr (RS::WGT)
      if (WID == W - 1)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(cx.wrr,
                                                 (lds_void_t*)(sbase + cx.slot_y + RS::WGT_OFF),
                                                 4, lane * 4, blk * RB * 8, 0, 0);
  };

  const int fl = lane & 15, q = lane >> 4;
  const bool icpt_lane = ic && fl == 0;
  for (int b = 0; b < kWaveSlots - 1 && b < cx.nb; ++b) issue(b);
  for (int b = 0; b < cx.nb; ++b) {
    static_assert(kWaveSlots == 2, "one block in flight: the wait is for all of this wave's DMA");
    wait_vmcnt<0>();  // this wave's pieces of block b landed
    wv_sync<W>();        // every wave's pieces landed; block b-1 fully consumed
    if (b + kWaveSlots - 1 < cx.nb) issue(b + kWaveSlots - 1);  // into the slot of block b-1
    const char* slot = smem + (b % kWaveSlots) * cx.slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (cx.row0 + (int64_t)b * RB) * p);
    double* xs = (double*)(slot + 16 + (start & 15));
    const double* ys = (const double*)(slot + cx.slot_y);
    const int rows_left = cx.nrows - b * RB;
    // The chunk's last block: rows past the chunk's end and what the last
    // row's padded-feature lanes read behind the block (the next chunk's rows,
    // or the bytes after X up to its 16-byte boundary) are zeroed in the slot
    // -- w = 0 does not keep a NaN out (0 * NaN) -- up to the slot's y.
    if (__builtin_expect(b == cx.nb - 1, 0)) {  // workgroup-uniform; no DMA in flight to this slot
      double* zs = xs + rows_left * p;
      const int lim = (cx.npieces * 1024 - (int)(start & 15)) / 8;  // doubles of X bytes in the slot
      const int nz = min(RB * p + PMAX, lim) - rows_left * p;
      for (int i = WID * 64 + lane; i < nz; i += 64 * W) zs[i] = 0.0;
      wv_sync<W>();
    }

    // ---- row phase: RW rows of this wave, LPR lanes per row -------------------
    {
      const bool valid = row < rows_left;
      double* xrw = xs + row * p + (sl - ic);
      double xv[M];
      double e0 = 0.0, e1 = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        double v = xrw[LPR * m];
        if constexpr (STD) {
          v = (v - stdv[sl + LPR * m]) * stdv[PMAX + sl + LPR * m];
          const int f = sl + LPR * m;
          // standardise in place for the tile phase (own row, own features;
          // the intercept slot f = 0 is the previous row's last value)
          if (f >= ic && f < P) xrw[LPR * m] = v;
        }
        if constexpr (OLS_NOMUL) {
          // OLS: w is 1 on rows of the chunk and 0 past it; zero the padded
          // rows' features in place so the tile phase can skip w * x
          const int f = sl + LPR * m;
          if (!valid && f >= ic && f < P) xrw[LPR * m] = 0.0;
        }
        if (m == 0 && ic && sl == 0) v = 1.0;
        xv[m] = v;
        if constexpr (!ETA0) {
          const double bm = bet[sl + LPR * m];
          if (m & 1)
            e1 = fma(v, bm, e1);
          else
            e0 = fma(v, bm, e0);
        }
      }
      double e = ETA0 ? 0.0 : wv_row_sum<RW>(e0 + e1);
      // the offset once, after the reduction; a padded row's (possibly the
      // next partition's, even NaN) stays behind the selects on `valid`
      if constexpr (RS::OFS) e += RS::offset(ys, row);
      const double yv = ys[row];
      // the prior weight (RowStreams, glm_row.hpp); 1 folds out of the products
      double om = 1.0;
      if constexpr (RS::WGT) om = valid ? ys[RS::WGT_OFF / 8 + row] : 0.0;
      double w, r;
      if constexpr (FAM == FAMILY_LOGISTIC) {
        const LogisticLink k = logistic_link<RCP_NEWTON>(e);
        w = k.w;
        r = yv - k.mu;
        if (valid && sl == 0)
          llacc += om * (yv * e - (fmax(e, 0.0) + wv_log12(1.0 + k.ea)));
      } else if constexpr (FAM == FAMILY_POISSON) {
        // log link, as in the cooperative pass: a padded row's eta is never
        // exponentiated; the constant -lgamma(y + 1) has its own sum
        const double mu = exp(valid ? e : 0.0);
        w = mu;
        r = yv - mu;
        if (valid && sl == 0) {
          llacc += om * (yv * e - mu);
          if (yv != 0.0 && yv != 1.0) llcacc -= om * lgamma1p(yv);  // 0 at y = 0, 1
        }
      } else {  // gaussian (OLS): mu = eta, w = 1, ll = -rss / 2
        w = 1.0;
        r = yv - e;
        if (valid && sl == 0) llacc -= 0.5 * r * r;
      }
      w *= om;  // once, after mu; ahead of the padded rows' zeroing
      r *= om;
      if (!valid) {
        w = 0.0;
        r = 0.0;
      }
#pragma unroll
      for (int m = 0; m < M; ++m) gacc[m] = fma(xv[m], r, gacc[m]);
      if (sl == 0) wv[row] = w;
    }
    // w (and standardised / zeroed x) of all rows visible.  (OLS without
    // standardisation could skip this barrier on full blocks, where w = 1; it
    // measured not faster: 15.2 vs 14.9-15.0 ms, profiles/r04h_ols_ab.txt)
    if constexpr (W > 1) wv_sync<W>();

    // ---- tile phase: KS k-steps of 4 rows, this wave's TW tiles ---------------
    // operands of k-step s+1 are read while the MFMAs of k-step s run
    double xo[2][NC], xso[2][NSA], wk[2];
    auto load = [&](int s, int u) {
      const double* xq = xs + (4 * s + q) * p + (fl - ic);
#pragma unroll
      for (int c = 0; c < NC; ++c) xo[u][c] = xq[16 * c];
      if constexpr (HAS_STRIP) {
        // strip A operand of sub-block r: feature 16 (NT - 1) + 4 r + (l & 3)
        const double* xt = xq + 16 * (NT - 1) + (lane & 3) - fl;
#pragma unroll
        for (int r = 0; r < NS; ++r) xso[u][r] = xt[4 * r];
      }
      wk[u] = wv[4 * s + q];
    };
    load(0, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int u = s & 1;
      if (s + 1 < KS) load(s + 1, u ^ 1);
      double xv[NC], av[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        double v = xo[u][c];
        if (c == 0 && icpt_lane) v = OLS_NOMUL ? wk[u] : 1.0;
        xv[c] = v;
        if ((TL::RM >> c) & 1u) av[c] = OLS_NOMUL ? v : v * wk[u];
      }
      double as[NSA];
      if constexpr (HAS_STRIP) {
#pragma unroll
        for (int r = 0; r < NS; ++r) as[r] = OLS_NOMUL ? xso[u][r] : xso[u][r] * wk[u];
      }
      // tiles in row order: a row's A operand is reused back to back
      static_for<TW>([&](auto iI) {
        constexpr int i = decltype(iI)::value;
        constexpr int I = TL::I_of(i), J = TL::J_of(i);
        if constexpr (strip(I)) {
#pragma unroll
          for (int r = 0; r < NS; ++r)
            sacc[i][r] = __builtin_amdgcn_mfma_f64_4x4x4f64(as[r], xv[J], sacc[i][r], 0, 0, 0);
        } else {
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I], xv[J], acc[i], 0, 0, 0);
        }
      });
    }
    // keep every 16x16x4 accumulator in AGPRs across the loop back edge (the
    // strip's 64-bit ones are left to the allocator: pinned one by one they
    // get shuffled between AGPRs; explicit capture: an asm operand alone does
    // not capture in a generic lambda)
    static_for<TW>([&acc](auto iI) {
      constexpr int i = decltype(iI)::value;
      if constexpr (!(NS > 0 && TL::I_of(i) == NT - 1)) asm volatile("" : "+a"(acc[i]));
    });
  }
  wait_vmcnt<0>();

  // ---- epilogue: this chunk's partials (newton_solve.hip slab layout) --------
  double* sH = a.slab_H + (int64_t)cx.chunk * (NT * (NT + 1) / 2) * 256;
  static_for<TW>([&](auto iI) {
    constexpr int i = decltype(iI)::value;
    constexpr int t = TL::I_of(i) * (TL::I_of(i) + 1) / 2 + TL::J_of(i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (strip(TL::I_of(i))) {
        // sub-block r: rows 4 r + (l >> 4), columns l & 15; rows past it: 0
        sH[t * 256 + (4 * r + q) * 16 + fl] = r < NS ? sacc[i][r < NSA ? r : 0] : 0.0;
      } else {  // f64 16x16x4 C/D map: row = (l >> 4) + 4 r, col = l & 15
        sH[t * 256 + (q + 4 * r) * 16 + fl] = acc[i][r];
      }
    }
  });
  // gradient: sum the RW row lanes of each feature group, then the W waves
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int o = 1; o < RW; o <<= 1) gacc[m] += __shfl_xor(gacc[m], o);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) llacc += __shfl_xor(llacc, o);
  constexpr bool LLC = FAM == FAMILY_POISSON;
  if constexpr (LLC) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) llcacc += __shfl_xor(llcacc, o);
  }
  // the ring is no longer needed: [W - 1][PMAX + 1], then (Poisson) [W - 1]
  double* red = (double*)smem;
  if constexpr (W > 1) {
    __syncthreads();
    if constexpr (WID > 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (rl == 0) red[(WID - 1) * (PMAX + 1) + sl + LPR * m] = gacc[m];
      if (lane == 0) red[(WID - 1) * (PMAX + 1) + PMAX] = llacc;
      if constexpr (LLC)
        if (lane == 0) red[(W - 1) * (PMAX + 1) + WID - 1] = llcacc;
    }
    __syncthreads();
  }
  if constexpr (WID == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      double v = gacc[m];
#pragma unroll
      for (int w = 1; w < W; ++w) v += red[(w - 1) * (PMAX + 1) + sl + LPR * m];
      if (rl == 0) a.slab_g[(int64_t)cx.chunk * PMAX + sl + LPR * m] = v;
    }
    double ll = llacc;
#pragma unroll
    for (int w = 1; w < W; ++w) ll += red[(w - 1) * (PMAX + 1) + PMAX];
    if (lane == 0) a.slab_ll[cx.chunk] = ll;
    if constexpr (LLC) {
      double c = llcacc;
#pragma unroll
      for (int w = 1; w < W; ++w) c += red[(W - 1) * (PMAX + 1) + w - 1];
      if (lane == 0) a.slab_llc[cx.chunk] = c;
    }
  }
}

// minimum waves per SIMD (register budget): OLS at P <= 64 fits 5 (48 VGPRs +
// <= 41 AGPRs, no scratch); the logistic kernels would spill there
constexpr int wave_min_waves(int NT, int W, int FAM) {
  return W == 1 ? 1 : (NT <= 4 && FAM == FAMILY_GAUSSIAN ? 5 : 2);
}

template <int NT, int NS, int W, bool STD, int FAM, int EX = EX_NONE>
__global__ __launch_bounds__(64 * W, wave_min_waves(NT, W, FAM)) void irls_wave_kernel(
    const typename pass_args_of<EX>::type a) {
  static_assert(!RowStreams<EX>::OFS || FAM == FAMILY_POISSON,
                "the offset is the Poisson family's");
  constexpr int RB = wave_rb(NT, W, FAM);
  constexpr int PMAX = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  WaveCtx cx;
  cx.chunk = blockIdx.x;
  cx.part = __builtin_amdgcn_readfirstlane(a.chunk_part[cx.chunk]);
  if (a.phase[cx.part] != a.want_phase) return;  // workgroup-uniform

  const int tid = threadIdx.x;
  const int p = a.p, P = a.P, ic = a.intercept;
  cx.row0 = uniform_row0(a.chunk_row0, cx.chunk);
  cx.nrows = __builtin_amdgcn_readfirstlane(a.chunk_rows[cx.chunk]);
  cx.nb = (cx.nrows + RB - 1) / RB;
  cx.npieces = wave_npieces(RB, p);
  cx.slot_bytes = wave_slot_bytes_impl(RB, p, ex_count(EX));
  cx.slot_y = 16 + cx.npieces * 1024;
  double* wv = (double*)(smem + kWaveSlots * cx.slot_bytes);
  double* bet = wv + RB;
  double* stdv = bet + PMAX;

  // the ring must hold finite values where no DMA lands (tails, pads): a
  // padded row reads them with w = 0, and 0 * NaN would poison the tiles
  for (int o = tid * 16; o < kWaveSlots * cx.slot_bytes; o += 64 * W * 16)
    *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
  for (int f = tid; f < PMAX; f += 64 * W)
    bet[f] = (f < P) ? a.theta[(int64_t)cx.part * P + f] : 0.0;
  if constexpr (STD) {
    for (int f = tid; f < PMAX; f += 64 * W) {
      const int j = f - ic;
      const bool in = j >= 0 && j < p;
      stdv[f] = in ? a.center[j] : 0.0;
      stdv[PMAX + f] = in ? 1.0 / a.scale[j] : 1.0;
    }
  }
  __syncthreads();

  cx.xcb = (uintptr_t)(a.X + cx.row0 * p) & ~(uintptr_t)15;
  cx.xr = uniform_rsrc(cx.xcb, a.x_last16 + 16 - cx.xcb);
  const uintptr_t ycb = (uintptr_t)(a.y + cx.row0);
  cx.yr = uniform_rsrc(ycb, a.y_last4 + 4 - ycb);
  if constexpr (RowStreams<EX>::OFS) {
    const uintptr_t ocb = (uintptr_t)(a.eta_offset + cx.row0);
    cx.orr = uniform_rsrc(ocb, a.o_last4 + 4 - ocb);
  }
  if constexpr (RowStreams<EX>::WGT) {
    const uintptr_t wcb = (uintptr_t)(a.row_weight + cx.row0);
    cx.wrr = uniform_rsrc(wcb, a.w_last4 + 4 - wcb);
  }
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  if constexpr (W == 1) {
    wave_body<NT, NS, 1, 0, STD, FAM, EX>(a, cx, smem);
  } else {
    if (wid == 0)
      wave_body<NT, NS, W, 0, STD, FAM, EX>(a, cx, smem);
    else
      wave_body<NT, NS, W, 1, STD, FAM, EX>(a, cx, smem);
  }
}

// requested: dlsa_fit_options.exact_waves (0 = automatic)
static inline int wave_w(int NT, int requested = 0) {
  const int w = requested;
  if ((w == 1 && NT <= 8) || (w == 2 && NT >= 2 && NT <= 7)) return w;
  return wave_w_default(NT);
}

template <int NT, int W, bool STD, int FAM, int EX = EX_NONE>
static hipError_t launch_wave_t(const typename pass_args_of<EX>::type& a, int n_chunks,
                                hipStream_t s) {
  const size_t lds = wave_lds_bytes_impl(NT, wave_rb(NT, W, FAM), a.p, ex_count(EX));
  switch (wave_strip_ns(NT, a.P)) {
    case 1:
      hipLaunchKernelGGL((irls_wave_kernel<NT, 1, W, STD, FAM, EX>), dim3(n_chunks), dim3(64 * W), lds,
                         s, a);
      break;
    case 2:
      hipLaunchKernelGGL((irls_wave_kernel<NT, 2, W, STD, FAM, EX>), dim3(n_chunks), dim3(64 * W), lds,
                         s, a);
      break;
    default:
      hipLaunchKernelGGL((irls_wave_kernel<NT, 0, W, STD, FAM, EX>), dim3(n_chunks), dim3(64 * W), lds,
                         s, a);
  }
  return hipGetLastError();
}

template <int NT, bool STD, int FAM, int EX = EX_NONE>
static hipError_t launch_wave_sf(const typename pass_args_of<EX>::type& a, int n_chunks,
                                 hipStream_t s) {
  if constexpr (NT >= 2 && NT <= 7) {
    if (wave_w(NT, a.waves) == 2) return launch_wave_t<NT, 2, STD, FAM, EX>(a, n_chunks, s);
  }
  return launch_wave_t<NT, 1, STD, FAM, EX>(a, n_chunks, s);
}

// The launcher of one (NT, family, row extras), guarded by the family's
// rules.  A kernel takes the slice of `a` its extras need.
template <int NT, int FAM, int EX>
static hipError_t launch_wave_nt(const PassArgsWgt& a, bool std_, int n_chunks, hipStream_t s) {
  constexpr FamilyRules R = family_rules(FAM);
  constexpr bool OFS = (EX & EX_OFS) != 0, WGT = (EX & EX_WGT) != 0;
  static_assert(!OFS || R.offset, "an offset kernel of a family without one");
  static_assert(!WGT || R.weights, "a weighted kernel of a family without weights");
  if (R.sums_ll_const && !a.slab_llc) return hipErrorInvalidValue;
  if (OFS && !a.eta_offset) return hipErrorInvalidValue;
  if (WGT && !a.row_weight) return hipErrorInvalidValue;
  const typename pass_args_of<EX>::type& ka = a;
  return std_ ? launch_wave_sf<NT, true, FAM, EX>(ka, n_chunks, s)
              : launch_wave_sf<NT, false, FAM, EX>(ka, n_chunks, s);
}

// Entry point of a compilation unit, one line per unit:
//   DLSA_WAVE_UNIT(name, family set (an IntList), row extras (EX_* mask), NT...)
// irls_wave.hip lists the units and routes to them.
typedef hipError_t WaveUnitFn(const PassArgsWgt& a, int NT, bool std_, int family, int n_chunks,
                              hipStream_t s);
#define DLSA_WAVE_UNIT(name, FAMS, EX, ...)                                                   \
  hipError_t name(const PassArgsWgt& a, int NT, bool std_, int family, int n_chunks,          \
                  hipStream_t s) {                                                            \
    return unit_dispatch(FAMS{}, IntList<__VA_ARGS__>{}, family, NT, [&](auto fam, auto nt) { \
      return launch_wave_nt<decltype(nt)::value, decltype(fam)::value, (EX)>(a, std_,         \
                                                                             n_chunks, s);    \
    });                                                                                       \
  }

}  // namespace dlsa
