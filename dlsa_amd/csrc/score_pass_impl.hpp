// Score outer-product pass on the dense layout -- the kernel template of
// score_pass.hip (logistic) and score_pass_pois.hip (Poisson).
//
// Per partition k, at its coefficient vector beta_k, one pass over X gives
//   G_k = sum_i d_i x_i x_i^T   and   g_k = sum_i s_i x_i,   s_i = omega_i (y_i - mu_i),
// with d_i = s_i^2 (GRAM_SCORE: the meat of the sandwich covariance) or
// d_i = omega_i w_i (GRAM_INFORMATION: the information matrix at beta_k).
//
// Geometry of the evaluation pass (eval_pass_impl.hpp): one 4-wave workgroup
// per chunk of one partition, 32-row blocks through an LDS-DMA ring of clamped
// global_load_lds pieces, 8 lanes per row in the row phase.  The tile phase is
// the per-wave fp64 pass's (irls_wave_impl.hpp: operand layout of
// v_mfma_f64_16x16x4, lower-triangle 16x16 tiles, the fit's slab layout), with
// the tile rows dealt to the four waves at compile time so that no wave holds
// more than 21 accumulators (NT = 12).  Per block:
//   barrier (block landed, block - 1 consumed) -> issue block + nslot - 1
//   [last block: rows past the chunk zeroed in the slot, barrier]
//   row phase: eta, mu, s, d; x standardised in place; g += s x; d to LDS
//   barrier -> tile phase: 8 k-steps of 4 rows, A = d x, B = x.
// A pad column (feature >= P) may hold anything: an MFMA is an outer product
// per k, so it only reaches rows / columns >= P of a tile, which the reduction
// never reads; eta takes it behind a select.  A padded row would reach every
// entry, so its X is zeroed in the slot (0 * NaN) and its d and s are selects.
#pragma once

#include <algorithm>

#include "dlsa_internal.hpp"
#include "glm_row.hpp"

namespace dlsa {

namespace {

constexpr int SPW = 4;    // waves
constexpr int SPRB = 32;  // rows per block
constexpr int SPKS = SPRB / 4;
constexpr int kScoreMaxNT = DLSA_MAX_P_FUSED / 16;
typedef double sp_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ int sp_npieces(int p) {
  return (SPRB * p * 8 + 16 + 1023) / 1024;
}
// [16 B][d * SPW KiB of X pieces][32 zero doubles: what the last row's pad
// columns read][y][eta_offset][row_weight]
__host__ __device__ __forceinline__ int sp_slot_x(int p) {
  return 16 + (sp_npieces(p) + SPW - 1) / SPW * SPW * 1024 + 256;
}
__host__ __device__ __forceinline__ int sp_slot_bytes(int p) {
  return sp_slot_x(p) + 3 * kRowStreamRows * 8;
}
// beyond the ring: d of the block's rows [32], beta [PMAX], center / 1/scale [2][PMAX]
__host__ __device__ __forceinline__ int sp_extra_bytes(int NT) { return (SPRB + 3 * 16 * NT) * 8; }

// tile rows of wave `wid`: rows dealt most expensive first to the lightest wave
// (NT = 7: {6}, {5, 0}, {4, 1}, {3, 2}, 7 tiles each; NT = 12: 21, 20, 19, 18)
constexpr unsigned sp_rows_mask(int NT, int wid) {
  int load[SPW] = {0, 0, 0, 0};
  unsigned m[SPW] = {0, 0, 0, 0};
  for (int I = NT - 1; I >= 0; --I) {
    int b = 0;
    for (int w = 1; w < SPW; ++w)
      if (load[w] < load[b]) b = w;
    load[b] += I + 1;
    m[b] |= 1u << I;
  }
  return m[wid];
}

template <int NT, int WID>
struct ScoreTiles {
  static constexpr unsigned RM = sp_rows_mask(NT, WID);
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

}  // namespace

// The block loop and epilogue of wave WID (a code path per wave: static tile
// indices, no branch merges of the accumulators).
template <int FAM, int NT, int WID>
__device__ __forceinline__ void score_body(const GramArgs& a, char* smem, int chunk) {
  using TL = ScoreTiles<NT, WID>;
  constexpr int PMAX = 16 * NT;
  constexpr int M = PMAX / 8;  // features per lane in the row phase
  constexpr int TW = TL::TW, NC = TL::NC;
  constexpr int TWA = TW > 0 ? TW : 1, NCA = NC > 0 ? NC : 1;

  const int lane = threadIdx.x & 63;
  const int p = a.p, P = a.P, ic = a.intercept;
  const int64_t row0 = a.chunk_row0[chunk];
  const int nrows = a.chunk_rows[chunk];
  const int nb = (nrows + SPRB - 1) / SPRB;
  const int nslot = a.nslot, slot_bytes = a.slot_bytes;
  const int npieces = sp_npieces(p);
  const int d = (npieces + SPW - 1) / SPW;
  const int slot_x = sp_slot_x(p);
  const bool std_ = a.center != nullptr;
  const bool ofs = a.eta_offset != nullptr, wgt = a.row_weight != nullptr;
  const int nld = 1 + (ofs ? 1 : 0) + (wgt ? 1 : 0);  // loads per block beside X
  double* dv = (double*)(smem + nslot * slot_bytes);  // [32] d of the block's rows
  double* bet = dv + SPRB;                            // [PMAX]
  double* stdv = bet + PMAX;                          // [2][PMAX]

  auto issue = [&](int blk) {
    const int bb = blk < nb ? blk : nb - 1;
    char* sbase = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)bb * SPRB) * p);
    const uintptr_t al = start & ~(uintptr_t)15;
    for (int i = 0; i < d; ++i) {
      const int j = WID + SPW * i;
      const int jj = j < npieces ? j : npieces - 1;
      uintptr_t src = al + (uintptr_t)jj * 1024 + (uintptr_t)lane * 16;
      src = src < a.x_last16 ? src : a.x_last16;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(sbase + 16 + j * 1024), 16,
                                       0, 0);
    }
    uintptr_t ys = (uintptr_t)(a.y + row0 + (int64_t)bb * SPRB) + (uintptr_t)lane * 4;
    ys = ys < a.y_last4 ? ys : a.y_last4;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)ys, (lds_void_t*)(sbase + slot_x), 4, 0, 0);
    if (ofs) {
      uintptr_t os = (uintptr_t)(a.eta_offset + row0 + (int64_t)bb * SPRB) + (uintptr_t)lane * 4;
      os = os < a.o_last4 ? os : a.o_last4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)os, (lds_void_t*)(sbase + slot_x + 256), 4, 0,
                                       0);
    }
    if (wgt) {
      uintptr_t wsrc = (uintptr_t)(a.row_weight + row0 + (int64_t)bb * SPRB) + (uintptr_t)lane * 4;
      wsrc = wsrc < a.w_last4 ? wsrc : a.w_last4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)wsrc, (lds_void_t*)(sbase + slot_x + 512), 4,
                                       0, 0);
    }
  };

  const int sl = lane & 7;
  const int rB = WID * 8 + (lane >> 3);
  const int fl = lane & 15, q = lane >> 4;
  const bool icpt_lane = ic && fl == 0;
  double gacc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) gacc[m] = 0.0;
  sp_d4 acc[TWA];
#pragma unroll
  for (int i = 0; i < TWA; ++i) acc[i] = sp_d4{0.0, 0.0, 0.0, 0.0};

  for (int b = 0; b < nslot - 1; ++b) issue(b);
  // d + nld loads per wave and block; nslot d <= 40 (the ring fits 160 KiB of
  // 4 KiB piece rows) and nslot <= 6: the nslot - 1 blocks ever outstanding are
  // at most 40 + 3 * 5 = 55 loads, below the 6-bit counter's 63; a keep above
  // 40 waits for more than it has to
  const int keep = (nslot - 2) * (d + nld);
  for (int blk = 0; blk < nb; ++blk) {
    wait_vmcnt_le<40>(keep);
    lds_barrier();
    issue(blk + nslot - 1);
    char* slot = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)blk * SPRB) * p);
    double* xs = (double*)(slot + 16 + (start & 15));
    const double* ys = (const double*)(slot + slot_x);
    const int rows_left = nrows - blk * SPRB;
    // The chunk's last block: the rows past its end (the next chunk's, or the
    // bytes behind X) are zeroed in the slot up to the end of its X pieces --
    // d = 0 does not keep a NaN out of a tile (0 * NaN).  No DMA is in flight
    // to this slot: the issues above went to the other nslot - 1.
    if (blk == nb - 1) {  // workgroup-uniform
      const int lim = (d * SPW * 1024 - (int)(start & 15)) / 8;
      for (int i = rows_left * p + threadIdx.x; i < lim; i += 64 * SPW) xs[i] = 0.0;
      lds_barrier();
    }

    // ---- row phase: 8 rows of this wave, 8 lanes per row ----------------------
    {
      const bool valid = rB < rows_left;
      double* xr = xs + rB * p + (sl - ic);
      double xv[M];
      double e0 = 0.0, e1 = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int f = sl + 8 * m;
        double v = xr[8 * m];
        if (std_) {
          v = (v - stdv[f]) * stdv[PMAX + f];
          // standardised in place for the tile phase (own row, own features;
          // the intercept slot f = 0 is the previous row's last value)
          if (f >= ic && f < P) xr[8 * m] = v;
        }
        if (m == 0 && ic && sl == 0) v = 1.0;
        // the pad columns hold the next row's first values, behind the last
        // row of X whatever lies there: a select, not 0 * NaN
        if (f >= P) v = 0.0;
        xv[m] = v;
        if (m & 1)
          e1 = fma(v, bet[f], e1);
        else
          e0 = fma(v, bet[f], e0);
      }
      double e = ev_red8(e0 + e1);
      if (ofs) e += ys[kRowStreamRows + rB];
      const double yv = ys[rB];
      double om = 1.0;
      if (wgt) om = valid ? ys[2 * kRowStreamRows + rB] : 0.0;
      // a padded row's eta (its offset may be the next partition's, even NaN)
      // is never exponentiated
      const RowMean k = row_mean<FAM>(valid ? e : 0.0);
      double s = om * (yv - k.mu);
      double dd = a.kind == GRAM_INFORMATION ? om * k.w : s * s;
      if (!valid) {
        s = 0.0;
        dd = 0.0;
      }
#pragma unroll
      for (int m = 0; m < M; ++m) gacc[m] = fma(xv[m], s, gacc[m]);
      if (sl == 0) dv[rB] = dd;
    }
    lds_barrier();  // d and the standardised x of all rows visible

    // ---- tile phase: 8 k-steps of 4 rows, this wave's TW tiles ----------------
    if constexpr (TW > 0) {
      double xo[2][NCA], wk[2];
      auto load = [&](int s, int u) {
        const double* xq = xs + (4 * s + q) * p + (fl - ic);
#pragma unroll
        for (int c = 0; c < NC; ++c) xo[u][c] = xq[16 * c];
        wk[u] = dv[4 * s + q];
      };
      load(0, 0);
#pragma unroll
      for (int s = 0; s < SPKS; ++s) {
        const int u = s & 1;
        if (s + 1 < SPKS) load(s + 1, u ^ 1);
        double bv[NCA], av[NCA];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          double v = xo[u][c];
          if (c == 0 && icpt_lane) v = 1.0;
          bv[c] = v;
          if ((TL::RM >> c) & 1u) av[c] = v * wk[u];
        }
        // tiles in row order: a row's A operand is reused back to back
        static_for<TW>([&](auto iI) {
          constexpr int i = decltype(iI)::value;
          constexpr int I = TL::I_of(i), J = TL::J_of(i);
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I], bv[J], acc[i], 0, 0, 0);
        });
      }
    }
  }
  wait_vmcnt<0>();

  // ---- epilogue: this chunk's partials --------------------------------------
  if constexpr (TW > 0) {
    double* sG = a.slab_G + (int64_t)chunk * (NT * (NT + 1) / 2) * 256;
    static_for<TW>([&](auto iI) {
      constexpr int i = decltype(iI)::value;
      constexpr int t = TL::I_of(i) * (TL::I_of(i) + 1) / 2 + TL::J_of(i);
      // f64 16x16x4 C/D map: row = (l >> 4) + 4 r, col = l & 15
#pragma unroll
      for (int r = 0; r < 4; ++r) sG[t * 256 + (q + 4 * r) * 16 + fl] = acc[i][r];
    });
  }
  // score: the 8 rows of each feature group, then the waves in order
#pragma unroll
  for (int m = 0; m < M; ++m) {
    gacc[m] += __shfl_xor(gacc[m], 8);
    gacc[m] += __shfl_xor(gacc[m], 16);
    gacc[m] += __shfl_xor(gacc[m], 32);
  }
  double* red = (double*)smem;  // [SPW][PMAX] in the ring, which nothing reads any more
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m)
    if (lane < 8) red[WID * PMAX + sl + 8 * m] = gacc[m];
  __syncthreads();
  for (int f = threadIdx.x; f < PMAX; f += 64 * SPW) {
    double v = 0.0;
    for (int w = 0; w < SPW; ++w) v += red[w * PMAX + f];
    a.slab_s[(int64_t)chunk * PMAX + f] = v;
  }
}

// two workgroups per CU while the accumulators leave room (<= 256 registers a lane)
constexpr int score_min_waves(int NT) { return NT <= 8 ? 2 : 1; }

template <int FAM, int NT>
__global__ __launch_bounds__(64 * SPW, score_min_waves(NT)) void score_pass_kernel(
    const GramArgs a) {
  constexpr int PMAX = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk = blockIdx.x;
  const int part = a.chunk_part[chunk];
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, P = a.P, ic = a.intercept;
  const int ring = a.nslot * a.slot_bytes;
  double* dv = (double*)(smem + ring);
  double* bet = dv + SPRB;
  double* stdv = bet + PMAX;

  // the ring must hold finite values where no DMA lands (pads, tails)
  for (int o = tid * 16; o < ring; o += 64 * SPW * 16) *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
  const double* beta = a.betas + part * a.beta_part_stride;
  for (int f = tid; f < PMAX; f += 64 * SPW) {
    bet[f] = f < P ? beta[f] : 0.0;
    const int j = f - ic;
    const bool in = a.center && j >= 0 && j < p;
    stdv[f] = in ? a.center[j] : 0.0;
    stdv[PMAX + f] = in ? 1.0 / a.scale[j] : 1.0;
  }
  __syncthreads();

  if (wid == 0)
    score_body<FAM, NT, 0>(a, smem, chunk);
  else if (wid == 1)
    score_body<FAM, NT, 1>(a, smem, chunk);
  else if (wid == 2)
    score_body<FAM, NT, 2>(a, smem, chunk);
  else
    score_body<FAM, NT, 3>(a, smem, chunk);
}

// ring depth: two workgroups per CU (80 KiB each) where two slots fit that,
// else one workgroup with up to six
inline int score_nslot(int NT, int p) {
  const int slot = sp_slot_bytes(p), extra = sp_extra_bytes(NT);
  if (score_min_waves(NT) > 1 && 2 * slot + extra <= 80 * 1024)
    return std::min((80 * 1024 - extra) / slot, 4);
  return std::max(2, std::min((160 * 1024 - extra) / slot, 6));
}

template <int FAM, int NT>
inline hipError_t launch_score_kernel(GramArgs a, int n_chunks, hipStream_t s) {
  auto kern = score_pass_kernel<FAM, NT>;
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  a.slot_bytes = sp_slot_bytes(a.p);
  a.nslot = score_nslot(NT, a.p);
  const size_t lds = (size_t)a.nslot * a.slot_bytes + sp_extra_bytes(NT);
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(64 * SPW), lds, s, a);
  return hipGetLastError();
}

// every NT of one family: the body of a unit's entry point
template <int FAM, int... NTS>
inline hipError_t launch_score_family(const GramArgs& a, int n_chunks, hipStream_t s,
                                      std::integer_sequence<int, NTS...>) {
  const int NT = (a.P + 15) / 16;
  hipError_t e = hipErrorInvalidValue;
  (void)((NT == NTS + 1 && ((e = launch_score_kernel<FAM, NTS + 1>(a, n_chunks, s)), true)) || ...);
  return e;
}
// the unit of the Poisson instantiations (score_pass_pois.hip)
hipError_t launch_score_unit_pois(const GramArgs& a, int n_chunks, hipStream_t s);

}  // namespace dlsa
