// Row diagnostics pass on the dense layout -- the kernel template of
// rows_pass.hip (logistic) and rows_pass_pois.hip (Poisson).
//
// Per row i of partition k, at its coefficient vector beta_k, one pass over X
// gives eta_i, mu_i, the signed deviance and Pearson residuals and the
// leverage h_i = d_i q_i, d_i = omega_i w_i, q_i = x_i^T S_k^-1 x_i = |R_k x_i|^2
// with R_k^T R_k = S_k^-1 (R_k lower triangular, row-major [P, P]).
//
// Geometry of the score pass (score_pass_impl.hpp, whose slot helpers and
// tile dealing this includes unchanged): one 4-wave workgroup per chunk of
// one partition, 32-row blocks through the LDS-DMA ring of clamped
// global_load_lds pieces, 8 lanes per row in the row phase.  Per block:
//   barrier (block landed, block - 1 consumed) -> issue block + nslot - 1
//   store block - 1 (its staged values and q partials: the other buffer)
//   row phase: eta, mu, d, residuals to LDS; x standardised in place
//   barrier -> tile phase: z = R x on the fp64 MFMA, q partials to LDS.
// The tile phase contracts over FEATURES: A = x (16 rows x 4 features),
// B = R (4 features x 16 rows of R), D = z (16 rows of x by 16 components).
// A pad feature (f >= P, the intercept slot) would reach every z of its row
// (0 * NaN), so it is a select in the A operand; a padded row reaches only
// its own z, which is not stored.  Every output of a row depends on the row,
// beta_k and R_k alone, in one summation order: the bits do not depend on the
// chunking.
#pragma once

#include "score_pass_impl.hpp"

namespace dlsa {

namespace {

// staged per block and buffer: eta, mu, d, dev_res, pearson_res [5][32], then
// the q partials of the four waves [4][32]
constexpr int kRowsStaged = 5;
constexpr int kRowsBuf = (kRowsStaged + SPW) * SPRB;
// beyond the ring: [2] buffers, beta [PMAX], center / 1/scale [2][PMAX]
__host__ __device__ __forceinline__ int rp_extra_bytes(int NT) {
  return (2 * kRowsBuf + 3 * 16 * NT) * 8;
}

// position of column tile J among the wave's owned tiles (ascending)
constexpr int rp_slot_of(unsigned rm, int J) {
  int c = 0;
  for (int j = 0; j < J; ++j)
    if ((rm >> j) & 1u) ++c;
  return c;
}
constexpr int rp_popcount(unsigned rm) {
  int c = 0;
  for (; rm; rm >>= 1) c += rm & 1u;
  return c;
}

}  // namespace

// The block loop of wave WID (a code path per wave: static tile indices).
template <int FAM, int NT, int WID>
__device__ __forceinline__ void rows_body(const RowsArgs& a, char* smem, int chunk, int part) {
  using TL = ScoreTiles<NT, WID>;  // its "rows" I are the owned column tiles J of z here
  constexpr int PMAX = 16 * NT;
  constexpr int M = PMAX / 8;  // features per lane in the row phase
  constexpr int TW = TL::TW, NC = TL::NC;
  constexpr int TWA = TW > 0 ? TW : 1;
  constexpr int NOWN = rp_popcount(TL::RM), NOWNA = NOWN > 0 ? NOWN : 1;

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
  const bool lev = a.leverage != nullptr;             // workgroup-uniform
  const int nld = 1 + (ofs ? 1 : 0) + (wgt ? 1 : 0);  // loads per block beside X
  double* stg = (double*)(smem + nslot * slot_bytes);  // [2][kRowsBuf]
  double* bet = stg + 2 * kRowsBuf;                    // [PMAX]
  double* stdv = bet + PMAX;                           // [2][PMAX]

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

  // Block blk's rows, one per lane of the low half-wave, a stream or two per
  // wave: 0 leverage, 1 eta and mu, 2 dev_res, 3 pearson_res.  The q of a row
  // is the waves' partials in wave order (a wave without tiles left its zero).
  auto store = [&](int blk) {
    const int rows_left = nrows - blk * SPRB;
    if (lane >= SPRB || lane >= rows_left) return;
    const double* sb = stg + (blk & 1) * kRowsBuf;
    const int64_t gi = row0 + (int64_t)blk * SPRB + lane;
    if constexpr (WID == 0) {
      if (lev) {
        const double* qp = sb + kRowsStaged * SPRB;
        const double qv = ((qp[lane] + qp[SPRB + lane]) + qp[2 * SPRB + lane]) + qp[3 * SPRB + lane];
        a.leverage[gi] = sb[2 * SPRB + lane] * qv;
      }
    } else if constexpr (WID == 1) {
      if (a.eta) a.eta[gi] = sb[lane];
      if (a.mu) a.mu[gi] = sb[SPRB + lane];
    } else if constexpr (WID == 2) {
      if (a.dev_res) a.dev_res[gi] = sb[3 * SPRB + lane];
    } else {
      if (a.pearson_res) a.pearson_res[gi] = sb[4 * SPRB + lane];
    }
  };

  const int sl = lane & 7;
  const int rB = WID * 8 + (lane >> 3);
  const int fl = lane & 15, q = lane >> 4;

  // ---- B operands: this wave's tile pairs of R, once per chunk ---------------
  // pair i = (J = TL::I_of(i), I = TL::J_of(i) <= J); lane (q, fl) holds
  // R[16 J + fl][16 I + 4 q + s], s = 0 .. 3: the feature map of the A operand
  sp_d4 bop[TWA];
  if constexpr (TW > 0) {
    if (lev) {
      const double* R = a.rfac + (int64_t)part * a.rfac_part_stride;
      static_for<TW>([&](auto iI) {
        constexpr int i = decltype(iI)::value;
        constexpr int J = TL::I_of(i), I = TL::J_of(i);
        const int r = 16 * J + fl, c0 = 16 * I + 4 * q;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bool in = r < P && c0 + s < P;
          const double v = R[in ? r * P + c0 + s : 0];
          bop[i][s] = in ? v : 0.0;
        }
      });
      // landed before the ring is primed, and held in registers from here on
      // (opaque values: neither a drain of the ring at the first use nor a
      // reload inside the block loop)
      wait_vmcnt<0>();
      static_for<TW>([&](auto iI) {
        constexpr int i = decltype(iI)::value;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          double v = bop[i][s];
          asm volatile("" : "+v"(v));
          bop[i][s] = v;
        }
      });
    }
  }

  for (int b = 0; b < nslot - 1; ++b) issue(b);
  // the score pass's count: at most 55 loads outstanding.  The stores of
  // store() count in vmcnt as well; they are younger than the block waited
  // for, so `keep` waits for it whichever way loads and stores retire.
  const int keep = (nslot - 2) * (d + nld);
  for (int blk = 0; blk < nb; ++blk) {
    wait_vmcnt_le<40>(keep);
    lds_barrier();
    issue(blk + nslot - 1);
    if (blk > 0) store(blk - 1);
    char* slot = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)blk * SPRB) * p);
    double* xs = (double*)(slot + 16 + (start & 15));
    const double* ys = (const double*)(slot + slot_x);
    const int rows_left = nrows - blk * SPRB;
    double* sb = stg + (blk & 1) * kRowsBuf;

    // ---- row phase: 8 rows of this wave, 8 lanes per row ----------------------
    {
      const bool valid = rB < rows_left;
      double* xr = xs + rB * p + (sl - ic);
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
      const double ev = valid ? e : 0.0;
      const RowMean k = row_mean<FAM>(ev);
      // the logistic saturated term is 0 for 0/1 data: its two logarithms only
      // where some row of the wave is a grouped one (the same value either way)
      double rc = 0.0;
      if (FAM == FAMILY_POISSON || __any(yv != 0.0 && yv != 1.0)) rc = row_gof_const<FAM>(yv);
      const RowGof g = row_gof<FAM>(ev, yv, om, rc);
      // the sign of y - mu from the unrounded side: r = y - mu (Poisson, exact
      // in sign), t = a + b ea (logistic, row_gof's)
      double sg;
      if constexpr (FAM == FAMILY_POISSON) {
        sg = yv - k.mu;
      } else {
        const double ea = exp(-fabs(ev));
        sg = fma(ev >= 0.0 ? yv : yv - 1.0, ea, ev >= 0.0 ? yv - 1.0 : yv);
      }
      // (a NaN stays one: no fmax)
      const double dres = copysign(sqrt(g.dev < 0.0 ? 0.0 : g.dev), sg);
      const double pres = copysign(sqrt(g.chi), sg);
      if (sl == 0) {
        sb[rB] = e;
        sb[SPRB + rB] = k.mu;
        sb[2 * SPRB + rB] = om * k.w;
        sb[3 * SPRB + rB] = dres;
        sb[4 * SPRB + rB] = pres;
      }
    }
    if (!lev) continue;  // no tile phase: the next block's first barrier orders the stage
    lds_barrier();       // the standardised x of all rows visible

    // ---- tile phase: z = R x of the block's two 16-row tiles ------------------
    if constexpr (TW > 0) {
      double* qp = sb + (kRowsStaged + WID) * SPRB;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        sp_d4 acc[NOWNA];
#pragma unroll
        for (int j = 0; j < NOWNA; ++j) acc[j] = sp_d4{0.0, 0.0, 0.0, 0.0};
        const double* xrow = xs + (16 * t + fl) * p + (4 * q - ic);
        static_for<NC>([&](auto II) {
          constexpr int I = decltype(II)::value;
          // A: x[16 t + fl][16 I + 4 q + s], four contiguous doubles of the slot
          double av[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            double v = xrow[16 * I + s];
            const int f = 16 * I + 4 * q + s;
            if (I == 0 && ic && f == 0) v = 1.0;
            if (I == NT - 1 && f >= P) v = 0.0;
            av[s] = v;
          }
          static_for<TW>([&](auto iI) {
            constexpr int i = decltype(iI)::value;
            if constexpr (TL::J_of(i) == I) {
              constexpr int j = rp_slot_of(TL::RM, TL::I_of(i));
#pragma unroll
              for (int s = 0; s < 4; ++s)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bop[i][s], acc[j], 0, 0, 0);
            }
          });
        });
        // f64 16x16x4 C/D map: row of x = (l >> 4) + 4 r, component = l & 15
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double v = 0.0;
#pragma unroll
          for (int j = 0; j < NOWN; ++j) v = fma(acc[j][r], acc[j][r], v);
          // the xor tree 1, 2, 4, 8 over the 16 lanes of a DPP row, in registers
          // (a shuffle would be an LDS round trip per stage)
          v = ev_red8(v);
          v += dpp_f64<0x128>(v);  // row_ror 8: l ^ 8
          if (fl == 0) qp[16 * t + q + 4 * r] = v;
        }
      }
    }
  }
  lds_barrier();
  if (nb > 0) store(nb - 1);
  wait_vmcnt<0>();
}

template <int FAM, int NT>
__global__ __launch_bounds__(64 * SPW, score_min_waves(NT)) void rows_pass_kernel(
    const RowsArgs a) {
  constexpr int PMAX = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk = blockIdx.x;
  const int part = a.chunk_part[chunk];
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, P = a.P, ic = a.intercept;
  const int ring = a.nslot * a.slot_bytes;
  double* stg = (double*)(smem + ring);
  double* bet = stg + 2 * kRowsBuf;
  double* stdv = bet + PMAX;

  // the ring must hold finite values where no DMA lands (pads, tails); the
  // q partials of a wave without tiles stay 0
  for (int o = tid * 16; o < ring + 2 * kRowsBuf * 8; o += 64 * SPW * 16)
    *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
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
    rows_body<FAM, NT, 0>(a, smem, chunk, part);
  else if (wid == 1)
    rows_body<FAM, NT, 1>(a, smem, chunk, part);
  else if (wid == 2)
    rows_body<FAM, NT, 2>(a, smem, chunk, part);
  else
    rows_body<FAM, NT, 3>(a, smem, chunk, part);
}

// ring depth by score_nslot's rule, with this pass's LDS beyond the ring
inline int rows_nslot(int NT, int p) {
  const int slot = sp_slot_bytes(p), extra = rp_extra_bytes(NT);
  if (score_min_waves(NT) > 1 && 2 * slot + extra <= 80 * 1024)
    return std::min((80 * 1024 - extra) / slot, 4);
  return std::max(2, std::min((160 * 1024 - extra) / slot, 6));
}

template <int FAM, int NT>
inline hipError_t launch_rows_kernel(RowsArgs a, int n_chunks, hipStream_t s) {
  auto kern = rows_pass_kernel<FAM, NT>;
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  a.slot_bytes = sp_slot_bytes(a.p);
  a.nslot = rows_nslot(NT, a.p);
  const size_t lds = (size_t)a.nslot * a.slot_bytes + rp_extra_bytes(NT);
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(64 * SPW), lds, s, a);
  return hipGetLastError();
}

// every NT of one family: the body of a unit's entry point
template <int FAM, int... NTS>
inline hipError_t launch_rows_family(const RowsArgs& a, int n_chunks, hipStream_t s,
                                     std::integer_sequence<int, NTS...>) {
  const int NT = (a.P + 15) / 16;
  hipError_t e = hipErrorInvalidValue;
  (void)((NT == NTS + 1 && ((e = launch_rows_kernel<FAM, NTS + 1>(a, n_chunks, s)), true)) || ...);
  return e;
}
// the unit of the Poisson instantiations (rows_pass_pois.hip)
hipError_t launch_rows_unit_pois(const RowsArgs& a, int n_chunks, hipStream_t s);

}  // namespace dlsa
