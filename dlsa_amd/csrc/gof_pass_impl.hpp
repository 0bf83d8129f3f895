// Goodness-of-fit pass on the dense layout -- the kernel template of
// gof_pass.hip.  Built like loglik_eval_kernel (eval_pass_impl.hpp), whose
// geometry, slot layout and LDS sizes it uses as they are: one 4-wave workgroup
// per chunk, 32-row blocks through the LDS-DMA ring, 8 lanes per row, the
// candidates and center / 1/scale in LDS.  What differs: two sums per
// candidate, the row's deviance and Pearson chi-square (row_gof, glm_row.hpp),
// the chunk's count of rows with omega > 0, and the candidates of partition k
// read at a.betas + k a.gof.beta_part_stride.  The log-likelihood kernels are
// not touched: wrapping their row loop in a function shared with this one
// changed the register allocation of all of them.
#pragma once

#include "eval_pass_impl.hpp"

namespace dlsa {

// FAM, EX: as loglik_eval_kernel.  At most kGofMaxB candidates.
template <int FAM, int EX>
__global__ __launch_bounds__(256) void gof_eval_kernel(const GofArgs a) {
  using RS = RowStreams<EX>;
  constexpr int NB = kGofMaxB;
  constexpr bool OFS = RS::OFS, WGT = RS::WGT;
  static_assert(!OFS || FAM == FAMILY_POISSON, "the offset is the Poisson family's");
  constexpr int NLD = RS::NLD;  // loads per block beside X: y and the row extras
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk = blockIdx.x;
  const int part = a.chunk_part[chunk];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, P = a.P, ic = a.intercept, B = a.nbeta;
  const int64_t row0 = a.chunk_row0[chunk];
  const int nrows = a.chunk_rows[chunk];
  const int nb = (nrows + ERB - 1) / ERB;
  const int nslot = a.nslot, slot_bytes = a.slot_bytes;
  const int npieces = ev_npieces(p);
  const int d = (npieces + EW - 1) / EW;
  const int slot_x = 16 + d * EW * 1024 + ((p + 8) / 8) * 8 * 8;
  const int PM = ((P + 7) / 8) * 8;  // features padded to the 8-lane stride
  double* bet = (double*)(smem + nslot * slot_bytes);  // [B][PM]
  double* stdv = bet + B * PM;                         // [2][PM]

  for (int o = tid * 16; o < nslot * slot_bytes; o += 256 * 16)
    *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
  const double* betas = a.betas + part * a.gof.beta_part_stride;
  for (int e = tid; e < B * PM; e += 256) {
    const int b = e / PM, f = e - b * PM;
    bet[e] = f < P ? betas[(int64_t)b * P + f] : 0.0;
  }
  for (int f = tid; f < PM; f += 256) {
    const int j = f - ic;
    const bool in = a.center && j >= 0 && j < p;
    stdv[f] = in ? a.center[j] : 0.0;
    stdv[PM + f] = in ? 1.0 / a.scale[j] : 1.0;
  }
  __syncthreads();

  auto issue = [&](int blk) {
    const int bb = blk < nb ? blk : nb - 1;
    char* sbase = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)bb * ERB) * p);
    const uintptr_t al = start & ~(uintptr_t)15;
    for (int i = 0; i < d; ++i) {
      const int j = wid + EW * i;
      const int jj = j < npieces ? j : npieces - 1;
      uintptr_t src = al + (uintptr_t)jj * 1024 + (uintptr_t)lane * 16;
      src = src < a.x_last16 ? src : a.x_last16;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(sbase + 16 + j * 1024), 16,
                                       0, 0);
    }
    uintptr_t ys = (uintptr_t)(a.y + row0 + (int64_t)bb * ERB) + (uintptr_t)lane * 4;
    ys = ys < a.y_last4 ? ys : a.y_last4;
    __builtin_amdgcn_global_load_lds((gbl_void_t*)ys, (lds_void_t*)(sbase + slot_x), 4, 0, 0);
    if constexpr (OFS) {
      uintptr_t os = (uintptr_t)(a.eta_offset + row0 + (int64_t)bb * ERB) + (uintptr_t)lane * 4;
      os = os < a.o_last4 ? os : a.o_last4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)os, (lds_void_t*)(sbase + slot_x + RS::OFS_OFF),
                                       4, 0, 0);
    }
    if constexpr (WGT) {
      uintptr_t wsrc = (uintptr_t)(a.row_weight + row0 + (int64_t)bb * ERB) + (uintptr_t)lane * 4;
      wsrc = wsrc < a.w_last4 ? wsrc : a.w_last4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)wsrc,
                                       (lds_void_t*)(sbase + slot_x + RS::WGT_OFF), 4, 0, 0);
    }
  };

  const int sl = lane & 7;
  const int rB = wid * 8 + (lane >> 3);
  double dvacc[NB], chacc[NB], npos = 0.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) dvacc[b] = chacc[b] = 0.0;

  for (int b = 0; b < nslot - 1; ++b) issue(b);
  // the loads per wave and block and the ring depths of loglik_eval_kernel:
  // its bound on the counted wait
  static_assert(4 * (6 + NLD) <= 40 && 5 * (6 + NLD) <= 63, "the counted wait's bound");
  const int keep = (nslot - 2) * (d + NLD);
  for (int blk = 0; blk < nb; ++blk) {
    wait_vmcnt_le<40>(keep);
    __syncthreads();
    issue(blk + nslot - 1);
    const char* slot = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)blk * ERB) * p);
    const double* xs = (const double*)(slot + 16 + (start & 15));
    const double* ys = (const double*)(slot + slot_x);
    const bool valid = rB < nrows - blk * ERB;
    const double* xr = xs + rB * p + (sl - ic);
    double eta[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) eta[b] = 0.0;
    for (int f = sl; f < PM; f += 8) {
      double v = xr[f - sl];
      v = (v - stdv[f]) * stdv[PM + f];
      if (f == 0 && ic) v = 1.0;
      // the pad columns f >= P hold the next row's first values, behind the
      // last row of X whatever lies there: a select, not 0 * NaN
      if (f >= P) v = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (b < B) eta[b] = fma(v, bet[b * PM + f], eta[b]);
    }
    const double yv = ys[rB];
    [[maybe_unused]] double ov = 0.0;
    if constexpr (OFS) ov = RS::offset(ys, rB);
    [[maybe_unused]] double om = 1.0;
    if constexpr (WGT) om = valid ? ys[RS::WGT_OFF / 8 + rB] : 0.0;
    double rc = 0.0;  // what of the deviance depends on y alone, once per row
    if (valid && sl == 0) {
      rc = row_gof_const<FAM>(yv);
      npos += om > 0.0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b < B) {
        double e = ev_red8(eta[b]);
        if constexpr (OFS) e += ov;
        if (valid && sl == 0) {
          const RowGof t = row_gof<FAM>(e, yv, om, rc);
          dvacc[b] += t.dev;
          chacc[b] += t.chi;
        }
      }
    }
  }
  wait_vmcnt<0>();
  __syncthreads();
  // the sum over the rows' lanes of a wave (lanes 0, 8, ..), left in lane 0
  auto wave_sum = [](double v) {
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
  };
  // [EW][2 NB + 1] wave sums, in the ring, which nothing reads any more (a
  // slot is at least 4 KiB)
  constexpr int NR = 2 * NB + 1;
  double* red = (double*)smem;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b < B) {
      const double dv = wave_sum(dvacc[b]), cv = wave_sum(chacc[b]);
      if (lane == 0) {
        red[wid * NR + b] = dv;
        red[wid * NR + NB + b] = cv;
      }
    }
  }
  const double nv = wave_sum(npos);
  if (lane == 0) red[wid * NR + 2 * NB] = nv;
  __syncthreads();
  if (tid < NR && (tid == 2 * NB || tid % NB < B)) {
    double s = 0.0;
    for (int w = 0; w < EW; ++w) s += red[w * NR + tid];
    if (tid == 2 * NB)
      a.gof.partial_npos[chunk] = s;
    else
      (tid < NB ? a.partial : a.gof.partial_chi)[(int64_t)chunk * B + tid % NB] = s;
  }
}

// One launch of the <FAM, EX> kernel (the dynamic LDS of the log-likelihood pass).
template <int FAM, int EX>
inline hipError_t launch_gof_kernel(const GofArgs& a, int n_chunks, hipStream_t s) {
  auto kern = gof_eval_kernel<FAM, EX>;
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(256), eval_lds_bytes(a), s, a);
  return hipGetLastError();
}

}  // namespace dlsa
