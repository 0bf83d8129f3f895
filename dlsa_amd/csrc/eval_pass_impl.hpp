// Log-likelihood evaluation pass -- the kernel template, included by
// eval_pass.hip (the unweighted instantiations) and eval_pass_wgt.hip (those
// with per-row prior weights).
#pragma once

#include "dlsa_internal.hpp"
#include "glm_row.hpp"

namespace dlsa {

namespace {

constexpr int EW = 4;    // waves
constexpr int ERB = 32;  // rows per block
constexpr int EMAXB = 16;
__host__ __device__ __forceinline__ int ev_npieces(int p) {
  return (ERB * p * 8 + 16 + 1023) / 1024;
}

}  // namespace

// (the X pieces, a pad, then the row streams: y and the row extras, glm_row.hpp)
inline int eval_slot_bytes_impl(int p, int n_extras) {
  const int d = (ev_npieces(p) + EW - 1) / EW;
  return 16 + d * EW * 1024 + ((p + 8) / 8) * 8 * 8 + row_streams_bytes(n_extras);
}
// dynamic LDS of a launch: the ring, the candidates, center / 1/scale, the reduction
inline size_t eval_lds_bytes(const EvalArgs& a) {
  const int PM = ((a.P + 7) / 8) * 8;
  return (size_t)a.nslot * a.slot_bytes +
         ((size_t)a.nbeta * PM + 2 * PM + EW * EMAXB) * sizeof(double);
}

// FAM: FAMILY_LOGISTIC, or FAMILY_POISSON (y eta - exp(eta) - lgamma(y + 1), the
// full log-likelihood; the constant once per row, not per candidate).
// EX (row extras, EX_* mask), each streamed like y, one more load per wave
// and block (the layout and the readers of RowStreams; the loads here address
// with clamped global pointers): EX_OFS (FAMILY_POISSON only) a.eta_offset[row] is added to every
// candidate's eta; EX_WGT every term of the row is multiplied by
// a.row_weight[row] (the weighted kernels take EvalArgsWgt).
template <int FAM, int EX = EX_NONE>
__global__ __launch_bounds__(256) void loglik_eval_kernel(const typename eval_args_of<EX>::type a) {
  using RS = RowStreams<EX>;
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
  double* red = stdv + 2 * PM;                         // [EW][EMAXB]

  for (int o = tid * 16; o < nslot * slot_bytes; o += 256 * 16)
    *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
  for (int e = tid; e < B * PM; e += 256) {
    const int b = e / PM, f = e - b * PM;
    bet[e] = f < P ? a.betas[(int64_t)b * P + f] : 0.0;
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
  double llacc[EMAXB];
#pragma unroll
  for (int b = 0; b < EMAXB; ++b) llacc[b] = 0.0;

  for (int b = 0; b < nslot - 1; ++b) issue(b);
  // d + NLD loads per wave and block; nslot d <= 40 (the ring fits 160 KiB of
  // 4 KiB piece rows) and nslot <= 6, so keep = (nslot - 2) (d + NLD) is at
  // most 4 (6 + NLD) at nslot = 6 (3 (8 + NLD), 2 (10 + NLD), 13 + NLD below
  // it): 36 with both extras, within the bound; and the nslot - 1 blocks ever
  // outstanding are at most 5 (6 + NLD) = 45 loads (two slots: d + NLD <= 36
  // at P = 512), below the 6-bit counter's 63
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
    double eta[EMAXB];
#pragma unroll
    for (int b = 0; b < EMAXB; ++b) eta[b] = 0.0;
    for (int f = sl; f < PM; f += 8) {
      double v = xr[f - sl];
      v = (v - stdv[f]) * stdv[PM + f];
      if (f == 0 && ic) v = 1.0;
#pragma unroll
      for (int b = 0; b < EMAXB; ++b)
        if (b < B) eta[b] = fma(v, bet[b * PM + f], eta[b]);
    }
    const double yv = ys[rB];
    [[maybe_unused]] double ov = 0.0;
    if constexpr (OFS) ov = RS::offset(ys, rB);
    [[maybe_unused]] double om = 1.0;
    if constexpr (WGT) om = valid ? ys[RS::WGT_OFF / 8 + rB] : 0.0;
    double lg = 0.0;  // lgamma(y + 1): 0 at y = 0 and y = 1
    if constexpr (FAM == FAMILY_POISSON)
      if (valid && sl == 0 && yv != 0.0 && yv != 1.0) lg = lgamma1p(yv);
#pragma unroll
    for (int b = 0; b < EMAXB; ++b) {
      if (b < B) {
        double e = ev_red8(eta[b]);
        if constexpr (OFS) e += ov;
        if (valid && sl == 0) llacc[b] += row_loglik<FAM>(e, yv, om, lg);
      }
    }
  }
  wait_vmcnt<0>();
  __syncthreads();
#pragma unroll
  for (int b = 0; b < EMAXB; ++b) {
    if (b < B) {
      double v = llacc[b];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane == 0) red[wid * EMAXB + b] = v;
    }
  }
  __syncthreads();
  if (tid < B) {
    double s = 0.0;
    for (int w = 0; w < EW; ++w) s += red[w * EMAXB + tid];
    a.partial[(int64_t)chunk * B + tid] = s;
  }
}

// One launch of the <FAM, EX> kernel on its slice of the arguments.
template <int FAM, int EX>
inline hipError_t launch_eval_kernel(const EvalArgsWgt& a, int n_chunks, hipStream_t s) {
  auto kern = loglik_eval_kernel<FAM, EX>;
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  const typename eval_args_of<EX>::type& slice = a;
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(256), eval_lds_bytes(a), s, slice);
  return hipGetLastError();
}
// the unit that holds the weighted instantiations (eval_pass_wgt.hip)
hipError_t launch_eval_unit_wgt(const EvalArgsWgt& a, int family, int n_chunks, hipStream_t s);

}  // namespace dlsa
