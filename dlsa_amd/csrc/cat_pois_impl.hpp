// Poisson regression (log link) on the categorical-code layout: what each of
// the four row-extras units (cat_pass_pois.hip: none, cat_pass_pois_ofs.hip,
// cat_pass_pois_wgt.hip, cat_pass_pois_ofs_wgt.hip) instantiates -- the pass
// kernels of cat_pass_impl.hpp with FAM = FAMILY_POISSON, and the presence
// kernel below.  The grids of this family are sized on the device before every
// pass (cat_pass_pois.hip).
#pragma once
#include "cat_pass_impl.hpp"

namespace dlsa {

// v > 0 and finite as ordered bits, else 0 (a value <= 0 or non-finite never
// raises a maximum: a negative or non-finite y, offset or omega has ended its
// partition already, launch_fit_prepass)
__device__ __forceinline__ unsigned long long pos_finite_bits(double v, bool in) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (in && v > 0.0 && u < 0x7FF0000000000000ull) ? u : 0ull;
}

// The presence pass of a Poisson fit: the weighted logistic one's row-oriented
// form (cat_presence_kernel<QS, true>: one row per lane, four rows in flight,
// every load unconditional; a level is present only in a row with omega > 0;
// codes >= levels[f] counted whatever the weight; colmax as there) for every
// mask, because it also takes, the way wmax is taken, ymax[chunk] = the
// chunk's largest finite y and (EX_OFS) omax[chunk] = its largest finite
// offset; wmax only with EX_WGT.  The launcher zeroes the outputs.
template <int QS, int RX>
__global__ __launch_bounds__(256) void cat_presence_pois_kernel(const CatArgsPois a, int S,
                                                                int32_t* counts, int32_t* bad,
                                                                double* colmax) {
  constexpr bool WGT = (RX & EX_WGT) != 0, OFS = (RX & EX_OFS) != 0;
  __shared__ int32_t flag[kCatPMax];
  __shared__ int32_t nbad;
  __shared__ unsigned long long cmax[kCatQMax];
  __shared__ unsigned long long rmaxs[3];   // y, offset, omega
  __shared__ int32_t t_nd[kCatMaxFactors];  // nlev | doff << 16
  const int chunk = blockIdx.x / S, sub = blockIdx.x - chunk * S;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int F = a.F, q = a.q;
  const int D = a.P - a.intercept - q;
  const int doff0 = a.intercept + q;
  for (int i = tid; i < kCatPMax; i += 256) flag[i] = 0;
  if (tid < kCatQMax) cmax[tid] = 0ull;
  if (tid < kCatMaxFactors) t_nd[tid] = a.nlev[tid] | ((a.doff[tid] - doff0) << 16);
  if (tid < 3) rmaxs[tid] = 0ull;
  if (tid == 0) nbad = 0;
  __syncthreads();
  const int nrows = a.chunk_rows[chunk];
  const int rps = (nrows + S - 1) / S;
  const int r_begin = min(nrows, sub * rps), r_end = min(nrows, r_begin + rps);
  const int64_t row0 = a.chunk_row0[chunk] + r_begin;
  const int rows = r_end - r_begin;

  // ---- y, the extras and the codes by row, rows [row0, row0 + rows) ----------
  if (rows > 0) {
    constexpr int U = 4;
    const uint8_t* cb = a.codes + row0 * F;  // (not dereferenced when F = 0)
    unsigned long long ym = 0ull, omx = 0ull, wm = 0ull;
    int nb = 0;
    for (int r0 = tid; r0 < rows; r0 += 256 * U) {
      int rr[U];
      double yv[U], om[U], of[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        rr[k] = min(r0 + 256 * k, rows - 1);
        yv[k] = a.y[row0 + rr[k]];
        om[k] = WGT ? a.row_weight[row0 + rr[k]] : 1.0;
        of[k] = OFS ? a.eta_offset[row0 + rr[k]] : 0.0;
      }
      for (int f = 0; f < F; ++f) {
        int c[U];
#pragma unroll
        for (int k = 0; k < U; ++k) c[k] = (int)cb[(int64_t)rr[k] * F + f];
        const int nd = t_nd[f];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const bool in = r0 + 256 * k < rows;
          const bool isbad = in && c[k] > (nd & 0xFFFF);
          nb += isbad ? 1 : 0;
          if (in && !isbad && c[k] > 0 && om[k] > 0.0) flag[(nd >> 16) + c[k] - 1] = 1;
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const bool in = r0 + 256 * k < rows;
        ym = max(ym, pos_finite_bits(yv[k], in));
        if constexpr (OFS) omx = max(omx, pos_finite_bits(of[k], in));
        if constexpr (WGT) wm = max(wm, pos_finite_bits(om[k], in));
      }
    }
    if (nb) atomicAdd(&nbad, nb);
    if (ym) __hip_atomic_fetch_max(&rmaxs[0], ym, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (omx) __hip_atomic_fetch_max(&rmaxs[1], omx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wm) __hip_atomic_fetch_max(&rmaxs[2], wm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }

  // ---- numeric columns: doubles [row0 q, (row0 + rows) q), as cat_presence_kernel
  if (q > 0 && rows > 0) {
    const double* xb = a.Xn + row0 * q;
    const int64_t ne = (int64_t)rows * q;
    const int64_t wstride = 4LL * q * 64;  // doubles per workgroup window (a multiple of q)
    unsigned long long mx[QS];  // max |x| as bits (|x| >= 0 orders like its bits)
#pragma unroll
    for (int s = 0; s < QS; ++s) mx[s] = 0ull;
    for (int64_t e0 = (int64_t)wid * q * 64; e0 < ne; e0 += 2 * wstride) {
      double v[2][QS];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < QS; ++s) {
          const int64_t e = e0 + h * wstride + s * 64 + lane;
          v[h][s] = __builtin_nontemporal_load(xb + ((s < q && e < ne) ? e : 0));
        }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < QS; ++s) asm volatile("" : "+v"(v[h][s]));
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < QS; ++s) {
          const int64_t e = e0 + h * wstride + s * 64 + lane;
          const unsigned long long u =
              (unsigned long long)__double_as_longlong(v[h][s]) & 0x7FFFFFFFFFFFFFFFull;
          const bool ok = s < q && e < ne && u < 0x7FF0000000000000ull;
          mx[s] = max(mx[s], ok ? u : 0ull);
        }
    }
#pragma unroll
    for (int s = 0; s < QS; ++s)
      if (s < q)
        __hip_atomic_fetch_max(&cmax[(s * 64 + lane) % q], mx[s], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int d = tid; d < D; d += 256)
    if (flag[d]) counts[(int64_t)chunk * D + d] = 1;
  if (tid == 0 && nbad) atomicAdd(&bad[chunk], nbad);
  if (tid < q && cmax[tid])
    __hip_atomic_fetch_max((unsigned long long*)&colmax[(int64_t)chunk * kCatQMax + tid], cmax[tid],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid < 3 && rmaxs[tid]) {
    double* dst = tid == 0 ? a.ymax : tid == 1 ? a.omax : a.wmax;
    __hip_atomic_fetch_max((unsigned long long*)&dst[chunk], rmaxs[tid], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the body of launch_cat_presence_pois_unit<RX>: clears the outputs (ymax,
// omax and wmax all three: the bounds kernel reads them whatever the mask)
template <int RX>
static hipError_t launch_cat_presence_pois_t(const CatArgsPois& a, int n_chunks, int32_t* counts,
                                             int32_t* bad, double* colmax, hipStream_t s) {
  if (n_chunks <= 0) return hipSuccess;
  if (!a.ymax || !a.omax || !a.wmax) return hipErrorInvalidValue;
  const int D = a.P - a.intercept - a.q;
  hipError_t e = hipMemsetAsync(counts, 0, 4LL * n_chunks * std::max(D, 1), s);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 4LL * n_chunks, s);
  if (e == hipSuccess) e = hipMemsetAsync(colmax, 0, 8LL * kCatQMax * n_chunks, s);
  for (double* p : {a.ymax, a.omax, a.wmax})
    if (e == hipSuccess) e = hipMemsetAsync(p, 0, 8LL * n_chunks, s);
  if (e != hipSuccess) return e;
  const int S = std::max(1, std::min(64, (4096 + n_chunks - 1) / n_chunks));
  auto kern = a.q <= 4 ? cat_presence_pois_kernel<4, RX>
              : a.q <= 8 ? cat_presence_pois_kernel<8, RX>
              : a.q <= 12 ? cat_presence_pois_kernel<12, RX> : cat_presence_pois_kernel<16, RX>;
  hipLaunchKernelGGL(kern, dim3(n_chunks * S), dim3(256), 0, s, a, S, counts, bad, colmax);
  return hipGetLastError();
}

// One unit: the two entry points of mask RX.
#define DLSA_CAT_POIS_UNIT(RX)                                                                   \
  template <>                                                                                    \
  hipError_t launch_cat_pass_pois_unit<RX>(const CatArgsPois& a, bool standardize, int n_chunks, \
                                           hipStream_t s) {                                      \
    return launch_cat_pass_t<FAMILY_POISSON, RX>(a, standardize, n_chunks, s);                   \
  }                                                                                              \
  template <>                                                                                    \
  hipError_t launch_cat_presence_pois_unit<RX>(const CatArgsPois& a, int n_chunks,               \
                                               int32_t* counts, int32_t* bad, double* colmax,    \
                                               hipStream_t s) {                                  \
    return launch_cat_presence_pois_t<RX>(a, n_chunks, counts, bad, colmax, s);                  \
  }

}  // namespace dlsa
