// dlsa_glm_gram_categorical: the score outer-product pass on the
// categorical-code layout (cat_gram_impl.hpp).  Two sweeps over the rows: the
// measuring sweep below, which sizes the fixed-point grids from the terms
// themselves and finds invalid codes, then the gram-mode categorical pass; the
// chunk partials are reduced by the dense entry's launch_gram_reduce (the slab
// layouts are the same).
#include "cat_gram_impl.hpp"
#include "fit_driver.hpp"

namespace dlsa {

namespace {

// |v| as ordered bits into mx, or the not-finite flag
__device__ __forceinline__ void gb_note(unsigned long long& mx, bool& nf, double v, bool in) {
  const unsigned long long u =
      (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;
  const bool fin = u < 0x7FF0000000000000ull;
  nf = nf || (in && !fin);
  mx = max(mx, (in && fin) ? u : 0ull);
}

// The measuring sweep: each chunk split over S workgroups (contiguous row
// ranges, as the presence pass is), one row per thread and step with the
// partition's coefficients in LDS; every load is unconditional (a lane past
// the range re-reads the range's last row and discards it).  A code >=
// levels[f] is counted and takes the baseline's 0.  The maxima and counts are
// order-free (integer max / add), so the grids are the same bits run to run.
template <int FAM, int QS>
__global__ __launch_bounds__(256) void cat_gram_bounds_kernel(const CatGramBoundsArgs a, int S) {
  __shared__ double th[kCatPMax];
  __shared__ double stdv[2 * kCatQMax];
  __shared__ unsigned long long smax[kCatQMax + 2];
  __shared__ int32_t sflag[2];  // bad codes, not finite
  __shared__ int32_t s_lev[kCatMaxFactors], s_doff[kCatMaxFactors];
  const int chunk = blockIdx.x / S, sub = blockIdx.x - chunk * S;
  const int tid = threadIdx.x;
  const int q = a.q, F = a.F, P = a.P, ic = a.intercept;
  const double* beta = a.betas + a.chunk_part[chunk] * a.beta_part_stride;
  for (int i = tid; i < kCatPMax; i += 256) th[i] = i < P ? beta[i] : 0.0;
  if (tid < kCatQMax) {
    const bool in = a.center && tid < q;
    stdv[tid] = in ? a.center[tid] : 0.0;
    stdv[kCatQMax + tid] = in ? 1.0 / a.scale[tid] : 1.0;
  }
  if (tid < kCatQMax + 2) smax[tid] = 0ull;
  if (tid < 2) sflag[tid] = 0;
  if (tid < kCatMaxFactors) {
    s_lev[tid] = tid < F ? a.levels[tid] : 1;
    s_doff[tid] = tid < F ? a.doff[tid] : 0;
  }
  __syncthreads();
  const int nrows = a.chunk_rows[chunk];
  const int rps = (nrows + S - 1) / S;
  const int r_begin = min(nrows, sub * rps), r_end = min(nrows, r_begin + rps);
  const int64_t row0 = a.chunk_row0[chunk] + r_begin;
  const int rows = r_end - r_begin;
  if (rows <= 0) return;  // workgroup-uniform

  unsigned long long mx[QS + 2];
#pragma unroll
  for (int i = 0; i < QS + 2; ++i) mx[i] = 0ull;
  int nb = 0;
  bool nf = false;
  const bool info = a.kind == GRAM_INFORMATION;
  for (int r0 = 0; r0 < rows; r0 += 256) {
    const bool in = r0 + tid < rows;
    const int64_t row = row0 + min(r0 + tid, rows - 1);
    double xv[QS];
    double e = ic ? th[0] : 0.0;
    if (q > 0) {
      const double* xr = a.Xn + row * q;
#pragma unroll
      for (int j = 0; j < QS; ++j) {
        double v = xr[j < q ? j : q - 1];
        v = (v - stdv[j < q ? j : 0]) * stdv[kCatQMax + (j < q ? j : 0)];
        xv[j] = j < q ? v : 0.0;
        e = fma(xv[j], th[ic + (j < q ? j : 0)], e);
      }
    } else {
#pragma unroll
      for (int j = 0; j < QS; ++j) xv[j] = 0.0;
    }
    if (F > 0) {
      const uint8_t* cr = a.codes + row * F;
      for (int f = 0; f < F; ++f) {
        const int c = (int)cr[f];
        const bool isbad = c >= s_lev[f];
        nb += (isbad && in) ? 1 : 0;
        const bool on = !isbad && c > 0;
        const double t = th[on ? s_doff[f] + c - 1 : 0];
        e += on ? t : 0.0;
      }
    }
    if (a.eta_offset) e += a.eta_offset[row];
    const double yv = a.y[row];
    const double om = a.row_weight ? a.row_weight[row] : 1.0;
    const RowMean k = row_mean<FAM>(e);
    const double s = om * (yv - k.mu);
    const double d = info ? om * k.w : s * s;
    gb_note(mx[0], nf, d, in);
    gb_note(mx[1], nf, s, in);
#pragma unroll
    for (int j = 0; j < QS; ++j) gb_note(mx[2 + j], nf, d * xv[j], in && j < q);
  }
#pragma unroll
  for (int i = 0; i < QS + 2; ++i)
    if (mx[i])
      __hip_atomic_fetch_max(&smax[i], mx[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (nb) atomicAdd(&sflag[0], nb);
  if (nf) sflag[1] = 1;
  __syncthreads();
  if (tid < kCatQMax + 2 && smax[tid])
    __hip_atomic_fetch_max(&a.bmax[(int64_t)chunk * (kCatQMax + 2) + tid], smax[tid],
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0 && sflag[0]) atomicAdd(&a.bad[chunk], sflag[0]);
  if (tid == 0 && sflag[1]) a.nonfinite[chunk] = 1;
}

template <int FAM>
hipError_t bounds_launch(const CatGramBoundsArgs& a, int n_chunks, int S, hipStream_t s) {
  auto kern = a.q <= 4 ? cat_gram_bounds_kernel<FAM, 4>
              : a.q <= 8 ? cat_gram_bounds_kernel<FAM, 8>
              : a.q <= 12 ? cat_gram_bounds_kernel<FAM, 12> : cat_gram_bounds_kernel<FAM, 16>;
  hipLaunchKernelGGL(kern, dim3(n_chunks * S), dim3(256), 0, s, a, S);
  return hipGetLastError();
}

// One wave per partition: lane i < kCatQMax + 2 takes slot i's maximum over
// the partition's chunks and writes its grid.
__global__ __launch_bounds__(64) void cat_gram_grid_kernel(const unsigned long long* bmax,
                                                           const int32_t* nonfinite,
                                                           const int32_t* pcb, double rmax,
                                                           double* hscale) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (lane >= kCatQMax + 2) return;
  const int cb = pcb[k], ce = pcb[k + 1];
  unsigned long long m = 0ull;
  int nf = 0;
  for (int c = cb; c < ce; ++c) {
    m = max(m, bmax[(int64_t)c * (kCatQMax + 2) + lane]);
    nf |= nonfinite[c];
  }
  double grid = 1.0;
  if (m) {
    const double B = __longlong_as_double((long long)m);
    // (log2 B + log2 R, not log2 (B R): the product may overflow)
    const double ex = floor(60.0 - (log2(B) + log2(rmax)));
    grid = ldexp(1.0, (int)fmin(900.0, fmax(-900.0, ex)));
  }
  if (nf && lane == 0) grid = __longlong_as_double(0x7FF8000000000000ll);  // a quiet NaN
  hscale[(int64_t)k * (kCatQMax + 2) + lane] = grid;
}

// dst [K, P]: K copies of src [P]
__global__ __launch_bounds__(256) void replicate_kernel(const double* src, int P, int64_t n,
                                                        double* dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i % P];
}

template <int FAM, int RX>
hipError_t gram_by_kind(const CatArgsPois& a, int kind, bool standardize, int n_chunks,
                        hipStream_t s) {
  // (the slice of CatArgsPois the kernels of (FAM, RX) take)
  const typename cat_pass_args_of<FAM, RX>::type& sl = a;
  return kind == GRAM_INFORMATION
             ? launch_cat_gram_unit<FAM, RX, CAT_ROW_GRAM_INFORMATION>(sl, standardize, n_chunks, s)
             : launch_cat_gram_unit<FAM, RX, CAT_ROW_GRAM_SCORE>(sl, standardize, n_chunks, s);
}

}  // namespace

hipError_t launch_cat_gram_bounds(const CatGramBoundsArgs& a, int family, int n_chunks,
                                  hipStream_t s) {
  if (n_chunks <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.bmax, 0, 8LL * (kCatQMax + 2) * n_chunks, s);
  if (e == hipSuccess) e = hipMemsetAsync(a.bad, 0, 4LL * n_chunks, s);
  if (e == hipSuccess) e = hipMemsetAsync(a.nonfinite, 0, 4LL * n_chunks, s);
  if (e != hipSuccess) return e;
  // ~16 workgroups per CU in total (a streaming sweep: loads in flight)
  const int S = std::max(1, std::min(64, (4096 + n_chunks - 1) / n_chunks));
  return family == FAMILY_POISSON ? bounds_launch<FAMILY_POISSON>(a, n_chunks, S, s)
                                  : bounds_launch<FAMILY_LOGISTIC>(a, n_chunks, S, s);
}

hipError_t launch_cat_gram_grid(const CatGramBoundsArgs& a, const int32_t* pcb, int K,
                                double rmax, double* hscale, hipStream_t s) {
  if (K <= 0) return hipSuccess;
  hipLaunchKernelGGL(cat_gram_grid_kernel, dim3(K), dim3(64), 0, s, a.bmax, a.nonfinite, pcb, rmax,
                     hscale);
  return hipGetLastError();
}

hipError_t launch_cat_gram(const CatArgsPois& a, int family, int kind, bool standardize,
                           int n_chunks, hipStream_t s) {
  if (kind != GRAM_SCORE && kind != GRAM_INFORMATION) return hipErrorInvalidValue;
  if (family == FAMILY_POISSON) {
    switch (pass_extras(a)) {
      case EX_NONE: return gram_by_kind<FAMILY_POISSON, EX_NONE>(a, kind, standardize, n_chunks, s);
      case EX_OFS: return gram_by_kind<FAMILY_POISSON, EX_OFS>(a, kind, standardize, n_chunks, s);
      case EX_WGT: return gram_by_kind<FAMILY_POISSON, EX_WGT>(a, kind, standardize, n_chunks, s);
      default:
        return gram_by_kind<FAMILY_POISSON, EX_OFS | EX_WGT>(a, kind, standardize, n_chunks, s);
    }
  }
  if (family != FAMILY_LOGISTIC || a.eta_offset) return hipErrorInvalidValue;
  return a.row_weight ? gram_by_kind<FAMILY_LOGISTIC, EX_WGT>(a, kind, standardize, n_chunks, s)
                      : gram_by_kind<FAMILY_LOGISTIC, EX_NONE>(a, kind, standardize, n_chunks, s);
}

}  // namespace dlsa

using namespace dlsa;

extern "C" int dlsa_glm_gram_categorical(int32_t family, int32_t kind, const double* Xn,
                                         const uint8_t* codes, const double* y,
                                         const double* eta_offset, const double* row_weight,
                                         const int64_t* offsets, int32_t K, int32_t q, int32_t F,
                                         const int32_t* levels, int32_t fit_intercept,
                                         const double* center, const double* scale,
                                         const double* betas, int64_t beta_part_stride,
                                         int32_t rows_per_chunk, double* gram, double* score,
                                         double* gram_sum, double* score_sum, void* stream_) {
  g_last_error.clear();
  hipStream_t stream = (hipStream_t)stream_;
  int rc = check_offsets(offsets, K);
  if (rc != DLSA_OK) return rc;
  if (family != FAMILY_LOGISTIC && family != FAMILY_POISSON) {
    set_error("dlsa_glm_gram_categorical: family must be DLSA_FAMILY_LOGISTIC or "
              "DLSA_FAMILY_POISSON");
    return DLSA_E_UNSUPPORTED;
  }
  const int ic = fit_intercept ? 1 : 0;
  int D = 0, P = 0;
  rc = check_cat_shape(q, F, levels, ic, DLSA_MAX_P_FUSED, "gram", &D, &P);
  if (rc != DLSA_OK) return rc;
  if (rows_per_chunk < 0 || !betas || !gram || !score ||
      (kind != GRAM_SCORE && kind != GRAM_INFORMATION) ||
      (center == nullptr) != (scale == nullptr)) {
    set_error("dlsa_glm_gram_categorical: invalid arguments (kind DLSA_GRAM_SCORE or "
              "DLSA_GRAM_INFORMATION, rows_per_chunk >= 0, center and scale both or neither)");
    return DLSA_E_INVALID;
  }
  if (eta_offset && !family_rules(family).offset) {
    set_error("eta_offset is the Poisson family's");
    return DLSA_E_INVALID;
  }
  if (beta_part_stride != 0 && beta_part_stride != P) {
    set_error("dlsa_glm_gram_categorical: beta_part_stride must be 0 or P");
    return DLSA_E_INVALID;
  }
  const int64_t n_total = offsets[K];
  if (n_total > 0 && (!y || (q > 0 && !Xn) || (F > 0 && !codes))) {
    set_error("null Xn, codes or y");
    return DLSA_E_INVALID;
  }
  CatArgsPois ca;  // (every kernel takes its slice: CatArgs, CatArgsWgt or all of it)
  memset(&ca, 0, sizeof(ca));
  ca.q = q;
  ca.F = F;
  ca.P = P;
  ca.intercept = ic;
  CatGramBoundsArgs ba;
  memset(&ba, 0, sizeof(ba));
  for (int f = 0, d = ic + q; f < F; ++f) {
    ca.doff[f] = d;
    ba.doff[f] = d;
    ba.levels[f] = levels[f];
    d += levels[f] - 1;
  }
  if (!cat_layout(ca, levels)) {
    set_error("categorical histograms do not fit the 160 KB LDS of a workgroup (P = " +
              std::to_string(P) + ")");
    return DLSA_E_UNSUPPORTED;
  }
  // the chunk plan of the categorical fit's full-data level (fit_cat.hip
  // cat_rpc): ~512 chunks, split evenly per partition, of at least 1024 rows
  int rpc = rows_per_chunk;
  if (rpc <= 0) {
    int64_t nmax = 0;
    for (int k = 0; k < K; ++k) nmax = std::max(nmax, offsets[k + 1] - offsets[k]);
    const int64_t per = std::max<int64_t>(1, 512 / std::max(K, 1));
    rpc = (int)std::max<int64_t>(1024, std::min<int64_t>((nmax + per - 1) / per, 1 << 24));
  }
  Plan pl;
  make_plan(offsets, K, P - ic, ic, rpc, pl, 1.0, 0, /*x_cols=*/q);
  const int64_t nc = std::max(pl.n_chunks, 1);
  const int64_t Kp = std::max(K, 1);
  Bump b;
  const int64_t off_row0 = b.take(8 * nc), off_rows = b.take(4 * nc), off_part = b.take(4 * nc);
  const int64_t off_pcb = b.take(4LL * (K + 1));
  const int64_t off_G = b.take(8 * nc * pl.T * 256), off_s = b.take(8 * nc * pl.PP);
  const int64_t off_bmax = b.take(8 * nc * (kCatQMax + 2));
  const int64_t off_bad = b.take(4 * nc), off_nf = b.take(4 * nc);
  const int64_t off_hs = b.take(8 * Kp * (kCatQMax + 2));
  const int64_t off_beta = beta_part_stride == 0 ? b.take(8 * Kp * P) : 0;
  Workspace ws(stream);  // stream-ordered scratch
  rc = ws.alloc(b.o);
  if (rc != DLSA_OK) return rc;
  int64_t* d_row0 = (int64_t*)ws.at(off_row0);
  int32_t* d_rows = (int32_t*)ws.at(off_rows);
  int32_t* d_part = (int32_t*)ws.at(off_part);
  int32_t* d_pcb = (int32_t*)ws.at(off_pcb);
  double* d_hs = (double*)ws.at(off_hs);
  GramArgs ga;  // (what launch_gram_reduce reads)
  memset(&ga, 0, sizeof(ga));
  ga.P = P;
  ga.slab_G = (double*)ws.at(off_G);
  ga.slab_s = (double*)ws.at(off_s);
  {
    // (from pageable vectors: each copy has left the host when the call returns)
    hipError_t e = hipSuccess;
    auto up = [&](void* dst, const void* src, int64_t bytes) {
      if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    };
    if (pl.n_chunks > 0) {
      up(d_row0, pl.chunk_row0.data(), 8LL * pl.n_chunks);
      up(d_rows, pl.chunk_rows.data(), 4LL * pl.n_chunks);
      up(d_part, pl.chunk_part.data(), 4LL * pl.n_chunks);
    }
    up(d_pcb, pl.part_chunk_begin.data(), 4LL * (K + 1));
    DLSA_HIP_TRY(e);
  }
  if (pl.n_chunks > 0) {
    ba.Xn = Xn;
    ba.codes = codes;
    ba.y = y;
    ba.eta_offset = eta_offset;
    ba.row_weight = row_weight;
    ba.chunk_row0 = d_row0;
    ba.chunk_rows = d_rows;
    ba.chunk_part = d_part;
    ba.center = center;
    ba.scale = scale;
    ba.betas = betas;
    ba.beta_part_stride = beta_part_stride;
    ba.bmax = (unsigned long long*)ws.at(off_bmax);
    ba.bad = (int32_t*)ws.at(off_bad);
    ba.nonfinite = (int32_t*)ws.at(off_nf);
    ba.q = q;
    ba.F = F;
    ba.P = P;
    ba.intercept = ic;
    ba.kind = kind;
    DLSA_HIP_TRY(launch_cat_gram_bounds(ba, family, pl.n_chunks, stream));
    // invalid codes end the call before the gram pass is launched
    std::vector<int32_t> h_bad(pl.n_chunks, 0);
    DLSA_HIP_TRY(hipMemcpyAsync(h_bad.data(), ba.bad, 4LL * pl.n_chunks, hipMemcpyDeviceToHost,
                                stream));
    DLSA_HIP_TRY(hipStreamSynchronize(stream));
    for (int k = 0; k < K; ++k) {
      int64_t nbad = 0;
      for (int c = pl.part_chunk_begin[k]; c < pl.part_chunk_begin[k + 1]; ++c) nbad += h_bad[c];
      if (nbad) {
        set_error("partition " + std::to_string(k) + ": " + std::to_string(nbad) +
                  " level codes >= levels[f]");
        return DLSA_E_INVALID;
      }
    }
    const double rmax = (double)std::max(1024, pl.max_chunk_rows);
    DLSA_HIP_TRY(launch_cat_gram_grid(ba, d_pcb, K, rmax, d_hs, stream));
    const double* theta = betas;
    if (beta_part_stride == 0) {  // one vector for all: replicated to [K, P]
      double* rep = (double*)ws.at(off_beta);
      const int64_t n = (int64_t)K * P;
      hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                         betas, P, n, rep);
      DLSA_HIP_TRY(hipGetLastError());
      theta = rep;
    }
    ca.Xn = Xn;
    ca.codes = codes;
    ca.y = y;
    ca.row_weight = row_weight;
    ca.eta_offset = eta_offset;
    ca.chunk_row0 = d_row0;
    ca.chunk_rows = d_rows;
    ca.chunk_part = d_part;
    ca.theta = theta;
    ca.center = center;
    ca.scale = scale;
    ca.slab_H = ga.slab_G;
    ca.slab_g = ga.slab_s;
    ca.NT = pl.NT;
    ca.hscale = d_hs;
    DLSA_HIP_TRY(launch_cat_gram(ca, family, kind, center != nullptr, pl.n_chunks, stream));
  }
  DLSA_HIP_TRY(launch_gram_reduce(ga, d_pcb, K, gram, score, gram_sum, score_sum, stream));
  DLSA_HIP_TRY(hipStreamSynchronize(stream));
  return DLSA_OK;
}
