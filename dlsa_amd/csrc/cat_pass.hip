// The categorical-code pass without prior weights: the unweighted
// instantiations of cat_pass_impl.hpp, and what both share -- the exact-bucket
// rule, the LDS size and the per-partition mark kernel.
#include "cat_pass_impl.hpp"

namespace dlsa {

// Per partition: a selected dummy level with no rows -> the reference's
// all-zero frame (models.py:84-91): status MISSING_LEVEL, phase DONE, outputs
// stay zero (fit_init zeroed theta / Sig_inv).  bad_part[k] = invalid codes.
__global__ __launch_bounds__(256) void cat_mark_kernel(const CatArgs a, const int32_t* pcb,
                                                       const int32_t* counts, const int32_t* bad,
                                                       int32_t* phase, int32_t* status,
                                                       int32_t* bad_part) {
  __shared__ int32_t flag[2];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int D = a.P - a.intercept - a.q;
  if (tid < 2) flag[tid] = 0;
  __syncthreads();
  const int cb = pcb[k], ce = pcb[k + 1];
  for (int d = tid; d < D; d += 256) {
    int64_t s = 0;
    for (int c = cb; c < ce; ++c) s += counts[(int64_t)c * D + d];
    if (s == 0) flag[0] = 1;
  }
  int nb = 0;
  for (int c = cb + tid; c < ce; c += 256) nb += bad[c];
  if (nb) atomicAdd(&flag[1], nb);
  __syncthreads();
  if (tid == 0) {
    bad_part[k] = flag[1];
    if (ce > cb && flag[0] && status[k] == STATUS_RUNNING) {
      status[k] = DLSA_STATUS_MISSING_LEVEL;
      phase[k] = PHASE_DONE;
    }
  }
}

// the exact-bucket instantiation (EX): intercept fitted, 1 + q equal to its
// column bucket, 1 <= F <= 8 (the host layout then names a fold factor)
bool cat_exact_bucket(const CatArgs& a) {
  return a.intercept == 1 && a.F >= 1 && a.F <= 8 && a.q + 1 == cat_qn(1 + a.q);
}

size_t cat_lds_bytes(const CatArgs& a) {
  const int QN = cat_qn(a.intercept + a.q);
  const int NR = QN * (QN + 1) / 2 + QN + 1;  // (the EX kernel's NR is smaller)
  const int NW = cat_threads_t(QN, a.F <= 8 ? 8 : 16) / 64;
  return 8 * ((size_t)a.hist_doubles + kCatPMax + 2 * kCatQMax + (size_t)(NW + 1) * NR);
}

hipError_t launch_cat_pass(const CatArgs& a, bool standardize, int n_chunks, hipStream_t s) {
  return launch_cat_pass_t<FAMILY_LOGISTIC, EX_NONE>(a, standardize, n_chunks, s);
}

hipError_t launch_cat_presence(const CatArgs& a, int n_chunks, int32_t* counts, int32_t* bad,
                               double* colmax, hipStream_t s) {
  return launch_cat_presence_t<false>(a, n_chunks, counts, bad, colmax, s);
}

hipError_t launch_cat_mark(const CatArgs& a, const int32_t* pcb, const int32_t* counts,
                           const int32_t* bad, int K, int32_t* phase, int32_t* status,
                           int32_t* bad_part, hipStream_t s) {
  hipLaunchKernelGGL(cat_mark_kernel, dim3(K), dim3(256), 0, s, a, pcb, counts, bad, phase,
                     status, bad_part);
  return hipGetLastError();
}

}  // namespace dlsa
