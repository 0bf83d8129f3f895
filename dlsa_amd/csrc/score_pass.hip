// Score outer-product pass on the dense layout: per partition the weighted
// Gram sum_i d_i x_i x_i^T -- the meat of the sandwich (Huber-White)
// covariance with d = s^2, s = omega (y - mu), or the information matrix with
// d = omega w -- and the score sum_i s_i x_i, at one coefficient vector per
// partition.  This unit holds the logistic kernels, the launcher and the
// fixed-order reductions of the chunk partials; score_pass_pois.hip the
// Poisson kernels (score_pass_impl.hpp).
#include "score_pass_impl.hpp"

namespace dlsa {

hipError_t launch_score_pass(const GramArgs& a, int family, int n_chunks, hipStream_t s) {
  const FamilyRules rules = family_rules(family);
  if (a.eta_offset && !rules.offset) return hipErrorInvalidValue;
  if (a.P < 1 || a.P > DLSA_MAX_P_FUSED) return hipErrorInvalidValue;
  if (family == FAMILY_POISSON) return launch_score_unit_pois(a, n_chunks, s);
  if (family != FAMILY_LOGISTIC) return hipErrorInvalidValue;
  return launch_score_family<FAMILY_LOGISTIC>(a, n_chunks, s,
                                              std::make_integer_sequence<int, kScoreMaxNT>{});
}

namespace {

// Partition blockIdx.x, elements e < P P of its Gram (the lower-triangle tile
// entry of (max(i, j), min(i, j)): both triangles from one value) and P <= e -
// P P < P of its score: the chunk partials summed in chunk order.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* slab_G,
                                                          const double* slab_s,
                                                          const int32_t* pcb, int P, int NT,
                                                          double* gram, double* score) {
  const int k = blockIdx.x;
  const int e = blockIdx.y * 256 + threadIdx.x;
  if (e >= P * P + P) return;
  const int c0 = pcb[k], c1 = pcb[k + 1];
  const int T = NT * (NT + 1) / 2, PMAX = 16 * NT;
  double v = 0.0;
  if (e < P * P) {
    const int i = e / P, j = e - i * P;
    const int r = i > j ? i : j, c = i > j ? j : i;
    const int I = r >> 4, J = c >> 4;
    const int64_t o = (int64_t)(I * (I + 1) / 2 + J) * 256 + (r & 15) * 16 + (c & 15);
    for (int ch = c0; ch < c1; ++ch) v += slab_G[(int64_t)ch * T * 256 + o];
    gram[(int64_t)k * P * P + e] = v;
  } else {
    const int f = e - P * P;
    for (int ch = c0; ch < c1; ++ch) v += slab_s[(int64_t)ch * PMAX + f];
    score[(int64_t)k * P + f] = v;
  }
}

// out[e] = sum over k ascending of in[k * n + e]
__global__ __launch_bounds__(256) void gram_total_kernel(const double* in, int K, int n,
                                                         double* out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double v = 0.0;
  for (int k = 0; k < K; ++k) v += in[(int64_t)k * n + e];
  out[e] = v;
}

}  // namespace

hipError_t launch_gram_reduce(const GramArgs& a, const int32_t* pcb, int K, double* gram,
                              double* score, double* gram_sum, double* score_sum, hipStream_t s) {
  const int P = a.P, NT = (P + 15) / 16;
  if (K > 0) {
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(K, (P * P + P + 255) / 256), dim3(256), 0, s,
                       a.slab_G, a.slab_s, pcb, P, NT, gram, score);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (gram_sum)
    hipLaunchKernelGGL(gram_total_kernel, dim3((P * P + 255) / 256), dim3(256), 0, s, gram, K,
                       P * P, gram_sum);
  if (score_sum)
    hipLaunchKernelGGL(gram_total_kernel, dim3((P + 255) / 256), dim3(256), 0, s, score, K, P,
                       score_sum);
  return hipGetLastError();
}

}  // namespace dlsa
