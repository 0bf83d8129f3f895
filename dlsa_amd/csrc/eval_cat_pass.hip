// Log-likelihood evaluation pass on the categorical-code layout, logistic
// family: the instantiations of eval_cat_pass_impl.hpp without and with prior
// weights, the plan every family shares and the job-level total.
#include "eval_cat_pass_impl.hpp"

namespace dlsa {

// Block rows and ring depth: the largest block whose ring of >= 2 slots fits
// the workgroup's LDS beside the tables; up to 4 slots while the workgroup
// stays within half a CU's LDS (two workgroups per CU: the pass is bound by
// the fp64 exp / log1p of every row and candidate, not only by HBM).
bool eval_cat_plan(EvalCatArgs& a, int extras) {
  const int BP = ec_bp(a.nbeta);
  const int fixed = ec_table_doubles(ec_entries(a), a.q, BP) * 8 + kEcStaticLds;
  const int cap = 160 * 1024 - 1024;
  for (int RB : {256, 128, 64}) {
    const int slot = ec_geom(RB, a.q, a.F, extras).slot_bytes;
    if (fixed + 2 * slot > cap) continue;
    a.rb = RB;
    int n = 2;
    while (n < kEcMaxSlots && fixed + (n + 1) * slot <= cap / 2) ++n;
    a.nslot = n;
    return true;
  }
  return false;
}

hipError_t launch_loglik_cat(const EvalCatArgsWgt& a, int n_chunks, hipStream_t s) {
  return a.row_weight ? ec_launch_bp<FAMILY_LOGISTIC, EX_WGT>(a, n_chunks, s)
                      : ec_launch_bp<FAMILY_LOGISTIC, EX_NONE>(a, n_chunks, s);
}

// total[b] = sum_k ll[k, b] in k order: the group-by sum of model_eval.py:38
__global__ void loglik_total_kernel(const double* ll, int K, int B, double* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += ll[(int64_t)k * B + b];
  out[b] = s;
}

hipError_t launch_loglik_total(const double* ll, int K, int B, double* out, hipStream_t s) {
  hipLaunchKernelGGL(loglik_total_kernel, dim3(1), dim3(64), 0, s, ll, K, B, out);
  return hipGetLastError();
}

}  // namespace dlsa
