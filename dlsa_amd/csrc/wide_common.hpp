// Wide-P IRLS path (DLSA_MAX_P_FUSED < P <= DLSA_MAX_P): BASELINE config 5
// (n = 5e6, p = 500, K = 32; mirrors projects/results/speedtest/
// logistic_LBFGS_local.py:12-13).  Same per-partition contract as the fused
// pass (dlsa/models.py:110-131: MLE theta_k, Sig_inv_k = X_k^T W X_k at
// theta_k), but the P x P Hessian no longer fits a workgroup's registers and
// LDS, so one Newton iteration is split into launches:
//
//   wide_fused.hip
//   wide_fused_bf16_kernel  PHASE_F32 partitions (MIXED mode): ONE stream of X
//                       gives eta, w, the fp64 gradient / log-lik AND the
//                       approximate Hessian Z^T Z, Z = bf16(sqrt(w) x)
//                       (bf16 MFMA 16x16x32, fp32 accumulation).
//   wide_exact.hip
//   wide_row_kernel     PHASE_F64 partitions: one streaming pass over X
//                       (HBM-bound): eta, mu, w = mu(1-mu), gradient, log-lik;
//                       writes w[row] (8 B/row) and per-chunk partials.
//   wide_gram_kernel    PHASE_F64: X^T diag(w) X as 128x128 lower-triangle
//                       output tiles, split over row groups (fp64 MFMA
//                       16x16x4, MFMA-bound).  blockIdx -> (row group, tile)
//                       is XCD-aware: all tiles of a row group run on one XCD,
//                       so its rows are fetched from HBM once and re-read from
//                       that XCD's L2 / the MALL.
//   wide_assemble_kernel  fixed-order sum of the row-group partials into the
//                       padded PP x PP Hessian of each partition (identity on
//                       the padding) -- deterministic.
//   wide_newton.hip
//   wide_newton_kernel  one 1024-thread workgroup per partition: step
//                       control (newton_step.hpp), publish Sig_inv, blocked
//                       right-looking Cholesky (32-column panels staged in
//                       LDS, trailing update on fp64 MFMA, the next diagonal
//                       block factored under the current trailing update),
//                       blocked triangular solves, update / convergence.
//
// This header: what those three files share.
#pragma once

#include "dlsa_internal.hpp"
#include "wave_math.hpp"  // wave_sum64, bcast_first

namespace dlsa {

typedef double d4w __attribute__((ext_vector_type(4)));

constexpr int GT = kWideTile;  // gram output tile edge (128)

// lower-triangle tile t -> (I, J), I >= J, row-major over I
__device__ __forceinline__ void tile_ij(int t, int& I, int& J) {
  I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  J = t - I * (I + 1) / 2;
}

}  // namespace dlsa
