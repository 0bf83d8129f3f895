// Log-likelihood evaluation pass on the categorical-code layout: the job-level
// second pass of the reference (dlsa/model_eval.py:10-42 over the per-partition
// body dlsa/models.py:151-225) on the rows the categorical fit consumes -- q
// numeric fp64 columns + F uint8 level codes per row, never the dummy matrix:
//   eta_ib = beta_b[0] ic + sum_j (x_ij - c_j) / s_j beta_b[ic + j] + sum_f T_b[f][code_if]
//   ll[k, b] = sum_i y_i eta_ib - softplus(eta_ib)
// Xn, codes and y are fetched once for all candidates: 8 q + F + 8 B/row.
//
// Geometry: one 4-wave workgroup per chunk, one row per thread, RB-row blocks
// (256; 128 / 64 when the tables leave less LDS) through an LDS-DMA ring like
// the dense pass's (eval_pass.hip).  The dummy coefficients sit in LDS
// entry-major, T[off_f + code][BP] with a zero entry per factor for code 0, so
// a row's lookup is branch-free and its BP candidates are contiguous 16-byte
// reads.  Each chunk writes one partial per candidate and its count of codes
// >= levels[f] (looked up as code 0); no atomics.
//
// WGT: prior weights, ll[k, b] = sum_i omega_i l_ib.  omega is one more stream
// travelling like y: 256-byte pieces behind y in the ring slot, clamped to the
// buffer by w_last4.  The row's term is multiplied by omega and added only for
// a valid row: the rows of a chunk's last block past its end hold the next
// partition's omega, whatever it is.  The weights are not checked here.
//
// FAM, RX: the family and the row-extras mask.  FAMILY_POISSON: the row's term
// is y eta - exp(eta) - lgamma(y + 1) with lgamma computed once per row, not
// per candidate, and eta = ... + eta_offset with EX_OFS, one more stream like
// omega's, between y and omega in the ring slot, clamped by o_last4.
//
// This header holds the kernel template and its launchers: eval_cat_pass.hip
// instantiates the logistic kernels (and holds the plan), eval_cat_pass_pois.hip
// the Poisson ones.
#pragma once
#include "dlsa_internal.hpp"
#include "glm_row.hpp"

namespace dlsa {

constexpr int CW = 4;  // waves

// 1 KiB pieces (64 lanes x 16 B) that cover `bytes` from any start inside a
// 16-byte granule
__host__ __device__ constexpr int ec_pieces16(int bytes) {
  return bytes > 0 ? (bytes + 16 + 1023) / 1024 : 0;
}

struct EcGeom {
  int npx, dx, npc, dc, npy, dy;  // pieces of a block and pieces per wave: X, codes, y
  int c_off, y_off, slot_bytes;
  int npo, dofs, o_off;  // the offset (EX_OFS), pieced like y
  int npw, dw, w_off;    // omega (EX_WGT), pieced like y
};
__host__ __device__ __forceinline__ EcGeom ec_geom(int RB, int q, int F, int ex) {
  EcGeom g;
  g.npx = ec_pieces16(RB * q * 8);
  g.dx = (g.npx + CW - 1) / CW;
  g.npc = ec_pieces16(RB * F);
  g.dc = (g.npc + CW - 1) / CW;
  g.npy = RB / 32;  // 256-byte pieces (64 lanes x 4 B)
  g.dy = (g.npy + CW - 1) / CW;
  g.c_off = g.dx * CW * 1024;
  g.y_off = g.c_off + g.dc * CW * 1024;
  g.npo = (ex & EX_OFS) ? RB / 32 : 0;
  g.dofs = (g.npo + CW - 1) / CW;
  g.o_off = g.y_off + g.dy * CW * 256;
  g.npw = (ex & EX_WGT) ? RB / 32 : 0;
  g.dw = (g.npw + CW - 1) / CW;
  g.w_off = g.o_off + g.dofs * CW * 256;
  g.slot_bytes = g.w_off + g.dw * CW * 256;
  return g;
}

__host__ __device__ __forceinline__ int ec_entries(const EvalCatArgs& a) {
  return a.F > 0 ? a.toff[a.F - 1] + a.levels[a.F - 1] : 0;
}
// doubles after the ring: table, numeric coefficients, centre / 1/scale, wave sums
__host__ __device__ __forceinline__ int ec_table_doubles(int entries, int q, int BP) {
  return entries * BP + (q + 1) * BP + 2 * (q + 1) + CW * kEvalCatMaxB;
}

template <int FAM, int RX>
struct ec_args_of {
  typedef typename std::conditional<
      FAM == FAMILY_POISSON, EvalCatArgsPois,
      typename std::conditional<(RX & EX_WGT) != 0, EvalCatArgsWgt, EvalCatArgs>::type>::type type;
};

// Outstanding loads against the vmcnt waits.  A wave issues per block
//   per_blk = dx + dc + dy + dofs + dw
// loads, at most 9 + 2 + 2 + 2 + 2 at RB = 256, q = 16, F = 16 (33 1-KiB pieces
// of X and 5 of codes, 8 256-B pieces each of y, the offset and omega, each
// over CW waves).
// When it waits for the oldest block, (nslot - 1) per_blk loads are in flight
// and (nslot - 2) per_blk are kept; nslot <= 4 (eval_cat_plan).  Both stay
// inside the 6-bit counter, and the kept count inside wait_vmcnt_le<40>.
constexpr int ec_ceil(int a, int b) { return (a + b - 1) / b; }
constexpr int kEcMaxPerBlk = ec_ceil(ec_pieces16(256 * kCatQMax * 8), CW) +
                             ec_ceil(ec_pieces16(256 * kCatMaxFactors), CW) +
                             3 * ec_ceil(256 / 32, CW);
constexpr int kEcMaxSlots = 4;
static_assert(kEcMaxPerBlk == 17, "per-block loads of a wave");
static_assert((kEcMaxSlots - 1) * kEcMaxPerBlk < 64, "loads in flight fit vmcnt (6 bits)");
static_assert((kEcMaxSlots - 2) * kEcMaxPerBlk <= 40, "kept loads fit wait_vmcnt_le<40>");

template <int BP, int FAM, int RX>
__global__ __launch_bounds__(256) void loglik_cat_kernel(
    const typename ec_args_of<FAM, RX>::type a) {
  constexpr bool WGT = (RX & EX_WGT) != 0, OFS = (RX & EX_OFS) != 0;
  static_assert(FAM == FAMILY_POISSON || !OFS, "the offset is the Poisson family's");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = a.q, F = a.F, P = a.P, ic = a.intercept, B = a.nbeta, RB = a.rb;
  const int64_t row0 = a.chunk_row0[chunk];
  const int nrows = a.chunk_rows[chunk];
  const int nb = (nrows + RB - 1) / RB;
  const int nslot = a.nslot;
  const EcGeom g = ec_geom(RB, q, F, RX);
  const int E = ec_entries(a);

  double* T = (double*)(smem + nslot * g.slot_bytes);  // [E][BP]
  double* bnum = T + E * BP;                           // [q + 1][BP]: intercept, numeric
  double* stdv = bnum + (q + 1) * BP;                  // [2][q + 1]: centre, 1 / scale
  double* red = stdv + 2 * (q + 1);                    // [CW][kEvalCatMaxB]
  __shared__ int32_t s_lev[kCatMaxFactors], s_off[kCatMaxFactors], s_bad[CW];

  if (tid < kCatMaxFactors) {
    s_lev[tid] = tid < F ? a.levels[tid] : 1;
    s_off[tid] = tid < F ? a.toff[tid] : 0;
  }
  for (int f = 0; f < F; ++f) {
    // entry c of factor f: 0 for the baseline, else parameter doff + c - 1,
    // doff = ic + q + (dummy columns of the factors before f) = ic + q + toff[f] - f
    const int off = a.toff[f], nl = a.levels[f], doff = ic + q + off - f;
    for (int e = tid; e < nl * BP; e += 256) {
      const int c = e / BP, b = e - c * BP;
      T[(off + c) * BP + b] = (c > 0 && b < B) ? a.betas[(int64_t)b * P + doff + c - 1] : 0.0;
    }
  }
  for (int e = tid; e < (q + 1) * BP; e += 256) {
    const int j = e / BP, b = e - j * BP;  // j = 0: intercept, j >= 1: numeric column j - 1
    const bool in = b < B && (j > 0 || ic);
    bnum[e] = in ? a.betas[(int64_t)b * P + (j > 0 ? ic + j - 1 : 0)] : 0.0;
  }
  for (int j = tid; j < q; j += 256) {
    stdv[j] = a.center ? a.center[j] : 0.0;
    stdv[q + 1 + j] = a.center ? 1.0 / a.scale[j] : 1.0;
  }
  __syncthreads();

  // DMA sources stay inside [lo, last16]: whole 16-byte granules of the
  // buffer.  A row with bytes outside [lo, hi) (the first / last partial
  // granule of a buffer whose ends are not 16-byte aligned) is read by its own
  // thread with exact-width loads instead.
  const bool xdma = a.x_lo < a.x_hi, cdma = a.c_lo < a.c_hi;
  auto issue = [&](int blk) {
    const int bb = blk < nb ? blk : nb - 1;
    char* sbase = smem + (blk % nslot) * g.slot_bytes;
    const int64_t r = row0 + (int64_t)bb * RB;
    if (xdma) {
      const uintptr_t al = (uintptr_t)(a.Xn + r * q) & ~(uintptr_t)15;
      for (int i = 0; i < g.dx; ++i) {
        const int j = wid + CW * i;
        const int jj = j < g.npx ? j : g.npx - 1;
        uintptr_t src = al + (uintptr_t)jj * 1024 + (uintptr_t)lane * 16;
        src = src < a.x_lo ? a.x_lo : src;
        src = src < a.x_hi - 16 ? src : a.x_hi - 16;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(sbase + j * 1024), 16, 0,
                                         0);
      }
    }
    if (cdma) {
      const uintptr_t al = (uintptr_t)(a.codes + r * F) & ~(uintptr_t)15;
      for (int i = 0; i < g.dc; ++i) {
        const int j = wid + CW * i;
        const int jj = j < g.npc ? j : g.npc - 1;
        uintptr_t src = al + (uintptr_t)jj * 1024 + (uintptr_t)lane * 16;
        src = src < a.c_lo ? a.c_lo : src;
        src = src < a.c_hi - 16 ? src : a.c_hi - 16;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src,
                                         (lds_void_t*)(sbase + g.c_off + j * 1024), 16, 0, 0);
      }
    }
    for (int i = 0; i < g.dy; ++i) {
      const int j = wid + CW * i;
      const int jj = j < g.npy ? j : g.npy - 1;
      uintptr_t src = (uintptr_t)(a.y + r) + (uintptr_t)jj * 256 + (uintptr_t)lane * 4;
      src = src < a.y_last4 ? src : a.y_last4;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)src,
                                       (lds_void_t*)(sbase + g.y_off + j * 256), 4, 0, 0);
    }
    if constexpr (OFS) {
      for (int i = 0; i < g.dofs; ++i) {
        const int j = wid + CW * i;
        const int jj = j < g.npo ? j : g.npo - 1;
        uintptr_t src = (uintptr_t)(a.eta_offset + r) + (uintptr_t)jj * 256 + (uintptr_t)lane * 4;
        src = src < a.o_last4 ? src : a.o_last4;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src,
                                         (lds_void_t*)(sbase + g.o_off + j * 256), 4, 0, 0);
      }
    }
    if constexpr (WGT) {
      for (int i = 0; i < g.dw; ++i) {
        const int j = wid + CW * i;
        const int jj = j < g.npw ? j : g.npw - 1;
        uintptr_t src = (uintptr_t)(a.row_weight + r) + (uintptr_t)jj * 256 + (uintptr_t)lane * 4;
        src = src < a.w_last4 ? src : a.w_last4;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src,
                                         (lds_void_t*)(sbase + g.w_off + j * 256), 4, 0, 0);
      }
    }
  };
  // loads per wave and block
  const int per_blk =
      (xdma ? g.dx : 0) + (cdma ? g.dc : 0) + g.dy + (OFS ? g.dofs : 0) + (WGT ? g.dw : 0);

  double llacc[BP];
#pragma unroll
  for (int b = 0; b < BP; ++b) llacc[b] = 0.0;
  int nbad = 0;

  for (int b = 0; b < nslot - 1; ++b) issue(b);
  const int keep = (nslot - 2) * per_blk;
  for (int blk = 0; blk < nb; ++blk) {
    wait_vmcnt_le<40>(keep);
    __syncthreads();
    issue(blk + nslot - 1);
    const char* slot = smem + (blk % nslot) * g.slot_bytes;
    const int64_t r = row0 + (int64_t)blk * RB;
    const bool valid = tid < RB && tid < nrows - blk * RB;
    const int rt = valid ? tid : 0;  // idle threads read row 0 of the block

    double eta[BP];
#pragma unroll
    for (int b = 0; b < BP; ++b) eta[b] = bnum[b];  // intercept (0 without one)

    if (q > 0) {
      const double* gx = a.Xn + (r + rt) * q;
      const uintptr_t g0 = (uintptr_t)gx;
      const bool xdirect = valid && !(g0 >= a.x_lo && g0 + (uintptr_t)q * 8 <= a.x_hi);
      const double* xr =
          (const double*)(slot + ((uintptr_t)(a.Xn + r * q) & 15)) + rt * q;
      for (int j = 0; j < q; ++j) {
        double v = xdirect ? gx[j] : xr[j];
        v = (v - stdv[j]) * stdv[q + 1 + j];
#pragma unroll
        for (int b = 0; b < BP; ++b) eta[b] = fma(v, bnum[(j + 1) * BP + b], eta[b]);
      }
    }
    if (F > 0) {
      const uint8_t* gc = a.codes + (r + rt) * F;
      const uintptr_t g0 = (uintptr_t)gc;
      const bool cdirect = valid && !(g0 >= a.c_lo && g0 + (uintptr_t)F <= a.c_hi);
      const uint8_t* cr =
          (const uint8_t*)(slot + g.c_off + ((uintptr_t)(a.codes + r * F) & 15)) + rt * F;
      for (int f = 0; f < F; ++f) {
        int c = cdirect ? gc[f] : cr[f];
        const bool bad = c >= s_lev[f];
        nbad += (bad && valid) ? 1 : 0;
        c = bad ? 0 : c;
        const double2* t = (const double2*)(T + (s_off[f] + c) * BP);
#pragma unroll
        for (int b2 = 0; b2 < BP / 2; ++b2) {
          const double2 tv = t[b2];
          eta[2 * b2] += tv.x;
          eta[2 * b2 + 1] += tv.y;
        }
      }
    }
    const double yv = ((const double*)(slot + g.y_off))[rt];
    double om = 1.0;  // (the literal 1 without weights)
    if constexpr (WGT) om = ((const double*)(slot + g.w_off))[rt];
    double lg = 0.0;  // lgamma(y + 1), once per row (the literal 0 for the logistic family)
    if constexpr (FAM == FAMILY_POISSON) lg = lgamma1p(yv);
    [[maybe_unused]] double ofv = 0.0;
    if constexpr (OFS) ofv = ((const double*)(slot + g.o_off))[rt];
#pragma unroll
    for (int b = 0; b < BP; ++b) {
      if (b < B) {
        double e = eta[b];
        if constexpr (OFS) e += ofv;
        if (valid) llacc[b] += row_loglik<FAM>(e, yv, om, lg);
      }
    }
  }
  wait_vmcnt<0>();
  __syncthreads();
#pragma unroll
  for (int b = 0; b < BP; ++b) {
    if (b < B) {
      double v = llacc[b];
      for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
      if (lane == 0) red[wid * kEvalCatMaxB + b] = v;
    }
  }
  for (int m = 1; m < 64; m <<= 1) nbad += __shfl_xor(nbad, m);
  if (lane == 0) s_bad[wid] = nbad;
  __syncthreads();
  if (tid < B) {
    double s = 0.0;
    for (int w = 0; w < CW; ++w) s += red[w * kEvalCatMaxB + tid];
    a.partial[(int64_t)chunk * B + tid] = s;
  }
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < CW; ++w) s += s_bad[w];
    a.bad[chunk] = s;
  }
}

constexpr int kEcStaticLds = 4 * (2 * kCatMaxFactors + CW);

template <int BP, int FAM, int RX>
static hipError_t ec_launch(const typename ec_args_of<FAM, RX>::type& a, int n_chunks, size_t lds,
                            hipStream_t s) {
  hipError_t e = ensure_max_lds((const void*)loglik_cat_kernel<BP, FAM, RX>, 160 * 1024 - 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((loglik_cat_kernel<BP, FAM, RX>), dim3(n_chunks), dim3(256), lds, s, a);
  return hipGetLastError();
}
inline int ec_bp(int B) { return B <= 2 ? 2 : B <= 4 ? 4 : B <= 8 ? 8 : 16; }
// the launch of one (family, mask): the dynamic LDS of a.rb, a.nslot (eval_cat_plan)
template <int FAM, int RX>
static hipError_t ec_launch_bp(const typename ec_args_of<FAM, RX>::type& a, int n_chunks,
                               hipStream_t s) {
  const int BP = ec_bp(a.nbeta);
  const size_t lds = (size_t)a.nslot * ec_geom(a.rb, a.q, a.F, RX).slot_bytes +
                     (size_t)ec_table_doubles(ec_entries(a), a.q, BP) * 8;
  switch (BP) {
    case 2: return ec_launch<2, FAM, RX>(a, n_chunks, lds, s);
    case 4: return ec_launch<4, FAM, RX>(a, n_chunks, lds, s);
    case 8: return ec_launch<8, FAM, RX>(a, n_chunks, lds, s);
    default: return ec_launch<16, FAM, RX>(a, n_chunks, lds, s);
  }
}

}  // namespace dlsa

