// Goodness-of-fit pass on the categorical-code layout -- the kernel template
// of gof_cat_pass.hip (logistic) and gof_cat_pass_pois.hip (Poisson).  Built
// like loglik_cat_kernel (eval_cat_pass_impl.hpp), whose geometry (ec_geom),
// plan (eval_cat_plan), LDS sizes and load accounting it uses as they are: one
// 4-wave workgroup per chunk, one row per thread, the dummy coefficients a
// table in LDS.  What differs: two sums per candidate, the row's deviance and
// Pearson chi-square (row_gof, glm_row.hpp), the chunk's count of rows with
// omega > 0, and the candidates of the chunk's partition k read at a.betas + k
// a.gof.beta_part_stride.  The log-likelihood kernels are not touched (see
// gof_pass_impl.hpp).
#pragma once

#include "eval_cat_pass_impl.hpp"

namespace dlsa {

static_assert(kGofMaxB <= kEvalCatMaxB, "the BP kernels and the plan of the log-likelihood pass");

template <int BP, int FAM, int RX>
__global__ __launch_bounds__(256) void gof_cat_kernel(const GofCatArgs a) {
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
  __shared__ int32_t s_lev[kCatMaxFactors], s_off[kCatMaxFactors], s_bad[CW];

  if (tid < kCatMaxFactors) {
    s_lev[tid] = tid < F ? a.levels[tid] : 1;
    s_off[tid] = tid < F ? a.toff[tid] : 0;
  }
  const double* betas = a.betas + a.chunk_part[chunk] * a.gof.beta_part_stride;
  for (int f = 0; f < F; ++f) {
    // entry c of factor f: 0 for the baseline, else parameter doff + c - 1,
    // doff = ic + q + (dummy columns of the factors before f) = ic + q + toff[f] - f
    const int off = a.toff[f], nl = a.levels[f], doff = ic + q + off - f;
    for (int e = tid; e < nl * BP; e += 256) {
      const int c = e / BP, b = e - c * BP;
      T[(off + c) * BP + b] = (c > 0 && b < B) ? betas[(int64_t)b * P + doff + c - 1] : 0.0;
    }
  }
  for (int e = tid; e < (q + 1) * BP; e += 256) {
    const int j = e / BP, b = e - j * BP;  // j = 0: intercept, j >= 1: numeric column j - 1
    const bool in = b < B && (j > 0 || ic);
    bnum[e] = in ? betas[(int64_t)b * P + (j > 0 ? ic + j - 1 : 0)] : 0.0;
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
    // y, the offset and omega: 256-byte pieces at byte offset `off` of the slot
    auto stream = [&](const double* v, uintptr_t last4, int npieces, int per_wave, int off) {
      for (int i = 0; i < per_wave; ++i) {
        const int j = wid + CW * i;
        const int jj = j < npieces ? j : npieces - 1;
        uintptr_t src = (uintptr_t)(v + r) + (uintptr_t)jj * 256 + (uintptr_t)lane * 4;
        src = src < last4 ? src : last4;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)(sbase + off + j * 256),
                                         4, 0, 0);
      }
    };
    stream(a.y, a.y_last4, g.npy, g.dy, g.y_off);
    if constexpr (OFS) stream(a.eta_offset, a.o_last4, g.npo, g.dofs, g.o_off);
    if constexpr (WGT) stream(a.row_weight, a.w_last4, g.npw, g.dw, g.w_off);
  };
  // loads per wave and block
  const int per_blk =
      (xdma ? g.dx : 0) + (cdma ? g.dc : 0) + g.dy + (OFS ? g.dofs : 0) + (WGT ? g.dw : 0);

  double dvacc[BP], chacc[BP], npos = 0.0;
#pragma unroll
  for (int b = 0; b < BP; ++b) dvacc[b] = chacc[b] = 0.0;
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
    const double rc = row_gof_const<FAM>(yv);  // what of the deviance depends on y alone
    npos += valid && om > 0.0 ? 1.0 : 0.0;
    [[maybe_unused]] double ofv = 0.0;
    if constexpr (OFS) ofv = ((const double*)(slot + g.o_off))[rt];
#pragma unroll
    for (int b = 0; b < BP; ++b) {
      if (b < B) {
        double e = eta[b];
        if constexpr (OFS) e += ofv;
        const RowGof t = row_gof<FAM>(e, yv, om, rc);
        if (valid) {
          dvacc[b] += t.dev;
          chacc[b] += t.chi;
        }
      }
    }
  }
  wait_vmcnt<0>();
  __syncthreads();
  // [CW][2 BP + 1] wave sums, in the ring, which nothing reads any more (two
  // slots are at least 2 KiB)
  constexpr int NR = 2 * BP + 1;
  double* red = (double*)smem;
#pragma unroll
  for (int b = 0; b < BP; ++b) {
    if (b < B) {
      double dv = dvacc[b], cv = chacc[b];
      for (int m = 1; m < 64; m <<= 1) {
        dv += __shfl_xor(dv, m);
        cv += __shfl_xor(cv, m);
      }
      if (lane == 0) {
        red[wid * NR + b] = dv;
        red[wid * NR + BP + b] = cv;
      }
    }
  }
  for (int m = 1; m < 64; m <<= 1) {
    npos += __shfl_xor(npos, m);
    nbad += __shfl_xor(nbad, m);
  }
  if (lane == 0) {
    red[wid * NR + 2 * BP] = npos;
    s_bad[wid] = nbad;
  }
  __syncthreads();
  if (tid < NR && (tid == 2 * BP || tid % BP < B)) {
    double s = 0.0;
    for (int w = 0; w < CW; ++w) s += red[w * NR + tid];
    if (tid == 2 * BP)
      a.gof.partial_npos[chunk] = s;
    else
      (tid < BP ? a.partial : a.gof.partial_chi)[(int64_t)chunk * B + tid % BP] = s;
  }
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < CW; ++w) s += s_bad[w];
    a.bad[chunk] = s;
  }
}

template <int BP, int FAM, int RX>
static hipError_t gc_launch(const GofCatArgs& a, int n_chunks, size_t lds, hipStream_t s) {
  hipError_t e = ensure_max_lds((const void*)gof_cat_kernel<BP, FAM, RX>, 160 * 1024 - 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((gof_cat_kernel<BP, FAM, RX>), dim3(n_chunks), dim3(256), lds, s, a);
  return hipGetLastError();
}
// the launch of one (family, mask): the dynamic LDS of a.rb, a.nslot (eval_cat_plan)
template <int FAM, int RX>
static hipError_t gc_launch_bp(const GofCatArgs& a, int n_chunks, hipStream_t s) {
  const int BP = ec_bp(a.nbeta);
  const size_t lds = (size_t)a.nslot * ec_geom(a.rb, a.q, a.F, RX).slot_bytes +
                     (size_t)ec_table_doubles(ec_entries(a), a.q, BP) * 8;
  switch (BP) {
    case 2: return gc_launch<2, FAM, RX>(a, n_chunks, lds, s);
    case 4: return gc_launch<4, FAM, RX>(a, n_chunks, lds, s);
    case 8: return gc_launch<8, FAM, RX>(a, n_chunks, lds, s);
    default: return gc_launch<16, FAM, RX>(a, n_chunks, lds, s);
  }
}

}  // namespace dlsa
