// Exact phase of the wide path (wide_common.hpp): the fp64 row pass, the fp64
// Gram pass and the assembly of the padded Hessian from the row-group
// partials (of either Gram pass: the fused bf16 one is wide_fused.hip).
#include <math.h>
#include <stdlib.h>

#include "glm_row.hpp"
#include "wide_common.hpp"

namespace dlsa {

// ---------------------------------------------------------------------------
// row pass: one 256-thread workgroup per row chunk; wave w takes rows
// 4w .. 4w+3 of every 16-row group; lane l holds features f = l + 64 m.
// ---------------------------------------------------------------------------
template <int MB, bool STD, int FAM>
__global__ __launch_bounds__(256) void wide_row_kernel(const WideArgs a) {
  const int chunk = blockIdx.x;
  const int part = a.rc_part[chunk];
  if (a.phase[part] != PHASE_F64) return;  // workgroup-uniform (PHASE_F32: fused pass)
  __shared__ double red[4 * 64 * MB + 4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int p = a.p, P = a.P, ic = a.intercept;
  const int64_t row0 = a.rc_row0[chunk];
  const int nrows = a.rc_rows[chunk];

  double beta[MB], gacc[MB], cen[MB], isc[MB];
  int col[MB];
  bool inb[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int f = lane + 64 * m;
    beta[m] = f < P ? a.theta[(int64_t)part * P + f] : 0.0;
    gacc[m] = 0.0;
    const int j = f - ic;
    inb[m] = j >= 0 && j < p;
    col[m] = inb[m] ? j : 0;
    cen[m] = 0.0;
    isc[m] = 1.0;
    if constexpr (STD) {
      if (inb[m]) {
        cen[m] = a.center[j];
        isc[m] = 1.0 / a.scale[j];
      }
    }
  }
  const bool icpt_lane = ic && lane == 0;
  double llacc = 0.0;
  // int8 exact Gram: running max of |sqrt(w) x| high dwords per feature
  const bool zm_on = a.slab_zmax != nullptr;
  uint32_t zmx[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) zmx[m] = 0u;
  constexpr int U = 4;  // rows per wave per step (all U rows' loads in flight)
  for (int base = wid * U; base < nrows; base += 4 * U) {
    double xv[U][MB], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = min(base + u, nrows - 1);
      const double* xr = a.X + (row0 + r) * (int64_t)p;
#pragma unroll
      for (int m = 0; m < MB; ++m) xv[u][m] = xr[col[m]];
      yv[u] = a.y[row0 + r];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool valid = base + u < nrows;
      double e = 0.0;
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        double v = inb[m] ? xv[u][m] : 0.0;
        if constexpr (STD) v = inb[m] ? (v - cen[m]) * isc[m] : 0.0;
        if (m == 0 && icpt_lane) v = 1.0;
        xv[u][m] = v;
        e = fma(v, beta[m], e);
      }
      e = bcast_first(wave_sum64(e));  // one value for the whole wave
      double w, r;
      if constexpr (FAM == FAMILY_LOGISTIC) {
        const LogisticLink k = logistic_link<RCP_DIV>(e);
        w = k.w;
        r = yv[u] - k.mu;
        if (valid && lane == 0) llacc += yv[u] * e - (fmax(e, 0.0) + log1p(k.ea));
      } else {  // gaussian (OLS): w = 1, ll = -rss/2
        w = 1.0;
        r = yv[u] - e;
        if (valid && lane == 0) llacc -= 0.5 * r * r;
      }
      if (!valid) r = 0.0;
#pragma unroll
      for (int m = 0; m < MB; ++m) gacc[m] = fma(xv[u][m], r, gacc[m]);
      if (zm_on) {
        const double sw = valid ? sqrt(w) : 0.0;
#pragma unroll
        for (int m = 0; m < MB; ++m)
          zmx[m] = max(zmx[m], (uint32_t)__double2hiint(xv[u][m] * sw) & 0x7FFFFFFFu);
      }
      if (valid && lane == 0) a.w[row0 + base + u] = w;
    }
  }
#pragma unroll
  for (int m = 0; m < MB; ++m) red[wid * 64 * MB + lane + 64 * m] = gacc[m];
  llacc = wave_sum64(llacc);
  if (lane == 0) red[4 * 64 * MB + wid] = llacc;
  __syncthreads();
  constexpr int PP = 64 * MB;
  for (int f = tid; f < PP; f += 256)
    a.slab_g[(int64_t)chunk * PP + f] =
        ((red[f] + red[PP + f]) + red[2 * PP + f]) + red[3 * PP + f];
  if (tid == 0)
    a.slab_ll[chunk] = ((red[4 * PP] + red[4 * PP + 1]) + red[4 * PP + 2]) + red[4 * PP + 3];
  if (zm_on) {
    __shared__ uint32_t zred[4 * 64 * MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) zred[wid * 64 * MB + lane + 64 * m] = zmx[m];
    __syncthreads();
    for (int f = tid; f < PP; f += 256)
      a.slab_zmax[(int64_t)chunk * PP + f] =
          max(max(zred[f], zred[PP + f]), max(zred[2 * PP + f], zred[3 * PP + f]));
  }
}

// ---------------------------------------------------------------------------
// exact Gram pass: 256 threads = 4 waves per 128x128 output tile (I, J),
// I >= J; wave (qi = w >> 1, qj = w & 1) owns the 64 x 64 quadrant rows
// 64 qi .., columns 64 qj .. (the strictly-upper quadrant of a diagonal tile
// is skipped): 4 x 4 accumulators of v_mfma_f64_16x16x4_f64 (128 AGPRs), 16
// MFMAs per k-step of 4 rows against 8 operand loads + w -- fp64 VALU work
// and fp64 MFMAs do not overlap on a SIMD, so the VALU per MFMA is what the
// wave tile has to minimise.  Operands come straight from X by raw buffer
// loads: lane l reads row (l >> 4) of the k-step at feature (l & 15) of each
// 16-wide sub-tile, per-lane offsets fixed, the k-step advancing the uniform
// soffset (no address VALU); rows past the row group and columns >= p read 0
// through the buffer range check.  Four k-steps of operands in flight.
// ---------------------------------------------------------------------------
template <bool STD>
__global__ __launch_bounds__(256, 2) void wide_gram_kernel(const WideArgs a) {
  const int NB = a.NB;
  const int TB = NB * (NB + 1) / 2;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, j8 = bid >> 3;  // workgroups are dealt to XCDs round-robin
  const int cl = j8 / TB, t = j8 - cl * TB;
  const int chunk = cl * 8 + xcd;  // all TB tiles of a row group on one XCD
  if (chunk >= a.n_gchunks) return;
  const int part = a.gc_part[chunk];
  if (a.phase[part] != PHASE_F64) return;
  int I, J;
  tile_ij(t, I, J);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = wid >> 1, qj = wid & 1;
  if (I == J && qi == 0 && qj == 1) return;  // strictly-upper quadrant of a diagonal tile
  const int p = a.p, ic = a.intercept;
  const int64_t row0 = a.gc_row0[chunk];
  const int nrows = __builtin_amdgcn_readfirstlane(a.gc_rows[chunk]);
  const int fl = lane & 15, kq = lane >> 4;

  // per-lane operand offsets (row kq of a k-step), 0x80000000 = column >= p
  int offA[4], offB[4];
  bool oneA = false, oneB = false;
  double cA[4], sA[4], cB[4], sB[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int fa = GT * I + 64 * qi + 16 * s + fl, ja = fa - ic;
    const int fb = GT * J + 64 * qj + 16 * s + fl, jb = fb - ic;
    offA[s] = (ja >= 0 && ja < p) ? (kq * p + ja) * 8 : (int)0x80000000;
    offB[s] = (jb >= 0 && jb < p) ? (kq * p + jb) * 8 : (int)0x80000000;
    if (s == 0) {
      oneA = ic && fa == 0;
      oneB = ic && fb == 0;
    }
    cA[s] = cB[s] = 0.0;
    sA[s] = sB[s] = 1.0;
    if constexpr (STD) {
      if (ja >= 0 && ja < p) {
        sA[s] = 1.0 / a.scale[ja];
        cA[s] = a.center[ja] * sA[s];
      }
      if (jb >= 0 && jb < p) {
        sB[s] = 1.0 / a.scale[jb];
        cB[s] = a.center[jb] * sB[s];
      }
    }
  }
  const __amdgpu_buffer_rsrc_t xr =
      uniform_rsrc((uintptr_t)(a.X + row0 * p), (uintptr_t)nrows * (uintptr_t)p * 8u);
  const __amdgpu_buffer_rsrc_t wr = uniform_rsrc((uintptr_t)(a.w + row0), (uintptr_t)nrows * 8u);

  d4w acc[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[s][u] = d4w{0, 0, 0, 0};

  struct Frag {
    double xa[4], xb[4], w;
  };
  auto load = [&](int step, Frag& F) {
    const int so = step * 4 * p * 8;  // k-step rows 4 step .. 4 step + 3
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      F.xa[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, offA[s], so, 0));
      F.xb[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, offB[s], so, 0));
    }
    F.w = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(wr, kq * 8, step * 32, 0));
  };
  auto compute = [&](const Frag& F) {
    double av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double x = F.xa[s], z = F.xb[s];
      if constexpr (STD) {
        x = fma(x, sA[s], -cA[s]);
        z = fma(z, sB[s], -cB[s]);
      }
      if (s == 0) {
        if (oneA) x = 1.0;
        if (oneB) z = 1.0;
      }
      av[s] = x * F.w;  // rows past the group: w = 0
      bv[s] = z;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        acc[s][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[u], acc[s][u], 0, 0, 0);
  };
  const int nsteps = (nrows + 3) / 4;
  constexpr int DEPTH = 4;  // k-steps of operands in flight
  if (nsteps > 0) {
    Frag f[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load(d, f[d]);  // past the end: range-checked zeros
    for (int s0 = 0; s0 < nsteps; s0 += DEPTH) {  // a ragged last group adds zeros
#pragma unroll
      for (int d = 0; d < DEPTH; ++d) {
        compute(f[d]);
        load(s0 + DEPTH + d, f[d]);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 4; ++u) asm volatile("" : "+a"(acc[s][u]));
    }
  }

  // C/D map of the f64 16x16x4 MFMA: row = (l >> 4) + 4 r, column = l & 15
  double* G = a.slab_G + ((int64_t)chunk * TB + t) * (GT * GT);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 64 * qi + 16 * s + kq + 4 * r;
        const int jc = 64 * qj + 16 * u + fl;
        G[i * GT + jc] = acc[s][u][r];
      }
}

// ---------------------------------------------------------------------------
// assemble: H[k] (PP x PP, both triangles, padding = identity) = sum of the
// row-group partials of partition k in row-group order.  grid (TB * 16, K):
// one workgroup per 32 x 32 block of a lower 128 x 128 tile (blocks above the
// diagonal of a diagonal tile exit); a thread sums 4 elements, all their
// row-group partials loaded before the adds (8 at a time), and the block is
// written row-major and, through LDS, transposed -- both coalesced.  (One
// workgroup per tile with one element's partials summed at a time, 320
// workgroups at config 5: 0.27 ms per launch.)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wide_assemble_kernel(const WideArgs a, const int32_t* gcb,
                                                            double* Hfull) {
  const int t = blockIdx.x >> 4, sb = blockIdx.x & 15, k = blockIdx.y;
  if (a.phase[k] != PHASE_F32 && a.phase[k] != PHASE_F64) return;
  const int NB = a.NB, TB = NB * (NB + 1) / 2, PP = GT * NB, P = a.P;
  int I, J;
  tile_ij(t, I, J);
  const int br = sb >> 2, bc = sb & 3;  // 32 x 32 block (br, bc) of the tile
  if (I == J && bc > br) return;
  __shared__ double tr[32][33];
  const int cb = gcb[k], ce = gcb[k + 1];
  double* H = Hfull + (int64_t)k * PP * PP;
  const int tc = threadIdx.x & 31, tr0 = threadIdx.x >> 5;
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = 0.0;
  const double* base = a.slab_G + (int64_t)t * (GT * GT) + (32 * br + tr0) * GT + 32 * bc + tc;
  const int64_t cstride = (int64_t)TB * (GT * GT);
  int c = cb;
  for (; c + 8 <= ce; c += 8) {
    double x[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) x[u][q] = base[(int64_t)(c + u) * cstride + 8 * q * GT];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += x[u][q];
  }
  for (; c < ce; ++c)
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += base[(int64_t)c * cstride + 8 * q * GT];
  const bool diag = I == J && br == bc;  // a block on the matrix diagonal
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int il = 32 * br + tr0 + 8 * q, jl = 32 * bc + tc;
    const int i = GT * I + il, j = GT * J + jl;
    double s = v[q];
    if (i >= P || j >= P) s = (i == j) ? 1.0 : 0.0;
    tr[tr0 + 8 * q][tc] = s;
  }
  __syncthreads();
  // row-major block (rows 32 br .., columns 32 bc ..); on the diagonal the
  // upper triangle mirrors the lower
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = tr0 + 8 * q;
    const int i = GT * I + 32 * br + r, j = GT * J + 32 * bc + tc;
    H[(int64_t)i * PP + j] = (diag && tc > r) ? tr[tc][r] : tr[r][tc];
  }
  if (diag) return;
  // transposed block: H[j][i]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = tr0 + 8 * q;  // row of the transposed block = column of tr
    const int j = GT * J + 32 * bc + r, i = GT * I + 32 * br + tc;
    H[(int64_t)j * PP + i] = tr[tc][r];
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <int MB, bool STD>
static hipError_t launch_row_t(const WideArgs& a, int family, int n_chunks, hipStream_t s) {
  if (!family_rules(family).iterates)  // the closed form: w = 1
    hipLaunchKernelGGL((wide_row_kernel<MB, STD, FAMILY_GAUSSIAN>), dim3(n_chunks), dim3(256), 0,
                       s, a);
  else
    hipLaunchKernelGGL((wide_row_kernel<MB, STD, FAMILY_LOGISTIC>), dim3(n_chunks), dim3(256), 0,
                       s, a);
  return hipGetLastError();
}

hipError_t launch_wide_row(const WideArgs& a, bool standardize, int family, int n_chunks,
                           hipStream_t s) {
  if (n_chunks <= 0) return hipSuccess;
  switch (2 * a.NB) {  // MB = PP / 64
    case 4: return standardize ? launch_row_t<4, true>(a, family, n_chunks, s)
                               : launch_row_t<4, false>(a, family, n_chunks, s);
    case 6: return standardize ? launch_row_t<6, true>(a, family, n_chunks, s)
                               : launch_row_t<6, false>(a, family, n_chunks, s);
    case 8: return standardize ? launch_row_t<8, true>(a, family, n_chunks, s)
                               : launch_row_t<8, false>(a, family, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

// exact (fp64) Gram pass of the PHASE_F64 partitions
hipError_t launch_wide_gram(const WideArgs& a, bool standardize, hipStream_t s) {
  if (a.n_gchunks <= 0) return hipSuccess;
  const int TB = a.NB * (a.NB + 1) / 2;
  const int grid = ((a.n_gchunks + 7) / 8) * 8 * TB;
  if (standardize)
    hipLaunchKernelGGL(wide_gram_kernel<true>, dim3(grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(wide_gram_kernel<false>, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wide_assemble(const WideArgs& a, const int32_t* gcb, double* Hfull, int K,
                                hipStream_t s) {
  const int TB = a.NB * (a.NB + 1) / 2;
  hipLaunchKernelGGL(wide_assemble_kernel, dim3(TB * 16, K), dim3(256), 0, s, a, gcb, Hfull);
  return hipGetLastError();
}

}  // namespace dlsa
