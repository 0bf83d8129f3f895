// Approximate phase of the wide path (wide_common.hpp): one stream of X per
// Newton iteration.
#include <math.h>
#include <stdlib.h>

#include "glm_row.hpp"
#include "wide_common.hpp"

namespace dlsa {

// ---------------------------------------------------------------------------
// fused approximate pass (MIXED mode, logistic, PHASE_F32 partitions): ONE
// stream of X per Newton iteration yields both the row quantities (eta, w, r,
// the fp64 gradient X^T (y - mu) and log-likelihood) and the approximate
// Hessian  H~ = Z^T Z,  Z = bf16(sqrt(w) x)  (positive semi-definite by
// construction; DESIGN.md 4.2: it only steers Newton, the fp64 pass fixes the
// solution and publishes Sig_inv).
//
// Register budget first: the fp32 accumulators of the P x P lower triangle
// (528 16x16 tiles = 528 KB at PP = 512) exceed a CU's register file, so
// S = 2 workgroups share a row group above PP = 256, each owning half of the
// tile rows; they are dispatched back to back onto one XCD, so the second
// stream of the rows is an L2 / MALL hit.  A workgroup is 4 waves, ONE per
// SIMD, so each wave has the full 512 registers: ~256 accumulator registers
// (AGPRs) + a 32-row block of X in flight (128 VGPRs) + the row work.
//
// Per 32-row block (wave w holds rows 8w .. 8w+7 in registers; raw buffer
// loads, 16 B per lane at even p: lane l owns columns 2l + 128 j (+1); rows or
// columns past the end read as 0 through the buffer range check):
//   1. eta of the 8 rows: lane partials, then a reduce-scatter over the lanes
//      (permlane32 / permlane16 swaps, one DPP swap, DPP within 8 lanes) --
//      lane group l >> 3 ends with row l >> 3, bitwise-identical in the group;
//   2. w, r, log-lik: ONE fp64 exp / reciprocal sequence for the 8 rows,
//      broadcast by readlane; the softplus sum is a running product
//      (frexp-normalised), one log per lane at the end;
//   3. per half of 4 rows: gradient FMAs (group 0 only), the half's Z plane
//      (see zplane_bytes), and the loads of the same half of block b+1 into
//      the freed registers -- in flight across the other half, the barrier
//      and the MFMA phase;
//   4. one LDS barrier (no vmcnt drain) and the MFMA phase:
//      v_mfma_f32_16x16x32_bf16, operand lane (i, kg) = feature i, rows
//      8 kg .. 8 kg + 7.
// Wave slot s = 4 sg + w owns the tile-row pairs q = s + 4 S k: rows q and
// NT16 - 1 - q, NT16 + 1 tiles per pair (2 pairs = 66 tiles at PP = 512).
// Double-buffered Z images: one barrier per block.  Output: the
// 128 x 128-tile slab layout of wide_gram_kernel (slab_G) and per-row-group
// gradient / log-lik partials (slab_gz / slab_llz) summed in fixed order --
// deterministic.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4w __attribute__((ext_vector_type(4)));
typedef float f4w __attribute__((ext_vector_type(4)));
typedef double d2w __attribute__((ext_vector_type(2)));

#ifndef DLSA_FUSED_ABLATE
#define DLSA_FUSED_ABLATE 0
#endif

namespace {
constexpr int FW = 4;   // waves per workgroup of the fused pass
// Z image of a 32-row block: 8 planes (wave w, half h = rows 8w + 4h .. +3),
// each [PP features][4 rows] bf16 (8 B per feature) + 64 B pad.  A half's
// store (one ds_write_b64 per lane and column, features 2 apart across the
// lanes) is 2-way conflicted; an MFMA operand (feature i, rows 8 kg .. +7) is
// two ds_read_b64 from planes 2 kg and 2 kg + 1, conflict-free: the plane
// pad moves kg = 1 (lanes 16-31) onto the other 32 banks of lanes 0-15.
__host__ __device__ constexpr int zplane_bytes(int NT16) { return 16 * NT16 * 8 + 64; }
__host__ __device__ constexpr int zimg_bytes(int NT16) { return 8 * zplane_bytes(NT16); }
__host__ __device__ constexpr int fused_groups(int NT16) { return NT16 > 16 ? 2 : 1; }
__host__ __device__ constexpr int fused_pairs_per_slot(int NT16) {
  return (NT16 / 2 + FW * fused_groups(NT16) - 1) / (FW * fused_groups(NT16));
}
// [2] Z images, [PP] scaled beta, [2][PP] 1/scale and center/scale,
// [FW][PP] gradient reduction, [32] misc
__host__ __device__ constexpr int fused_lds_bytes(int NT16) {
  return 2 * zimg_bytes(NT16) + (3 + FW) * 16 * NT16 * 8 + 256;
}

// Sum over the 64 lanes; every lane ends with the bitwise-identical total
// (each step adds a value and its partner's under a lane involution, so the
// pair computes a + b and b + a).
__device__ __forceinline__ double wave_allsum(double v) {
  v += dpp_f64<0x141>(v);  // row_half_mirror: i <-> 7 - i
  v += dpp_f64<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_f64<0x140>(v);  // row_mirror: i <-> 15 - i
  v = wv_xor16(v);
  v = wv_xor32(v);
  return v;
}

// v_permlane32_swap / v_permlane16_swap of a double pair (a, b): after the
// swap, lanes of the lower half of each 2H-lane group see (a, a of lane + H),
// lanes of the upper half (b of lane - H, b)
template <int H>
__device__ __forceinline__ double swap_add(double a, double b) {
  const unsigned alo = __double2loint(a), ahi = __double2hiint(a);
  const unsigned blo = __double2loint(b), bhi = __double2hiint(b);
  if constexpr (H == 32) {
    const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
  } else {
    const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
  }
}

// 4 row partials per lane -> lane l holds the total of row l >> 4 (every lane
// of the 16-lane group bitwise-identical)
__device__ __forceinline__ double reduce_scatter4(const double (&v)[4], int lane) {
  (void)lane;
  // lanes 0-31 rows 0, 1; lanes 32-63 rows 2, 3
  const double s0 = swap_add<32>(v[0], v[2]), s1 = swap_add<32>(v[1], v[3]);
  // 16-lane groups: rows 0, 1, 2, 3
  double r = swap_add<16>(s0, s1);
  r += dpp_f64<0x141>(r);  // row_half_mirror: i <-> 7 - i
  r += dpp_f64<0xB1>(r);   // quad_perm [1, 0, 3, 2]
  r += dpp_f64<0x4E>(r);   // quad_perm [2, 3, 0, 1]
  r += dpp_f64<0x140>(r);  // row_mirror: i <-> 15 - i
  return r;
}

// 8 row partials per lane -> lane l holds the total of row l >> 3 (every lane
// of the 8-lane group bitwise-identical)
__device__ __forceinline__ double reduce_scatter8(const double (&v)[8], int lane) {
  // lanes 0-31 rows 0..3, lanes 32-63 rows 4..7
  const double s0 = swap_add<32>(v[0], v[4]), s1 = swap_add<32>(v[1], v[5]);
  const double s2 = swap_add<32>(v[2], v[6]), s3 = swap_add<32>(v[3], v[7]);
  // 16-lane groups: t0 rows 0, 2, 4, 6; t1 rows 1, 3, 5, 7
  const double t0 = swap_add<16>(s0, s2), t1 = swap_add<16>(s1, s3);
  // 8-lane groups: lanes with bit 3 clear keep t0's row, set keep t1's
  const bool b3 = (lane & 8) != 0;
  const double keep = b3 ? t1 : t0, give = b3 ? t0 : t1;
  double r = keep + dpp_f64<0x128>(give);  // row_ror 8: lane l ^ 8 within 16
  r += dpp_f64<0x141>(r);                  // row_half_mirror: i <-> 7 - i
  r += dpp_f64<0xB1>(r);                   // quad_perm [1, 0, 3, 2]
  r += dpp_f64<0x4E>(r);                   // quad_perm [2, 3, 0, 1]
  return r;
}

__device__ __forceinline__ double rdlane_f64(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

typedef float f2w __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2w __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {  // v_cvt_pk_bf16_f32
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f2w{a, b}, bf16x2w));
}
}  // namespace

template <bool STD, int NT16, bool VEC2>
__global__ __launch_bounds__(64 * FW, 1) void wide_fused_bf16_kernel(const WideArgs a) {
  constexpr int S = fused_groups(NT16);
  constexpr int PP = 16 * NT16;
  constexpr int NF = PP / 64;     // columns per lane of each row
  constexpr int HALF = NT16 / 2;  // tile-row pairs
  constexpr int PPS = fused_pairs_per_slot(NT16);
  constexpr int TPP = NT16 + 1;   // tiles per pair
  constexpr int NT = 64 * FW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ZPL = zplane_bytes(NT16), ZIMG = zimg_bytes(NT16);
  char* zimg = smem;                            // [2] Z images
  double* bl = (double*)(smem + 2 * ZIMG);      // [PP] beta (x 1/scale) by column
  double* sd = bl + PP;                         // [2][PP] 1/scale, center/scale (STD)
  double* red = sd + 2 * PP;                    // [FW][PP] gradient of each wave
  double* misc = red + FW * PP;                 // [0] eta offset, [8..] log-lik, [16..] sum r

  const int bid = blockIdx.x;
  const int xcd = bid & 7, j8 = bid >> 3;
  const int sg = j8 % S, cl = j8 / S;
  const int chunk = cl * 8 + xcd;  // the S workgroups of a row group on one XCD
  if (chunk >= a.n_gchunks) return;
  const int part = __builtin_amdgcn_readfirstlane(a.gc_part[chunk]);
  if (a.phase[part] != PHASE_F32) return;  // workgroup-uniform
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, P = a.P, ic = a.intercept;
  const int64_t row0 = a.gc_row0[chunk];
  const int nrows = __builtin_amdgcn_readfirstlane(a.gc_rows[chunk]);
  const int nb = (nrows + 31) / 32;
  const double* th = a.theta + (int64_t)part * P;

  // ---- setup: zero Z images (padding features stay 0), beta, eta offset ----
  for (int o = tid * 16; o < 2 * ZIMG; o += NT * 16) *(uint4*)(zimg + o) = make_uint4(0, 0, 0, 0);
  for (int c = tid; c < PP; c += NT) {
    double is = 1.0, cs = 0.0;
    if constexpr (STD) {
      if (c < p) {
        is = 1.0 / a.scale[c];
        cs = a.center[c] * is;
      }
    }
    bl[c] = c < p ? th[c + ic] * is : 0.0;
    sd[c] = is;
    sd[PP + c] = cs;
  }
  if (wid == 0) {  // eta offset: intercept - sum_c beta_c center_c / scale_c
    double s = 0.0;
    if constexpr (STD)
      for (int c = lane; c < p; c += 64) s += th[c + ic] * (a.center[c] / a.scale[c]);
    s = wave_allsum(s);
    if (lane == 0) misc[0] = (ic ? th[0] : 0.0) - s;
  }
  __syncthreads();
  const double eoff = bcast_first(misc[0]);

  auto colf = [&](int m) { return VEC2 ? 2 * lane + 128 * (m >> 1) + (m & 1) : lane + 64 * m; };
  const int rl = lane >> 3;  // the row of the wave this lane's transcendental work is for

  // per-lane byte offset of each column group in the wave's first row (out of
  // range columns: an offset past any buffer -> reads 0); row u adds u p 8
  // through the uniform soffset
  constexpr int NV = VEC2 ? NF / 2 : NF;
  int voff[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = colf(VEC2 ? 2 * v : v);
    voff[v] = c < p ? (8 * wid * p + c) * 8 : 0x7FFFFFF0;
  }
  double xv[8][NF];
  double yv = 0.0;
  // rows 4 h .. 4 h + 3 of this wave in block b (with h = 0: y of row rl).
  // Block nb (one past the last) is issued too, with an empty buffer range
  // (all loads return 0, no memory access): every loop iteration then has
  // the same loads in flight, so the compiler's vmcnt bookkeeping never
  // merges an "issued" and a "not issued" path into a full drain.
  auto issue = [&](int b, int h) {
#if DLSA_FUSED_ABLATE == 1  // profiling only: every block re-reads block 0 (L2-resident)
    const int64_t rb = row0 + 32LL * min(b, nb > 0 ? 0 : b);
#else
    const int64_t rb = row0 + 32LL * b;
#endif
    const int rows = max(0, min(32, nrows - 32 * b));
    const __amdgpu_buffer_rsrc_t xr =
        uniform_rsrc((uintptr_t)(a.X + rb * p), (uintptr_t)rows * (uintptr_t)p * 8u);
    const __amdgpu_buffer_rsrc_t yr = uniform_rsrc((uintptr_t)(a.y + rb), (uintptr_t)rows * 8u);
#pragma unroll
    for (int u = 4 * h; u < 4 * h + 4; ++u) {
      const int so = u * p * 8;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if constexpr (VEC2) {
          const d2w d =
              __builtin_bit_cast(d2w, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[v], so, 0));
          xv[u][2 * v] = d.x;
          xv[u][2 * v + 1] = d.y;
        } else {
          xv[u][v] =
              __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(xr, voff[v], so, 0));
        }
      }
    }
    if (h == 0)
      yv = __builtin_bit_cast(double,
                              __builtin_amdgcn_raw_buffer_load_b64(yr, (8 * wid + rl) * 8, 0, 0));
  };

  double gacc[NF];
#pragma unroll
  for (int m = 0; m < NF; ++m) gacc[m] = 0.0;
  // log-lik: sum of y eta - max(eta, 0) on the first lane of each row group,
  // and the softplus term as a running product of t = 1 + exp(-|eta|) in
  // [1, 2] kept as mantissa x 2^lexp (frexp each block: exact) -- one log per
  // lane at the end instead of one per row, and no more rounding than a sum
  // of per-row logs
  double rsum = 0.0, llacc = 0.0, lprod = 1.0;
  int lexp = 0;
  f4w acc[PPS][TPP];
#pragma unroll
  for (int k = 0; k < PPS; ++k)
#pragma unroll
    for (int i = 0; i < TPP; ++i) acc[k][i] = f4w{0.f, 0.f, 0.f, 0.f};
  const int slot = sg * FW + wid;
  const int fl = lane & 15, kg = lane >> 4;

  if (nb > 0) {
    issue(0, 0);
    issue(0, 1);
  }
  for (int b = 0; b < nb; ++b) {
    // ---- row phase: eta, w, r, log-lik of the wave's 8 rows (one
    // transcendental sequence), then per half of 4 rows the gradient, the Z
    // entries and the loads of that half of block b+1: those stay in flight
    // across the other half, the barrier and the MFMA phase ----------------
    double e8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      double e0 = 0.0, e1 = 0.0;
#pragma unroll
      for (int m = 0; m < NF; ++m) {
        const double bm = bl[colf(m)];
        if (m & 1)
          e1 = fma(xv[u][m], bm, e1);
        else
          e0 = fma(xv[u][m], bm, e0);
      }
      e8[u] = e0 + e1;
    }
    const double eu = reduce_scatter8(e8, lane) + eoff;  // row rl of the wave
    const bool vrow = 32 * b + 8 * wid + rl < nrows;
    const LogisticLink k = logistic_link<RCP_NEWTON>(eu);
    const double ea = k.ea, w = k.w;
    const double r = vrow ? yv - k.mu : 0.0;
    if (sg == 0 && (lane & 7) == 0 && vrow) {
      llacc += yv * eu - fmax(eu, 0.0);
      lprod *= 1.0 + ea;
    }
    {
      int e2;
      lprod = frexp(lprod, &e2);
      lexp += e2;
    }
    const float swl = vrow ? sqrtf((float)w) : 0.f;
    char* zb = zimg + (b & 1) * ZIMG;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float sw[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        sw[u] = __builtin_bit_cast(
            float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, swl), 8 * (4 * h + u)));
      if (sg == 0) {  // workgroup-uniform: group 0 accumulates the gradient
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double ru = rdlane_f64(r, 8 * (4 * h + u));
          rsum += ru;
#pragma unroll
          for (int m = 0; m < NF; ++m) gacc[m] = fma(xv[4 * h + u][m], ru, gacc[m]);
        }
      }
      // Z entries: plane (wid, h), this half's 4 rows of each of the lane's columns
      char* zp = zb + (2 * wid + h) * ZPL;
#pragma unroll
      for (int m = 0; m < NF; ++m) {
        const int c = colf(m);
        float zf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          double v = xv[4 * h + u][m];
          if constexpr (STD) v = fma(v, sd[c], -sd[PP + c]);
          float f = (float)v;
          asm volatile("" : "+v"(f));  // keep f64 -> f32 -> bf16 (see irls_coop_impl.hpp)
          zf[u] = f * sw[u];
        }
        // columns c >= p read as 0 and write 0 into padding features; only the
        // last column can map past the plane (c + ic = PP)
        if (m < NF - 1 || c + ic < PP)
          *(uint2*)(zp + (c + ic) * 8) = make_uint2(pack_bf16x2(zf[0], zf[1]), pack_bf16x2(zf[2], zf[3]));
      }
      if (ic && lane == 0)  // intercept column: z = sqrt(w)
        *(uint2*)zp = make_uint2(pack_bf16x2(sw[0], sw[1]), pack_bf16x2(sw[2], sw[3]));
      issue(b + 1, h);
    }
    // this wave's Z writes done; every wave's image b complete and image b-1 consumed
    lds_barrier();

    // ---- MFMA phase: per pair q, tile rows NT16 - 1 - q (J < nh) and q ------
    // operand (feature 16 J + fl, rows 8 kg .. 8 kg + 7): planes 2 kg, 2 kg + 1
    const char* base = zimg + (b & 1) * ZIMG + 2 * kg * ZPL + fl * 8;
    auto op = [&](int J) {
      const bf16x4w lo = *(const bf16x4w*)(base + 16 * J * 8);
      const bf16x4w hi = *(const bf16x4w*)(base + ZPL + 16 * J * 8);
      return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    // Tile i of pair q: the upper row NT16 - 1 - q holds i < nh = NT16 - q
    // (J = i), the lower row q the rest, stored from the end (J = NT16 - i).
    // Over the slots that share pair index k, q spans [qlo, qhi], so tiles
    // i < NT16 - qhi are upper-row and i >= NT16 - qlo lower-row for every
    // slot -- compile-time operands; only the 7 tiles in between pick their
    // row at run time (uniform LDS offsets, no register selects).
    constexpr int D = 2;  // B operands read D tiles ahead of their MFMA
#pragma unroll
    for (int k = 0; k < PPS; ++k) {
      const int q = slot + FW * S * k;
      if (q < HALF) {  // wave-uniform
        const int nh = NT16 - q;
        const int qlo = FW * S * k, qhi = min(HALF - 1, FW * S * k + FW * S - 1);
        const int st_hi = NT16 - qhi, st_lo = NT16 - qlo;  // compile-time after unrolling
        const bf16x8w ahi = op(NT16 - 1 - q), alo = op(q);
        auto jof = [&](int i) { return (i < st_hi || (i < st_lo && i < nh)) ? i : NT16 - i; };
        bf16x8w bq[D + 1], aq[D + 1];
        auto rd = [&](int i) {
          bq[i % (D + 1)] = op(jof(i));
          if (i >= st_hi && i < st_lo) aq[i % (D + 1)] = op(i < nh ? NT16 - 1 - q : q);
        };
#pragma unroll
        for (int i = 0; i < D; ++i) rd(i);
#pragma unroll
        for (int i = 0; i < TPP; ++i) {
          if (i + D < TPP) rd(i + D);
          const bf16x8w av = i < st_hi ? ahi : (i >= st_lo ? alo : aq[i % (D + 1)]);
          acc[k][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bq[i % (D + 1)], acc[k][i], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    // keep the accumulators in AGPRs across the loop back edge (the first 64
    // tiles: 256 AGPRs; at PP = 512 the last 2 tiles of a slot stay in VGPRs)
#pragma unroll
    for (int k = 0; k < PPS; ++k)
#pragma unroll
      for (int i = 0; i < TPP; ++i) {
        if (k * TPP + i < 64)
          asm volatile("" : "+a"(acc[k][i]));
        else
          asm volatile("" : "+v"(acc[k][i]));
      }
  }

  // ---- epilogue: Gram tiles (C/D map of the f32 16x16 MFMAs: row = 4 kg + r,
  // column = fl), 128 x 128-tile slab layout -----------------------------------
  {
    constexpr int NB = NT16 / 8;
    constexpr int TB = NB * (NB + 1) / 2;
#pragma unroll
    for (int k = 0; k < PPS; ++k) {
      const int q = slot + FW * S * k;
      if (q >= HALF) continue;
      const int nh = NT16 - q;
#pragma unroll
      for (int i = 0; i < TPP; ++i) {
        const bool hi = i < nh;
        const int I = hi ? NT16 - 1 - q : q;
        const int J = hi ? i : NT16 - i;
        const int I8 = I >> 3, J8 = J >> 3;
        double* G = a.slab_G + ((int64_t)chunk * TB + I8 * (I8 + 1) / 2 + J8) * (GT * GT);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          G[(16 * (I & 7) + 4 * kg + r) * GT + 16 * (J & 7) + fl] = (double)acc[k][i][r];
      }
    }
  }
  if (sg != 0) return;  // workgroup-uniform: group 0 publishes the gradient
  // ---- gradient / log-lik partials: fixed-order sum over the waves ---------
#pragma unroll
  for (int m = 0; m < NF; ++m) red[wid * PP + colf(m)] = gacc[m];
  if ((lane & 7) == 0) llacc -= log(lprod) + lexp * 0.6931471805599453094;
  llacc = wave_allsum(llacc);
  if (lane == 0) {
    misc[8 + wid] = llacc;
    misc[16 + wid] = rsum;
  }
  __syncthreads();
  double rs = 0.0;
#pragma unroll
  for (int v = 0; v < FW; ++v) rs += misc[16 + v];
  for (int f = tid; f < PP; f += NT) {
    const int c = f - ic;
    double g = 0.0;
    if (ic && f == 0) {
      g = rs;
    } else if (c < p) {
      double s = 0.0;
#pragma unroll
      for (int v = 0; v < FW; ++v) s += red[v * PP + c];
      g = STD ? fma(sd[c], s, -sd[PP + c] * rs) : s;
    }
    a.slab_gz[(int64_t)chunk * PP + f] = g;
  }
  if (tid == 0) {
    double ll = 0.0;
#pragma unroll
    for (int v = 0; v < FW; ++v) ll += misc[8 + v];
    a.slab_llz[chunk] = ll;
  }
}

template <bool STD, int NT16>
static hipError_t launch_fused_t(const WideArgs& a, hipStream_t s) {
  const bool vec2 = (a.p % 2 == 0) && ((uintptr_t)a.X % 16 == 0);
  const void* kern = vec2 ? (const void*)wide_fused_bf16_kernel<STD, NT16, true>
                          : (const void*)wide_fused_bf16_kernel<STD, NT16, false>;
  const int lds = fused_lds_bytes(NT16);
  {
    hipError_t e = ensure_max_lds(kern, lds);
    if (e != hipSuccess) return e;
  }
  const int grid = ((a.n_gchunks + 7) / 8) * 8 * fused_groups(NT16);
  if (vec2)
    hipLaunchKernelGGL((wide_fused_bf16_kernel<STD, NT16, true>), dim3(grid), dim3(64 * FW), lds, s,
                       a);
  else
    hipLaunchKernelGGL((wide_fused_bf16_kernel<STD, NT16, false>), dim3(grid), dim3(64 * FW), lds,
                       s, a);
  return hipGetLastError();
}

hipError_t launch_wide_fused(const WideArgs& a, bool standardize, hipStream_t s) {
  if (a.n_gchunks <= 0) return hipSuccess;
  switch (a.NB) {
    case 2: return standardize ? launch_fused_t<true, 16>(a, s) : launch_fused_t<false, 16>(a, s);
    case 3: return standardize ? launch_fused_t<true, 24>(a, s) : launch_fused_t<false, 24>(a, s);
    case 4: return standardize ? launch_fused_t<true, 32>(a, s) : launch_fused_t<false, 32>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
