// Exact (fp64-accurate) IRLS pass on the int8 matrix cores (gfx950 / CDNA4):
// X^T W X by integer digit slices (the Ozaki scheme), the gradient and the
// log-likelihood in fp64.  Instantiated by irls_oz.hip / irls_oz_g2.hip.
//
// Replaces, per exact Newton iteration, the per-partition work of the
// reference map stage -- sklearn newton-cg's Hessian, predict_proba and
// Sig_inv = X^T diag(p(1-p)) X (dlsa/models.py:110-131) -- with ONE pass over
// X, like irls_wave_impl.hpp, but without the fp64 MFMA: on gfx950 a
// v_mfma_f64_16x16x4 issues every ~70 cycles per SIMD (72 TF/s,
// profiles/r03h_mfma_rate_probe.txt) and fp64 VALU work never overlaps it, so
// the fp64 pass is MFMA-bound at ~2x the HBM time of its 808 B/row (config 2:
// 24 ms against the 14 ms of a bf16 pass).  A v_mfma_i32_16x16x64_i8 issues
// every 16 cycles and accumulates exactly in int32.
//
// Numerics.  z = sqrt(w) x (the fp64 row weight times the
// fp64 feature).  Per chunk and feature f an exponent E_f with |z_f| < 2^E_f
// for every row of the chunk (digit_exponent below): from the max |z_f| that
// the partition's last full-data bf16 pass recorded at theta_rec
// (PassArgs::zcolmax), grown by exp(|theta - theta_rec|_1 max|x| / 2), the
// most sqrt(w) can grow between the two points (|d log sqrt(w) / d eta| <=
// 1/2), and never above max |x_f| / 2 (sqrt(w) <= 1/2 at every theta).
// F = round(z 2^(38 - E_f)), |F| < 2^38, by ONE fp64 FMA against
// 1.5 2^52 + B (B = 0x8080808080): the low 40 mantissa bits of the result are
// F + B, whose five bytes XOR 0x80 are the balanced signed digits d_0 (most
// significant) .. d_4 of F = sum_s d_s 2^(8(4-s)).  Then
//   sum_rows F_i F_j = 2^64 sum_k 2^(-8k) L_k,  L_k = sum_{a+b=k} sum_rows d_a(i) d_b(j),
// keeping the levels k < NL: H_ij = 2^(E_i + E_j - 12) sum_{k<NL} 2^(-8k) L_k.
// The integer sums are exact and order-free; the error is the rounding of z
// to 38 bits below 2^E_f and the dropped levels (~2^(-8 NL) of a row's leading
// product, random in sign): 2.15e-12 against the oracle at config 2, as the
// fp64 pass (profiles/r03w_bench_c2.json), and within 1e-11 of the fp64 pass at
// the same iterate (tests/test_gpu_ozaki.py).
//
// MFMA pairing.  One v_mfma_i32_16x16x64_i8 sums 64 k slots; a 32-row block
// fills them with TWO digit products: lane group g holds the 8 rows of
// producer wave g, bytes 0-7 of its fragment digit a (A features) / b (B
// features), bytes 8-15 digit a+1 / b-1 -- both products of level a+b.  A and
// B fragments of one lane hold the same k slots, so this needs no knowledge
// of the instruction's k order.  a in {0, 2, 4}: 9 MFMAs per tile per 32 rows
// cover the 15 products of levels 0-4 (out-of-range digits are zeroed in the
// register).
//
// Workgroup = 4 producer + 4 consumer waves, one workgroup per CU; an
// iteration is two 32-row blocks (b0 = 2m, b1 = 2m + 1):
//   producers (oz_producer): the row phase of both blocks and the digits of
//     those rows straight from the registers.  A wave owns 8 rows of each
//     block; lane (q, s) = (lane >> 4, lane & 15) holds 4 of them for the
//     features 16 k + s, so a digit plane of 4 rows is a byte transpose of the
//     lane's own words.  The image of a wave's 8 rows (5 planes x 16 NT
//     features x 8 bytes) is written over those rows' own x bytes in the ring
//     slot, once they are read;
//   consumers (OzConsumer): the lower-triangle 16x16 tiles of X^T W X by
//     column strips from the previous iteration's two images, NL int32 level
//     accumulators per tile in registers.
// Both issue the LDS-DMA of the next iteration's two blocks into a 6-slot
// ring (the DMA section of irls_oz_kernel).  One barrier per iteration.
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <array>
#include <utility>

#include "dlsa_internal.hpp"
#include "wave_math.hpp"

namespace dlsa {

typedef int oz_i4 __attribute__((ext_vector_type(4)));

namespace ozk {

constexpr int NPW = 4;           // producer waves
constexpr int NCW = 4;           // consumer waves
constexpr int RB = 32;           // rows per DMA block
constexpr int RPW = RB / NPW;    // rows per producer wave per block (8)
constexpr int NSLOT = 6;         // ring: 2 in flight, 2 producing, 2 consuming
// Ring-slot ownership.  Between barriers B_m and B_{m+1}:
//   slots of blocks 2m+2, 2m+3: written only by the LDS-DMA, read by nobody;
//   slots of blocks 2m, 2m+1: producer wave pw reads and then overwrites
//     ONLY the bytes of its own 8 rows (rows 8 pw .. 8 pw + 7 of each block)
//     -- there is no barrier between one producer wave's reads and another's
//     image stores, so a value read from another wave's rows may already be
//     digit bytes (the padding features f >= P of row 8 pw + 7 read row
//     8 pw + 8 and are zeroed, never used);
//   slots of blocks 2m-2, 2m-1: read only (the consumers' operands).
// DLSA_OZ_CHECK builds poison (NaN) any producer read of a feature f < P
// outside the reading wave's own rows, so a violation ends the partition
// nonfinite in the tests.
static_assert(NSLOT >= 6, "2 blocks in flight + 2 producing + 2 consuming");
#ifndef DLSA_OZ_CHECK
#define DLSA_OZ_CHECK 0
#endif
constexpr int ND = 5;            // digits per value
constexpr int GBITS = 38;        // F = round(z 2^(GBITS - E)), |F| <= 2^GBITS (8 ND - 2)
constexpr int NL = 5;            // levels k = a + b of digit products kept
constexpr int EMIN = -985;       // 2^(38 - EMIN) stays finite
constexpr int EMAX = 1009;       // MAGIC 2^(EMAX - 38) stays finite (|z| >= 2^1009
                                 // overflows the fp64 Gram anyway)
// 1.5 2^52 + B, B = 0x8080808080: t = fma(x, c, MAGIC) holds F + B in its low
// 40 bits
constexpr double MAGIC = 6755399441055744.0 + 551911719040.0;

// Ring slot: [16 B pad][x: the block's bytes from its 16-B-aligned start][y: 256 B].
// The x span is cut to what the block needs (the last 1-KiB DMA piece is the
// span's final 1 KiB, overlapping the piece before it), so six slots of
// p = 100 fit the CU.
__host__ __device__ constexpr int xspan(int p) { return (RB * p * 8 + 16 + 15) & ~15; }
__host__ __device__ constexpr int npieces(int p) { return (xspan(p) + 1023) / 1024; }
__host__ __device__ constexpr int slot_bytes(int p) { return 16 + xspan(p) + 256; }
// a wave's image: [feature][digit plane][8 rows] bytes, 48 B per feature (5
// planes + an unwritten sixth), so a lane's operand pair of planes (a, a+1),
// a even, is one aligned 16-byte read
constexpr int kFeatBytes = 48;
constexpr int kMaxPiecesPerWave = 7;  // 1-KiB DMA pieces of a block per wave
// byte offset of digit plane d in a feature's 48-byte image entry
__host__ __device__ constexpr int plane_off(int d) { return 8 * d; }
// profiling-only ablations (bits): 1 producers skip the row phase and digits, 2
// consumers skip the MFMAs
#ifndef DLSA_OZ_ABLATE
#define DLSA_OZ_ABLATE 0
#endif
__host__ __device__ constexpr int img_bytes(int NT) { return 16 * NT * kFeatBytes; }
// LDS after the ring: theta, center / 1/scale [PMAX] fp64, digit exponents [PMAX]
__host__ __device__ constexpr int extra_bytes(int NT) { return 3 * 16 * NT * 8 + 16 * NT * 4; }
__host__ __device__ constexpr int lds_bytes(int NT, int p) {
  return NSLOT * slot_bytes(p) + extra_bytes(NT);
}
// the pass applies when a wave's image fits in the x bytes of its 8 rows and
// the ring fits the CU.  The first condition gives 768 NT <= 64 p, so
// p >= 12 and xspan(p) >= 3088: a block always has a final 1 KiB for its last
// DMA piece.
__host__ __device__ constexpr bool fits(int NT, int p) {
  return img_bytes(NT) <= RPW * p * 8 && lds_bytes(NT, p) <= 160 * 1024 &&
         npieces(p) <= NCW * kMaxPiecesPerWave;
}

// Column strips J (tiles (I, J), I = J .. NT-1) dealt to the consumer waves,
// largest first, each to the wave with the fewest tiles (NT = 7: {0}, {1, 6},
// {2, 5}, {3, 4}: 7 tiles each).
constexpr unsigned strip_mask(int NT, int cw) {
  int load[NCW] = {0, 0, 0, 0};
  unsigned m[NCW] = {0, 0, 0, 0};
  for (int J = 0; J < NT; ++J) {
    int best = 0;
    for (int w = 1; w < NCW; ++w)
      if (load[w] < load[best]) best = w;
    load[best] += NT - J;
    m[best] |= 1u << J;
  }
  return m[cw];
}

template <int NT, int CW>
struct Tiles {
  static constexpr unsigned SM = strip_mask(NT, CW);
  static constexpr int count() {
    int c = 0;
    for (int J = 0; J < NT; ++J)
      if ((SM >> J) & 1u) c += NT - J;
    return c;
  }
  static constexpr int TW = count();
  // tile index of (I, J) in this wave (strips ascending, I ascending)
  static constexpr int index(int I, int J) {
    int c = 0;
    for (int j = 0; j < NT; ++j)
      if ((SM >> j) & 1u) {
        if (j == J) return c + (I - J);
        c += NT - j;
      }
    return -1;
  }
  static constexpr int I_of(int i) {
    for (int j = 0; j < NT; ++j)
      if ((SM >> j) & 1u) {
        if (i < NT - j) return j + i;
        i -= NT - j;
      }
    return -1;
  }
  static constexpr int J_of(int i) {
    for (int j = 0; j < NT; ++j)
      if ((SM >> j) & 1u) {
        if (i < NT - j) return j;
        i -= NT - j;
      }
    return -1;
  }
  static constexpr int strip_ordinal(int J) {  // strips of this wave before J
    int c = 0;
    for (int j = 0; j < J; ++j) c += (SM >> j) & 1u;
    return c;
  }
};

// v_perm_b32: byte s of the result = byte sel_s of {a (bytes 4-7), b (0-3)}
__device__ __forceinline__ uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
  return __builtin_amdgcn_perm(a, b, sel);
}

// sum_k 2^(-8k) L_k of one accumulator element
__device__ __forceinline__ double level_value(const oz_i4 (&L)[NL], int r) {
  double v = (double)L[NL - 1][r];
#pragma unroll
  for (int k = NL - 2; k >= 0; --k) v = fma(v, 0x1p-8, (double)L[k][r]);
  return v;
}

// Upper bound of |x| from a recorded max |x| high dword (low dword all ones).
__device__ __forceinline__ double xbound(uint32_t hi) {
  return __hiloint2double((int)(hi & 0x7FFFFFFFu), (int)0xFFFFFFFFu);
}
// Digit exponent E (bound < 2^E) of a feature of a chunk.  xhi: recorded max
// |x| high dword; zbits = recorded max |z| (fp32 bits, z32 =
// fl32(fl32(x) sqrtf(fl32(w))), within 5 fp32 ulp of z wherever |z| >= 2^-120
// and w is an fp32 normal), growth = exp(dB / 2) >= the factor sqrt(w) can
// have grown by since the record.  Rows the fp32 record cannot see have
// |z| < 2^-120 or sqrt(w) < 2^-60 (w below the fp32 normals), hence the two
// floors; and sqrt(w) <= 1/2 always.
__device__ __forceinline__ int digit_exponent(uint32_t xhi, uint32_t zbits, double growth) {
  const double xb = xbound(xhi);
  const double zb = (double)__uint_as_float(zbits & 0x7FFFFFFFu) * (1.0 + 0x1p-16);
  double bound = fmax(fmax(zb, 0x1p-120), xb * 0x1p-60) * growth;
  bound = fmin(bound, 0.5 * xb);  // (also when growth overflowed to inf)
  const int e = __builtin_amdgcn_frexp_exp(bound);
  return max(e, EMIN);  // above EMAX: the caller fails the chunk (digit_overflow)
}
// |z| >= 2^EMAX: the digits of F = round(z 2^(38 - E)) would wrap at the
// clamped exponent (a finite, wrong Hessian), so such a chunk publishes a NaN
// log-likelihood instead -- the partition then fails as nonfinite, as the
// fp64 Gram's inf would make it
__device__ __forceinline__ bool digit_overflow(int e) { return e > EMAX; }

}  // namespace ozk

// Profiling build (DLSA_OZ_PROF, tools/build_variants.sh ozprof): per-wave
// cycle stamps (s_memtime) of the iteration's phases, summed over the chunk
// and added to g_oz_prof[slot] at its end (one vector atomic per wave).
#ifdef DLSA_OZ_PROF
static __device__ unsigned long long g_oz_prof[32];  // per translation unit: [4 wid + i]
static inline int oz_prof_read_impl(unsigned long long* out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_oz_prof), 32 * 8) != hipSuccess) return -1;
  unsigned long long z[32] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_oz_prof), z, 32 * 8) == hipSuccess ? 0 : -1;
}
#define OZ_STAMP(v) const uint64_t v = __builtin_readcyclecounter()
#define OZ_STAMP_VAR(v) uint64_t v = 0
#define OZ_STAMP_SET(v) v = __builtin_readcyclecounter()
#define OZ_ADD(i, d) prof[i] += (d)
#define OZ_DECL uint64_t prof[4] = {0, 0, 0, 0}
#define OZ_FLUSH(base)                                                        \
  if (lane == 0)                                                              \
    for (int i_ = 0; i_ < 4; ++i_) atomicAdd(&g_oz_prof[(base) + i_], prof[i_])
#else
#define OZ_STAMP(v)
#define OZ_STAMP_VAR(v)
#define OZ_STAMP_SET(v)
#define OZ_ADD(i, d)
#define OZ_DECL
#define OZ_FLUSH(base)
#endif

// ---- consumer waves: tiles of X^T W X -------------------------------------
template <int NT, int CW>
struct OzConsumer {
  using TL = ozk::Tiles<NT, CW>;
  static constexpr int TW = TL::TW;
  static constexpr int PMAX = 16 * NT;
  oz_i4 acc[TW > 0 ? TW : 1][ozk::NL];

  __device__ __forceinline__ void init() {
    static_for<(TW > 0 ? TW : 1)>([&](auto iI) {
      constexpr int i = decltype(iI)::value;
#pragma unroll
      for (int k = 0; k < ozk::NL; ++k) acc[i][k] = oz_i4{0, 0, 0, 0};
    });
  }

  // the image of one 32-row block whose x started at xs (LDS); tick() is
  // called after every tile's MFMAs (the DMA of the next blocks rides along).
  // Software-pipelined: the operands of tile t+1 (and of the next strip) are
  // read while the MFMAs of tile t issue.
  template <typename Tick>
  __device__ __forceinline__ void consume(const char* xs, int p, int lane, Tick&& tick) {
    if constexpr (TW > 0) {
      const int i = lane & 15, g = lane >> 4;
      // lane group g: the image of producer wave g (its 8 rows of the block)
      const char* im = xs + g * ozk::RPW * p * 8 + i * ozk::kFeatBytes;
      using u2 = unsigned __attribute__((ext_vector_type(2)));
      oz_i4 A0[2], A2[2];
      u2 A4[2];
      u2 Bd[2][ozk::ND];
      auto loadB = [&](auto jJ, int u) {
        constexpr int fo = 16 * decltype(jJ)::value * ozk::kFeatBytes;
#pragma unroll
        for (int b = 0; b < ozk::ND; ++b) Bd[u][b] = *(const u2*)(im + fo + 8 * b);
      };
      auto loadA = [&](auto tI, int u) {
        constexpr int fa = 16 * TL::I_of(decltype(tI)::value) * ozk::kFeatBytes;
        // A quad a: digits (a, a+1) of the feature -- one 16-byte read
        A0[u] = *(const oz_i4*)(im + fa);
        A2[u] = *(const oz_i4*)(im + fa + 16);
        A4[u] = *(const u2*)(im + fa + 32);
      };
      loadB(std::integral_constant<int, TL::J_of(0)>{}, 0);
      loadA(std::integral_constant<int, 0>{}, 0);
      static_for<TW>([&](auto tI) {
        constexpr int t = decltype(tI)::value;
        constexpr int J = TL::J_of(t);
        constexpr int ua = t & 1;
        constexpr int ub = TL::strip_ordinal(J) & 1;
        if constexpr (t + 1 < TW) {
          constexpr int Jn = TL::J_of(t + 1);
          if constexpr (Jn != J) loadB(std::integral_constant<int, Jn>{}, ub ^ 1);
          loadA(std::integral_constant<int, t + 1>{}, ua ^ 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        // B quad b: bytes 0-7 digit b, bytes 8-15 digit b - 1 (zero for b = 0)
        const u2* d = Bd[ub];
        oz_i4 Bq[ozk::ND];
        Bq[0] = oz_i4{(int)d[0].x, (int)d[0].y, 0, 0};
#pragma unroll
        for (int b = 1; b < ozk::ND; ++b)
          Bq[b] = oz_i4{(int)d[b].x, (int)d[b].y, (int)d[b - 1].x, (int)d[b - 1].y};
        const oz_i4 a0 = A0[ua], a2 = A2[ua];
        const oz_i4 a4 = oz_i4{(int)A4[ua].x, (int)A4[ua].y, 0, 0};  // digit 5 = 0
        // A quad a against B quad b: the products (a, b) and (a+1, b-1) of level a + b
        acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, Bq[0], acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, Bq[1], acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, Bq[2], acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, Bq[3], acc[t][3], 0, 0, 0);
        acc[t][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, Bq[4], acc[t][4], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, Bq[0], acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, Bq[1], acc[t][3], 0, 0, 0);
        acc[t][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, Bq[2], acc[t][4], 0, 0, 0);
        acc[t][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a4, Bq[0], acc[t][4], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        tick(std::integral_constant<int, t>{});
      });
      // keep the level accumulators in registers across the loop
      static_for<TW>([this](auto iI) {
        constexpr int t = decltype(iI)::value;
#pragma unroll
        for (int k = 0; k < ozk::NL; ++k) asm volatile("" : "+v"(acc[t][k]));
      });
    }
  }

  // H tiles into the chunk's slab (newton_solve.hip layout), scaled back
  __device__ __forceinline__ void store(double* sH, const int* ex, int lane) {
    if constexpr (TW > 0) {
      const int fl = lane & 15, q = lane >> 4;
      static_for<TW>([&](auto iI) {
        constexpr int t = decltype(iI)::value;
        constexpr int I = TL::I_of(t), J = TL::J_of(t);
        constexpr int ts = I * (I + 1) / 2 + J;
        const int ej = ex[16 * J + fl];
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // i32 16x16 C/D map: row 4 (l >> 4) + r, col l & 15
          const int row = 4 * q + r;
          const double v = ozk::level_value(acc[t], r);
          sH[ts * 256 + row * 16 + fl] = __builtin_amdgcn_ldexp(v, ej + ex[16 * I + row] - 12);
        }
      });
    }
  }
};

// ---- producer waves: row phase and digit images ----------------------------
// Lane (q, s) = (lane >> 4, lane & 15) holds 4 rows of features 16 k + s,
// k = 0 .. NT-1: rows 4 (q & 1) .. 4 (q & 1) + 3 of this wave's 8 rows of
// block 2m + (q >> 1).  With the 4 rows of a feature in one lane, a digit
// plane of 4 rows is a byte transpose of the lane's own words (8 v_perm for
// the four low-dword planes, 3 for the top digit), the x reads of a wave row
// are 16 consecutive doubles (no bank conflicts), and theta, the gradient
// partials and the digit constants take NT register pairs per lane.
// eta of the 4 rows: 4 FMA chains over the lane's NT features, then a
// reduce-scatter over the 16 lanes of the feature slots (DPP row_ror:8,
// row_half_mirror, 2 quad_perm) leaves lane s with row s >> 2; one
// transcendental chain for the 16 rows of the wave (4 replicas per row);
// row_newbcast brings each row's sqrt(w) and residual back to the 16 lanes.
// The digits: t = fma(x, sqrt(w), mg) against the per-feature magic
// mg = MAGIC 2^(E_f - 38) carries the mantissa of fma(x, sqrt(w) 2^(38 - E_f),
// MAGIC) (a power-of-two scaling of the same rounding), so no per-value ldexp.
template <int NT, bool STD, typename SlotX, typename Dma>
__device__ __forceinline__ void oz_producer(const PassArgs& a, char* smem, int wid, int lane,
                                            int tid, int nb, int nit, int sbytes, int xs_bytes,
                                            SlotX&& slot_x, const double* bet,
                                            const double* stdv, const int* ex, int chunk,
                                            bool chunk_ovf, Dma&& issue_pair) {
  using namespace ozk;
  constexpr int PMAX = 16 * NT;
  const int p = a.p, P = a.P, ic = a.intercept;
  const int nrows = __builtin_amdgcn_readfirstlane(a.chunk_rows[blockIdx.x]);
  const int pw = wid;
  const int q = lane >> 4, s = lane & 15;
  const int Xq = q >> 1, hq = q & 1;
  const int rbase = pw * RPW + 4 * hq;  // block row of this lane's row 0
  const bool up8 = s >= 8, up4 = ((s >> 2) & 1) != 0;
  const int myrow = s >> 2;             // the row whose eta this lane ends with
  double beta[NT], gacc[NT], mg[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int f = 16 * k + s;
    beta[k] = bet[f];
    mg[k] = __builtin_amdgcn_ldexp(MAGIC, ex[f] - GBITS);
    gacc[k] = 0.0;
  }
  const bool fin_last = 16 * (NT - 1) + s < P;  // the last tile's feature is < P
  double llacc = 0.0, lprod = 1.0;

  // the producers' DMA share (piece 0 of each block, issue_pair): each wave
  // waits for its own pieces before the next barrier, which then publishes
  // all of them
  issue_pair(-1);
  wait_vmcnt<0>();
  OZ_DECL;
  for (int m = 0; m < nit; ++m) {
    OZ_STAMP(t0);
    wait_vmcnt<0>();
    lds_barrier();  // B_m
    OZ_STAMP(t1);
    OZ_ADD(0, t1 - t0);
    issue_pair(m);
    if (2 * m >= nb || (DLSA_OZ_ABLATE & 1)) continue;  // the last iteration only consumes
    const int b = 2 * m + Xq;
    char* xq = slot_x(b);
    const double* yq = (const double*)(smem + (b % NSLOT) * sbytes + 16 + xs_bytes);
    const int leftq = nrows - b * RB;
    // workgroup-uniform: both blocks full
    const bool full = nrows - 2 * m * RB >= 2 * RB;
    double v[4][NT], e[4];
    auto row_phase = [&](auto maskI) {
      constexpr bool MASK = decltype(maskI)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rowB = rbase + r;
        const bool valid = rowB < leftq;
        const double* xr = (const double*)xq + rowB * p + (s - ic);
        double er = 0.0;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
          const int f = 16 * k + s;
          double x = xr[16 * k];
          if constexpr (DLSA_OZ_CHECK) {  // ownership rule: own rows for f < P
            const int el = rowB * p + f - ic;
            if (f >= ic && f < P && (el < pw * RPW * p || el >= (pw + 1) * RPW * p))
              x = __builtin_nan("");
          }
          if constexpr (STD) x = (x - stdv[f]) * stdv[PMAX + f];
          if (k == 0 && ic && s == 0) x = 1.0;
          const bool fin = k < NT - 1 || fin_last;  // padding features f >= P: 0
          if constexpr (MASK)
            x = (valid && fin) ? x : 0.0;
          else
            x = fin ? x : 0.0;
          v[r][k] = x;
          er = fma(x, beta[k], er);
        }
        e[r] = er;
      }
    };
    if (full)
      row_phase(std::false_type{});
    else
      row_phase(std::true_type{});
    // reduce-scatter of the 4 row sums over the 16 feature slots
    double e01, e23;
    {
      const double s0 = up8 ? e[0] : e[2], s1 = up8 ? e[1] : e[3];  // the partner's rows
      const double k0 = up8 ? e[2] : e[0], k1 = up8 ? e[3] : e[1];  // kept
      e01 = k0 + dpp_f64<0x128>(s0);  // row_ror:8 = lane s ^ 8
      e23 = k1 + dpp_f64<0x128>(s1);
    }
    double eh;
    {
      const double sn = up4 ? e01 : e23, kp = up4 ? e23 : e01;
      eh = kp + dpp_f64<0x141>(sn);  // row_half_mirror: bit 2 of s flipped
    }
    eh += dpp_f64<0xB1>(eh);  // quad_perm [1,0,3,2]
    eh += dpp_f64<0x4E>(eh);  // quad_perm [2,3,0,1]
    // one transcendental chain for the wave's 16 rows (row rbase + myrow)
    double swh, rh;
    {
      const bool valid = rbase + myrow < leftq;
      const double yv = valid ? yq[rbase + myrow] : 0.0;
      // logistic_link (glm_row.hpp) through the half angle: eqv = sqrt(ea)
      // gives sqrt(w) = eqv * inv without a square root
      const double eqv = exp(-0.5 * fabs(eh));
      const double ea = eqv * eqv;
      const double inv = wv_rcp(1.0 + ea);
      const double mu = eh >= 0.0 ? inv : ea * inv;
      swh = eqv * inv;
      rh = yv - mu;
      if (valid && (s & 3) == 0) {
        llacc += yv * eh - fmax(eh, 0.0);
        lprod *= 1.0 + ea;
      }
      if (!valid) {
        swh = 0.0;
        rh = 0.0;
      }
    }
    double sw[4], res[4];
    sw[0] = dpp_f64<0x150>(swh);  // row_newbcast:4r -- row r's values to the 16 lanes
    sw[1] = dpp_f64<0x154>(swh);
    sw[2] = dpp_f64<0x158>(swh);
    sw[3] = dpp_f64<0x15C>(swh);
    res[0] = dpp_f64<0x150>(rh);
    res[1] = dpp_f64<0x154>(rh);
    res[2] = dpp_f64<0x158>(rh);
    res[3] = dpp_f64<0x15C>(rh);
    OZ_STAMP(t2);
    OZ_ADD(1, t2 - t1);
    // ---- gradient and the digit image of the 4 rows ---------------------------
    char* img = xq + pw * RPW * p * 8 + 4 * hq;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      gacc[k] = fma(v[0][k], res[0], gacc[k]);
      gacc[k] = fma(v[1][k], res[1], gacc[k]);
      gacc[k] = fma(v[2][k], res[2], gacc[k]);
      gacc[k] = fma(v[3][k], res[3], gacc[k]);
      uint32_t lo[4], hi[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double t = fma(v[r][k], sw[r], mg[k]);
        lo[r] = __double2loint(t);
        hi[r] = __double2hiint(t);
      }
      // byte j of lo = digit 4 - j; byte 0 of hi = digit 0 (row order = byte order)
      const uint32_t u01 = perm(lo[1], lo[0], 0x05010400u), w01 = perm(lo[1], lo[0], 0x07030602u);
      const uint32_t u23 = perm(lo[3], lo[2], 0x05010400u), w23 = perm(lo[3], lo[2], 0x07030602u);
      const uint32_t d4 = perm(u23, u01, 0x05040100u) ^ 0x80808080u;
      const uint32_t d3 = perm(u23, u01, 0x07060302u) ^ 0x80808080u;
      const uint32_t d2 = perm(w23, w01, 0x05040100u) ^ 0x80808080u;
      const uint32_t d1 = perm(w23, w01, 0x07060302u) ^ 0x80808080u;
      const uint32_t d0 = perm(perm(hi[3], hi[2], 0x05010400u), perm(hi[1], hi[0], 0x05010400u),
                               0x05040100u) ^ 0x80808080u;
      char* fe = img + (16 * k + s) * kFeatBytes;
      *(uint32_t*)(fe + plane_off(0)) = d0;
      *(uint32_t*)(fe + plane_off(1)) = d1;
      *(uint32_t*)(fe + plane_off(2)) = d2;
      *(uint32_t*)(fe + plane_off(3)) = d3;
      *(uint32_t*)(fe + plane_off(4)) = d4;
    }
#ifdef DLSA_OZ_PROF
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    OZ_STAMP(t3);
    OZ_ADD(2, t3 - t2);
  }
  OZ_FLUSH(4 * pw);
  __syncthreads();  // S1 (the consumers' S1): the ring is free

  // ---- epilogue: gradient and log-likelihood partials --------------------------
  double* red = (double*)smem;  // the ring: [NPW][PMAX + 1]
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    double g = gacc[k];
    g += __shfl_xor(g, 16);
    g += __shfl_xor(g, 32);
    if (q == 0) red[pw * (PMAX + 1) + 16 * k + s] = g;
  }
  llacc -= log(lprod);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) llacc += __shfl_xor(llacc, o);
  if (lane == 0) red[pw * (PMAX + 1) + PMAX] = llacc;
  __syncthreads();  // S2
  for (int f = tid; f < PMAX; f += 64 * NPW) {
    double sg = 0.0;
#pragma unroll
    for (int w = 0; w < NPW; ++w) sg += red[w * (PMAX + 1) + f];
    a.slab_g[(int64_t)chunk * PMAX + f] = sg;
  }
  if (tid == 0) {
    double sg = 0.0;
#pragma unroll
    for (int w = 0; w < NPW; ++w) sg += red[w * (PMAX + 1) + PMAX];
    // a digit exponent past EMAX (clamped in ex[]) would publish wrapped
    // digits: the chunk's NaN log-likelihood fails its partition visibly
    // (chunk_ovf is wave 0's ballot; tid 0 is in wave 0)
    a.slab_ll[chunk] = chunk_ovf ? __builtin_nan("") : sg;
  }
}

template <int NT, bool STD>
__global__ __launch_bounds__(64 * (ozk::NPW + ozk::NCW), 1) void irls_oz_kernel(const PassArgs a) {
  using namespace ozk;
  constexpr int PMAX = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int chunk = blockIdx.x;
  const int part = __builtin_amdgcn_readfirstlane(a.chunk_part[chunk]);
  if (a.phase[part] != a.want_phase) return;  // workgroup-uniform

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, P = a.P, ic = a.intercept;
  const int64_t row0 = uniform_row0(a.chunk_row0, chunk);
  const int nrows = __builtin_amdgcn_readfirstlane(a.chunk_rows[chunk]);
  const int nb = (nrows + RB - 1) / RB;
  const int nit = (nb + 1) / 2 + 1;  // iterations (the last only consumes)
  const int sbytes = slot_bytes(p);
  const int np = npieces(p);
  const int xs_bytes = xspan(p);
  double* bet = (double*)(smem + NSLOT * sbytes);  // [PMAX] theta of the partition
  double* stdv = bet + PMAX;                        // [2][PMAX] center, 1/scale
  int* ex = (int*)(stdv + 2 * PMAX);                // [PMAX] digit exponents E_f

  // digit scales: |theta - theta_rec|_1 and the chunk's max |x| over all
  // features (PMAX <= 112 < the 512 threads: one feature per thread), reduced
  // in a fixed order, so every thread forms the same growth factor
  double dth = 0.0;
  uint32_t xh = 0;
  bool e_ovf = false;
  if (tid < PMAX) {
    const double th = (tid < P) ? a.theta[(int64_t)part * P + tid] : 0.0;
    bet[tid] = th;
    if (tid < P) dth = fabs(th - a.theta_rec[(int64_t)part * P + tid]);
    xh = a.colmax[(int64_t)chunk * PMAX + tid] & 0x7FFFFFFFu;
    if constexpr (STD) {
      const int j = tid - ic;
      const bool in = j >= 0 && j < p;
      stdv[tid] = in ? a.center[j] : 0.0;
      stdv[PMAX + tid] = in ? 1.0 / a.scale[j] : 1.0;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    dth += __shfl_xor(dth, o);
    xh = max(xh, (uint32_t)__shfl_xor((int)xh, o));
  }
  double* dred = (double*)smem;  // the ring's first bytes, before any DMA
  uint32_t* xred = (uint32_t*)(dred + (NPW + NCW));
  if (lane == 0) {
    dred[wid] = dth;
    xred[wid] = xh;
  }
  __syncthreads();
  if (tid < PMAX) {
    double sd = 0.0;
    uint32_t xm = 0;
#pragma unroll
    for (int w = 0; w < NPW + NCW; ++w) {
      sd += dred[w];
      xm = max(xm, xred[w]);
    }
    const double growth = exp(0.5 * sd * ozk::xbound(xm)) * (1.0 + 0x1p-40);
    const int e = digit_exponent(a.colmax[(int64_t)chunk * PMAX + tid],
                                 a.zcolmax[(int64_t)chunk * PMAX + tid], growth);
    ex[tid] = min(e, ozk::EMAX);
    if (wid == 0) {  // wave 0 (whose tid 0 publishes slab_ll) also checks wave 1's features
      e_ovf = ozk::digit_overflow(e);
      if (tid + 64 < PMAX)
        e_ovf = e_ovf || ozk::digit_overflow(digit_exponent(
                             a.colmax[(int64_t)chunk * PMAX + tid + 64],
                             a.zcolmax[(int64_t)chunk * PMAX + tid + 64], growth));
    }
  }
  // (no __syncthreads_or: its __shared__ word would push the LDS past 160 KB)
  const bool chunk_ovf = wid == 0 && __ballot(e_ovf) != 0;
  // (the ring needs no zeroing: past-the-chunk rows are zeroed in registers
  // and nothing reads a slot's bytes that the DMA did not write)
  __syncthreads();

  auto slot_x = [&](int blk) -> char* {
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)blk * RB) * p);
    return smem + (blk % NSLOT) * sbytes + 16 + (start & 15);
  };

  // ---- LDS-DMA of the X / y blocks --------------------------------------------
  // Both wave types issue it; dw = the issuing wave's index among its four.
  // Wave dw's pieces of a block: X pieces dw, dw + 4, ... and (dw = 3) the
  // block's y.  Scalar bases per block; piece i (a compile-time index) is two
  // scalar adds and the DMA.  The last piece is the block's final 1 KiB,
  // overlapping the piece before it with the same bytes: whole-wave, no lane
  // predicate (xspan(p) >= 1024, see fits()).
  // The schedule, for blocks 2m+2, 2m+3 (into the slots of 2m-4, 2m-3, free
  // since B_m): the producers issue piece i = 0 right after B_m (and before the
  // loop for blocks 0, 1), so the DMA issue cost is split between the two wave
  // types; the consumers issue the pieces i >= KP and y, one piece of each
  // block per tile during the first image's MFMAs and then the rest, so the
  // last pieces land while the second image's MFMAs run instead of in front
  // of the iteration's final wait.
  constexpr int KP = 1;  // the producers' pieces of a block: i < KP
  const int dw = wid >= NPW ? wid - NPW : wid;
  const uintptr_t xcb = (uintptr_t)(a.X + row0 * p) & ~(uintptr_t)15;
  const __amdgpu_buffer_rsrc_t xr = uniform_rsrc(xcb, a.x_last16 + 16 - xcb);
  const uintptr_t ycb = (uintptr_t)(a.y + row0);
  const __amdgpu_buffer_rsrc_t yr = uniform_rsrc(ycb, a.y_last4 + 4 - ycb);
  const int npw = (np - dw + NCW - 1) / NCW;
  // a block's slot LDS offset and the buffer offset of its 16-B-aligned start
  auto blk_lds = [&](int blk) { return __builtin_amdgcn_readfirstlane((blk % NSLOT) * sbytes); };
  auto blk_soff = [&](int blk) {
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)blk * RB) * p);
    return __builtin_amdgcn_readfirstlane((int)((start & ~(uintptr_t)15) - xcb));
  };
  auto issue_x = [&](auto iI, int lds, int soff) {
    constexpr int i = decltype(iI)::value;
    if (i < npw) {  // uniform
      const int j = dw + NCW * i;
      const int off = j == np - 1 ? xs_bytes - 1024 : j * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void_t*)(smem + lds + 16 + off), 16,
                                               lane * 16, soff + off, 0, DLSA_OZ_DMA_AUX);
    }
  };
  auto issue_y = [&](int blk, int lds) {
    if (dw == NCW - 1)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(yr, (lds_void_t*)(smem + lds + 16 + xs_bytes), 4,
                                               lane * 4, blk * RB * 8, 0, 0);
  };
  // the consumers' share: a block's pieces from piece I0 on, and its y
  auto issue_rest = [&](auto I0, int blk, int lds, int soff) {
    static_for<kMaxPiecesPerWave>([&](auto iI) {
      if constexpr (decltype(iI)::value >= decltype(I0)::value) issue_x(iI, lds, soff);
    });
    issue_y(blk, lds);
  };
  // the producers' share: piece 0 of blocks 2m+2, 2m+3 (m = -1: blocks 0, 1)
  static_assert(KP == 1, "issue_pair issues piece 0 only");
  auto issue_pair = [&](int m) {
#pragma unroll
    for (int X = 2; X < 4; ++X) {
      const int blk = 2 * m + X;
      if (blk < nb) issue_x(std::integral_constant<int, 0>{}, blk_lds(blk), blk_soff(blk));
    }
  };

  if (wid >= NPW) {
    // ======================= consumer waves ==================================
    const int cw = wid - NPW;
    auto run = [&](auto cwI) {
      constexpr int CW = decltype(cwI)::value;
      constexpr int TW = OzConsumer<NT, CW>::TW;
      // consumers at priority 1: the younger half of the workgroup otherwise
      // gets only the producers' leftover issue slots (MI355X_MICROARCH.md "Two
      // waves per SIMD", items 2 and 4)
      __builtin_amdgcn_s_setprio(1);
      OzConsumer<NT, CW> C;
      C.init();
      for (int b = 0; b < 2 && b < nb; ++b)
        issue_rest(std::integral_constant<int, KP>{}, b, blk_lds(b), blk_soff(b));
      wait_vmcnt<0>();
      OZ_DECL;
      for (int m = 0; m < nit; ++m) {
        OZ_STAMP(t0);
        lds_barrier();  // B_m: blocks 2m, 2m+1 landed; the images of 2m-2, 2m-1 written
        OZ_STAMP(t1);
        // the DMA of blocks 2m+2, 2m+3: piece KP + t of each after tile t's MFMAs
        // of the first image, the rest after it (all of them when no image is
        // consumed); nothing during the second image
        const bool d0 = 2 * m + 2 < nb, d1 = 2 * m + 3 < nb;
        const int l0 = blk_lds(2 * m + 2), s0 = blk_soff(2 * m + 2);
        const int l1 = blk_lds(2 * m + 3), s1 = blk_soff(2 * m + 3);
        const bool c0 = m >= 1 && !(DLSA_OZ_ABLATE & 2);
        const bool c1 = c0 && 2 * m - 1 < nb;
        OZ_STAMP_VAR(t2);
        auto tickA = [&](auto tI) {
          constexpr int i = KP + decltype(tI)::value;
          if (d0) issue_x(std::integral_constant<int, i>{}, l0, s0);
          if (d1) issue_x(std::integral_constant<int, i>{}, l1, s1);
        };
        auto tickN = [&](auto) {};
        if (c0) C.consume(slot_x(2 * m - 2), p, lane, tickA);
        if (c0) {
          if (d0) issue_rest(std::integral_constant<int, KP + TW>{}, 2 * m + 2, l0, s0);
          if (d1) issue_rest(std::integral_constant<int, KP + TW>{}, 2 * m + 3, l1, s1);
        } else {
          if (d0) issue_rest(std::integral_constant<int, KP>{}, 2 * m + 2, l0, s0);
          if (d1) issue_rest(std::integral_constant<int, KP>{}, 2 * m + 3, l1, s1);
        }
        if (c1) C.consume(slot_x(2 * m - 1), p, lane, tickN);
        OZ_STAMP_SET(t2);
        OZ_STAMP(t3);
        wait_vmcnt<0>();
        OZ_STAMP(t4);
        OZ_ADD(0, t1 - t0);
        OZ_ADD(1, t3 - t2);
        OZ_ADD(2, t2 - t1);
        OZ_ADD(3, t4 - t3);
      }
      OZ_FLUSH(4 * (NPW + CW));
      __syncthreads();  // S1
      C.store(a.slab_H + (int64_t)chunk * (NT * (NT + 1) / 2) * 256, ex, lane);
      __syncthreads();  // S2 (the producers' reduction)
    };
    switch (cw) {
      case 0: run(std::integral_constant<int, 0>{}); break;
      case 1: run(std::integral_constant<int, 1>{}); break;
      case 2: run(std::integral_constant<int, 2>{}); break;
      default: run(std::integral_constant<int, 3>{}); break;
    }
    return;
  }

  oz_producer<NT, STD>(a, smem, wid, lane, tid, nb, nit, sbytes, xs_bytes, slot_x, bet, stdv,
                       ex, chunk, chunk_ovf, issue_pair);
}

template <int NT, bool STD>
static hipError_t launch_oz_t(const PassArgs& a, int n_chunks, hipStream_t s) {
  auto kern = irls_oz_kernel<NT, STD>;
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(64 * (ozk::NPW + ozk::NCW)),
                     ozk::lds_bytes(NT, a.p), s, a);
  return hipGetLastError();
}

template <int NT>
static hipError_t launch_oz_nt(const PassArgs& a, bool std_, int n_chunks, hipStream_t s) {
  return std_ ? launch_oz_t<NT, true>(a, n_chunks, s) : launch_oz_t<NT, false>(a, n_chunks, s);
}

// Entry point of a compilation unit, one line per unit (the family with digit
// scales only): DLSA_OZ_UNIT(name, NT...); irls_oz.hip routes to them.
typedef hipError_t OzUnitFn(const PassArgs& a, int NT, bool std_, int family, int n_chunks,
                            hipStream_t s);
#define DLSA_OZ_UNIT(name, ...)                                                                  \
  hipError_t name(const PassArgs& a, int NT, bool std_, int family, int n_chunks, hipStream_t s) { \
    return unit_dispatch(FamLogistic{}, IntList<__VA_ARGS__>{}, family, NT, [&](auto, auto nt) { \
      return launch_oz_nt<decltype(nt)::value>(a, std_, n_chunks, s);                            \
    });                                                                                          \
  }

}  // namespace dlsa
