// Cooperative fused IRLS pass (gfx950 / CDNA4) -- kernel templates, included
// by the irls_coop*.hip translation units (one per group of NT values, so the
// instantiations compile in parallel).
//
// Cooperative fused IRLS pass: one 4-wave workgroup streams
// a chunk of rows of one partition through a shared LDS-DMA ring.
//
// Replaces, per Newton iteration, the per-partition work of the reference map
// stage (sklearn newton-cg Hessian-vector passes, predict_proba and
// Sig_inv = X^T diag(p(1-p)) X, dlsa/models.py:110-131) with ONE pass over X.
//
// Per 32-row block:
//   B1  barrier: the block's DMA pieces (issued by all 4 waves, each waiting
//       on its own counted vmcnt) have landed; the slot of block b-1 is free
//       and receives block b+S-1 (S-1 blocks always in flight).
//   B   row phase: rows split over the waves, 8 lanes per row.  eta = x.theta
//       (fp64, 8-lane DPP reduction), mu, w = mu(1-mu), r = y - mu, the
//       gradient x*r and the log-likelihood are computed ONCE per row; w and r
//       are published in LDS (PREC_F32 / PREC_F64; the bf16 tiles read only the
//       operand image the row phase writes).
//   B2  barrier.
//   C   tile phase: the lower-triangle 16x16 tiles of X^T W X are split over
//       the waves (contiguous tile ranges, so each wave touches few column
//       tiles).  PREC_BF16: one v_mfma_f32_16x16x32_bf16 per tile per block;
//       PREC_F32 / PREC_F64: 8 k-steps of v_mfma_*_16x16x4 (fp32 / fp64).
// The bf16 / fp32 Hessians only steer Newton (the fp64 gradient fixes the
// fixed point); the returned Sig_inv always comes from a PREC_F64 pass.
#include <stdlib.h>

#include <type_traits>
#include <utility>

#pragma once

#include "dlsa_internal.hpp"
#include "glm_row.hpp"

namespace dlsa {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2c __attribute__((ext_vector_type(2)));
typedef float f2c __attribute__((ext_vector_type(2)));

namespace {

constexpr int RB = kCoopRows;   // rows per block

// Profiling-only ablations (tools/build_variants.sh builds them into separate
// .so files; the product build has DLSA_ABLATE = 0): 1 no tile phase, 2 no
// transcendentals in the row phase, 3 stream only, 4 no row phase.
#ifndef DLSA_ABLATE
#define DLSA_ABLATE 0
#endif
// bf16 operands (round 2): ONE image Z = bf16(sqrt(w) x), H~ = Z^T Z (positive
// semi-definite by construction, as in the wide fused pass), instead of the
// two images x and w x -- half the image stores and LDS: 9.87 -> 9.37 ms per
// config-2 launch (profiles/r02ac_zimage_ab.txt)

constexpr int tile_I(int t) {
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  return I;
}
constexpr int tile_J(int t) { return t - tile_I(t) * (tile_I(t) + 1) / 2; }

template <int NT, int W_>
struct CG {
  static constexpr int W = W_;                // waves per workgroup (4 or 8)
  static constexpr int RPW = RB / W;          // rows per wave in the row phase
  static constexpr int LPR = 64 / RPW;        // lanes per row in the row phase (8 or 16)
  static constexpr int PMAX = 16 * NT;
  static constexpr int T = NT * (NT + 1) / 2;
  static constexpr int TPW = (T + W - 1) / W;  // tiles per wave (contiguous ranges)
  static constexpr int M = PMAX / LPR;         // features per lane in the row phase
  static constexpr int PAD = 16;
  static constexpr int OBS = RB + 16;           // bf16 image: elements per feature row; 96 B
                                               // (24 dwords) makes the ds_read_b128 operand
                                               // reads (lane groups of MI355X_MICROARCH.md
                                               // "LDS") conflict-free -- 80 B is 2-way
  static constexpr int MAX_PIECES = (RB * PMAX * 8 + 8 + 1023) / 1024;  // coop_slot, unaligned
  // tiles of wave `wid`: t in [wid*TPW, min(T, (wid+1)*TPW))
  static constexpr unsigned col_mask(int wid) {
    unsigned m = 0;
    for (int t = wid * TPW; t < T && t < (wid + 1) * TPW; ++t)
      m |= (1u << tile_I(t)) | (1u << tile_J(t));
    return m;
  }
  static constexpr unsigned row_mask(int wid) {
    unsigned m = 0;
    for (int t = wid * TPW; t < T && t < (wid + 1) * TPW; ++t) m |= 1u << tile_I(t);
    return m;
  }
};

}  // namespace

// Waves per workgroup: 4 for P <= 128 (8 lanes per row in the row phase),
// 8 above (16 lanes per row keeps the per-lane feature count <= 12).
constexpr int coop_waves(int NT) { return NT > 8 ? 8 : 4; }

// The ring slot of one 32-row block, the one definition the kernel, the host's
// slot size (coop_slot_bytes) and the ring depth (set_pass_args) share:
//   [PAD 16 B][npieces KiB pieces of X][PMAX doubles of pad][y][row extras]
// A block's rows are RB p 8 bytes from `start`, DMA'd from start & ~15 on, so
// the pieces cover span = RB p 8 + s bytes, s the largest start & 15 a block of
// the launch can have: 0 when p is even and X is 16-byte aligned (every block
// then starts on a 16-byte boundary), 8 otherwise.  With p % 4 == 0 and s = 0
// the span is a whole number of KiB and no piece reaches into the next block
// (which, streamed non-temporally, would fetch that KiB from HBM twice).
// The pad: the lanes of the padded features f >= P of the block's last row
// read up to PMAX doubles behind the block.  Where the last piece ends with
// the block no DMA ever writes those bytes, and nothing else does but the last
// block's zeroing: they stay the zeros of the ring's initial clear (they are
// multiplied by beta = 0 / w = 0 only, but must be finite).
// Behind the pad the row streams: y and the row extras (glm_row.hpp).
static_assert(RB == kRowStreamRows, "a block's rows are one row stream of the slot");
struct CoopSlot {
  int npieces;  // KiB pieces of X per block
  int rows_off;  // byte offset of y (the row extras follow)
  int bytes;
};
constexpr CoopSlot coop_slot(int NT, int p, int n_extras, bool aligned) {
  const int np = (RB * p * 8 + (aligned ? 0 : 8) + 1023) / 1024;
  const int rows_off = 16 + np * 1024 + 16 * NT * 8;
  return CoopSlot{np, rows_off, rows_off + row_streams_bytes(n_extras)};
}
// Whether every block of a launch over X starts on a 16-byte boundary: decided
// from the X pointer of the fit, by the host (set_pass_args) and by the kernel
// (from PassArgs::X) alike.
__host__ __device__ __forceinline__ bool coop_x_aligned(const double* X, int p) {
  return (p & 1) == 0 && ((uintptr_t)X & 15) == 0;
}
// DMA loads per block of the wave with the most: the pieces, y and the row
// extras dealt round robin over the W waves, each issued once
constexpr int coop_max_loads(int NT, int W, int nld) {
  return (coop_slot(NT, 16 * NT, 0, false).npieces + nld + W - 1) / W;
}

// LDS beyond the ring: w, r of the block [2][RB] fp64, center / 1/scale
// [2][PMAX] fp64, and the bf16 MFMA operand image of the block z = sqrt(w) x,
// [PMAX][RB + 16] bf16 (feature-major, so one lane's 8 consecutive k are one
// 16-byte read).
constexpr int coop_extra_bytes_impl(int NT) {
  return (2 * RB + 2 * 16 * NT) * 8 + 16 * NT * (RB + 16) * 2;
}

// The smallest ring (nslot = 2) of the widest slot of every NT (unaligned), with
// both row extras, fits the LDS share of a workgroup (set_pass_args, fit_fused.hip:
// two workgroups per CU below NT = 8).
constexpr bool coop_ring_fits(int n_extras) {
  for (int NT = 1; NT <= 12; ++NT)
    if (2 * coop_slot(NT, 16 * NT, n_extras, false).bytes + coop_extra_bytes_impl(NT) >
        160 * 1024 / (NT < 8 ? 2 : 1))
      return false;
  return true;
}
static_assert(coop_ring_fits(2), "a two-slot ring with the offset and the weight fits the LDS");

// Tile phase of wave WID for one 32-row block.
template <int NT, int W, int PREC, bool STD, int WID, typename Acc>
__device__ __forceinline__ void tile_phase(Acc (&acc)[(CG<NT, W>::TPW)], const double* xs,
                                           const double* wr, int p, int ic, int lane,
                                           const double* stdv, const __bf16* obx) {
  using G = CG<NT, W>;
  constexpr unsigned CM = G::col_mask(WID);
  constexpr unsigned RM = G::row_mask(WID);
  const int fl = lane & 15, q = lane >> 4;
  const bool icpt_lane = ic && fl == 0;
  const double* xq = xs + q * p + (fl - ic);  // row q of the block, this lane's feature
  static_assert(PREC != PREC_BF16, "bf16 tiles are issued by the kernel body");
  {
    // 8 k-steps of 4 rows: k-step s uses block rows 4s + q (k = q)
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const double ws = wr[4 * s + q];
      double xv[NT], av[NT];
      static_for<NT>([&](auto cI) {
        constexpr int c = decltype(cI)::value;
        if constexpr ((CM >> c) & 1u) {
          double v = xq[4 * s * p + 16 * c];
          if constexpr (STD) v = (v - stdv[16 * c + fl]) * stdv[G::PMAX + 16 * c + fl];
          if (c == 0 && icpt_lane) v = 1.0;
          xv[c] = v;
          if constexpr ((RM >> c) & 1u) av[c] = v * ws;
        }
      });
      static_for<G::TPW>([&](auto iI) {
        constexpr int i = decltype(iI)::value;
        constexpr int t = WID * G::TPW + i;
        if constexpr (t < G::T) {
          constexpr int I = tile_I(t), J = tile_J(t);
          if constexpr (PREC == PREC_F64)
            acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I], xv[J], acc[i], 0, 0, 0);
          else
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)av[I], (float)xv[J], acc[i], 0,
                                                          0, 0);
        }
      });
    }
  }
}

template <int NT, int W, int PREC, bool STD, int WID, typename Acc>
__device__ __forceinline__ void store_tiles(Acc (&acc)[(CG<NT, W>::TPW)], double* sH, int lane) {
  using G = CG<NT, W>;
  const int fl = lane & 15, q = lane >> 4;
  static_for<G::TPW>([&](auto iI) {
    constexpr int i = decltype(iI)::value;
    constexpr int t = WID * G::TPW + i;
    if constexpr (t < G::T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // f64 16x16x4 C/D map: row = (l>>4) + 4*reg; f32 16x16 maps: 4*(l>>4) + reg
        const int row = (PREC == PREC_F64) ? (q + 4 * r) : (4 * q + r);
        sH[t * 256 + row * 16 + fl] = (double)acc[i][r];
      }
    }
  });
}

// Profiling-only A/B (tools/build_variants.sh cmabl; product 0): the CM & 1
// pass skips its per-value max |x| update (the record reads 0).
#ifndef DLSA_CM_ABLATE
#define DLSA_CM_ABLATE 0
#endif
// CM (bits): also record the chunk's per-feature max |x| into a.colmax (1:
// the fit's first full-data bf16 pass) and max |z| (z = sqrt(w) x, the fp32
// value of the bf16 image) into a.zcolmax (2: the bf16 passes of partitions
// near convergence); the Ozaki exact pass takes its digit scales from the
// last records (irls_oz_impl.hpp)
// EX (row extras, EX_* mask): each streams like y, one more load per block,
// placed behind y (RowStreams, glm_row.hpp).
//   EX_OFS (FAMILY_POISSON only): eta = x . theta + a.eta_offset[row]
//   EX_WGT: prior weights omega = a.row_weight[row]: w, r and the row's
//   log-likelihood terms are multiplied by omega once, after mu (so the bf16 /
//   fp32 images are sqrt(omega w) x); CM = 0 only
template <int NT, int W, int PREC, bool STD, int FAM, int CM = 0, int EX = EX_NONE>
__global__ __launch_bounds__(64 * W, (W == 8 || NT < 8) ? 2 : 1)
void irls_coop_kernel(const typename pass_args_of<EX>::type a) {
  using G = CG<NT, W>;
  using Acc = typename std::conditional<PREC == PREC_F64, d4, f4>::type;
  constexpr int RPW = G::RPW, LPR = G::LPR;
  constexpr int M = G::M;
  using RS = RowStreams<EX>;
  static_assert(!RS::OFS || FAM == FAMILY_POISSON, "the offset is the Poisson family's");
  static_assert(!RS::WGT || CM == 0, "no digit-scale records of a weighted pass");
  constexpr int NLD = RS::NLD;                // loads per block beside X: y and the row extras
  static_assert(NLD <= W, "at most one row stream per wave");
  constexpr int MAXL = coop_max_loads(NT, W, NLD);  // a wave's loads per block, at most
  constexpr int MAXW = 4 * MAXL;                    // nslot <= 6
  // a wave has at most nslot - 1 <= 5 blocks of its <= MAXL loads outstanding:
  // within the 6-bit vmcnt (5 x 9 = 45 at NT = 8, 33 + 3 items over 4 waves)
  static_assert(5 * MAXL <= 63, "outstanding loads exceed the vmcnt counter");
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
  const int nslot = a.nslot;
  const CoopSlot sg = coop_slot(NT, p, ex_count(EX), coop_x_aligned(a.X, p));
  const int slot_bytes = sg.bytes;  // == a.slot_bytes (launch_c)
  const int npieces = sg.npieces;
  const int slot_x = sg.rows_off;  // y (then the row extras)
  static_assert(G::PAD == 16, "coop_slot's pad");
  double* wr = (double*)(smem + nslot * slot_bytes);       // [2][RB]: w, r of the block
  double* stdv = wr + 2 * RB;  // [2][PMAX]: center, 1/scale by feature (STD only)
  __bf16* obx = (__bf16*)(stdv + 2 * G::PMAX);  // [2][PMAX][OBS] bf16 operands (PREC_BF16)

  // ---- row-phase constants: lane = (feature group sl, row lane % RPW);
  // lane handles features f = sl + LPR m of its row.  Row-major ring reads of
  // one instruction cover RPW rows x LPR consecutive doubles per half-wave
  // (conflict-free at p = 100), and one feature's RPW rows are written to the
  // bf16 image by RPW consecutive lanes.
  const int sl = lane / RPW;
  const int rB = wid * RPW + lane % RPW;  // block row of this lane in the row phase
  double beta[M], gacc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int f = sl + LPR * m;
    beta[m] = (f < P) ? a.theta[(int64_t)part * P + f] : 0.0;
    gacc[m] = 0.0;
  }
  // re-define beta by an opaque instruction so its loads are waited for here,
  // once: otherwise the compiler's loop-carried wait for them sits inside the
  // block loop as vmcnt(1) and drains the ring
#pragma unroll
  for (int m = 0; m < M; ++m) asm volatile("" : "+v"(beta[m]));
  double llacc = 0.0;
  [[maybe_unused]] double llcacc = 0.0;  // Poisson fp64 pass: -sum lgamma(y + 1)
  // CM: running max of |x| per feature, kept as the high dword of |x| (what
  // the digit exponents read: ozk::xbound sets the low dword to all ones) --
  // 32-bit integer max instead of a v_max_f64 per value, half the registers.
  // No row mask: the rows of a chunk's last block past its end are the next
  // chunk's rows (or the range check's zeros), so the recorded max is an upper
  // bound over the chunk's rows, which is all the digit exponents need (a
  // looser bound only moves the digits down a bit).
  uint32_t cmx[(CM & 1) ? M : 1];
  float zmx[(CM & 2) ? M : 1];  // running max |z| (fp32 image values; rows past the end have w = 0)
#pragma unroll
  for (int m = 0; m < (CM ? M : 1); ++m) {
    if constexpr (CM & 1) cmx[m] = 0u;
    if constexpr (CM & 2) zmx[m] = 0.0f;
  }
  // this wave's tiles (bf16 path).  The last wave's surplus entries (t >= T)
  // name tile T - 1 again: the tile phase runs them like the others, without
  // a branch, into accumulators that store_tiles never writes out
  int tI[G::TPW], tJ[G::TPW];
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) {
    const int t = min(wid * G::TPW + i, G::T - 1);
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    tI[i] = __builtin_amdgcn_readfirstlane(I);
    tJ[i] = __builtin_amdgcn_readfirstlane(t - I * (I + 1) / 2);
  }
  Acc acc[G::TPW];
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) acc[i] = Acc{0, 0, 0, 0};

  // zero the ring once: pads/tails and never-DMA'd bytes must be finite
  for (int o = tid * 16; o < nslot * slot_bytes; o += 64 * W * 16)
    *(uint4*)(smem + o) = make_uint4(0, 0, 0, 0);
  if constexpr (STD) {
    for (int f = tid; f < G::PMAX; f += 64 * W) {
      const int j = f - ic;
      const bool in = j >= 0 && j < p;
      stdv[f] = in ? a.center[j] : 0.0;
      stdv[G::PMAX + f] = in ? 1.0 / a.scale[j] : 1.0;
    }
  }
  __syncthreads();

  // Buffer resources over this chunk's rows (bounds-checked raw buffers: a
  // tail piece past the end of X reads zeros instead of faulting), so a DMA
  // piece is one buffer_load ... lds with a scalar offset -- no per-lane
  // 64-bit address arithmetic.
  const uintptr_t xcb = (uintptr_t)(a.X + row0 * p) & ~(uintptr_t)15;
  const uintptr_t xend = a.x_last16 + 16;
  const __amdgpu_buffer_rsrc_t xr_rsrc = uniform_rsrc(xcb, xend - xcb);
  const int vx = lane * 16, vy = lane * 4;
  // The block's loads are npieces + NLD items -- the X pieces, then y and the
  // row extras -- and wave wid issues items wid, wid + W, ...: each once.  So a
  // wave has nx pieces and at most one row stream (NLD <= W); which one, its
  // resource and its place in the slot are wave-uniform and fixed here, and
  // the block loop runs two counted loops without a branch per item.
  const int nx = __builtin_amdgcn_readfirstlane(wid < npieces ? (npieces - wid + W - 1) / W : 0);
  const int rs = __builtin_amdgcn_readfirstlane((wid + W - npieces % W) % W);  // item npieces + rs
  const int nrs = rs < NLD ? 1 : 0;
  uintptr_t rcb = (uintptr_t)(a.y + row0), rend = a.y_last4 + 4;
  int rs_off = slot_x;
  if constexpr (RS::OFS) {
    if (rs == 1) {
      rcb = (uintptr_t)(a.eta_offset + row0);
      rend = a.o_last4 + 4;
      rs_off = slot_x + RS::OFS_OFF;
    }
  }
  if constexpr (RS::WGT) {
    if (rs == (RS::OFS ? 2 : 1)) {
      rcb = (uintptr_t)(a.row_weight + row0);
      rend = a.w_last4 + 4;
      rs_off = slot_x + RS::WGT_OFF;
    }
  }
  const __amdgpu_buffer_rsrc_t rs_rsrc = uniform_rsrc(rcb, rend - rcb);
  auto issue = [&](int blk) {
    const int bb = blk < nb ? blk : nb - 1;  // tail: harmless re-fetch, fixed counts
    char* sbase = smem + (blk % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)bb * RB) * p);
    const int so = __builtin_amdgcn_readfirstlane((int)((start & ~(uintptr_t)15) - xcb));
    for (int i = 0; i < nx; ++i) {
      const int j = wid + W * i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          xr_rsrc, (lds_void_t*)(sbase + G::PAD + j * 1024), 16, vx, so + j * 1024, 0,
          (PREC == PREC_BF16 && NT == 7) ? DLSA_COOP_NT7_DMA_AUX : DLSA_X_DMA_AUX);
    }
    for (int i = 0; i < nrs; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_rsrc, (lds_void_t*)(sbase + rs_off), 4, vy,
                                               bb * RB * 8, 0, 0);
  };

  // a wave issues its nx + nrs loads per block, in block order: with at most
  // that many per block in flight for the nslot - 2 blocks after b, every
  // load of block b (and before) has landed.  vmcnt counts per wave, so the
  // waves' counts need not be equal
  for (int b = 0; b < nslot - 1; ++b) issue(b);
  const int keep = (nslot - 2) * (nx + nrs);

  for (int b = 0; b < nb; ++b) {
    wait_vmcnt_le<MAXW>(keep);  // this wave's pieces of block b landed
    lds_barrier();              // B1: everyone's pieces landed, block b-1 fully consumed
    issue(b + nslot - 1);

    const char* slot = smem + (b % nslot) * slot_bytes;
    const uintptr_t start = (uintptr_t)(a.X + (row0 + (int64_t)b * RB) * p);
    const double* xs = (const double*)(slot + G::PAD + (start & 15));
    const double* ys = (const double*)(slot + slot_x);
    const int rows_left = nrows - b * RB;
    // The chunk's last block: its rows past the chunk's end, and the PMAX
    // doubles behind the block that the last row's lanes of the padded
    // features f >= P read, are the next chunk's rows (another partition's,
    // possibly non-finite) or the bytes after X up to its 16-byte boundary.
    // They carry w = r = 0 and beta = 0, but 0 * NaN is NaN: zero them in the
    // slot, for the row phase and the tile phase alike.  (No DMA is in flight
    // to this slot: the tail re-fetches go to the other slots.)
    if (__builtin_expect(b == nb - 1, 0)) {  // workgroup-uniform
      double* zs = (double*)(smem + (b % nslot) * slot_bytes + G::PAD + (start & 15));
      zs += rows_left * p;
      const int nz = (RB - rows_left) * p + G::PMAX;
      for (int i = tid; i < nz; i += 64 * W) zs[i] = 0.0;
      lds_barrier();
    }

    // ---- B: row phase ------------------------------------------------------
    if constexpr (DLSA_ABLATE != 3 && DLSA_ABLATE != 4) {
      const bool valid = rB < rows_left;
      const double* xr = xs + rB * p + (sl - ic);
      double xv[M];
      double e0 = 0.0, e1 = 0.0;  // two FMA chains: half the latency of the dot product
#pragma unroll
      for (int m = 0; m < M; ++m) {
        double v = xr[LPR * m];
        if constexpr (STD) v = (v - stdv[sl + LPR * m]) * stdv[G::PMAX + sl + LPR * m];
        if (m == 0 && ic && sl == 0) v = 1.0;
        xv[m] = v;
        if constexpr ((CM & 1) && !DLSA_CM_ABLATE)
          cmx[m] = max(cmx[m], (uint32_t)__double2hiint(v) & 0x7FFFFFFFu);
        if (m & 1)
          e1 = fma(v, beta[m], e1);
        else
          e0 = fma(v, beta[m], e0);
      }
      // bitwise-identical in all lanes of the row
      double e = wv_row_sum<RPW, true>(e0 + e1);
      // the offset once, after the reduction (every lane of the row adds the
      // same value); a padded row's may be the next partition's, even NaN: the
      // selects on `valid` below keep it out of w, r and the log-likelihood
      if constexpr (RS::OFS) e += RS::offset(ys, rB);
      const double yv = ys[rB];
      // the prior weight (RowStreams, glm_row.hpp); 1 folds out of the products
      double om = 1.0;
      if constexpr (RS::WGT) om = valid ? ys[RS::WGT_OFF / 8 + rB] : 0.0;
      double w, r;
      if constexpr (FAM == FAMILY_LOGISTIC && DLSA_ABLATE == 2) {
        w = 0.25;
        r = yv - 0.5 - 0.25 * e;
        if (valid && sl == 0) llacc += e;
      } else if constexpr (FAM == FAMILY_LOGISTIC) {
        const LogisticLink k = logistic_link<RCP_DIV>(e);
        w = k.w;
        r = yv - k.mu;
        if (valid && sl == 0) {
          // exact fp64 in the fp64 pass (its value is returned); fp32 log in
          // the approximate passes, where it only drives step halving
          const double sp = (PREC == PREC_F64) ? log1p(k.ea) : (double)__logf(1.0f + (float)k.ea);
          llacc += om * (yv * e - (fmax(e, 0.0) + sp));
        }
      } else if constexpr (FAM == FAMILY_POISSON) {
        // log link: mu = w = exp(eta).  A padded row's eta is never
        // exponentiated (its w and r are zeroed below either way).  llacc is
        // the constant-free sum y eta - mu in every precision -- the quantity
        // the step halving compares across passes; the constant -lgamma(y + 1)
        // goes to its own sum, in the fp64 pass only (it is published there)
        const double mu = exp(valid ? e : 0.0);
        w = mu;
        r = yv - mu;
        if (valid && sl == 0) {
          llacc += om * (yv * e - mu);
          if constexpr (PREC == PREC_F64)
            if (yv != 0.0 && yv != 1.0) llcacc -= om * lgamma1p(yv);  // 0 at y = 0, 1
        }
      } else {  // gaussian (OLS): mu = eta, w = 1, ll = -rss/2
        w = 1.0;
        r = yv - e;
        if (valid && sl == 0) llacc -= 0.5 * r * r;
      }
      w *= om;  // once, after mu; ahead of the padded rows' zeroing
      r *= om;
      if (!valid) {
        w = 0.0;
        r = 0.0;
      }
#pragma unroll
      for (int m = 0; m < M; ++m) gacc[m] = fma(xv[m], r, gacc[m]);
      if constexpr (PREC != PREC_BF16) {  // the bf16 tiles read the image alone
        if (sl == 0) {
          wr[rB] = w;
          wr[RB + rB] = r;
        }
      }
      if constexpr (PREC == PREC_BF16) {
        // stage the bf16 MFMA operand z = sqrt(w) x once per row; one
        // v_cvt_pk_bf16_f32 converts two of the lane's features
        const float swf = __builtin_sqrtf((float)w);
#pragma unroll
        for (int m = 0; m < M; m += 2) {
          float z0 = (float)xv[m];
          float z1 = m + 1 < M ? (float)xv[m + 1] : 0.0f;
          // opaque: otherwise (bf16)(float)x folds into a direct f64 -> bf16
          // conversion with round-to-odd fix-ups
          asm volatile("" : "+v"(z0), "+v"(z1));
          const f2c pr = {z0 * swf, z1 * swf};
          if constexpr ((CM & 2) != 0) {
            zmx[m] = __builtin_fmaxf(zmx[m], __builtin_fabsf(pr[0]));
            if (m + 1 < M) zmx[m + 1] = __builtin_fmaxf(zmx[m + 1], __builtin_fabsf(pr[1]));
          }
          const bf16x2c pk = __builtin_convertvector(pr, bf16x2c);
          obx[(sl + LPR * m) * G::OBS + rB] = pk[0];
          if (m + 1 < M) obx[(sl + LPR * (m + 1)) * G::OBS + rB] = pk[1];
        }

      }
    }
    lds_barrier();  // B2: w, r (and the bf16 operand images) of all 32 rows visible

    // ---- C: tile phase -----------------------------------------------------
    if constexpr (DLSA_ABLATE != 1 && DLSA_ABLATE != 3) {
      if constexpr (PREC == PREC_BF16) {
        // one code path for every wave: the wave's tile indices are
        // wave-uniform registers (no per-wave copies of the loop body, whose
        // merge would copy the accumulators every block), and no branch per
        // tile: straight-line code, so the operand reads of all the wave's
        // tiles are issued ahead of the MFMAs instead of one LDS round trip
        // per tile -- the tile phase sits in the workgroup's serial chain
        // B1, row phase, B2, tile phase
        const int fl = lane & 15, q = lane >> 4;
        bf16x8 Av[G::TPW], Bv[G::TPW];
#pragma unroll
        for (int i = 0; i < G::TPW; ++i) {
          Av[i] = *(const bf16x8*)(obx + (16 * tI[i] + fl) * G::OBS + 8 * q);
          Bv[i] = *(const bf16x8*)(obx + (16 * tJ[i] + fl) * G::OBS + 8 * q);
        }
#pragma unroll
        for (int i = 0; i < G::TPW; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Av[i], Bv[i], acc[i], 0, 0, 0);
      } else {
        static_for<W>([&](auto wI) {
          constexpr int WID = decltype(wI)::value;
          if (wid == WID) tile_phase<NT, W, PREC, STD, WID>(acc, xs, wr, p, ic, lane, stdv, obx);
        });
      }
    }
  }
  wait_vmcnt<0>();  // drain the tail re-fetches
  __syncthreads();

  // ---- epilogue ------------------------------------------------------------
  double* sH = a.slab_H + (int64_t)chunk * G::T * 256;
  static_for<W>([&](auto wI) {
    constexpr int WID = decltype(wI)::value;
    if (wid == WID) store_tiles<NT, W, PREC, STD, WID>(acc, sH, lane);
  });
  // gradient: sum the row lanes of each feature group (xor 1 .. RPW/2), then the waves
  double* red = (double*)smem;  // ring is no longer needed: [W][PMAX] + [W]
#pragma unroll
  for (int m = 0; m < M; ++m) {
    double v = gacc[m];
#pragma unroll
    for (int o = 1; o < RPW; o <<= 1) v += __shfl_xor(v, o);
    if (lane % RPW == 0) red[wid * G::PMAX + sl + LPR * m] = v;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) llacc += __shfl_xor(llacc, o);
  if (lane == 0) red[W * G::PMAX + wid] = llacc;
  constexpr bool LLC = FAM == FAMILY_POISSON && PREC == PREC_F64;
  if constexpr (LLC) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) llcacc += __shfl_xor(llcacc, o);
    if (lane == 0) red[W * G::PMAX + W + wid] = llcacc;
  }
  __syncthreads();
  for (int f = tid; f < G::PMAX; f += 64 * W) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) s += red[w * G::PMAX + f];
    a.slab_g[(int64_t)chunk * G::PMAX + f] = s;
  }
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < W; ++w) s += red[W * G::PMAX + w];
    a.slab_ll[chunk] = s;
    if constexpr (LLC) {
      double c = 0.0;
#pragma unroll
      for (int w = 0; w < W; ++w) c += red[W * G::PMAX + W + w];
      a.slab_llc[chunk] = c;
    }
  }
  if constexpr (CM) {
    __syncthreads();  // red is reused
    uint32_t* cred = (uint32_t*)smem;  // [2][W][PMAX]: max |x| high dwords, max |z| fp32 bits
#pragma unroll
    for (int m = 0; m < M; ++m) {
      uint32_t v = 0, u = 0;
      if constexpr (CM & 1) v = cmx[m];
      if constexpr (CM & 2) u = __float_as_uint(zmx[m]) & 0x7FFFFFFFu;  // ordered as integers
#pragma unroll
      for (int o = 1; o < RPW; o <<= 1) {
        if constexpr (CM & 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
        if constexpr (CM & 2) u = max(u, (uint32_t)__shfl_xor((int)u, o));
      }
      if (lane % RPW == 0) {
        cred[wid * G::PMAX + sl + LPR * m] = v;
        cred[(W + wid) * G::PMAX + sl + LPR * m] = u;
      }
    }
    __syncthreads();
    // a pass enqueued before the host read the near-switch count records only
    // if that count is > 0 (the running max costs one fp32 max per value)
    const bool zon = (CM & 2) && (a.zrec_gate == nullptr || a.zrec_gate[0] > 0);
    for (int f = tid; f < G::PMAX; f += 64 * W) {
      uint32_t v = 0, u = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        v = max(v, cred[w * G::PMAX + f]);
        u = max(u, cred[(W + w) * G::PMAX + f]);
      }
      if constexpr (CM & 1) a.colmax[(int64_t)chunk * G::PMAX + f] = v;
      if constexpr (CM & 2)
        if (zon) a.zcolmax[(int64_t)chunk * G::PMAX + f] = u;
    }
  }
}

template <int NT, int W, int PREC, bool STD, int FAM, int CM = 0, int EX = EX_NONE>
static hipError_t launch_c(const typename pass_args_of<EX>::type& a, int n_chunks,
                           hipStream_t s) {
  auto kern = irls_coop_kernel<NT, W, PREC, STD, FAM, CM, EX>;
  // the kernel lays its ring out by coop_slot from the same X and p
  if (a.slot_bytes != coop_slot(NT, a.p, ex_count(EX), coop_x_aligned(a.X, a.p)).bytes)
    return hipErrorInvalidValue;
  const size_t lds =
      (size_t)a.nslot * a.slot_bytes + coop_extra_bytes_impl(NT);
  hipError_t e = ensure_max_lds((const void*)kern, 160 * 1024);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(n_chunks), dim3(64 * W), lds, s, a);
  return hipGetLastError();
}

template <int V>
using int_c = std::integral_constant<int, V>;

// The launcher of one (NT, family, row extras): the precision, CM and
// standardisation selection, each arm guarded by the family's rules, so a
// unit instantiates the kernels its families may launch and no other (no CM
// kernel without digit scales, above kOzMaxNT or with weights, one precision
// for a family that does not iterate, an extra only with its array).  A
// kernel takes the slice of `a` its extras need.
template <int NT, int FAM, int EX>
static hipError_t launch_coop_nt(const PassArgsWgt& a, int prec, bool std_, int n_chunks,
                                 hipStream_t s) {
  constexpr FamilyRules R = family_rules(FAM);
  constexpr int W = coop_waves(NT);
  constexpr bool OFS = (EX & EX_OFS) != 0, WGT = (EX & EX_WGT) != 0;
  static_assert(!OFS || R.offset, "an offset kernel of a family without one");
  static_assert(!WGT || R.weights, "a weighted kernel of a family without weights");
  if (!R.iterates && prec != PREC_F64) return hipErrorInvalidValue;
  if ((!R.digit_scales || WGT) && (a.colmax || a.zcolmax)) return hipErrorInvalidValue;
  if (R.sums_ll_const && prec == PREC_F64 && !a.slab_llc) return hipErrorInvalidValue;
  if (OFS && !a.eta_offset) return hipErrorInvalidValue;
  if (WGT && !a.row_weight) return hipErrorInvalidValue;
  const typename pass_args_of<EX>::type& ka = a;
  auto go = [&](auto prec_c, auto cm_c) {
    constexpr int PREC = decltype(prec_c)::value, CM = decltype(cm_c)::value;
    return std_ ? launch_c<NT, W, PREC, true, FAM, CM, EX>(ka, n_chunks, s)
                : launch_c<NT, W, PREC, false, FAM, CM, EX>(ka, n_chunks, s);
  };
  if constexpr (R.iterates) {
    if (prec == PREC_BF16) {
      if constexpr (R.digit_scales && NT <= kOzMaxNT && !WGT) {
        switch ((a.colmax ? 1 : 0) | (a.zcolmax ? 2 : 0)) {
          case 1: return go(int_c<PREC_BF16>{}, int_c<1>{});
          case 2: return go(int_c<PREC_BF16>{}, int_c<2>{});
          case 3: return go(int_c<PREC_BF16>{}, int_c<3>{});
        }
      }
      return go(int_c<PREC_BF16>{}, int_c<0>{});
    }
    if (prec == PREC_F32) return go(int_c<PREC_F32>{}, int_c<0>{});
  }
  return go(int_c<PREC_F64>{}, int_c<0>{});
}

// Entry point of a compilation unit, one line per unit:
//   DLSA_COOP_UNIT(name, family set (an IntList), row extras (EX_* mask), NT...)
// irls_coop.hip lists the units and routes to them.
typedef hipError_t CoopUnitFn(const PassArgsWgt& a, int NT, int prec, bool std_, int family,
                              int n_chunks, hipStream_t s);
#define DLSA_COOP_UNIT(name, FAMS, EX, ...)                                                  \
  hipError_t name(const PassArgsWgt& a, int NT, int prec, bool std_, int family, int n_chunks, \
                  hipStream_t s) {                                                           \
    return unit_dispatch(FAMS{}, IntList<__VA_ARGS__>{}, family, NT, [&](auto fam, auto nt) { \
      return launch_coop_nt<decltype(nt)::value, decltype(fam)::value, (EX)>(a, prec, std_,  \
                                                                             n_chunks, s);   \
    });                                                                                      \
  }

}  // namespace dlsa
