// Score outer-product pass on the categorical-code layout: per partition k, at
// its coefficient vector beta_k, the weighted Gram G_k = sum_i d_i z_i z_i^T
// and the score g_k = sum_i s_i z_i of the dummy-expanded rows z_i, with
// s_i = omega_i (y_i - mu_i) and d_i = s_i^2 (GRAM_SCORE, the meat of the
// sandwich covariance) or omega_i w_i (GRAM_INFORMATION) -- what
// score_pass_impl.hpp computes on the dense layout, at 8 q + F + 8 bytes per
// row (plus 8 per row extra) instead of 8 P.
//
// The pass is the categorical Newton pass (cat_pass_impl.hpp) in a gram row
// mode: (w, res) := (d, s) after the link, the histograms, the fold factor,
// the pair cells and the slab epilogue as they are.  The gram kernels are
// instantiated in units of their own (cat_gram_*.hip: logistic none / weighted,
// Poisson none / ofs / wgt / both, each for the two kinds); gram_cat.hip holds
// the routing, the two small kernels below it and the entry point.
//
// Grids.  The fit sizes its fixed-point grids from bounds valid for a whole
// Newton trajectory (fit_cat.hip cat_grids; cat_pass_pois.hip's A(theta)).
// Here beta_k is an input, so a measuring sweep over the same rows
// (cat_gram_bounds_kernel) takes, per chunk, the largest |d|, |s| and
// |d x~_j| (x~ the standardised numeric column j) of the terms themselves, the
// count of codes >= levels[f] and a flag for a term that is not finite, and a
// grid kernel (one wave per partition) writes
//   hscale[k][slot] = 2^floor(60 - log2(B R)),   clamped to 2^+-900,
// B the measured maximum of the slot's term over the partition's chunks (slot 0:
// d and the pair cells, 1: s, 2 + j: d x~_j; B = 0 gives grid 1) and R =
// max(rows of the largest chunk, 1024) as in cat_grids.  The sweep forms eta
// in its own summation order, so the two etas of a row differ by a few ulps
// of eta, mu by about |eta| eps relative (Poisson: mu = exp(eta)) and s^2 by
// twice that -- at most 2e-13 for the |eta| < 710 a finite mu allows.  A term
// of the pass can exceed B by that factor: B R 2^E <= 2^60 leaves every term
// below 2^50 (1 + 2e-13), inside the 2^51 the rounding trick of fx_term needs
// (a factor 2 of room), and a bin below 2^60 (1 + 2e-13) of int64's 2^63.
// A partition with the flag gets hscale[0] = NaN: the pass writes NaN into
// every slab value of its chunks, so its gram and score come out all NaN and
// no other partition is touched -- the dense entry's rule for a non-finite
// omega, y or offset.
//
// Error.  Each histogram term is rounded once to its grid step h = 2^-E <=
// 2 B R 2^-60, an error of at most h / 2 per term; the integer sums and the
// sums over chunks of exactly representable multiples of h are exact up to
// the final roundings to fp64.  So an entry of a dummy row or column of
// partition k (n_k rows) is within n_k R 2^-60 B of the fp64-exact sum in the
// worst case (B of its slot: d for dummy x dummy, d x~_j for dummy x numeric
// j, s for the score's dummy part; with an intercept folded into the
// histograms, EX, its row too).  The numeric x numeric block and the numeric
// part of the score are fp64 register sums with fixed-order reductions.
#pragma once

#include "cat_pass_impl.hpp"

namespace dlsa {

// One unit per (family, row-extras mask, kind): its gram kernels -- the pass
// kernels of cat_pass_impl.hpp with the row mode in RX, through the Newton
// pass's own launch chain (the same buckets, thread counts, exact-bucket rule
// and LDS size) -- behind this entry point.  a.theta is [K, P]; a.hscale the
// measured grids.
template <int FAM, int RX, int MODE>
hipError_t launch_cat_gram_unit(const typename cat_pass_args_of<FAM, RX>::type& a,
                                bool standardize, int n_chunks, hipStream_t s);
#define DLSA_CAT_GRAM_UNIT(FAM, RX, MODE)                                                  \
  template <>                                                                              \
  hipError_t launch_cat_gram_unit<FAM, RX, MODE>(                                          \
      const typename cat_pass_args_of<FAM, RX>::type& a, bool standardize, int n_chunks,   \
      hipStream_t s) {                                                                     \
    return launch_cat_pass_t<FAM, cat_rx(RX, MODE)>(a, standardize, n_chunks, s);          \
  }

// Arguments of the measuring sweep (gram_cat.hip).  The row extras and the
// standardisation are run-time nullable pointers; partition k reads its
// coefficients at betas + k beta_part_stride (0 or P).
struct CatGramBoundsArgs {
  const double* Xn;
  const uint8_t* codes;
  const double* y;
  const double* eta_offset;
  const double* row_weight;
  const int64_t* chunk_row0;
  const int32_t* chunk_rows;
  const int32_t* chunk_part;
  const double* center;
  const double* scale;
  const double* betas;
  int64_t beta_part_stride;
  // outputs, cleared by the launcher: the maxima as ordered bits of
  // non-negative doubles [n_chunks][kCatQMax + 2] (slot 0 |d|, 1 |s|, 2 + j
  // |d x~_j|), the codes >= levels[f] [n_chunks], the not-finite flag [n_chunks]
  unsigned long long* bmax;
  int32_t* bad;
  int32_t* nonfinite;
  int32_t q, F, P, intercept, kind;
  int32_t levels[kCatMaxFactors];
  int32_t doff[kCatMaxFactors];  // parameter index of factor f's first dummy
};
hipError_t launch_cat_gram_bounds(const CatGramBoundsArgs& a, int family, int n_chunks,
                                  hipStream_t s);
// hscale [K][kCatQMax + 2] from the sweep's per-chunk maxima; rmax: the most
// rows of a chunk, at least 1024
hipError_t launch_cat_gram_grid(const CatGramBoundsArgs& a, const int32_t* pcb, int K,
                                double rmax, double* hscale, hipStream_t s);
// the gram pass of (family, a.eta_offset, a.row_weight, kind): each kernel is
// handed the slice of CatArgsPois it takes
hipError_t launch_cat_gram(const CatArgsPois& a, int family, int kind, bool standardize,
                           int n_chunks, hipStream_t s);

}  // namespace dlsa
