// Ozaki-scheme exact pass (irls_oz_impl.hpp): host entry point and the table
// of its units; NT = 7 is instantiated in irls_oz_g2.hip so the two halves
// compile in parallel.
#include "irls_oz_impl.hpp"

namespace dlsa {

// entry point, families, row extras (none: no int8 pass with any), first and last NT
#define DLSA_OZ_UNITS(U)                           \
  U(launch_irls_oz_g1, FamLogistic, EX_NONE, 1, 6) \
  U(launch_irls_oz_g2, FamLogistic, EX_NONE, 7, 7)
#define DLSA_DECLARE(name, fams, ex, lo, hi) OzUnitFn name;
#define DLSA_ROW(name, fams, ex, lo, hi) {fams::mask, ex, lo, hi, name},
DLSA_OZ_UNITS(DLSA_DECLARE)
static const UnitRow<OzUnitFn> kOzUnits[] = {DLSA_OZ_UNITS(DLSA_ROW)};

DLSA_OZ_UNIT(launch_irls_oz_g1, 1, 2, 3, 4, 5, 6)

bool oz_applies(int NT, int p) { return NT >= 1 && NT <= kOzMaxNT && ozk::fits(NT, p); }

// Only a family with digit scales: the pass takes them from the records of a
// full-data approximate pass, which a Gaussian fit (one exact pass) never runs
// and a Poisson fit (unbounded weights) does not record.
hipError_t launch_irls_oz(const PassArgs& a, int NT, bool standardize, int family, int n_chunks,
                          hipStream_t s) {
  if (!family_rules(family).digit_scales) return hipErrorInvalidValue;
  if (!oz_applies(NT, a.p) || !a.colmax || !a.zcolmax || !a.theta_rec) return hipErrorInvalidValue;
  OzUnitFn* unit = find_unit(kOzUnits, family, EX_NONE, NT);
  return unit ? unit(a, NT, standardize, family, n_chunks, s) : hipErrorInvalidValue;
}

}  // namespace dlsa

#ifdef DLSA_OZ_PROF
// profiling build only: read and reset this unit's stamp sums (producer wave
// 0: [0] barrier, [1] row phase, [2] digits + gradient; consumer wave 0:
// [8] barrier, [9] DMA issue, [10] MFMA phase, [11] DMA wait)
extern "C" int dlsa_oz_prof_read(unsigned long long* out) { return dlsa::oz_prof_read_impl(out); }
#endif
