// Cooperative fused IRLS pass: host entry point and the table of the units
// that hold the kernels (irls_coop_impl.hpp; one DLSA_COOP_UNIT line in each
// irls_coop_*.hip).
#include "irls_coop_impl.hpp"

namespace dlsa {

// entry point, families, offset, first and last NT
#define DLSA_COOP_UNITS(U)                                         \
  U(launch_irls_coop_g1, FamLogisticGaussian, false, 1, 4)         \
  U(launch_irls_coop_g2, FamLogisticGaussian, false, 5, 6)         \
  U(launch_irls_coop_g3, FamLogisticGaussian, false, 7, 7)         \
  U(launch_irls_coop_g4, FamLogisticGaussian, false, 8, 8)         \
  U(launch_irls_coop_g5, FamLogisticGaussian, false, 9, 10)        \
  U(launch_irls_coop_g6, FamLogisticGaussian, false, 11, 12)       \
  U(launch_irls_coop_pois_g1, FamPoisson, false, 1, 4)             \
  U(launch_irls_coop_pois_g2, FamPoisson, false, 5, 8)             \
  U(launch_irls_coop_pois_g3, FamPoisson, false, 9, 12)            \
  U(launch_irls_coop_pois_ofs_g1, FamPoisson, true, 1, 4)          \
  U(launch_irls_coop_pois_ofs_g2, FamPoisson, true, 5, 8)          \
  U(launch_irls_coop_pois_ofs_g3, FamPoisson, true, 9, 12)
#define DLSA_DECLARE(name, fams, ofs, lo, hi) CoopUnitFn name;
#define DLSA_ROW(name, fams, ofs, lo, hi) {fams::mask, ofs, lo, hi, name},
DLSA_COOP_UNITS(DLSA_DECLARE)
static const UnitRow<CoopUnitFn> kCoopUnits[] = {DLSA_COOP_UNITS(DLSA_ROW)};

int coop_slot_bytes(int NT, int p, bool eta_offset) {
  return coop_slot_bytes_impl(NT, p, eta_offset);
}
int coop_extra_bytes(int NT) { return coop_extra_bytes_impl(NT); }

hipError_t launch_irls_coop(const PassArgsOfs& a, int NT, int prec, bool standardize, int family,
                            int n_chunks, hipStream_t s) {
  if (a.eta_offset && !family_rules(family).offset) return hipErrorInvalidValue;
  CoopUnitFn* unit = find_unit(kCoopUnits, family, a.eta_offset != nullptr, NT);
  return unit ? unit(a, NT, prec, standardize, family, n_chunks, s) : hipErrorInvalidValue;
}

}  // namespace dlsa
