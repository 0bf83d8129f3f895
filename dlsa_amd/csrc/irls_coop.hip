// Cooperative fused IRLS pass: host entry point and the table of the units
// that hold the kernels (irls_coop_impl.hpp; one DLSA_COOP_UNIT line in each
// irls_coop_*.hip).
#include "irls_coop_impl.hpp"

namespace dlsa {

// entry point, families, row extras, first and last NT
#define DLSA_COOP_UNITS(U)                                                  \
  U(launch_irls_coop_g1, FamLogisticGaussian, EX_NONE, 1, 4)                \
  U(launch_irls_coop_g2, FamLogisticGaussian, EX_NONE, 5, 6)                \
  U(launch_irls_coop_g3, FamLogisticGaussian, EX_NONE, 7, 7)                \
  U(launch_irls_coop_g4, FamLogisticGaussian, EX_NONE, 8, 8)                \
  U(launch_irls_coop_g5, FamLogisticGaussian, EX_NONE, 9, 10)               \
  U(launch_irls_coop_g6, FamLogisticGaussian, EX_NONE, 11, 12)              \
  U(launch_irls_coop_pois_g1, FamPoisson, EX_NONE, 1, 4)                    \
  U(launch_irls_coop_pois_g2, FamPoisson, EX_NONE, 5, 8)                    \
  U(launch_irls_coop_pois_g3, FamPoisson, EX_NONE, 9, 12)                   \
  U(launch_irls_coop_pois_ofs_g1, FamPoisson, EX_OFS, 1, 4)                 \
  U(launch_irls_coop_pois_ofs_g2, FamPoisson, EX_OFS, 5, 8)                 \
  U(launch_irls_coop_pois_ofs_g3, FamPoisson, EX_OFS, 9, 12)                \
  U(launch_irls_coop_wgt_g1, FamLogistic, EX_WGT, 1, 4)                     \
  U(launch_irls_coop_wgt_g2, FamLogistic, EX_WGT, 5, 8)                     \
  U(launch_irls_coop_wgt_g3, FamLogistic, EX_WGT, 9, 12)                    \
  U(launch_irls_coop_pois_wgt_g1, FamPoisson, EX_WGT, 1, 4)                 \
  U(launch_irls_coop_pois_wgt_g2, FamPoisson, EX_WGT, 5, 8)                 \
  U(launch_irls_coop_pois_wgt_g3, FamPoisson, EX_WGT, 9, 12)                \
  U(launch_irls_coop_pois_ofs_wgt_g1, FamPoisson, EX_OFS | EX_WGT, 1, 4)    \
  U(launch_irls_coop_pois_ofs_wgt_g2, FamPoisson, EX_OFS | EX_WGT, 5, 8)    \
  U(launch_irls_coop_pois_ofs_wgt_g3, FamPoisson, EX_OFS | EX_WGT, 9, 12)
#define DLSA_DECLARE(name, fams, ex, lo, hi) CoopUnitFn name;
#define DLSA_ROW(name, fams, ex, lo, hi) {fams::mask, ex, lo, hi, name},
DLSA_COOP_UNITS(DLSA_DECLARE)
static const UnitRow<CoopUnitFn> kCoopUnits[] = {DLSA_COOP_UNITS(DLSA_ROW)};

int coop_slot_bytes(int NT, const double* X, int p, int n_extras) {
  return coop_slot(NT, p, n_extras, coop_x_aligned(X, p)).bytes;
}
int coop_extra_bytes(int NT) { return coop_extra_bytes_impl(NT); }

hipError_t launch_irls_coop(const PassArgsWgt& a, int NT, int prec, bool standardize, int family,
                            int n_chunks, hipStream_t s) {
  if (a.eta_offset && !family_rules(family).offset) return hipErrorInvalidValue;
  if (a.row_weight && !family_rules(family).weights) return hipErrorInvalidValue;
  CoopUnitFn* unit = find_unit(kCoopUnits, family, pass_extras(a), NT);
  return unit ? unit(a, NT, prec, standardize, family, n_chunks, s) : hipErrorInvalidValue;
}

}  // namespace dlsa
