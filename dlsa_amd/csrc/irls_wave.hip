// Per-wave fp64 IRLS pass: host entry point and the table of the units that
// hold the kernels (irls_wave_impl.hpp; one DLSA_WAVE_UNIT line each: NT 1..6
// of the logistic and Gaussian families here, the others in irls_wave_*.hip,
// so they compile in parallel).
#include "irls_wave_impl.hpp"

namespace dlsa {

// entry point, families, row extras, first and last NT
#define DLSA_WAVE_UNITS(U)                                                \
  U(launch_irls_wave_g1, FamLogisticGaussian, EX_NONE, 1, 6)              \
  U(launch_irls_wave_g2, FamLogisticGaussian, EX_NONE, 7, 8)              \
  U(launch_irls_wave_pois_g1, FamPoisson, EX_NONE, 1, 6)                  \
  U(launch_irls_wave_pois_g2, FamPoisson, EX_NONE, 7, 8)                  \
  U(launch_irls_wave_pois_ofs_g1, FamPoisson, EX_OFS, 1, 6)               \
  U(launch_irls_wave_pois_ofs_g2, FamPoisson, EX_OFS, 7, 8)               \
  U(launch_irls_wave_wgt_g1, FamLogistic, EX_WGT, 1, 6)                   \
  U(launch_irls_wave_wgt_g2, FamLogistic, EX_WGT, 7, 8)                   \
  U(launch_irls_wave_pois_wgt_g1, FamPoisson, EX_WGT, 1, 6)               \
  U(launch_irls_wave_pois_wgt_g2, FamPoisson, EX_WGT, 7, 8)               \
  U(launch_irls_wave_pois_ofs_wgt_g1, FamPoisson, EX_OFS | EX_WGT, 1, 6)  \
  U(launch_irls_wave_pois_ofs_wgt_g2, FamPoisson, EX_OFS | EX_WGT, 7, 8)
#define DLSA_DECLARE(name, fams, ex, lo, hi) WaveUnitFn name;
#define DLSA_ROW(name, fams, ex, lo, hi) {fams::mask, ex, lo, hi, name},
DLSA_WAVE_UNITS(DLSA_DECLARE)
static const UnitRow<WaveUnitFn> kWaveUnits[] = {DLSA_WAVE_UNITS(DLSA_ROW)};

DLSA_WAVE_UNIT(launch_irls_wave_g1, FamLogisticGaussian, EX_NONE, 1, 2, 3, 4, 5, 6)

// (the logistic ring is the larger one; the Poisson pass has its geometry)
int wave_lds_bytes(int NT, int p) {
  return wave_lds_bytes_impl(NT, wave_rb(NT, wave_w(NT), FAMILY_LOGISTIC), p);
}

hipError_t launch_irls_wave(const PassArgsWgt& a, int NT, bool standardize, int family,
                            int n_chunks, hipStream_t s) {
  if (a.eta_offset && !family_rules(family).offset) return hipErrorInvalidValue;
  if (a.row_weight && !family_rules(family).weights) return hipErrorInvalidValue;
  WaveUnitFn* unit = find_unit(kWaveUnits, family, pass_extras(a), NT);
  return unit ? unit(a, NT, standardize, family, n_chunks, s) : hipErrorInvalidValue;
}

}  // namespace dlsa
