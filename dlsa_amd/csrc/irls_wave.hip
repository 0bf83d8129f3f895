// Per-wave fp64 IRLS pass: host entry point and the table of the units that
// hold the kernels (irls_wave_impl.hpp; one DLSA_WAVE_UNIT line each: NT 1..6
// of the logistic and Gaussian families here, the others in irls_wave_*.hip,
// so they compile in parallel).
#include "irls_wave_impl.hpp"

namespace dlsa {

// entry point, families, offset, first and last NT
#define DLSA_WAVE_UNITS(U)                                     \
  U(launch_irls_wave_g1, FamLogisticGaussian, false, 1, 6)     \
  U(launch_irls_wave_g2, FamLogisticGaussian, false, 7, 8)     \
  U(launch_irls_wave_pois_g1, FamPoisson, false, 1, 6)         \
  U(launch_irls_wave_pois_g2, FamPoisson, false, 7, 8)         \
  U(launch_irls_wave_pois_ofs_g1, FamPoisson, true, 1, 6)      \
  U(launch_irls_wave_pois_ofs_g2, FamPoisson, true, 7, 8)
#define DLSA_DECLARE(name, fams, ofs, lo, hi) WaveUnitFn name;
#define DLSA_ROW(name, fams, ofs, lo, hi) {fams::mask, ofs, lo, hi, name},
DLSA_WAVE_UNITS(DLSA_DECLARE)
static const UnitRow<WaveUnitFn> kWaveUnits[] = {DLSA_WAVE_UNITS(DLSA_ROW)};

DLSA_WAVE_UNIT(launch_irls_wave_g1, FamLogisticGaussian, false, 1, 2, 3, 4, 5, 6)

// (the logistic ring is the larger one; the Poisson pass has its geometry)
int wave_lds_bytes(int NT, int p) {
  return wave_lds_bytes_impl(NT, wave_rb(NT, wave_w(NT), FAMILY_LOGISTIC), p);
}

hipError_t launch_irls_wave(const PassArgsOfs& a, int NT, bool standardize, int family,
                            int n_chunks, hipStream_t s) {
  if (a.eta_offset && !family_rules(family).offset) return hipErrorInvalidValue;
  WaveUnitFn* unit = find_unit(kWaveUnits, family, a.eta_offset != nullptr, NT);
  return unit ? unit(a, NT, standardize, family, n_chunks, s) : hipErrorInvalidValue;
}

}  // namespace dlsa
