// Per-wave fp64 IRLS pass: host entry point (kernel in irls_wave_impl.hpp;
// NT = 7, 8 are instantiated in irls_wave_g2.hip so the two halves compile in
// parallel).
#include "irls_wave_impl.hpp"

namespace dlsa {

hipError_t launch_irls_wave_g2(const PassArgs& a, int NT, bool std_, int family, int n_chunks,
                               hipStream_t s);
// the Poisson family's instantiations (irls_wave_pois_g*.hip)
hipError_t launch_irls_wave_pois_g1(const PassArgs& a, int NT, bool std_, int n_chunks,
                                    hipStream_t s);
hipError_t launch_irls_wave_pois_g2(const PassArgs& a, int NT, bool std_, int n_chunks,
                                    hipStream_t s);
// ... with a per-row offset, a.eta_offset set (irls_wave_pois_ofs_g*.hip)
hipError_t launch_irls_wave_pois_ofs_g1(const PassArgsOfs& a, int NT, bool std_, int n_chunks,
                                        hipStream_t s);
hipError_t launch_irls_wave_pois_ofs_g2(const PassArgsOfs& a, int NT, bool std_, int n_chunks,
                                        hipStream_t s);

// (the logistic ring is the larger one; the Poisson pass has its geometry)
int wave_lds_bytes(int NT, int p) {
  return wave_lds_bytes_impl(NT, wave_rb(NT, wave_w(NT), FAMILY_LOGISTIC), p);
}

hipError_t launch_irls_wave(const PassArgsOfs& a, int NT, bool standardize, int family,
                            int n_chunks, hipStream_t s) {
  if (a.eta_offset && family != FAMILY_POISSON) return hipErrorInvalidValue;
  if (family == FAMILY_POISSON && a.eta_offset)
    return NT <= 6 ? launch_irls_wave_pois_ofs_g1(a, NT, standardize, n_chunks, s)
                   : launch_irls_wave_pois_ofs_g2(a, NT, standardize, n_chunks, s);
  if (family == FAMILY_POISSON)
    return NT <= 6 ? launch_irls_wave_pois_g1(a, NT, standardize, n_chunks, s)
                   : launch_irls_wave_pois_g2(a, NT, standardize, n_chunks, s);
  switch (NT) {
    case 1: return launch_wave_nt<1>(a, standardize, family, n_chunks, s);
    case 2: return launch_wave_nt<2>(a, standardize, family, n_chunks, s);
    case 3: return launch_wave_nt<3>(a, standardize, family, n_chunks, s);
    case 4: return launch_wave_nt<4>(a, standardize, family, n_chunks, s);
    case 5: return launch_wave_nt<5>(a, standardize, family, n_chunks, s);
    case 6: return launch_wave_nt<6>(a, standardize, family, n_chunks, s);
    default: return launch_irls_wave_g2(a, NT, standardize, family, n_chunks, s);
  }
}

}  // namespace dlsa
