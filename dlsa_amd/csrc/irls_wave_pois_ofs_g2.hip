// Poisson instantiations of the per-wave fp64 pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {7, 8}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_pois_ofs_g2, FamPoisson, EX_OFS, 7, 8)

}  // namespace dlsa
