// Poisson instantiations of the per-wave fp64 pass for NT in {1, 2, 3, 4, 5, 6}.
#include "irls_wave_impl.hpp"

namespace dlsa {

DLSA_WAVE_UNIT(launch_irls_wave_pois_g1, FamPoisson, EX_NONE, 1, 2, 3, 4, 5, 6)

}  // namespace dlsa
