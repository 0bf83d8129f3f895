// Poisson instantiations of the per-wave fp64 pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {1, 2, 3, 4, 5, 6}.
#include "irls_wave_impl.hpp"

namespace dlsa {

hipError_t launch_irls_wave_pois_ofs_g1(const PassArgsOfs& a, int NT, bool std_, int n_chunks,
                                         hipStream_t s) {
  switch (NT) {
    case 1: return launch_wave_poisson_nt<1, true>(a, std_, n_chunks, s);
    case 2: return launch_wave_poisson_nt<2, true>(a, std_, n_chunks, s);
    case 3: return launch_wave_poisson_nt<3, true>(a, std_, n_chunks, s);
    case 4: return launch_wave_poisson_nt<4, true>(a, std_, n_chunks, s);
    case 5: return launch_wave_poisson_nt<5, true>(a, std_, n_chunks, s);
    case 6: return launch_wave_poisson_nt<6, true>(a, std_, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
