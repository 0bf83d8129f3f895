// Poisson instantiations of the per-wave fp64 pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {7, 8}.
#include "irls_wave_impl.hpp"

namespace dlsa {

hipError_t launch_irls_wave_pois_ofs_g2(const PassArgsOfs& a, int NT, bool std_, int n_chunks,
                                         hipStream_t s) {
  switch (NT) {
    case 7: return launch_wave_poisson_nt<7, true>(a, std_, n_chunks, s);
    case 8: return launch_wave_poisson_nt<8, true>(a, std_, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
