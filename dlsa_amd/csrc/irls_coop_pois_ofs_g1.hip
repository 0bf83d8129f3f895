// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {1, 2, 3, 4}.
#include "irls_coop_impl.hpp"

namespace dlsa {

hipError_t launch_irls_coop_pois_ofs_g1(const PassArgsOfs& a, int NT, int prec, bool std_,
                                         int n_chunks, hipStream_t s) {
  switch (NT) {
    case 1: return launch_coop_poisson_nt<1, true>(a, prec, std_, n_chunks, s);
    case 2: return launch_coop_poisson_nt<2, true>(a, prec, std_, n_chunks, s);
    case 3: return launch_coop_poisson_nt<3, true>(a, prec, std_, n_chunks, s);
    case 4: return launch_coop_poisson_nt<4, true>(a, prec, std_, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
