// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {5, 6, 7, 8}.
#include "irls_coop_impl.hpp"

namespace dlsa {

hipError_t launch_irls_coop_pois_ofs_g2(const PassArgsOfs& a, int NT, int prec, bool std_,
                                         int n_chunks, hipStream_t s) {
  switch (NT) {
    case 5: return launch_coop_poisson_nt<5, true>(a, prec, std_, n_chunks, s);
    case 6: return launch_coop_poisson_nt<6, true>(a, prec, std_, n_chunks, s);
    case 7: return launch_coop_poisson_nt<7, true>(a, prec, std_, n_chunks, s);
    case 8: return launch_coop_poisson_nt<8, true>(a, prec, std_, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
