// Poisson instantiations of the cooperative pass with a per-row offset
// (eta = x . theta + eta_offset) for NT in {9, 10, 11, 12}.
#include "irls_coop_impl.hpp"

namespace dlsa {

hipError_t launch_irls_coop_pois_ofs_g3(const PassArgsOfs& a, int NT, int prec, bool std_,
                                         int n_chunks, hipStream_t s) {
  switch (NT) {
    case 9: return launch_coop_poisson_nt<9, true>(a, prec, std_, n_chunks, s);
    case 10: return launch_coop_poisson_nt<10, true>(a, prec, std_, n_chunks, s);
    case 11: return launch_coop_poisson_nt<11, true>(a, prec, std_, n_chunks, s);
    case 12: return launch_coop_poisson_nt<12, true>(a, prec, std_, n_chunks, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dlsa
