// Score outer-product pass: the Poisson instantiations (score_pass.hip holds
// the logistic ones, the launcher and the reductions).
#include "score_pass_impl.hpp"

namespace dlsa {

hipError_t launch_score_unit_pois(const GramArgs& a, int n_chunks, hipStream_t s) {
  return launch_score_family<FAMILY_POISSON>(a, n_chunks, s,
                                             std::make_integer_sequence<int, kScoreMaxNT>{});
}

}  // namespace dlsa
