// Row diagnostics pass: the Poisson instantiations (rows_pass.hip holds the
// logistic ones and the launcher).
#include "rows_pass_impl.hpp"

namespace dlsa {

hipError_t launch_rows_unit_pois(const RowsArgs& a, int n_chunks, hipStream_t s) {
  return launch_rows_family<FAMILY_POISSON>(a, n_chunks, s,
                                            std::make_integer_sequence<int, kScoreMaxNT>{});
}

}  // namespace dlsa
