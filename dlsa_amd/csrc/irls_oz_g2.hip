// Ozaki-scheme exact pass: NT = 7 (see irls_oz.hip; NT = 8 keeps the fp64
// pass: its level accumulators do not fit the register file).
#include "irls_oz_impl.hpp"

namespace dlsa {

DLSA_OZ_UNIT(launch_irls_oz_g2, 7)

}  // namespace dlsa

#ifdef DLSA_OZ_PROF
// profiling build only: read and reset this unit's stamp sums (producer wave
// 0: [0] barrier, [1] row phase, [2] digits + gradient; consumer wave 0:
// [8] barrier, [9] DMA issue, [10] MFMA phase, [11] DMA wait)
extern "C" int dlsa_oz_prof_read_g2(unsigned long long* out) { return dlsa::oz_prof_read_impl(out); }
#endif
