// The resident half of the LRP12 launch table of the distributive-model throughput kernel (pk_dist_fast12.hpp; resident layout:
// pk_dist_fast.hpp, R and P in slots 0 and 1 of the G x RPL lane layout, nothing shadowed), a translation unit of its own so that the
// two halves of the table compile side by side.  launch_dist_fast12 (pk_inst_dist_fast12.hip) calls it for the sizes that fit.
#include "pk_dist_fast12.hpp"

namespace pk {

void launch_dist_fast12_resident(const SolveArgs& a, bool wg256, hipStream_t st) { launch_table12<true>(a, wg256, st); }

}  // namespace pk
