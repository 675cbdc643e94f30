// Metric flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensMetricArgs), successive model.
#include "pk_inst_sens.inc"
hipError_t launch_sens_succ(const SensMetricArgs& a, hipStream_t st) { return launch_sens_chain<M_SUCC>(a, st); }
}  // namespace pk
