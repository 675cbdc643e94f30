// Metric flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensMetricArgs), distributive model.
#include "pk_inst_sens.inc"
hipError_t launch_sens_dist(const SensMetricArgs& a, hipStream_t st) { return launch_sens_chain<M_DIST>(a, st); }
}  // namespace pk
