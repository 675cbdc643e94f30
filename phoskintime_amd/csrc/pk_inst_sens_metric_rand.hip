// Metric flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensMetricArgs) for the random model, n <= 5, and the
// flavour's entry into the dispatch: the same kernel per (model, n_sites) as launch_sens takes.
#include "pk_inst_sens.inc"
hipError_t launch_sens_metric(const SensMetricArgs& a, int model, hipStream_t st) { return launch_sens_any(a, model, st); }
}  // namespace pk
