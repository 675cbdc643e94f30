// Metric flavour of the rows-per-lane forward-sensitivity kernel (pk_sens_rows.hpp, SensMetricArgs), distributive model.
#include "pk_sens_rows.hpp"
#include "pk_launch.hpp"
namespace pk {
hipError_t launch_sens_rows_dist(const SensMetricArgs& a, hipStream_t st) { return launch_sens_rows_model<M_DIST>(a, st); }
}  // namespace pk
