// VJP flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensVjpArgs), distributive model.
#include "pk_inst_sens.inc"
hipError_t launch_sens_dist(const SensVjpArgs& a, hipStream_t st) { return launch_sens_chain<M_DIST>(a, st); }
}  // namespace pk
