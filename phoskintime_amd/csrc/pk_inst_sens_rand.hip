// Plain flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensArgs) for the random model, n <= 5, and what the
// dispatch of all three flavours (launch_sens_any, pk_inst_sens.inc) asks: which sizes have a kernel, and which of them the rows kernel takes.
#include "pk_env.hpp"
#include "pk_inst_sens.inc"

bool sens_available(int model, int n_sites) {
  if (model == M_RAND) return n_sites <= 7;
  return n_sites <= 62;
}

// true where the rows-per-lane kernel (pk_sens_rows.hpp) takes a chain model: the one place that reads the switches, for every flavour
bool sens_takes_rows(int model, int n_sites) {
  // PK_SENS_ROWS=1: the rows-per-lane kernel at every size -- the A/B switch the tests use to hold the two kernels to agreement
  const int rows_env = env().sens_rows, rows_min_env = env().sens_rows_min;
  // PK_SENS_ROWS_MIN (dev): smallest size the rows-per-lane kernel takes by default
  // [r3] measured crossover (tools/gpu_sens_one.py, B = 32 768, column kernel vs rows kernel): distmod n = 9: 4.6 vs 6.4 ms, n = 10: 7.1 vs
  // 6.5, n = 14: 7.2 vs 4.3 (B = 16 384);  succmod n = 4: 1.5 vs 3.1, n = 6: 5.0 vs 4.6, n = 10: 8.5 vs 6.2, n = 14: 8.1 vs 4.7 (B = 16 384)
  const int rows_min = rows_min_env > 0 ? rows_min_env : (model == M_DIST ? 10 : 6);
  return model != M_RAND && (n_sites > 14 || rows_env == 1 || (rows_env != 2 && n_sites >= rows_min));
}

hipError_t launch_sens(const SensArgs& a, int model, hipStream_t st) { return launch_sens_any(a, model, st); }

}  // namespace pk
