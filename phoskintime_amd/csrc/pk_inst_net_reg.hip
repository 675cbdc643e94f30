// Instantiations + launcher of the register-resident order-3 network integrator (pk_network_solve_reg.hpp: topologies 0 / 1 / 4, site
// classes 4 / 6 / 8; pk_network_solve_reg2.hpp: combinatorial, 2 or 3 sites).
#include "pk_network_solve_reg2.hpp"

namespace pk {

void launch_net_reg(const NetDev& n, const NetSolveArgs& a, int max_sites, long long B, int threads, size_t lds, hipStream_t st) {
#define PK_REG_LAUNCH(K) hipLaunchKernelGGL((K), dim3((unsigned)B), dim3(threads), lds, st, n, a)
  if (n.model == 2) {
    if (max_sites <= 2) PK_REG_LAUNCH(net_solve_reg2_kernel<2>); else PK_REG_LAUNCH(net_solve_reg2_kernel<3>);
    return;
  }
#define PK_REG(MS)                                                                                                                   \
  do {                                                                                                                               \
    if (n.model == 0) PK_REG_LAUNCH((net_solve_reg_kernel<0, MS>)); else if (n.model == 1) PK_REG_LAUNCH((net_solve_reg_kernel<1, MS>)); \
    else PK_REG_LAUNCH((net_solve_reg_kernel<4, MS>));                                                                                \
  } while (0)
  if (max_sites <= 4) PK_REG(4); else if (max_sites <= 6) PK_REG(6); else PK_REG(8);
#undef PK_REG
#undef PK_REG_LAUNCH
}

}  // namespace pk
