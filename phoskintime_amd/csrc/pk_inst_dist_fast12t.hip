// The traced build of the benchmark's distmod kernel (pk_dist_fast.hpp, TRACE = 1: 4 x 8 resident, parked, one wave per workgroup,
// DistSolSum) in a translation unit of its own, with the device global that carries its record buffer.  Selected by PK_DIST_TRACE=1
// (launch_dist_fast12, pk_inst_dist_fast12.hip); tools/dist_wave_timeline.py reads the records.
#include "pk_dist_fast12.hpp"

namespace pk {

__device__ DistTraceBuf g_dist_trace = {nullptr, 0};
template <> struct DistTrace<1> {
  static __device__ __forceinline__ DistTraceBuf get() { return g_dist_trace; }
};

void launch_dist_fast12_traced(const SolveArgs& a, hipStream_t st) { launch_cfg<4, 8, true, 64, DistSolSum, true, 1>(a, st); }

// synchronous: the records of a launch are read after the caller's own synchronisation, and a launch sees the buffer set before it
hipError_t dist_trace_set(void* records, long long capacity) {
  const DistTraceBuf b = {(DistTraceRec*)records, records ? capacity : 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_dist_trace), &b, sizeof(b));
}

}  // namespace pk
