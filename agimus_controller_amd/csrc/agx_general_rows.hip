// agx_general_rows.hip -- translation unit of the general-cost-row kernels of large models (agx_general_rows.hpp), linked into
// libagimus_hip.so next to the per-capacity units of agimus_hip.hip; the unit of the capacities 16 / 30 / 32 calls the two
// launchers below.  It is compiled with that unit's AGX_GROUP (DevOcp ends in the constraint tables, sized per group).
#define agx agx_general_rows  // the shared headers once more, in a namespace of this unit
#include <hip/hip_runtime.h>

#include <type_traits>

#include "agx_general_rows.hpp"

extern "C" {

// k_general_rows_wg<nv, prismatic, dest> on `units` workgroups (B T + B: every node, B T: the running nodes); nv: a capacity of
// the workgroup path.  Returns the hipError_t of the launch, -1 without an instantiation for nv.
int agx_general_rows_launch(int dest, void *stream, int nv, int prismatic, long long units, const DevModel *m, const DevOcp *o, const double *dts,
                            const double *xs, const double *us, const RefView *rv, double *out0, double *out1, double *out2, const DevState *st,
                            int phase, int only, int R) {
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto NVc, auto PRc, auto DESTc) {
    hipLaunchKernelGGL((agx::k_general_rows_wg<decltype(NVc)::value, decltype(PRc)::value, decltype(DESTc)::value>), dim3((unsigned)units), dim3(256), 0,
                       s, m, o, dts, xs, us, *rv, out0, out1, out2, st, phase, only, R);
  };
  auto by_dest = [&](auto NVc, auto PRc) {
    if (dest == agx::kGenToQp) launch(NVc, PRc, std::integral_constant<int, agx::kGenToQp>());
    else if (dest == agx::kGenToCanonical) launch(NVc, PRc, std::integral_constant<int, agx::kGenToCanonical>());
    else launch(NVc, PRc, std::integral_constant<int, agx::kGenItems>());
  };
  auto by_joint = [&](auto NVc) {
    if (prismatic) by_dest(NVc, std::true_type()); else by_dest(NVc, std::false_type());
  };
  switch (nv) {
    case 16: by_joint(std::integral_constant<int, 16>()); break;
    case 30: by_joint(std::integral_constant<int, 30>()); break;
    case 32: by_joint(std::integral_constant<int, 32>()); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

// k_node_kkt_big_gen<nv> on the grid of k_node_kkt_big (two nodes per wave)
int agx_general_kkt_launch(void *stream, int nv, long long nodes, const DevOcp *o, const double *qts, const double *auxs, const double *auxg,
                           const double *dxs, const double *wss, double *dus, double *nodestat, const DevState *st) {
  const dim3 grid((unsigned)((nodes + 1) / 2)), blk(64);
  hipStream_t s = (hipStream_t)stream;
  switch (nv) {
    case 16: hipLaunchKernelGGL((agx::k_node_kkt_big_gen<16>), grid, blk, 0, s, o, qts, auxs, auxg, dxs, wss, dus, nodestat, st); break;
    case 30: hipLaunchKernelGGL((agx::k_node_kkt_big_gen<30>), grid, blk, 0, s, o, qts, auxs, auxg, dxs, wss, dus, nodestat, st); break;
    case 32: hipLaunchKernelGGL((agx::k_node_kkt_big_gen<32>), grid, blk, 0, s, o, qts, auxs, auxg, dxs, wss, dus, nodestat, st); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
