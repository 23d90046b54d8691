// agx_cost_pairs.hip -- translation unit of the wide-cost-set kernels (agx_cost_pairs.hpp), linked into libagimus_hip.so next
// to the per-capacity units of agimus_hip.hip, which call the two launchers below.
#include <hip/hip_runtime.h>

#include "agx_cost_pairs.hpp"

extern "C" {

// k_cost_pairs<7, dest> on a grid of 8 lanes per node; returns the hipError_t of the launch.  obs: null, or the device table of
// agx_ocp_set_obstacle_placements (agx::ObstaclePlacements): the instantiations that read it
int agx_cost_pairs_launch(int dest, void *stream, long long nodes, const DevModel *m, const DevOcp *o, const DevCostWide *w, const double *dts,
                          const double *xs, const RefView *rv, double *out, double *auxs, const DevState *st, int phase, int sel, int which,
                          const void *obs) {
  const dim3 grid((unsigned)((nodes * 8 + 63) / 64)), blk(64);
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto... src) {  // src: nothing, or the table behind the template pack it names
    auto to = [&](auto DESTc) {
      hipLaunchKernelGGL((agx::k_cost_pairs<7, decltype(DESTc)::value, std::remove_const_t<std::remove_pointer_t<decltype(src)>>...>), grid, blk, 0, s,
                         m, o, w, dts, xs, *rv, out, auxs, st, phase, sel, which, src...);
    };
    if (dest == agx::kPairsToQp) to(std::integral_constant<int, agx::kPairsToQp>());
    else if (dest == agx::kPairsToCanonical) to(std::integral_constant<int, agx::kPairsToCanonical>());
    else if (dest == agx::kPairsItems) to(std::integral_constant<int, agx::kPairsItems>());
    else to(std::integral_constant<int, agx::kPairsDistance>());
  };
  if (obs) launch((const agx::ObstaclePlacements *)obs); else launch();
  return (int)hipGetLastError();
}

int agx_cost_pairs_fill_launch(void *stream, const DevCostWide *w, const double *gw_item, double *traj, long long units, int stride) {
  hipLaunchKernelGGL(agx::k_cost_pairs_fill, dim3((unsigned)((units * 2 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, gw_item, traj, units, stride);
  return (int)hipGetLastError();
}

// k_cost_pairs_fill_ring for the chunk a stream append adds (see the kernel)
int agx_cost_pairs_fill_ring_launch(void *stream, const DevCostWide *w, const double *gw_item, double *traj, int B, int m_new, int end, int cap,
                                    int mirror, int stride) {
  const long long n = (long long)B * m_new * 2;
  hipLaunchKernelGGL(agx::k_cost_pairs_fill_ring, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, gw_item, traj, B, m_new,
                     end, cap, mirror, stride);
  return (int)hipGetLastError();
}

}  // extern "C"
