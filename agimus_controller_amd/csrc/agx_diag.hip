// agx_diag.hip -- translation unit of the diagnostics kernels, linked into libagimus_hip.so next to the per-capacity units of
// agimus_hip.hip, which call the launchers below:
//   k_iter_log    the per-iteration solver log (agx_ocp_iter_log): a copy of DevState fields into records, launched only while
//                 the log is on;
//   k_item_costs  value and gradient of every cost item of every node on its own (agx_ocp_item_costs), built on node_costs /
//                 node_costs_general, the device functions behind k_calc_diff and k_residuals.
// A unit of its own for the reason agx_cost_pairs.hip is one: kernels instantiated next to the solver's change the register
// allocation of unrelated kernels there.  It is compiled once, for every capacity, and therefore touches nothing whose layout
// depends on the capacity group (DevOcp ends in the constraint tables, sized per group): it is handed the row tables, T and B.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "agx_tiles.hpp"

namespace agx {

// One thread per instance.  An instance takes part in SQP iteration `it` when the head of that iteration has worked on it
// (DevState::dir_iter == it; an instance that finished earlier keeps an older value).
// phase 0, right behind k_sqp_head of iteration `it`: the evaluation the head has just summed (what agx_status reports if the
//   solve ends here), the regularisation of the direction, and how the head left the instance -- converged, searching, or ended
//   at once on a discarded direction (sqp_iteration_end has then moved preg / dreg on: the values the direction was computed
//   with are in gains_preg / gains_dreg).  A searching instance gets trials = -1: the outcome is still open.
// phase 1, behind the trial rounds of iteration `it`: the outcome of the search for the records phase 0 left open.  Accepted:
//   tiles_ok (k_sqp_accept), step 2^-ls_n after ls_n + 1 trials; all ten rejected: tiles stale, step 0.
// Records at or beyond `capacity` are dropped; n[b] counts them all the same.
__global__ void k_iter_log(const DevState *__restrict__ st, int B, int it, int phase, agx_iter_record *__restrict__ rec,
                           int *__restrict__ n, int capacity) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const DevState &S = st[b];
  if (S.dir_iter != it) return;
  agx_iter_record *r = rec + (long long)b * capacity + it;
  if (phase == 0) {
    n[b] = it + 1;
    if (it >= capacity) return;
    const bool conv = S.done && S.solved;
    const bool search = S.searching != 0;
    const bool ended = !conv && !search;
    agx_iter_record v;
    v.kkt = S.kkt; v.cost = S.cost; v.merit = S.merit; v.gap_norm = S.gap; v.constraint_norm = S.con;
    v.step = 0.0;
    v.preg = ended ? S.gains_preg : S.preg;
    v.dreg = ended ? S.gains_dreg : S.dreg;
    v.iter = it; v.qp_iters = S.qp_iters; v.trials = search ? -1 : 0;
    v.flags = conv ? 1 : (ended ? 2 : 0);
    *r = v;
  } else {
    if (it >= capacity || r->trials != -1) return;
    const int ls_n = S.ls_n;
    r->trials = ls_n + 1;
    if (S.tiles_ok) r->step = ldexp(1.0, -ls_n);
    else r->flags |= 4;
  }
}

// One lane per (node, row): the node's kinematics, then node_costs / node_costs_general on a row table that holds this row
// alone, at its own offset of the node's reference tile and with its own column of the frame-id table.  What the accumulators
// hold afterwards is the item: item weight x a(r) and item weight x R' a'(r), without the Euler factor dt.  Stores into
// cost [B][T+1][R], Lx [B][T+1][R][2 NV], Lu [B][T+1][R][NV] (zeroed by the caller: inactive rows, rows a node type does not
// have and the terminal Lu stay zero).  rows2: the running and the terminal table.
template <int NV, bool CHAIN, class... OBS>
__global__ void __launch_bounds__(64) k_item_costs(const DevModel *__restrict__ mp, const DevRows *__restrict__ rows2, int B, int T,
                                                   const double *__restrict__ xs, const double *__restrict__ us, RefView rv, int R,
                                                   double *__restrict__ cost, double *__restrict__ Lx, double *__restrict__ Lu,
                                                   const OBS *__restrict__... obs) {
  constexpr int NX = 2 * NV, NU = NV;
  const DevModel &m = *mp;
  const long long unit = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (unit >= (long long)B * (T + 1) * R) return;
  const int r = (int)(unit % R);
  const long long node = unit / R;
  const int b = (int)(node / (T + 1)), t = (int)(node % (T + 1));
  const bool term = t == T;
  const DevRows &rows = rows2[term ? 1 : 0];
  if (r >= rows.n || !rows.active[r]) return;
  DevRows one;
  one.n = 1;
  one.kind[0] = rows.kind[r]; one.act[0] = rows.act[r]; one.active[0] = 1; one.frame[0] = rows.frame[r]; one.frame_b[0] = rows.frame_b[r];
  one.off[0] = rows.off[r]; one.nref[0] = rows.nref[r]; one.nr[0] = rows.nr[r];
  one.alpha[0] = rows.alpha[r]; one.weight[0] = rows.weight[r];
  one.general = rows.general; one.nvu = rows.nvu;
  double x[NX], u[NU];
  const double *xp = xs + node * NX;
AGX_UNROLL_NV
  for (int i = 0; i < NX; ++i) x[i] = xp[i];
AGX_UNROLL_NV
  for (int i = 0; i < NU; ++i) u[i] = term ? 0.0 : us[((long long)b * T + t) * NU + i];
  const double *ref = ref_at(rv, b, t, T);
  const int *fr = frames_at(rv, b, t, T);
  if (fr) fr += r;
  Kin<NV> k;
  kinematics<NV, CHAIN>(m, x, k);
  CostAcc<NV> c;
  if (term) {
    node_costs<NV, CHAIN, true, true>(m, one, k, x, nullptr, ref, fr, c, world_of(b, obs...));
    if constexpr (NV <= 7) {
      CostGen<NV> g;
      node_costs_general<NV, CHAIN, true, true>(m, one, k, x, nullptr, ref, fr, c, g);
    }
  } else {
    node_costs<NV, CHAIN, false, true>(m, one, k, x, u, ref, fr, c, world_of(b, obs...));
    if constexpr (NV <= 7) {
      CostGen<NV> g;
      node_costs_general<NV, CHAIN, false, true>(m, one, k, x, u, ref, fr, c, g);
    }
  }
  cost[unit] = c.cost;
AGX_UNROLL_NV
  for (int i = 0; i < NV; ++i) {
    Lx[unit * NX + i] = c.Lq[i];
    Lx[unit * NX + NV + i] = c.Lv[i];
    if (!term) Lu[unit * NU + i] = c.Lu[i];
  }
}

}  // namespace agx

extern "C" {

// returns the hipError_t of the launch
int agx_diag_iter_log_launch(void *stream, const DevState *st, int B, int it, int phase, agx_iter_record *rec, int *n, int capacity) {
  hipLaunchKernelGGL(agx::k_iter_log, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, (hipStream_t)stream, st, B, it, phase, rec, n, capacity);
  return (int)hipGetLastError();
}

// k_item_costs at the capacity nv (7: serial chain or tree; 16 / 30 / 32: the tree code serves chains too); obs: null, or the
// device table of agx_ocp_set_obstacle_placements (7-joint capacity).  -1: no instantiation for nv.
int agx_diag_item_costs_launch(void *stream, int nv, int chain, const DevModel *m, const DevRows *rows2, int B, int T, const double *xs,
                               const double *us, const RefView *rv, int R, double *cost, double *Lx, double *Lu, const void *obs) {
  const long long units = (long long)B * (T + 1) * R;
  const dim3 grid((unsigned)((units + 63) / 64)), blk(64);
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto NVc, auto CHc, auto... src) {
    hipLaunchKernelGGL((agx::k_item_costs<decltype(NVc)::value, decltype(CHc)::value, std::remove_const_t<std::remove_pointer_t<decltype(src)>>...>),
                       grid, blk, 0, s, m, rows2, B, T, xs, us, *rv, R, cost, Lx, Lu, src...);
  };
  const auto *op = (const agx::ObstaclePlacements *)obs;
  switch (nv) {
    case 7:
      if (chain) { if (op) launch(std::integral_constant<int, 7>(), std::true_type(), op); else launch(std::integral_constant<int, 7>(), std::true_type()); }
      else { if (op) launch(std::integral_constant<int, 7>(), std::false_type(), op); else launch(std::integral_constant<int, 7>(), std::false_type()); }
      break;
    case 16: launch(std::integral_constant<int, 16>(), std::false_type()); break;
    case 30: launch(std::integral_constant<int, 30>(), std::false_type()); break;
    case 32: launch(std::integral_constant<int, 32>(), std::false_type()); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // extern "C"
