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

#include <climits>
#include <cmath>
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

// Clearance report (agx_ocp_clearance): the signed distance of every pair of a caller's pair list at a caller's configurations.
// One workgroup of kClearLanes lanes takes kClearSamples consecutive samples of one instance (grid: B x chunks).  The joint count
// is a run-time value and nothing per lane is indexed by joint -- the joints' world placements live in LDS, 12 doubles each
// (rotation row-major, origin) -- so one kernel serves every capacity and needs no scratch.
//   phase 1a  a lane per (sample, joint): the joint's own transform R_fix R(q) (revolute; R_fix for a prismatic joint) into its slot;
//   phase 1b  a lane per sample walks the parent table (parents come first) and composes the slots in place, the arithmetic of
//             kinematics() in agx_device.hpp; the world axis of a prismatic joint is formed where its origin moves and not kept
//             (a distance needs no Jacobian column);
//   phase 2   the (sample, pair) items of the chunk dealt over the lanes in order, so that `dist` is stored coalesced: both
//             geometries placed from LDS -- a world-fixed frame from world_of(b, obs...), a per-lane load as in k_cost_pairs --
//             then collision_distance_placed.  That routine returns the points on the capsule AXES (a sphere's centre) and on the
//             box; the witness stored here is moved to the surfaces, pa = ca - ra n, pb = cb + rb n, so pa - pb = dist n.
//   minimum   every lane keeps the smallest (distance, item) of its items, a tree over the workgroup picks the chunk's, lane 0
//             stores it; k_clearance_min then walks the chunks of an instance in order.  Ties go to the lower item -- the lower
//             sample, then the lower pair -- whatever the order of the comparisons, so there is nothing to race and no atomic.
// q: sample s of instance b starts at q + b qb + s qs (the iterate: xs, qs = 2 nv; the caller's joints: a padded copy, qs = nv).
constexpr int kClearLanes = 256, kClearSamples = 8;

AGX_DEV bool clear_less(double d, int i, double d2, int i2) { return d < d2 || (d == d2 && i < i2); }

template <class... OBS>
__global__ void __launch_bounds__(kClearLanes) k_clearance(const DevModel *__restrict__ mp, int n_pairs, const int *__restrict__ fa,
                                                           const int *__restrict__ fb, const double *__restrict__ q, long long qb, int qs,
                                                           int m_samples, int chunks, double *__restrict__ dist, double *__restrict__ witness,
                                                           double *__restrict__ cmin, int *__restrict__ cidx, const OBS *__restrict__... obs) {
  extern __shared__ double lds[];
  const DevModel &m = *mp;
  const int nv = m.nv, tid = threadIdx.x;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int s0 = chunk * kClearSamples, ns = min(kClearSamples, m_samples - s0);
  double *sk = lds;                                  // [kClearSamples][nv][12]
  double *red_d = lds + kClearSamples * nv * 12;     // [kClearLanes]
  int *red_i = (int *)(red_d + kClearLanes);         // [kClearLanes]
  const double *qc = q + (long long)b * qb + (long long)s0 * qs;
  for (int u = tid; u < ns * nv; u += kClearLanes) {
    const int s = u / nv, i = u % nv;
    double *slot = sk + (long long)u * 12;
    if ((m.prismatic >> i) & 1u) {
#pragma unroll
      for (int e = 0; e < 9; ++e) slot[e] = m.placement[i][e];
    } else {
      const double *ax = m.axis[i];
      double sn, cs;
      sincos(qc[(long long)s * qs + i], &sn, &cs);
      const double omc = 1.0 - cs;
      double Rq[9], Rl[9];
      Rq[0] = cs + omc * ax[0] * ax[0];
      Rq[1] = omc * ax[0] * ax[1] - sn * ax[2];
      Rq[2] = omc * ax[0] * ax[2] + sn * ax[1];
      Rq[3] = omc * ax[1] * ax[0] + sn * ax[2];
      Rq[4] = cs + omc * ax[1] * ax[1];
      Rq[5] = omc * ax[1] * ax[2] - sn * ax[0];
      Rq[6] = omc * ax[2] * ax[0] - sn * ax[1];
      Rq[7] = omc * ax[2] * ax[1] + sn * ax[0];
      Rq[8] = cs + omc * ax[2] * ax[2];
      mm3(m.placement[i], Rq, Rl);
#pragma unroll
      for (int e = 0; e < 9; ++e) slot[e] = Rl[e];
    }
  }
  __syncthreads();
  if (tid < ns) {
    double *sj = sk + (long long)tid * nv * 12;
    for (int i = 0; i < nv; ++i) {
      double *slot = sj + i * 12;
      const int par = m.parent[i];
      double R[9], p[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) R[e] = slot[e];
      if (par >= 0) {
        const double *Rp = sj + par * 12, *pp = Rp + 9;
        double t[3];
        mm3(Rp, R, R);
        mv3(Rp, &m.placement[i][9], t);
        p[0] = pp[0] + t[0]; p[1] = pp[1] + t[1]; p[2] = pp[2] + t[2];
      } else {
        p[0] = m.placement[i][9]; p[1] = m.placement[i][10]; p[2] = m.placement[i][11];
      }
      if ((m.prismatic >> i) & 1u) {
        const double qi = qc[(long long)tid * qs + i];
        double z[3];
        mv3(R, m.axis[i], z);
#pragma unroll
        for (int e = 0; e < 3; ++e) p[e] += z[e] * qi;
      }
#pragma unroll
      for (int e = 0; e < 9; ++e) slot[e] = R[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) slot[9 + e] = p[e];
    }
  }
  __syncthreads();
  double best_d = INFINITY;
  int best_i = INT_MAX;
  const long long base = ((long long)b * m_samples + s0) * n_pairs;
  for (int u = tid; u < ns * n_pairs; u += kClearLanes) {
    const int s = u / n_pairs, pr = u % n_pairs;
    const int fr[2] = {fa[pr], fb[pr]};
    double Rg[2][9], pg[2][3];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const double *fpl = m.frame_placement[fr[gi]];
      const int jf = m.frame_parent[fr[gi]];
      if (jf >= 0) {
        const double *Rp = sk + ((long long)s * nv + jf) * 12, *pp = Rp + 9;
        double tt[3];
        mm3(Rp, fpl, Rg[gi]);
        mv3(Rp, fpl + 9, tt);
        pg[gi][0] = pp[0] + tt[0]; pg[gi][1] = pp[1] + tt[1]; pg[gi][2] = pp[2] + tt[2];
      } else {
        const double *wpl = world_of(b, obs...).world(fpl, fr[gi]);
#pragma unroll
        for (int e = 0; e < 9; ++e) Rg[gi][e] = wpl[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) pg[gi][e] = wpl[9 + e];
      }
    }
    double ca[3], cb[3], nn[3];
    const double d = collision_distance_placed(m, fr[0], fr[1], Rg[0], pg[0], Rg[1], pg[1], ca, cb, nn);
    dist[base + u] = d;
    if (witness) {
      const double ra = m.frame_radius[fr[0]], rb = m.frame_radius[fr[1]];
      double *w = witness + (base + u) * 9;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        w[e] = ca[e] - ra * nn[e];
        w[3 + e] = cb[e] + rb * nn[e];
        w[6 + e] = nn[e];
      }
    }
    if (clear_less(d, u, best_d, best_i)) { best_d = d; best_i = u; }
  }
  red_d[tid] = best_d;
  red_i[tid] = best_i;
  __syncthreads();
  for (int w = kClearLanes / 2; w > 0; w >>= 1) {
    if (tid < w && clear_less(red_d[tid + w], red_i[tid + w], red_d[tid], red_i[tid])) { red_d[tid] = red_d[tid + w]; red_i[tid] = red_i[tid + w]; }
    __syncthreads();
  }
  if (tid == 0) {
    cmin[blockIdx.x] = red_d[0];
    cidx[blockIdx.x] = red_i[0] == INT_MAX ? -1 : s0 * n_pairs + red_i[0];  // item (sample, pair) of the instance; -1: no finite distance
  }
}

// second pass of the minimum: a lane per instance over its chunks, in order (a later chunk holds later samples: strict `<`)
__global__ void k_clearance_min(int B, int chunks, int n_pairs, const double *__restrict__ cmin, const int *__restrict__ cidx,
                                double *__restrict__ min_dist, int *__restrict__ min_where) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double d = INFINITY;
  int at = -1;
  for (int c = 0; c < chunks; ++c) {
    const double dc = cmin[(long long)b * chunks + c];
    if (dc < d) { d = dc; at = cidx[(long long)b * chunks + c]; }
  }
  min_dist[b] = d;
  min_where[2 * b] = at < 0 ? -1 : at / n_pairs;
  min_where[2 * b + 1] = at < 0 ? -1 : at % n_pairs;
}

}  // namespace agx

extern "C" {

// chunks of samples per instance of k_clearance (the caller sizes cmin / cidx [B][chunks] with it)
int agx_diag_clearance_chunks(int m_samples) { return (m_samples + agx::kClearSamples - 1) / agx::kClearSamples; }

// The launches of agx_ocp_clearance: k_clearance over B x chunks workgroups, then k_clearance_min when the minimum is wanted
// (min_dist non-null).  nv: the joints of the model at mp, for the size of the LDS block.  obs as below.  Returns the hipError_t
// of the launches.
int agx_diag_clearance_launch(void *stream, const DevModel *mp, int nv, int B, int n_pairs, const int *fa, const int *fb, const double *q,
                              long long qb, int qs, int m_samples, double *dist, double *witness, double *cmin, int *cidx, double *min_dist,
                              int *min_where, const void *obs) {
  const int chunks = agx_diag_clearance_chunks(m_samples);
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = sizeof(double) * ((size_t)agx::kClearSamples * nv * 12 + agx::kClearLanes) + sizeof(int) * agx::kClearLanes;
  const dim3 grid((unsigned)((long long)B * chunks)), blk(agx::kClearLanes);
  const auto *op = (const agx::ObstaclePlacements *)obs;
  if (op) hipLaunchKernelGGL((agx::k_clearance<agx::ObstaclePlacements>), grid, blk, lds, s, mp, n_pairs, fa, fb, q, qb, qs, m_samples, chunks, dist, witness, cmin, cidx, op);
  else hipLaunchKernelGGL((agx::k_clearance<>), grid, blk, lds, s, mp, n_pairs, fa, fb, q, qb, qs, m_samples, chunks, dist, witness, cmin, cidx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !min_dist) return (int)e;
  hipLaunchKernelGGL(agx::k_clearance_min, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, s, B, chunks, n_pairs, cmin, cidx, min_dist, min_where);
  return (int)hipGetLastError();
}

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
