// agx_cost_pairs.hpp -- soft collision avoidance at width: the trailing ResidualDistanceCollision cost rows of a WIDE cost set
// (up to AGX_MAX_COST_PAIRS per node type, include/agimus_hip.h) for serial chains of the 7-joint capacity.
//
// A collision row depends on q only, so what it adds to a node is purely additive:
//   cost += w a(d),   Lq += w a'(d) g,   Lqq += w a''(d) g g'     (g: gradient of the distance in q; the Gauss-Newton form of the
// COLL variant of k_calc_qp_lj).  K1 therefore runs on the non-collision prefix of the row table and k_cost_pairs, launched right
// behind it on the same node grid, adds the pairs into the tiles K1 has just written.
//
// The kernels of this header are compiled in a translation unit of their own (agx_cost_pairs.hip): instantiated next to the
// other kernels of the 7-joint group they changed the register allocation of an unrelated one (k_node_kkt, 66 -> 80 VGPRs).
// It needs agx_device.hpp and agx_tiles.hpp only.
#pragma once

#include <type_traits>

#include "agx_tiles.hpp"

namespace agx {

// 8 lanes per node, as k_con_eval_pairs: lane j forms the world placement of joint j (SE3 prefix product) and stages it in LDS with
// the joint's world axis; the pairs are dealt round-robin over the lanes (lane l: pairs l, l + 8, ...).  A lane evaluates the
// closest points of its pairs, the scalar activation and the whole gradient row in q, and accumulates cost, Lq and the upper
// triangle of Lqq in registers; a fixed 8-lane DPP butterfly sums the partials (no atomics: the pair-to-lane assignment and the
// order of the sums are fixed, so the result is the same bit for bit from run to run) and leaves lane l with column l.
// DEST kPairsToQp: the sums, scaled as K1 scales its own rows (dt on running nodes), are added into the node's QP tile (Hqq, the q
//   half of gx, cost) and aux tile (Lqq) by read-modify-write of whole 64-byte lines; nodes are selected by K1's own predicate
//   (k1_node_active) so that a tile K1 rewrote is added to once and a tile K1 kept is left alone.
// DEST kPairsToCanonical: into Lx[q], Lxx[qq] and cost of the canonical tile (agx_ocp_calc_diff); `st` may be null.
// DEST kPairsDistance: the distance of pair `which` at the running nodes, out [B][T] (agx_ocp_get_residuals).
// DEST kPairsItems: every pair on its own (agx_ocp_item_costs): the lane that evaluates pair p stores its value w a(d) into
//   out [B][T+1][which] and its gradient row w a'(d) g into the q half of auxs [B][T+1][which][2 NV] at row `first + p` of the
//   caller's table (which: rows per node of those arrays), unscaled; no butterfly, nothing is summed.  `st` may be null.
// sel: 0 every node, 1 running nodes, 2 terminal nodes.
// OBS: empty, or ObstaclePlacements with one more argument (agx_ocp_set_obstacle_placements): a world-fixed geometry listed in
// the table is placed at the pose of the node's instance, a per-lane load in place of the model's entry.
template <int NV, int DEST, class... OBS>
__global__ void __launch_bounds__(64) k_cost_pairs(const DevModel *__restrict__ mp, const DevOcp *__restrict__ op,
                                                   const DevCostWide *__restrict__ wp, const double *__restrict__ dts,
                                                   const double *__restrict__ xs, RefView rv, double *__restrict__ out,
                                                   double *__restrict__ auxs, const DevState *__restrict__ st, int phase, int sel,
                                                   int which, const OBS *__restrict__... obs) {
  constexpr int NX = 2 * NV, NH = NV * (NV + 1) / 2;
  static_assert(NV <= 7, "8 lanes per node: one lane per joint, lane 7 carries the padding column");
  __shared__ double s_mod[8][16];     // placement 12 | axis 3 of every joint
  __shared__ double s_kin[8][8][16];  // [node of the block][joint]: world rotation 9 | origin 3 | axis 3
  const DevModel &m = *mp;
  const DevOcp &o = *op;
  const int T = o.T, l8 = threadIdx.x & 7, grp = threadIdx.x >> 3;
  const long long n_nodes = (long long)o.B * (T + 1);
  const long long node_raw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const bool ok = node_raw < n_nodes;
  const long long node = ok ? node_raw : n_nodes - 1;
  const int b = (int)(node / (T + 1)), t = (int)(node % (T + 1));
  const bool term = t == T;
  const DevCostPairs &P = wp->lay[term ? 1 : 0];
  bool act = ok && P.n > 0 && (sel == 0 || (sel == 2) == term);
  if constexpr (DEST == kPairsToQp) act = act && k1_node_active(st[b], phase, term, t, T);
  else act = act && !(st && st[b].done);
  if (!__any(act)) return;  // the block is one wave
  if (threadIdx.x < 8) {
    const int jj = threadIdx.x < NV ? threadIdx.x : NV - 1;
#pragma unroll
    for (int e = 0; e < 12; ++e) s_mod[threadIdx.x][e] = m.placement[jj][e];
#pragma unroll
    for (int e = 0; e < 3; ++e) s_mod[threadIdx.x][12 + e] = m.axis[jj][e];
  }
  __syncthreads();
  const int j = l8 < NV ? l8 : NV - 1;
  const double qj = xs[node * NX + j];
  {  // kinematics of k_con_eval_pairs, staged for the lanes of the node
    double *kin = s_kin[grp][l8];
    const double *mj = s_mod[l8];
    const double *ax3 = mj + 12;
    double R[9], p[3], z[3];
    double sn, cs;
    sincos(qj, &sn, &cs);
    const double omc = 1.0 - cs;
    double Rq[9];
    Rq[0] = cs + omc * ax3[0] * ax3[0];
    Rq[1] = omc * ax3[0] * ax3[1] - sn * ax3[2];
    Rq[2] = omc * ax3[0] * ax3[2] + sn * ax3[1];
    Rq[3] = omc * ax3[1] * ax3[0] + sn * ax3[2];
    Rq[4] = cs + omc * ax3[1] * ax3[1];
    Rq[5] = omc * ax3[1] * ax3[2] - sn * ax3[0];
    Rq[6] = omc * ax3[2] * ax3[0] - sn * ax3[1];
    Rq[7] = omc * ax3[2] * ax3[1] + sn * ax3[0];
    Rq[8] = cs + omc * ax3[2] * ax3[2];
    mm3(mj, Rq, R);
    p[0] = mj[9]; p[1] = mj[10]; p[2] = mj[11];
    auto se3_step = [&](auto OFFc) {
      constexpr int OFF = decltype(OFFc)::value;
      double Rp[9], pp[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) Rp[e] = dpp_mov<0x110 + OFF>(R[e]);  // row_shr:OFF, lane i reads lane i - OFF (g_up of agx_k1_lanes.hpp)
#pragma unroll
      for (int e = 0; e < 3; ++e) pp[e] = dpp_mov<0x110 + OFF>(p[e]);
      if (l8 >= OFF) {
        double tt[3];
        mv3(Rp, p, tt);
        p[0] = pp[0] + tt[0]; p[1] = pp[1] + tt[1]; p[2] = pp[2] + tt[2];
        mm3(Rp, R, R);
      }
    };
    se3_step(std::integral_constant<int, 1>());
    se3_step(std::integral_constant<int, 2>());
    se3_step(std::integral_constant<int, 4>());
    mv3(R, ax3, z);  // joint axis in the world
#pragma unroll
    for (int e = 0; e < 9; ++e) kin[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) { kin[9 + e] = p[e]; kin[12 + e] = z[e]; }
  }
  wave_lds_sync();  // the block is one wave: the joints of every node are staged
  const double(*sk)[16] = s_kin[grp];
  const double *gref = ref_at(rv, b, t, T) + P.prefix;
  double cost = 0.0, gq[8], H[NH];
#pragma unroll
  for (int i = 0; i < 8; ++i) gq[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NH; ++i) H[i] = 0.0;
  for (int pi = l8; pi < P.n; pi += 8) {
    if (!P.active[pi]) continue;
    if (DEST == kPairsDistance && pi != which) continue;
    const int fr[2] = {P.fa[pi], P.fb[pi]};
    double Rg[2][9], pg[2][3];
    int jp[2];
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const double *fpl = m.frame_placement[fr[gi]];
      const int jf = m.frame_parent[fr[gi]];
      jp[gi] = jf;
      if (jf >= 0) {
        const double *Rp = sk[jf], *pp = sk[jf] + 9;
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
    if constexpr (DEST == kPairsDistance) {
      if (act) out[(long long)b * T + t] = d;
      continue;
    }
    double grow[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {  // serial chain: joints up to a frame's parent move it; a self pair gets the terms of both frames
      const double *pj = sk[i] + 9, *zj = sk[i] + 12;
      double da[3], db[3], ta[3], tb[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) { da[e] = ca[e] - pj[e]; db[e] = cb[e] - pj[e]; }
      cross3(zj, da, ta);
      cross3(zj, db, tb);
      grow[i] = (i <= jp[0] ? dot3(nn, ta) : 0.0) - (i <= jp[1] ? dot3(nn, tb) : 0.0);
    }
    const double wi = gref[2 * pi], aw0 = gref[2 * pi + 1];
    double a, ar, arr;
    activation1(P.act[pi], P.alpha[pi], aw0, d, a, ar, arr);
    cost += wi * a;
    if constexpr (DEST == kPairsItems) {
      if (act) {
        const long long row = node * which + P.first + pi;
        out[row] = wi * a;
#pragma unroll
        for (int i = 0; i < NV; ++i) auxs[row * NX + i] = wi * ar * grow[i];
      }
      continue;
    }
    const double c1 = wi * ar, c2 = wi * arr;
    int h = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      gq[i] += c1 * grow[i];
      const double cg = c2 * grow[i];
#pragma unroll
      for (int k = i; k < NV; ++k) H[h++] += cg * grow[k];
    }
  }
  if constexpr (DEST == kPairsDistance || DEST == kPairsItems) return;
  // ---- 8-lane butterfly: every lane ends with the node's cost and column l8 of Lq / Lqq
  const double sc = term ? 1.0 : dts[term ? 0 : t];
  cost += dpp_xor4(cost); cost += dpp_xor2(cost); cost += dpp_xor1(cost);
  const double gcol = sc * transpose_reduce8(gq, l8);
  double hcol[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double prow[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      // element (i, k) of the symmetric matrix in the packed upper triangle (row r starts at r NV - r (r - 1) / 2)
      const int r = i < k ? i : k, c = i < k ? k : i;
      prow[k] = k < NV ? H[r * NV - r * (r - 1) / 2 + (c - r)] : 0.0;
    }
    hcol[i] = sc * transpose_reduce8(prow, l8);
  }
  if (!act) return;
  if constexpr (DEST == kPairsToQp) {
    typedef QT<NV> Q;
    typedef AUX<NV> A;
    const long long sid = (long long)b * (T + 1) + tile_slot(o, t);
    double *qt = out + sid * Q::SIZE, *ax = auxs + sid * A::SIZE;
    // every statement below is the 8 lanes of the node on one aligned 64-byte line: lane 7 adds 0 to the padding column of a block
    // row, to the first velocity entry of gx and, with lanes 1 .. 6, to the zeros behind the cost
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      qt[Q::Hqq + i * 8 + l8] += hcol[i];
      ax[A::Lqq + i * 8 + l8] += hcol[i];
    }
    qt[Q::gx + l8] += gcol;
    qt[Q::cost + l8] += l8 == 0 ? sc * cost : 0.0;
  } else {
    typedef TileOff<NV> TO;
    double *tile = out + node * TO::SIZE;
    if (l8 < NV) {
      tile[TO::Lx + l8] += gcol;
#pragma unroll
      for (int i = 0; i < NV; ++i) tile[TO::Lxx + i * NX + l8] += hcol[i];
    }
    if (l8 == 0) tile[TO::cost] += sc * cost;
  }
}

// Resident trajectories (k_sine_fill writes the rows of the prefix): [item weight | activation weight = 1] of every pair row in
// both layouts of every sample; gw_item [B][n_points] (optional) schedules the item weight of all of them.
__global__ void k_cost_pairs_fill(const DevCostWide *__restrict__ wp, const double *__restrict__ gw_item, double *__restrict__ traj,
                                  long long units, int stride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= units * 2) return;
  const long long unit = i >> 1;
  const int layout = (int)(i & 1);
  const DevCostPairs &P = wp->lay[layout];
  double *tile = traj + unit * 2 * stride + (long long)layout * stride + P.prefix;
  for (int p = 0; p < P.n; ++p) {
    tile[2 * p] = gw_item ? gw_item[unit] : P.weight[p];
    tile[2 * p + 1] = 1.0;
  }
}

// The same for the samples agx_traj_stream_append adds to a streamed ring (k_traj_append: `cap` slots + `mirror` mirror slots per
// instance, n_points = cap + mirror): sample j of the chunk [B][m_new] goes to slot (end + j) mod cap and to its mirror slot;
// gw_item [B][m_new] (optional) is the chunk's scheduled item weight.
__global__ void k_cost_pairs_fill_ring(const DevCostWide *__restrict__ wp, const double *__restrict__ gw_item, double *__restrict__ traj,
                                       int B, int m_new, int end, int cap, int mirror, int stride) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * m_new * 2) return;
  const long long unit = i >> 1;
  const int layout = (int)(i & 1);
  const int b = (int)(unit / m_new), j = (int)(unit % m_new);
  const int slot = (int)(((long long)end + j) % cap);
  const DevCostPairs &P = wp->lay[layout];
  const double w = gw_item ? gw_item[unit] : 0.0;
  for (int copy = 0; copy < 2; ++copy) {
    if (copy && slot >= mirror) break;
    const long long dst = (long long)b * (cap + mirror) + slot + (copy ? cap : 0);
    double *tile = traj + dst * 2 * stride + (long long)layout * stride + P.prefix;
    for (int p = 0; p < P.n; ++p) {
      tile[2 * p] = gw_item ? w : P.weight[p];
      tile[2 * p + 1] = 1.0;
    }
  }
}

}  // namespace agx
