// agx_general_rows.hpp -- the general cost rows (agx_general.hpp: ResidualModelControlGrav, ResidualModelFrameVelocity) for
// large models (capacities 16 / 30 / 32, chains and trees, revolute and prismatic joints) on the workgroup-per-node path.
//
// Everything such a row adds to a node is additive in the Hessian and gradient blocks, so K1 (k_calc_qp_wg) runs on the row
// table as before -- it skips the two kinds -- and k_general_rows_wg, launched right behind it on the same iterate, phase and node
// predicate (k1_active), read-modify-writes what the rows add into the tiles K1 has just written (the shape of k_cost_pairs).
// With s = dt on running nodes and 1 on the terminal node, W = s sum_rows (item weight x activation weights) of the ControlGrav
// rows, G = dg/dq and A = tq - G (r = u - g(q) in the acceleration input: dr = M dw + A dq + tv dv):
//   running QP tile   Hww += M W M,  Hqw += A' W M,  Hvw += tv' W M,  Hqq += Lqq_fv + A' W A,  Hqv += Lqv_fv + A' W tv,
//                     Hvv += Lvv_fv + tv' W tv,  gw += M lu,  gx[q] += Lq_fv + A' lu,  gx[v] += Lv_fv + tv' lu,  cost += c
//                     (lu = W (u - g); the same sums as  Lqu + tq' W  etc. of calc_qp_body<.., GEN>, with Lqu = -G' W folded in)
//   running aux tile  Luu += W,  Lu += lu,  Lqq += Lqq_fv + G' W G   (the diagonal Lvv is left alone)
//   terminal node     ControlGrav skipped; FrameVelocity adds Lqq, Lqv, Lvv, Lq, Lv, c to Hqq, Hqv, Hvv, gx, cost and aux Lqq
//   general blocks    auxg [B][T+1][3 NV 32] = Lqv | Lvvd | Lqu  (row stride 32, the layout k_node_kkt_gen indexes)
// g(q) is the RNEA at rest and G its derivative at (q, 0, 0): with v = 0 and qdd = 0 every body accelerates by a0 = (-gravity; 0),
// so f^C_i = Ic_i a0, psi_i = a0 x S_i, and of the matrices of wg_node's derivative phase only
//   G[r][c] = (Ic_r S_r) . psi_c                  c on the path root..r
//           = S_r . (S_c x* f^C_c + Ic_c psi_c)   r a strict ancestor of c
// is left (Sd, f0, E and Dt vanish).  Kinematics, joint axes and body inertias are wg_node's own (kin_only).
// The dense contractions run on v_mfma_f64_16x16x4_f64 (wg_mma / wg_op of agx_big_k1.hpp, wave w owns tile (w >> 1, w & 1));
// every sum has a fixed order and nothing is accumulated with atomics: the same solve twice gives the same bits.
//
// k_node_kkt_big_gen is K3 (k_node_kkt_big: 32 lanes per node, sum32 butterflies) with every block of the identities written
// above k_node_kkt_gen.
//
// The kernels of this header are compiled in a translation unit of their own (agx_general_rows.hip), as agx_cost_pairs.hip is:
// the kernels of the large-model unit keep their register allocation.
#pragma once

#include "agx_kernels.hpp"

namespace agx {

// acc added into tile (ti, tj) of a 32-column block: the lane pairing of wg_store_tile, whole 16-byte pieces read and written
__device__ __forceinline__ void wg_add_tile(double *__restrict__ blk, const agx_v4d &acc, int ti, int tj, int lane, int nv) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const bool even = !(l15 & 1);
#pragma unroll
  for (int qp = 0; qp < 2; ++qp) {
    const double a = acc[2 * qp], b = acc[2 * qp + 1];
    const double y = dpp_mov<0xB1>(even ? b : a);  // quad_perm [1,0,3,2]: swap with the neighbour lane
    const double2 v = even ? make_double2(a, y) : make_double2(y, b);
    const int row = 16 * ti + l4 + 4 * (2 * qp + (even ? 0 : 1));
    if (row < nv) {
      double2 *p = reinterpret_cast<double2 *>(blk + row * 32 + 16 * tj + (l15 & 14));
      const double2 old = *p;
      *p = make_double2(old.x + v.x, old.y + v.y);
    }
  }
}

// First reference-tile double of a general row, over both node types: k_general_rows_wg stages the tile from there on (the host
// checks that piece against kWgRef, agx_ocp_create).
__device__ __forceinline__ int general_ref_lo(const DevOcp &o) {
  int lo = o.stride;
  for (int lay = 0; lay < 2; ++lay)
    for (int r = 0; r < o.rows[lay].n; ++r)
      if (row_is_general(o.rows[lay].kind[r])) lo = min(lo, o.rows[lay].off[r]);
  return lo;
}

// One FrameVelocity row by one wave: lane j forms column j of Rq | Rv (frame_velocity of agx_general.hpp on the node's LDS
// kinematics) into J[0..5][j] | J[8..13][j], lane 0 the weights s wi aw into wJ[0..5]; returns the row's value wi a(r) on every
// lane and adds the lane's gradient entries into Lq[j], Lv[j] (scaled by s).
template <int NV, bool PRISM>
__device__ __forceinline__ double wg_frame_velocity_row(WgNode<NV> &L, const DevModel &m, int frame, int type, const double *tile, int nref,
                                                        double s, int lane) {
  const int kk = lane < NV ? lane : NV - 1;
  const bool jl = lane < NV;
  const double wi = tile[0];
  const double *rr = tile + 1, *aw = rr + nref;
  const double *qd = L.x + NV;
  double RF[9], pF[3];
  int jf;
  wg_frame_world<NV>(L, m, frame, RF, pF, &jf);
  const unsigned path = jf >= 0 ? L.anc[jf] : 0u;  // joints between the root and the frame's joint
  double v0[6] = {0, 0, 0, 0, 0, 0}, below[6] = {0, 0, 0, 0, 0, 0};
  for (int j = 0; j < NV; ++j) {
    if (!((path >> j) & 1u)) continue;  // uniform over the wave
    const double qj = qd[j];
    const bool under = j != kk && ((L.anc[j] >> kk) & 1u);  // j strictly below kk
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const double c = L.S[j][e] * qj;
      v0[e] += c;
      below[e] += under ? c : 0.0;
    }
  }
  double wxp[3], lwa[6], vel[6];
  cross3(v0 + 3, pF, wxp);
#pragma unroll
  for (int e = 0; e < 3; ++e) { lwa[e] = v0[e] + wxp[e]; lwa[3 + e] = v0[3 + e]; }
  if (type == 0) {
#pragma unroll
    for (int e = 0; e < 6; ++e) vel[e] = v0[e];
  } else if (type == 2) {
#pragma unroll
    for (int e = 0; e < 6; ++e) vel[e] = lwa[e];
  } else {
    mtv3(RF, lwa, vel);
    mtv3(RF, lwa + 3, vel + 3);
  }
  const bool on = (path >> kk) & 1u;
  double dq[6] = {0, 0, 0, 0, 0, 0}, dv[6] = {0, 0, 0, 0, 0, 0};
  if (on) {
    const double *Sk = L.S[kk];
    double dW[6];
    mcross(Sk, below, dW);  // WORLD: d v0 / d q_kk ;  d v0 / d qd_kk = S_kk
    if (type == 0) {
#pragma unroll
      for (int e = 0; e < 6; ++e) { dq[e] = dW[e]; dv[e] = Sk[e]; }
    } else {
      // LOCAL_WORLD_ALIGNED: lin = v0_lin + w x pF,  d pF / d q_kk = z x (pF - p_kk) (prismatic: S_lin; there z = S_ang = 0)
      const double *z = Sk + 3, *pk = L.w.c.pw[kk];
      double d[3], dp[3], t1[3], t2[3], t3[3];
      d[0] = pF[0] - pk[0]; d[1] = pF[1] - pk[1]; d[2] = pF[2] - pk[2];
      cross3(z, d, dp);
      prismatic_column(PRISM && ((m.prismatic >> kk) & 1u), Sk, dp);
      cross3(dW + 3, pF, t1);
      cross3(v0 + 3, dp, t2);
      cross3(z, pF, t3);
      double lq[6], lv[6];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        lq[e] = dW[e] + t1[e] + t2[e]; lq[3 + e] = dW[3 + e];
        lv[e] = Sk[e] + t3[e];         lv[3 + e] = z[e];
      }
      if (type == 2) {
#pragma unroll
        for (int e = 0; e < 6; ++e) { dq[e] = lq[e]; dv[e] = lv[e]; }
      } else {
        // LOCAL: a_loc = RF' a_lwa,  d RF' / d q_kk = -RF' [z]x
        double c1[3], c2[3], a1[3], a2[3];
        cross3(z, lwa, c1);
        cross3(z, lwa + 3, c2);
#pragma unroll
        for (int e = 0; e < 3; ++e) { a1[e] = lq[e] - c1[e]; a2[e] = lq[3 + e] - c2[e]; }
        mtv3(RF, a1, dq);
        mtv3(RF, a2, dq + 3);
        mtv3(RF, lv, dv);
        mtv3(RF, lv + 3, dv + 3);
      }
    }
  }
  double a = 0.0, gq = 0.0, gv = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const double res = vel[e] - rr[e], w = wi * aw[e];
    a += 0.5 * w * res * res;
    gq += dq[e] * (w * res);
    gv += dv[e] * (w * res);
    if (jl) { L.w.c.J[e][kk] = dq[e]; L.w.c.J[8 + e][kk] = dv[e]; }
    if (lane == 0) L.w.c.wJ[e] = s * w;
  }
  if (jl) { L.Lq[kk] += s * gq; L.Lv[kk] += s * gv; }
  return a;
}

// One workgroup per node behind k_calc_qp_wg (same grid: running nodes first, then the terminal ones; a grid of B T
// workgroups covers the running nodes alone).
// DEST kGenToQp: into the QP / aux tiles and the general blocks, as above (out0 = qts, out1 = auxs, out2 = auxg); nodes by K1's
//   predicate.
// DEST kGenToCanonical: into Lx, Lu, Lxx, Lxu, Luu and cost of the canonical tiles (agx_ocp_calc_diff; out0) behind k_calc_diff,
//   which leaves the rows out; `st` may be null.  The same arithmetic with M = tq = tv = 0 (A = -G).
// DEST kGenItems: row `only` on its own, unscaled (agx_ocp_item_costs): value into out0 [B][T+1][R], gradient into out1
//   [B][T+1][R][2 NV] and out2 [B][T+1][R][NV] at row `only`; `st` may be null.
// only: -1 every general row of the node, else that row alone.
constexpr int kGenToQp = 0, kGenToCanonical = 1, kGenItems = 2;
template <int NV, bool PRISM, int DEST>
__global__ void __launch_bounds__(256) k_general_rows_wg(const DevModel *__restrict__ mp, const DevOcp *__restrict__ op,
                                                         const double *__restrict__ dts, const double *__restrict__ xs,
                                                         const double *__restrict__ us, RefView rv, double *__restrict__ out0,
                                                         double *__restrict__ out1, double *__restrict__ out2,
                                                         const DevState *__restrict__ st, int phase, int only, int R) {
  constexpr int NX = 2 * NV, NT = 256, LDM = 32;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  __shared__ WgNode<NV> L;
  __shared__ double sG[NV][LDM];  // G = dg/dq of the ControlGrav rows (columns >= NV zero)
  static_assert(sizeof(WgNode<NV>) + sizeof(double) * NV * LDM <= 65536, "LDS of one workgroup");
  const DevOcp &o = *op;
  const DevModel &m = *mp;
  const int T = o.T;
  const long long unit = blockIdx.x, n_run = (long long)o.B * T;
  const bool term = unit >= n_run;
  const int b = term ? (int)(unit - n_run) : (int)(unit / T), t = term ? T : (int)(unit % T);
  if (DEST == kGenToQp ? !k1_active(st[b], phase) : (st && st[b].done)) return;  // kGenToQp: the nodes K1 has just rewritten
  const DevRows &rows = o.rows[term ? 1 : 0];
  if (!rows.general) return;  // (the node type's general blocks stay zero)
  auto taken = [&](int r, int kind) { return rows.active[r] && rows.kind[r] == kind && (only < 0 || only == r); };  // uniform
  const long long node = (long long)b * (T + 1) + t;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = wave >> 1, tj = wave & 1, l15 = lane & 15, l4 = lane >> 4;
  const double s = (term || DEST == kGenItems) ? 1.0 : dts[t];

  // kinematics, joint axes and body inertias of the node into LDS (wg_node stops behind them); the control of the terminal node
  // is never used (it reads the last running node's)
  WgIn in;
  in.x = xs + node * NX; in.dx = nullptr; in.xn = in.x; in.dxn = nullptr;
  in.u = us + ((long long)b * T + (term ? T - 1 : t)) * NV; in.du = nullptr;
  in.alpha = 0.0; in.dt = 0.0; in.preg = 0.0; in.mu_dyn = 0.0;
  const int lo = general_ref_lo(o);  // the staged piece of the tile: rows.off[r] - lo
  in.ref = ref_at(rv, b, t, T) + lo; in.stride = o.stride - lo; in.frames = frames_at(rv, b, t, T);
  in.kin_only = true;
  wg_node<NV, false, false, PRISM>(L, m, rows, in, nullptr, nullptr);

  bool grav = false, fvel = false;  // uniform: functions of the row table
  for (int r = 0; r < rows.n; ++r) {
    grav = grav || (!term && taken(r, AGX_RES_CONTROL_GRAV));
    fvel = fvel || taken(r, AGX_RES_FRAME_VELOCITY);
  }
  if (!grav && !fvel) return;
  for (int e = tid; e < NV * LDM; e += NT) (&sG[0][0])[e] = 0.0;
  for (int e = tid; e < kWgJ * LDM; e += NT) (&L.w.c.J[0][0])[e] = 0.0;
  if (tid < kWgJ) L.w.c.wJ[tid] = 0.0;
  if (DEST == kGenToQp && !term) {  // M | tq | tv of the node as K1 left them in the aux tile (columns >= NV are zero there)
    const double *ax = out1 + node * A::SIZE;
    for (int e = 2 * tid; e < NV * LDM; e += 2 * NT) {
      *reinterpret_cast<double2 *>(&L.M[0][0] + e) = *reinterpret_cast<const double2 *>(ax + A::M + e);
      *reinterpret_cast<double2 *>(&L.tq[0][0] + e) = *reinterpret_cast<const double2 *>(ax + A::tq + e);
      *reinterpret_cast<double2 *>(&L.tv[0][0] + e) = *reinterpret_cast<const double2 *>(ax + A::tv + e);
    }
  } else {
    for (int e = tid; e < NV * LDM; e += NT) { (&L.M[0][0])[e] = 0.0; (&L.tq[0][0])[e] = 0.0; (&L.tv[0][0])[e] = 0.0; }
  }
  if (grav) {
    // composite inertias: Ic_i = sum over the subtree of i, fixed order
    for (int e = tid; e < NV * 10; e += NT) {
      const int i = e / 10, c = e % 10;
      const unsigned sub = L.desc[i];
      double acc = 0.0;
      for (int k = 0; k < NV; ++k) acc += ((sub >> k) & 1u) ? L.Ib[k][c] : 0.0;
      L.Ic[i][c] = acc;
    }
  }
  __syncthreads();
  if (grav && tid < NV) {
    const int i = tid;
    const double a0[6] = {-m.gravity[0], -m.gravity[1], -m.gravity[2], 0.0, 0.0, 0.0};
    const double *Si = L.S[i], *Ic = L.Ic[i];
    double psi[6], fC[6], m6[6], sxf[6], IcPs[6];
    mcross(a0, Si, psi);
    iapply(Ic, a0, fC);
    iapply(Ic, Si, m6);
    fcross(Si, fC, sxf);
    iapply(Ic, psi, IcPs);
#pragma unroll
    for (int e = 0; e < 6; ++e) { L.v[i][e] = psi[e]; L.m6[i][e] = m6[e]; L.Sd[i][e] = sxf[e] + IcPs[e]; }
    L.nle[i] = dot6(Si, fC);  // g_i(q)
  }
  __syncthreads();
  if (grav) {
    for (int e = tid; e < NV * NV; e += NT) {
      const int r = e / NV, c = e % NV;
      const bool path = (L.anc[r] >> c) & 1u, above = (L.anc[c] >> r) & 1u;
      sG[r][c] = path ? dot6(L.m6[r], L.v[c]) : (above ? dot6(L.S[r], L.Sd[c]) : 0.0);
    }
    if (tid < NV) {  // W, lu and the rows' value, component tid
      double w = 0.0;
      for (int r = 0; r < rows.n; ++r)
        if (taken(r, AGX_RES_CONTROL_GRAV)) {
          const double *tile = L.w.c.ref + (rows.off[r] - lo);
          w += tile[0] * tile[1 + rows.nref[r] + tid];
        }
      const double res = L.u[tid] - L.nle[tid];
      L.D[tid] = s * w;
      L.lu[tid] = s * w * res;
      L.cpart[tid] = 0.5 * w * res * res;
    }
  }
  __syncthreads();
  if (grav)  // A = tq - G in place
    for (int e = tid; e < NV * LDM; e += NT) (&L.tq[0][0])[e] -= (&sG[0][0])[e];

  // ---- FrameVelocity rows, one after the other: wave 0 forms Rq | Rv, then every wave its tile of Rq' W Rq, Rq' W Rv, Rv' W Rv
  const agx_v4d zero4 = {0.0, 0.0, 0.0, 0.0};
  agx_v4d fqq = zero4, fqv = zero4, fvv = zero4;
  double cost_fv = 0.0;  // wave 0: the rows' values in row order
  if (fvel)
    for (int r = 0; r < rows.n; ++r) {
      if (!taken(r, AGX_RES_FRAME_VELOCITY)) continue;
      __syncthreads();  // the tiles of the row before have been read
      if (wave == 0) {
        int frame = in.frames ? in.frames[r] : -1;
        if (frame < 0) frame = rows.frame[r];
        cost_fv += wg_frame_velocity_row<NV, PRISM>(L, m, frame, rows.frame_b[r], L.w.c.ref + (rows.off[r] - lo), rows.nref[r], s, lane);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int k = 4 * ks + l4;
        const double w = L.w.c.wJ[k];
        const double aq = L.w.c.J[k][16 * ti + l15], av = L.w.c.J[8 + k][16 * ti + l15];
        const double bq = w * L.w.c.J[k][16 * tj + l15], bv = w * L.w.c.J[8 + k][16 * tj + l15];
        fqq = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bq, fqq, 0, 0, 0);
        fqv = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bv, fqv, 0, 0, 0);
        fvv = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, fvv, 0, 0, 0);
      }
    }
  __syncthreads();

  // ---- ControlGrav: the contraction of wg_node's last phase with (M, A, tv) and W, and G' W G for the aux tile
  agx_v4d hww = zero4, hqw = zero4, hvw = zero4, hqq = zero4, hqv = zero4, hvv = zero4, gwg = zero4;
  if (grav) {
    const int ca = 16 * ti + l15, cb = 16 * tj + l15;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int k = 4 * ks + l4;
      const double d = L.D[k];
      const double aM = wg_op<NV>(L.M, k, ca), aq = wg_op<NV>(L.tq, k, ca), av = wg_op<NV>(L.tv, k, ca), aG = wg_op<NV>(sG, k, ca);
      const double bM = d * wg_op<NV>(L.M, k, cb), bq = d * wg_op<NV>(L.tq, k, cb), bv = d * wg_op<NV>(L.tv, k, cb), bG = d * wg_op<NV>(sG, k, cb);
      hww = __builtin_amdgcn_mfma_f64_16x16x4f64(aM, bM, hww, 0, 0, 0);
      hqw = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bM, hqw, 0, 0, 0);
      hvw = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bM, hvw, 0, 0, 0);
      hqq = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bq, hqq, 0, 0, 0);
      hqv = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bv, hqv, 0, 0, 0);
      hvv = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, hvv, 0, 0, 0);
      gwg = __builtin_amdgcn_mfma_f64_16x16x4f64(aG, bG, gwg, 0, 0, 0);
    }
  }

  if constexpr (DEST == kGenToQp) {
    // ---- the tiles: what the rows add, and the general blocks
    double *qt = out0 + node * Q::SIZE, *ax = out1 + node * A::SIZE, *ag = out2 + node * (3 * A::B2);
    if (grav) {
      wg_add_tile(qt + Q::Hww, hww, ti, tj, lane, NV);
      wg_add_tile(qt + Q::Hqw, hqw, ti, tj, lane, NV);
      wg_add_tile(qt + Q::Hvw, hvw, ti, tj, lane, NV);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { hqq[q] += fqq[q]; hqv[q] += fqv[q]; hvv[q] += fvv[q]; gwg[q] += fqq[q]; }
    wg_add_tile(qt + Q::Hqq, hqq, ti, tj, lane, NV);
    wg_add_tile(qt + Q::Hqv, hqv, ti, tj, lane, NV);
    wg_add_tile(qt + Q::Hvv, hvv, ti, tj, lane, NV);
    wg_add_tile(ax + A::Lqq, gwg, ti, tj, lane, NV);
    wg_store_tile(ag, fqv, ti, tj, lane, NV);
    wg_store_tile(ag + A::B2, fvv, ti, tj, lane, NV);
    for (int e = 2 * tid; e < NV * LDM; e += 2 * NT) {  // Lqu[j][i] = -W_i G[i][j], whole rows
      const int j = e / LDM, i = e % LDM;
      double2 v = make_double2(0.0, 0.0);
      if (grav) {
        if (i < NV) v.x = -L.D[i] * sG[i][j];
        if (i + 1 < NV) v.y = -L.D[i + 1] * sG[i + 1][j];
      }
      *reinterpret_cast<double2 *>(ag + 2 * A::B2 + e) = v;
    }
    if (tid < 3 * NV) {  // gradients: gw += M lu, gx += Lx_fv + [A tv]' lu
      const int which = tid / NV, i = tid % NV;
      double g = which == 0 ? 0.0 : (which == 1 ? L.Lq[i] : L.Lv[i]);
      if (grav) {
        if (which == 0) for (int l = 0; l < NV; ++l) g += L.M[i][l] * L.lu[l];
        else if (which == 1) for (int l = 0; l < NV; ++l) g += L.tq[l][i] * L.lu[l];
        else for (int l = 0; l < NV; ++l) g += L.tv[l][i] * L.lu[l];
      }
      if (!(term && which == 0)) qt[(which == 0 ? Q::gw : (which == 1 ? Q::gx : Q::gx + NV)) + i] += g;
    } else if (grav && tid >= 128 && tid < 128 + NV) {
      const int i = tid - 128;
      ax[A::Luu + i] += L.D[i];
      ax[A::Lu + i] += L.lu[i];
    }
    if (tid == 0) {  // node cost: fixed summation order (wave 0 holds the FrameVelocity values)
      double c = cost_fv;
      if (grav)
        for (int e = 0; e < NV; ++e) c += L.cpart[e];
      qt[Q::cost] += s * c;
    }
  } else {
    // gradient in q of the rows: Lq_fv - G' lu (L.tq holds -G)
    double gq = 0.0;
    if (tid < NV) {
      gq = L.Lq[tid];
      if (grav)
        for (int l = 0; l < NV; ++l) gq += L.tq[l][tid] * L.lu[l];
    }
    double c = cost_fv;
    if (tid == 0 && grav)
      for (int e = 0; e < NV; ++e) c += L.cpart[e];
    if constexpr (DEST == kGenToCanonical) {
      typedef TileOff<NV> TO;
      double *tile = out0 + node * TO::SIZE;
#pragma unroll
      for (int q = 0; q < 4; ++q) gwg[q] += fqq[q];
      wg_scatter(gwg, ti, tj, lane, [&](int r, int cc, double val) { if (r < NV && cc < NV) tile[TO::Lxx + r * NX + cc] += val; });
      wg_scatter(fqv, ti, tj, lane, [&](int r, int cc, double val) {
        if (r < NV && cc < NV) { tile[TO::Lxx + r * NX + NV + cc] += val; tile[TO::Lxx + (NV + cc) * NX + r] += val; }
      });
      wg_scatter(fvv, ti, tj, lane, [&](int r, int cc, double val) { if (r < NV && cc < NV) tile[TO::Lxx + (NV + r) * NX + NV + cc] += val; });
      if (grav)
        for (int e = tid; e < NV * NV; e += NT) {
          const int j = e / NV, i = e % NV;
          tile[TO::Lxu + j * NV + i] += -L.D[i] * sG[i][j];
        }
      if (tid < NV) {
        tile[TO::Lx + tid] += gq;
        tile[TO::Lx + NV + tid] += L.Lv[tid];
        if (grav) { tile[TO::Lu + tid] += L.lu[tid]; tile[TO::Luu + tid * NV + tid] += L.D[tid]; }
      }
      if (tid == 0) tile[TO::cost] += s * c;
    } else {
      const long long item = node * R + only;
      if (tid < NV) {
        out1[item * NX + tid] = gq;
        out1[item * NX + NV + tid] = L.Lv[tid];
        if (grav) out2[item * NV + tid] = L.lu[tid];
      }
      if (tid == 0) out0[item] = c;
    }
  }
}

// K3 of large models with every block (k_node_kkt_big plus the general blocks of auxg, identities above k_node_kkt_gen):
//   Lu + Fu' lam' = -(Lqu' dq + (Luu + preg) du)
//   Lx + Fx' lam' - lam = -(Lxx dx + Lxu du + dreg dx),  Lxx = [[Lqq, Lqv], [Lqv', diag(Lvv) + Lvvd]]
// 32 lanes per node, lane l = column l of every matrix row: the products with a row are sum32 butterflies, the products with a
// column (Lqu' dq, Lqv' dq) are accumulated on the column's lane from the broadcast entry of dq.
template <int NV>
__global__ void __launch_bounds__(64) k_node_kkt_big_gen(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                         const double *__restrict__ auxs, const double *__restrict__ auxg,
                                                         const double *__restrict__ dxs, const double *__restrict__ wss,
                                                         double *__restrict__ dus, double *__restrict__ nodestat,
                                                         const DevState *__restrict__ st) {
  static_assert(NV <= 32, "a matrix row per 32 lanes");
  constexpr int NX = 2 * NV;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  const DevOcp &o = *op;
  const int T = o.T, l = threadIdx.x & 31, half = threadIdx.x & 32;
  const long long n_nodes = (long long)o.B * (T + 1);
  const long long node_raw = (long long)blockIdx.x * 2 + (threadIdx.x >> 5);
  const bool ok = node_raw < n_nodes;
  const long long node = ok ? node_raw : n_nodes - 1;
  const int b = (int)(node / (T + 1)), t = (int)(node % (T + 1));
  const DevState &S = st[b];
  const bool act = ok && !S.done;
  if (!__any(act)) return;  // both nodes of the wave finished
  const double preg = S.preg, dreg = S.dreg;
  const double *qt = qts + node * Q::SIZE;
  const double *ax = auxs + node * A::SIZE;
  const double *ag = auxg + node * (3 * A::B2);
  const double *Lqv = ag, *Lvvd = ag + A::B2, *Lqu = ag + 2 * A::B2;
  const double *dx = dxs + node * NX;
  const bool in = l < NV;
  const int lc = in ? l : 0;
  const double m = in ? 1.0 : 0.0;
  const double dq = dx[lc] * m, dv = dx[NV + lc] * m;
  double kkt = 0.0, gap = 0.0;
  if (t < T) {  // uniform over the node's 32 lanes
    const double fq = qt[Q::f + lc] * m, fv = qt[Q::f + NV + lc] * m;
    kkt = fmax(fabs(fq), fabs(fv));
    gap = fabs(fq) + fabs(fv);
  }
  const double w = (t < T) ? wss[((long long)b * T + t) * NV + lc] * m : 0.0;
  const double tm = (t < T) ? 1.0 : 0.0, sm = (t > 0) ? 1.0 : 0.0;
  double du = 0.0, hq = 0.0, hv = 0.0, cu = 0.0, cv = 0.0;  // row sums of row l; column sums Lqu' dq, Lqv' dq of column l
#pragma unroll 2
  for (int i = 0; i < NV; ++i) {
    const double p = (ax[A::M + i * A::LD + lc] * w + ax[A::tq + i * A::LD + lc] * dq + ax[A::tv + i * A::LD + lc] * dv) * tm;
    const double q = ax[A::Lqq + i * A::LD + lc] * dq + Lqv[i * A::LD + lc] * dv;
    const double r = Lvvd[i * A::LD + lc] * dv;
    const double dqi = __shfl(dq, half + i, 64);
    cu += Lqu[i * A::LD + lc] * dqi;
    cv += Lqv[i * A::LD + lc] * dqi;
    const double s = sum32(p), h = sum32(q), g = sum32(r);
    if (l == i) { du = s; hq = h; hv = g; }
  }
#pragma unroll 2
  for (int i = 0; i < NV; ++i) {  // Lxu du needs every component of du
    const double h = sum32(Lqu[i * A::LD + lc] * du);
    if (l == i) hq += h;
  }
  if (in) {
    if (t < T) {
      if (act) dus[((long long)b * T + t) * NV + l] = du;
      kkt = fmax(kkt, fabs((ax[A::Luu + l] + preg) * du + cu));
    }
    kkt = fmax(kkt, sm * fmax(fabs(hq + dreg * dq), fabs((ax[A::Lvv + l] + dreg) * dv + hv + cv)));
  }
  kkt = max32(kkt);
  gap = sum32(gap);
  if (act && l == 0) {
    double *ns = nodestat + node * 4;
    ns[0] = kkt; ns[1] = qt[Q::cost]; ns[2] = gap;
    if (!o.has_con) ns[3] = 0.0;  // as k_node_kkt_big
  }
}

}  // namespace agx
