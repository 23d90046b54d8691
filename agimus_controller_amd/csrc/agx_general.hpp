// agimus_controller_amd -- cost rows whose Gauss-Newton Hessian does not fit the structure the fast
// kernels exploit ({dense qq, diagonal vv, diagonal uu}, Lxu = 0):
//
//   ResidualModelControlGrav    r = u - g(q)                       (ocp_croco_generic.py:186-194)
//       Rq = -dg/dq, Ru = I  ->  Lqq, Lqu (dense), Luu (diagonal)
//   ResidualModelFrameVelocity  r = v_frame(q, qd) - v_ref         (ocp_croco_generic.py:360-432)
//       reference frame WORLD / LOCAL / LOCAL_WORLD_ALIGNED (row field frame_b = 0 / 1 / 2)
//       Rq, Rv dense  ->  Lqq, Lqv, Lvv (dense)
//
// Problems with such rows run on the one-lane-per-node kernels instantiated with GEN = true
// (correctness path, nv <= 7); the extra Hessian blocks travel in CostGen next to CostAcc.
// Large models (capacities 16 / 30 / 32): agx_general_rows.hpp restates this arithmetic for the
// workgroup-per-node path (k_general_rows_wg behind k_calc_qp_wg, k_node_kkt_big_gen).
//
// (included by agx_device.hpp users after node_costs is defined)
#pragma once

namespace agx {

template <int NV>
struct CostGen {
  double Lqv[NV][NV];   // d2/dq dv
  double Lvvd[NV][NV];  // dense part of d2/dv2 (CostAcc::Lvv keeps the diagonal rows' share)
  double Lqu[NV][NV];   // d2/dq du
};

AGX_DEV bool row_is_general(int kind) { return kind == AGX_RES_CONTROL_GRAV || kind == AGX_RES_FRAME_VELOCITY; }

// Frame velocity [linear; angular] in the requested reference frame and (DIFF) its partial
// derivatives Rq, Rv (6 x nv).  World-frame spatial algebra: k.S[j] is joint j's axis seen at the world
// origin, v0 = sum_{j on the path} S_j qd_j, d v0 / d q_k = S_k x (part of v0 contributed below k).
template <int NV, bool CHAIN, bool DIFF>
AGX_DEV void frame_velocity(const DevModel &m, const Kin<NV> &k, int frame, int type, const double *qd, double *vel,
                            double (*Rq)[NV], double (*Rv)[NV]) {
  double RF[9], pF[3];
  int jf;
  frame_world<NV>(m, k, frame, RF, pF, &jf);
  double v0[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const bool on = (jf >= 0) && (CHAIN ? (j <= jf) : ((m.anc[jf >= 0 ? jf : 0] >> j) & 1u));
    if (on) {
#pragma unroll
      for (int e = 0; e < 6; ++e) v0[e] += k.S[j][e] * qd[j];
    }
  }
  // value in LOCAL_WORLD_ALIGNED form: velocity of the frame origin, world axes
  double wxp[3], lwa[6];
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
  if (!DIFF) return;
#pragma unroll
  for (int kk = 0; kk < NV; ++kk) {
    const bool on = (jf >= 0) && (CHAIN ? (kk <= jf) : ((m.anc[jf >= 0 ? jf : 0] >> kk) & 1u));
    double dq[6] = {0, 0, 0, 0, 0, 0}, dv[6] = {0, 0, 0, 0, 0, 0};
    if (on) {
      // below = contribution to v0 of the joints strictly below kk on the path
      double below[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const bool onj = (jf >= 0) && (CHAIN ? (j <= jf) : ((m.anc[jf >= 0 ? jf : 0] >> j) & 1u));
        const bool under = CHAIN ? (j > kk) : (j != kk && ((m.anc[j] >> kk) & 1u));
        if (onj && under) {
#pragma unroll
          for (int e = 0; e < 6; ++e) below[e] += k.S[j][e] * qd[j];
        }
      }
      double dW[6];
      mcross(k.S[kk], below, dW);  // WORLD: d v0 / d q_kk ;  d v0 / d qd_kk = S_kk
      if (type == 0) {
#pragma unroll
        for (int e = 0; e < 6; ++e) { dq[e] = dW[e]; dv[e] = k.S[kk][e]; }
      } else {
        // LOCAL_WORLD_ALIGNED: lin = v0_lin + w x pF,  d pF / d q_kk = z x (pF - p_kk) (prismatic: S_lin; there z = S_ang = 0)
        const double *z = k.S[kk] + 3;
        double d[3], dp[3], t1[3], t2[3], t3[3];
        d[0] = pF[0] - k.p[kk][0]; d[1] = pF[1] - k.p[kk][1]; d[2] = pF[2] - k.p[kk][2];
        cross3(z, d, dp);
        prismatic_column(is_prismatic<NV, CHAIN>(m, kk), k.S[kk], dp);
        cross3(dW + 3, pF, t1);
        cross3(v0 + 3, dp, t2);
        cross3(z, pF, t3);
        double lq[6], lv[6];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          lq[e] = dW[e] + t1[e] + t2[e]; lq[3 + e] = dW[3 + e];
          lv[e] = k.S[kk][e] + t3[e];    lv[3 + e] = z[e];
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
#pragma unroll
    for (int e = 0; e < 6; ++e) { Rq[e][kk] = dq[e]; Rv[e][kk] = dv[e]; }
  }
}

// The general rows of one node: adds to the accumulators of node_costs (call it first) and fills the
// extra blocks.  DIFF = false: value only (line search).
template <int NV, bool CHAIN, bool TERM, bool DIFF>
AGX_DEV void node_costs_general(const DevModel &m, const DevRows &rows, const Kin<NV> &k, const double *x, const double *u,
                                const double *ref, const int *frames, CostAcc<NV> &c, CostGen<NV> &g) {
  if (DIFF) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < NV; ++j) { g.Lqv[i][j] = 0.0; g.Lvvd[i][j] = 0.0; g.Lqu[i][j] = 0.0; }
  }
  for (int r = 0; r < rows.n; ++r) {
    if (!rows.active[r]) continue;
    const int kind = rows.kind[r];
    if (!row_is_general(kind)) continue;
    const double *tile = ref + rows.off[r];
    const double wi = tile[0];
    const double *rr = tile + 1;
    const double *aw = rr + rows.nref[r];
    if (kind == AGX_RES_CONTROL_GRAV) {
      if (TERM) continue;
      // g(q) = nle(q, 0); dg/dq = RNEA derivative at zero velocity and acceleration
      Dyn<NV> d0;
      double g0[NV], M0[NV][NV], zero[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) zero[i] = 0.0;
      bias_and_inertia<NV, CHAIN>(m, k, zero, d0, g0, M0);
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < NV; ++i) a += 0.5 * aw[i] * (u[i] - g0[i]) * (u[i] - g0[i]);
      c.cost += wi * a;
      if (DIFF) {
        double Gq[NV][NV], Gv[NV][NV];
        rnea_derivatives<NV, CHAIN>(m, k, d0, zero, zero, Gq, Gv);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const double w = wi * aw[i], wr = w * (u[i] - g0[i]);
          c.Lu[i] += wr;
          c.Luu[i] += w;
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            c.Lq[j] -= Gq[i][j] * wr;
            g.Lqu[j][i] -= w * Gq[i][j];
#pragma unroll
            for (int l = 0; l < NV; ++l) c.Lqq[j][l] += w * Gq[i][j] * Gq[i][l];
          }
        }
      }
    } else {  // AGX_RES_FRAME_VELOCITY
      int frame = frames ? frames[r] : -1;
      if (frame < 0) frame = rows.frame[r];
      double vel[6], Rq[6][NV], Rv[6][NV];
      frame_velocity<NV, CHAIN, DIFF>(m, k, frame, rows.frame_b[r], x + NV, vel, Rq, Rv);
      double a = 0.0, wr[6];
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const double res = vel[e] - rr[e];
        a += 0.5 * aw[e] * res * res;
        wr[e] = wi * aw[e] * res;
      }
      c.cost += wi * a;
      if (DIFF) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          double gq = 0.0, gv = 0.0;
#pragma unroll
          for (int e = 0; e < 6; ++e) { gq += Rq[e][i] * wr[e]; gv += Rv[e][i] * wr[e]; }
          c.Lq[i] += gq;
          c.Lv[i] += gv;
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            double hqq = 0.0, hqv = 0.0, hvv = 0.0;
#pragma unroll
            for (int e = 0; e < 6; ++e) {
              const double w = wi * aw[e];
              hqq += w * Rq[e][i] * Rq[e][j];
              hqv += w * Rq[e][i] * Rv[e][j];
              hvv += w * Rv[e][i] * Rv[e][j];
            }
            c.Lqq[i][j] += hqq;
            g.Lqv[i][j] += hqv;
            g.Lvvd[i][j] += hvv;
          }
        }
      }
    }
  }
}

}  // namespace agx
