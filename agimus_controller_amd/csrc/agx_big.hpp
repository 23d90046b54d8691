// agimus_controller_amd -- large models (7 < nv <= 32, e.g. the 30-DoF humanoid of BASELINE configs[4]): the node-parallel kernels.
//
// Same tiles (row stride 32), same acceleration-input QP, same outputs as the nv <= 7 path, one node (or one instance and
// node) per wave or workgroup, no recursion over the horizon:
//   k_node_kkt_big, k_node_kkt_gen        K3: du and the KKT / cost / gap share of every node
//   k_admm_tile_big, k_admm_update_big    the node kernels of the ADMM loop (constraints, agx_admm.hpp)
//   k_sigma_tile_big                      the sigma-augmented tiles of the exit path (feedback gains)
//   k_gains_to_u_big, k_gains_to_u_mfma   K = M Kw - taux
// The serial part, the Riccati sweep, is k_riccati_blk (agx_big_k2.hpp); the derivative pass and the line-search trials
// are the workgroup-per-node kernels of agx_big_k1.hpp (LDS + fp64 MFMA, no scratch).
//
// (included at the end of agx_kernels.hpp)
#pragma once

namespace agx {

// K3 for large nv (see k_node_kkt for the identities): 32 lanes per node, lane l = column l of every matrix row (one
// coalesced 256-byte row load per matrix and row), the row sums  du_i = sum_l M[i][l] w_l + tq[i][l] dq_l + tv[i][l] dv_l
// and  (Lqq dq)_i  as 32-lane butterflies on the VALU (DPP inside the 16-lane rows, v_permlane16_swap across them).
// One lane per node with serial loops (round 1) read its 31 KB at 3 TB/s with 0.4 waves per SIMD.
__device__ __forceinline__ double sum32(double p) {
  p += dpp_xor1(p); p += dpp_xor2(p); p += dpp_xor4(p);
  p += dpp_mov<0x128>(p);  // row_ror:8
  const unsigned lo = __double2loint(p), hi = __double2hiint(p);
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  const u2 a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), c = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double(c.x, a.x) + __hiloint2double(c.y, a.y);
}
__device__ __forceinline__ double max32(double p) {
  p = fmax(p, dpp_xor1(p)); p = fmax(p, dpp_xor2(p)); p = fmax(p, dpp_xor4(p));
  p = fmax(p, dpp_mov<0x128>(p));
  const unsigned lo = __double2loint(p), hi = __double2hiint(p);
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  const u2 a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), c = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return fmax(__hiloint2double(c.x, a.x), __hiloint2double(c.y, a.y));
}
template <int NV>
__global__ void __launch_bounds__(64) k_node_kkt_big(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                     const double *__restrict__ auxs, const double *__restrict__ dxs,
                                                     const double *__restrict__ wss, double *__restrict__ dus,
                                                     double *__restrict__ nodestat, const DevState *__restrict__ st) {
  static_assert(NV <= 32, "a matrix row per 32 lanes");
  constexpr int NX = 2 * NV;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  const DevOcp &o = *op;
  const int T = o.T, l = threadIdx.x & 31;
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
  // the butterflies run on whole waves: both nodes walk the rows together, a terminal node with zero operands
  const double w = (t < T) ? wss[((long long)b * T + t) * NV + lc] * m : 0.0;
  const double tm = (t < T) ? 1.0 : 0.0, sm = (t > 0) ? 1.0 : 0.0;
  double du = 0.0, hq = 0.0;
#pragma unroll 2
  for (int i = 0; i < NV; ++i) {
    const double p = (ax[A::M + i * A::LD + lc] * w + ax[A::tq + i * A::LD + lc] * dq + ax[A::tv + i * A::LD + lc] * dv) * tm;
    const double q = ax[A::Lqq + i * A::LD + lc] * dq;
    const double s = sum32(p), h = sum32(q);
    if (l == i) { du = s; hq = h; }
  }
  if (in) {
    if (t < T) {
      if (act) dus[((long long)b * T + t) * NV + l] = du;
      kkt = fmax(kkt, fabs((ax[A::Luu + l] + preg) * du));
    }
    kkt = fmax(kkt, sm * fmax(fabs(hq + dreg * dq), fabs((ax[A::Lvv + l] + dreg) * dv)));
  }
  kkt = max32(kkt);
  gap = sum32(gap);
  if (act && l == 0) {
    double *ns = nodestat + node * 4;
    ns[0] = kkt; ns[1] = qt[Q::cost]; ns[2] = gap;
    if (!o.has_con) ns[3] = 0.0;  // constrained problems: the violation share of the constraint evaluation (which may run before this kernel) stays
  }
}

// ---------------------------------------------------------------------------
// Constraints for large models (8 < nv <= 32) through the ADMM loop of agx_admm.hpp: ConstraintModelControlLimit
// (`ocp_croco_generic.py:624-640`: lower / upper bounds on u; identity Jacobian on u, i.e. the rows [taux | M] in the (dx, w)
// coordinates of the QP tiles) and collision-distance rows (`ocp_traj_tracking_collision_avoidance.yaml:48-56`; one Jacobian row
// on q each, k_con_eval_wg in agx_big_k1.hpp).  Correctness-first: every ADMM iteration factorises again (k_riccati_blk on the
// augmented tile; the stored-factor gradient sweeps of the 7-joint path have no counterpart here), the node kernels follow
// k_admm_tile / k_admm_update.  Other constraint kinds are refused for nv > 7.
// ---------------------------------------------------------------------------
// Augmented QP tile of one node (k_admm_tile for large models; instances whose rho changed, or at the first ADMM iteration):
//   H += [taux M]' diag(sigma + rho_u) [taux M] + sigma I_x,    g += [taux M]' (h_u - sigma du_c) - sigma dx_c,   h = y - rho z
// one 256-thread workgroup per node, M | tq | tv staged in LDS, thread (i, j) forms element [i][j] of the six blocks.
template <int NV>
__global__ void __launch_bounds__(256) k_admm_tile_big(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                       double *__restrict__ qt2s, const double *__restrict__ auxs,
                                                       const double *__restrict__ cxs, const double *__restrict__ dus,
                                                       const double *__restrict__ cjac, const double *__restrict__ ys,
                                                       const double *__restrict__ zs, const DevState *__restrict__ st) {
  constexpr int NX = 2 * NV;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  __shared__ double sM[NV * NV], sq[NV * NV], sv[NV * NV], wu[32], eu[32];
  __shared__ double sg[AGX_MAX_DENSE][32], srho[AGX_MAX_DENSE], sh[AGX_MAX_DENSE];  // rows on q: Jacobian row, rho, h = y - rho z
  __shared__ double sxr[2][32], sxh[2][32];  // state bounds: rho and h of the q | v component of every joint
  const DevOcp &o = *op;
  const int T = o.T, tid = threadIdx.x, nt = blockDim.x;
  const long long node = blockIdx.x;
  const int b = (int)(node / (T + 1)), t = (int)(node % (T + 1));
  const DevState &S = st[b];
  if (S.done || S.admm_conv || !S.admm_refactor) return;  // uniform over the workgroup
  const double *qt = qts + node * Q::SIZE;
  double *q2 = qt2s + node * Q::SIZE;
  const double *ax = auxs + node * A::SIZE;
  const double *cx = cxs + node * NX;
  const DevCons &c = o.cons[t == T ? 1 : 0];
  const double sig = kSigma, rs = S.rho_sparse;
  if (t < T) {
    for (int e = tid; e < NV * NV; e += nt) {
      const int i = e / NV, j = e % NV;
      sM[e] = ax[A::M + i * A::LD + j]; sq[e] = ax[A::tq + i * A::LD + j]; sv[e] = ax[A::tv + i * A::LD + j];
    }
    if (tid < NV) {
      double w = sig, h = 0.0;
      for (int r = 0; r < c.n; ++r) {
        if (c.kind[r] != AGX_RES_CONTROL) continue;
        const int k = c.off[r] + tid;
        const double rho = admm_rho(c.lb[k], c.ub[k], rs);
        w += rho;
        h += ys[node * AGX_MAX_NC + k] - rho * zs[node * AGX_MAX_NC + k];
      }
      wu[tid] = w;
      eu[tid] = h - sig * dus[((long long)b * T + t) * NV + tid];
    }
  }
  if (tid < NV) {
    double rq = 0.0, rv = 0.0, hq = 0.0, hv = 0.0;
    for (int r = 0; r < c.n; ++r) {
      if (c.kind[r] != AGX_RES_STATE) continue;
      const int kq = c.off[r] + tid, kv = kq + NV;
      const double a = admm_rho(c.lb[kq], c.ub[kq], rs), bb = admm_rho(c.lb[kv], c.ub[kv], rs);
      rq += a; rv += bb;
      hq += ys[node * AGX_MAX_NC + kq] - a * zs[node * AGX_MAX_NC + kq];
      hv += ys[node * AGX_MAX_NC + kv] - bb * zs[node * AGX_MAX_NC + kv];
    }
    sxr[0][tid] = rq; sxr[1][tid] = rv; sxh[0][tid] = hq; sxh[1][tid] = hv;
  }
  int nd = 0;  // dense rows of this node type (uniform)
  for (int r = 0; r < c.n; ++r)
    if (c.kind[r] != AGX_RES_CONTROL && c.kind[r] != AGX_RES_STATE)  // rows with Jacobian rows on q: collision distance (1), frame translation / rotation (3), placement (6)
      for (int e = 0; e < c.nr[r]; ++e) {
        const int k = c.off[r] + e;
        if (tid < 32) sg[nd][tid] = tid < NV ? cjac[(node * AGX_MAX_DENSE + c.coll_slot[r] + e) * 32 + tid] : 0.0;
        if (tid == 32) {
          const double rho = admm_rho(c.lb[k], c.ub[k], rs);
          srho[nd] = rho;
          sh[nd] = ys[node * AGX_MAX_NC + k] - rho * zs[node * AGX_MAX_NC + k];
        }
        ++nd;
      }
  __syncthreads();
  for (int e = tid; e < NV * NV; e += nt) {
    const int i = e / NV, j = e % NV;
    double hww = 0.0, hqw = 0.0, hvw = 0.0, hqq = 0.0, hqv = 0.0, hvv = 0.0;
    if (t < T)
      for (int l = 0; l < NV; ++l) {
        const double d = wu[l];
        const double Mli = sM[l * NV + i], tqli = sq[l * NV + i], tvli = sv[l * NV + i];
        const double Mlj = d * sM[l * NV + j], tqlj = d * sq[l * NV + j], tvlj = d * sv[l * NV + j];
        hww += Mli * Mlj; hqw += tqli * Mlj; hvw += tvli * Mlj;
        hqq += tqli * tqlj; hqv += tqli * tvlj; hvv += tvli * tvlj;
      }
    for (int s = 0; s < nd; ++s) hqq += srho[s] * sg[s][i] * sg[s][j];  // rho g g' of the rows on q
    const double d = (i == j) ? sig : 0.0;
    const int o2 = i * Q::LD + j;
    q2[Q::Hqq + o2] = qt[Q::Hqq + o2] + hqq + d + ((i == j) ? sxr[0][i] : 0.0);
    q2[Q::Hqv + o2] = qt[Q::Hqv + o2] + hqv;
    q2[Q::Hvv + o2] = qt[Q::Hvv + o2] + hvv + d + ((i == j) ? sxr[1][i] : 0.0);
    if (t < T) {
      q2[Q::Hww + o2] = qt[Q::Hww + o2] + hww;
      q2[Q::Hqw + o2] = qt[Q::Hqw + o2] + hqw;
      q2[Q::Hvw + o2] = qt[Q::Hvw + o2] + hvw;
    }
  }
  if (tid < NV) {  // gradient, gap, cost
    const int i = tid;
    double gw = 0.0, gq = -sig * cx[i] + sxh[0][i], gv = -sig * cx[NV + i] + sxh[1][i];
    if (t < T)
      for (int l = 0; l < NV; ++l) { gw += sM[l * NV + i] * eu[l]; gq += sq[l * NV + i] * eu[l]; gv += sv[l * NV + i] * eu[l]; }
    for (int s = 0; s < nd; ++s) gq += sh[s] * sg[s][i];
    if (t < T) q2[Q::gw + i] = qt[Q::gw + i] + gw;
    q2[Q::gx + i] = qt[Q::gx + i] + gq;
    q2[Q::gx + NV + i] = qt[Q::gx + NV + i] + gv;
    q2[Q::f + i] = qt[Q::f + i];
    q2[Q::f + NV + i] = qt[Q::f + NV + i];
  }
  if (tid == 255) q2[Q::cost] = qt[Q::cost];
}

// After the sweep on the augmented tiles (k_admm_update for large models, control-limit rows): du, z / y update, the node's
// shares of the ADMM residual norms and of the KKT residual, the gradient of the next iteration's augmented tile.
// 32 lanes per node, lane l = component l / column l of every matrix row (as k_node_kkt_big).
template <int NV>
__global__ void __launch_bounds__(64) k_admm_update_big(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                        const double *__restrict__ auxs, const double *__restrict__ dxs,
                                                        const double *__restrict__ wss, double *__restrict__ dus,
                                                        double *__restrict__ cxs, const double *__restrict__ cg,
                                                        const double *__restrict__ cjac, double *__restrict__ ys, double *__restrict__ zs,
                                                        double *__restrict__ nodestat, double *__restrict__ admmstat,
                                                        double *__restrict__ qt2s, const DevState *__restrict__ st) {
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
  const bool act = ok && !S.done && !S.admm_conv && !S.dir_fail;
  if (!__any(act)) return;
  const double preg = S.preg, dreg = S.dreg, rs = S.rho_sparse, sig = kSigma;
  const double *qt = qts + node * Q::SIZE;
  const double *ax = auxs + node * A::SIZE;
  const double *dx = dxs + node * NX;
  double *cx = cxs + node * NX;
  double *y = ys + node * AGX_MAX_NC, *z = zs + node * AGX_MAX_NC;
  const double *g = cg + node * AGX_MAX_NC;
  const DevCons &c = o.cons[t == T ? 1 : 0];
  const bool in = l < NV;
  const int lc = in ? l : 0;
  const double m = in ? 1.0 : 0.0;
  const double dq = dx[lc] * m, dv = dx[NV + lc] * m, cq = cx[lc] * m, cv = cx[NV + lc] * m;
  double kkt = 0.0, gap = 0.0;
  if (t < T) {
    const double fq = qt[Q::f + lc] * m, fv = qt[Q::f + NV + lc] * m;
    kkt = fmax(fabs(fq), fabs(fv));
    gap = fabs(fq) + fabs(fv);
  }
  const double w = (t < T) ? wss[((long long)b * T + t) * NV + lc] * m : 0.0;
  const double tm = (t < T) ? 1.0 : 0.0, sm = (t > 0) ? 1.0 : 0.0;
  double du = 0.0, hq = 0.0;
#pragma unroll 2
  for (int i = 0; i < NV; ++i) {
    const double p = (ax[A::M + i * A::LD + lc] * w + ax[A::tq + i * A::LD + lc] * dq + ax[A::tv + i * A::LD + lc] * dv) * tm;
    const double q = ax[A::Lqq + i * A::LD + lc] * dq;
    const double s = sum32(p), h = sum32(q);
    if (l == i) { du = s; hq = h; }
  }
  const double duc = (t < T && in) ? dus[((long long)b * T + t) * NV + l] : 0.0;
  // control-limit rows: component l on lane l, C d = du
  double primal = 0.0, primal_rel = 0.0, dual_u = 0.0, drel_u = 0.0, e_u = 0.0, hn_u = 0.0;
  if (in && t < T)
    for (int r = 0; r < c.n; ++r) {
      if (c.kind[r] != AGX_RES_CONTROL) continue;
      const int k = c.off[r] + l;
      const double rho = admm_rho(c.lb[k], c.ub[k], rs);
      const double z0 = z[k], y0 = y[k];
      const double zrel = kAlphaRelax * du + (1.0 - kAlphaRelax) * z0;
      double zn = zrel + y0 / rho;
      zn = fmin(fmax(zn, c.lb[k] - g[k]), c.ub[k] - g[k]);
      const double yn = y0 + rho * (zrel - zn);
      primal = fmax(primal, fabs(du - zn));
      primal_rel = fmax(primal_rel, fmax(fabs(du), fabs(zn)));
      dual_u += rho * (zn - z0);
      drel_u += yn;
      e_u += rho * du + (y0 - rho * z0) - yn;
      hn_u += yn - rho * zn;
      if (act) { z[k] = zn; y[k] = yn; }
    }
  // rows on q (collision distance, frame residuals): one Jacobian row per component, C d = g . dq (the same on the 32 lanes of the node)
  double dual_q = 0.0, drel_q = 0.0, e_q = 0.0, hn_q = 0.0;
  double dual_v = 0.0, drel_v = 0.0, e_v = 0.0, hn_v = 0.0;
  if (in)
    for (int r = 0; r < c.n; ++r) {  // state bounds: components q_l and v_l on lane l
      if (c.kind[r] != AGX_RES_STATE) continue;
#pragma unroll
      for (int hv = 0; hv < 2; ++hv) {
        const int k = c.off[r] + hv * NV + l;
        const double Cd = hv ? dv : dq;
        const double rho = admm_rho(c.lb[k], c.ub[k], rs);
        const double z0 = z[k], y0 = y[k];
        const double zrel = kAlphaRelax * Cd + (1.0 - kAlphaRelax) * z0;
        double zn = zrel + y0 / rho;
        zn = fmin(fmax(zn, c.lb[k] - g[k]), c.ub[k] - g[k]);
        const double yn = y0 + rho * (zrel - zn);
        primal = fmax(primal, fabs(Cd - zn));
        primal_rel = fmax(primal_rel, fmax(fabs(Cd), fabs(zn)));
        const double dz = rho * (zn - z0), de = rho * Cd + (y0 - rho * z0) - yn, hn = yn - rho * zn;
        if (hv) { dual_v += dz; drel_v += yn; e_v += de; hn_v += hn; }
        else { dual_q += dz; drel_q += yn; e_q += de; hn_q += hn; }
        if (act) { z[k] = zn; y[k] = yn; }
      }
    }
  for (int r = 0; r < c.n; ++r)
  for (int e = 0; e < ((c.kind[r] != AGX_RES_CONTROL && c.kind[r] != AGX_RES_STATE) ? c.nr[r] : 0); ++e) {
    const int k = c.off[r] + e;
    const double gq = in ? cjac[(node * AGX_MAX_DENSE + c.coll_slot[r] + e) * 32 + l] : 0.0;
    const double Cd = sum32(gq * dq);
    const double rho = admm_rho(c.lb[k], c.ub[k], rs);
    const double z0 = z[k], y0 = y[k];
    const double zrel = kAlphaRelax * Cd + (1.0 - kAlphaRelax) * z0;
    double zn = zrel + y0 / rho;
    zn = fmin(fmax(zn, c.lb[k] - g[k]), c.ub[k] - g[k]);
    const double yn = y0 + rho * (zrel - zn);
    primal = fmax(primal, fabs(Cd - zn));
    primal_rel = fmax(primal_rel, fmax(fabs(Cd), fabs(zn)));
    dual_q += gq * rho * (zn - z0);
    drel_q += gq * yn;
    e_q += gq * (rho * Cd + (y0 - rho * z0) - yn);
    hn_q += gq * (yn - rho * zn);
    __builtin_amdgcn_wave_barrier();  // every lane has read z0, y0
    if (act && l == 0) { z[k] = zn; y[k] = yn; }
  }
  if (in) {
    if (t < T) kkt = fmax(kkt, fabs((ax[A::Luu + l] + preg) * du + sig * (du - duc) + e_u));
    kkt = fmax(kkt, sm * fmax(fabs(hq + dreg * dq + sig * (dq - cq) + e_q), fabs((ax[A::Lvv + l] + dreg) * dv + sig * (dv - cv) + e_v)));
  }
  kkt = max32(kkt);
  gap = sum32(gap);
  primal = max32(primal);
  primal_rel = max32(primal_rel);
  const double dual = max32(fmax(fabs(dual_u), fmax(fabs(dual_q), fabs(dual_v)))), drel = max32(fmax(fabs(drel_u), fmax(fabs(drel_q), fabs(drel_v))));
  // gradient of the next iteration's augmented tile:  g = g0 + [taux M]' (h_u - sigma du) - sigma dx
  const double e_own = (t < T && in) ? hn_u - sig * du : 0.0;
  double gwn = 0.0, gqn = hn_q - sig * dq, gvn = hn_v - sig * dv;
  for (int k = 0; k < NV; ++k) {
    const double e = __shfl(e_own, half + k, 64);
    gwn += ax[A::M + k * A::LD + lc] * e * tm;
    gqn += ax[A::tq + k * A::LD + lc] * e * tm;
    gvn += ax[A::tv + k * A::LD + lc] * e * tm;
  }
  if (act) {
    if (in) {
      double *q2 = qt2s + node * Q::SIZE;
      if (t < T) q2[Q::gw + l] = qt[Q::gw + l] + gwn;
      q2[Q::gx + l] = qt[Q::gx + l] + gqn;
      q2[Q::gx + NV + l] = qt[Q::gx + NV + l] + gvn;
      if (t < T) dus[((long long)b * T + t) * NV + l] = du;
      cx[l] = dq; cx[NV + l] = dv;  // prox centre of the next iteration
    }
    if (l == 0) {
      double *ns = nodestat + node * 4;
      ns[0] = kkt; ns[1] = qt[Q::cost]; ns[2] = gap;
      double *as = admmstat + node * 4;
      as[0] = primal; as[1] = dual; as[2] = primal_rel; as[3] = drel;
    }
  }
}

// K3 for problems with general cost rows (agx_general.hpp): the optimality identities with every block,
//   Lu + Fu' lam' = -(Lqu' dq + (Luu + preg) du)
//   Lx + Fx' lam' - lam = -(Lxx dx + Lxu du + dreg dx),  Lxx = [[Lqq, Lqv], [Lqv', diag(Lvv) + Lvvd]]
// one lane per node; auxg = Lqv | Lvvd | Lqu of the node.
template <int NV>
__global__ void __launch_bounds__(64) k_node_kkt_gen(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                     const double *__restrict__ auxs, const double *__restrict__ auxg,
                                                     const double *__restrict__ dxs, const double *__restrict__ wss,
                                                     double *__restrict__ dus, double *__restrict__ nodestat,
                                                     const DevState *__restrict__ st) {
  constexpr int NX = 2 * NV;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  const DevOcp &o = *op;
  const int T = o.T;
  const long long node = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= (long long)o.B * (T + 1)) return;
  const int b = (int)(node / (T + 1)), t = (int)(node % (T + 1));
  const DevState &S = st[b];
  if (S.done) return;
  const double preg = S.preg, dreg = S.dreg;
  const double *qt = qts + node * Q::SIZE;
  const double *ax = auxs + node * A::SIZE;
  const double *ag = auxg + node * (3 * A::B2);
  const double *Lqv = ag, *Lvvd = ag + A::B2, *Lqu = ag + 2 * A::B2;
  const double *dx = dxs + node * NX;
  double kkt = 0.0, gap = 0.0, du[NV];
  for (int i = 0; i < NV; ++i) du[i] = 0.0;
  if (t < T) {
    const double *w = wss + ((long long)b * T + t) * NV;
    for (int i = 0; i < NX; ++i) { kkt = fmax(kkt, fabs(qt[Q::f + i])); gap += fabs(qt[Q::f + i]); }
    for (int i = 0; i < NV; ++i) {
      double s = 0.0;
      for (int l = 0; l < NV; ++l)
        s += ax[A::M + i * A::LD + l] * w[l] + ax[A::tq + i * A::LD + l] * dx[l] + ax[A::tv + i * A::LD + l] * dx[NV + l];
      du[i] = s;
      dus[((long long)b * T + t) * NV + i] = s;
    }
    for (int i = 0; i < NV; ++i) {
      double s = (ax[A::Luu + i] + preg) * du[i];
      for (int l = 0; l < NV; ++l) s += Lqu[l * A::LD + i] * dx[l];
      kkt = fmax(kkt, fabs(s));
    }
  }
  if (t > 0)
    for (int i = 0; i < NV; ++i) {
      double hq = dreg * dx[i], hv = (ax[A::Lvv + i] + dreg) * dx[NV + i];
      for (int j = 0; j < NV; ++j) {
        hq += ax[A::Lqq + i * A::LD + j] * dx[j] + Lqv[i * A::LD + j] * dx[NV + j] + Lqu[i * A::LD + j] * du[j];
        hv += Lqv[j * A::LD + i] * dx[j] + Lvvd[i * A::LD + j] * dx[NV + j];
      }
      kkt = fmax(kkt, fmax(fabs(hq), fabs(hv)));
    }
  double *ns = nodestat + node * 4;
  ns[0] = kkt; ns[1] = qt[Q::cost]; ns[2] = gap;
  if (!o.has_con) ns[3] = 0.0;  // as k_node_kkt
}

// Exit path for large nv: the Hessian blocks of every node with CSQP's proximal terms,
//   H + sigma ([taux M]' [taux M] + I_x),  into a second tile; one 256-thread workgroup per node,
// M | tq | tv staged in LDS, thread (i, j) forms element [i][j] of the six blocks.
template <int NV>
__global__ void __launch_bounds__(256) k_sigma_tile_big(const DevOcp *__restrict__ op, const double *__restrict__ qts,
                                                        double *__restrict__ qt2s, const double *__restrict__ auxs) {
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  __shared__ double sM[NV * NV], sq[NV * NV], sv[NV * NV];
  const DevOcp &o = *op;
  const int T = o.T, tid = threadIdx.x, nt = blockDim.x;
  const long long node = blockIdx.x;
  const int t = (int)(node % (T + 1));
  const double *qt = qts + node * Q::SIZE;
  double *q2 = qt2s + node * Q::SIZE;
  const double *ax = auxs + node * A::SIZE;
  const double sig = kSigma;
  if (t < T) {
    for (int e = tid; e < NV * NV; e += nt) {
      const int i = e / NV, j = e % NV;
      sM[e] = ax[A::M + i * A::LD + j]; sq[e] = ax[A::tq + i * A::LD + j]; sv[e] = ax[A::tv + i * A::LD + j];
    }
  }
  __syncthreads();
  for (int e = tid; e < NV * NV; e += nt) {
    const int i = e / NV, j = e % NV;
    double hww = 0.0, hqw = 0.0, hvw = 0.0, hqq = 0.0, hqv = 0.0, hvv = 0.0;
    if (t < T)
      for (int l = 0; l < NV; ++l) {
        const double Mli = sM[l * NV + i], tqli = sq[l * NV + i], tvli = sv[l * NV + i];
        const double Mlj = sM[l * NV + j], tqlj = sq[l * NV + j], tvlj = sv[l * NV + j];
        hww += Mli * Mlj; hqw += tqli * Mlj; hvw += tvli * Mlj;
        hqq += tqli * tqlj; hqv += tqli * tvlj; hvv += tvli * tvlj;
      }
    const double d = (i == j) ? sig : 0.0;
    const int o2 = i * Q::LD + j;
    q2[Q::Hqq + o2] = qt[Q::Hqq + o2] + sig * hqq + d;
    q2[Q::Hqv + o2] = qt[Q::Hqv + o2] + sig * hqv;
    q2[Q::Hvv + o2] = qt[Q::Hvv + o2] + sig * hvv + d;
    if (t < T) {
      q2[Q::Hww + o2] = qt[Q::Hww + o2] + sig * hww;
      q2[Q::Hqw + o2] = qt[Q::Hqw + o2] + sig * hqw;
      q2[Q::Hvw + o2] = qt[Q::Hvw + o2] + sig * hvw;
    }
  }
}

// K = M Kw - taux for large nv: 64 lanes per node, lane j < 2 nv = column of K
template <int NV>
__global__ void __launch_bounds__(256) k_gains_to_u_big(const DevOcp *__restrict__ op, const double *__restrict__ auxs,
                                                        const double *__restrict__ Kws, double *__restrict__ Kout,
                                                        const DevState *__restrict__ st) {
  constexpr int NX = 2 * NV;
  typedef AUX<NV> A;
  const DevOcp &o = *op;
  const int T = o.T;
  const long long unit = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long node = unit >> 6;
  const int j = (int)(unit & 63);
  if (node >= (long long)o.B * T || j >= NX) return;
  const int b = (int)(node / T), t = (int)(node % T);
  if (st ? !st[b].ls_acc : false) return;  // the sigma sweep in front of this launch skipped the instance: its Kws hold direction gains (st == null: every instance, constrained path)
  const double *ax = auxs + ((long long)b * (T + 1) + t) * A::SIZE;
  const double *Kw = Kws + node * NV * NX;
  double *K = Kout + node * NV * NX;
  const double *tx = (j < NV) ? ax + A::tq + j : ax + A::tv + (j - NV);
  for (int i = 0; i < NV; ++i) {
    double acc = -tx[i * A::LD];
    for (int l = 0; l < NV; ++l) acc += ax[A::M + i * A::LD + l] * Kw[l * NX + j];
    K[i * NX + j] = acc;
  }
}

// The dense feedback-gain GEMM of the exit path on the matrix cores:  K = M Kw - taux  per node,
// (nv x nv) (nv x 2nv) with nv = 30 padded to 32 x 64, as 2 x 4 output tiles of
// v_mfma_f64_16x16x4_f64 (8 k-steps each); one wave per node.  Operand maps (cdna_hip_programming.md,
// "f64 MFMA"): A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], C/D col = l & 15, row = (l >> 4) + 4 reg.
typedef double agx_d4 __attribute__((ext_vector_type(4)));
template <int NV>
__global__ void __launch_bounds__(64) k_gains_to_u_mfma(const DevOcp *__restrict__ op, const double *__restrict__ auxs,
                                                        const double *__restrict__ Kws, double *__restrict__ Kout,
                                                        const DevState *__restrict__ st) {
  static_assert(NV > 16 && NV <= 32, "tiling below assumes 16 < nv <= 32");
  constexpr int NX = 2 * NV;
  typedef AUX<NV> A;
  const DevOcp &o = *op;
  const int T = o.T, lane = threadIdx.x;
  const long long node = blockIdx.x;  // b * T + t
  const int b = (int)(node / T), t = (int)(node % T);
  if (!st[b].ls_acc) return;  // not swept by the sigma pass in front of this launch
  const double *ax = auxs + ((long long)b * (T + 1) + t) * A::SIZE;
  const double *Kw = Kws + node * NV * NX;
  double *K = Kout + node * NV * NX;
  const int l15 = lane & 15, l4 = lane >> 4;
  // Every operand is loaded unconditionally (clamped index, 0 / 1 factor) and ahead of the MFMA chain that consumes it:
  // a load inside a condition is a branch, and a load between two MFMAs of one accumulator chain exposes its latency
  // 64 times per node (this kernel was 0.42 ms for 0.9 GB that way).
  // this lane's A operands for the 8 k-steps of both row tiles: M[16 ti + l15][4 ks + l4]
  double a[2][8];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti) {
    const int arow = 16 * ti + l15, ar = arow < NV ? arow : NV - 1;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kk = 4 * ks + l4, kc = kk < NV ? kk : NV - 1;
      a[ti][ks] = ax[A::M + ar * A::LD + kc] * ((arow < NV && kk < NV) ? 1.0 : 0.0);
    }
  }
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    const int col = 16 * tj + l15, cc = col < NX ? col : NX - 1;
    const bool cq = cc < NV;
    double bv[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int kk = 4 * ks + l4, kc = kk < NV ? kk : NV - 1;
      bv[ks] = Kw[kc * NX + cc] * ((kk < NV && col < NX) ? 1.0 : 0.0);
    }
    agx_d4 acc[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // C <- -taux tile: taux = [tq | tv], element [row][col]
        const int row = 16 * ti + l4 + 4 * r, rc = row < NV ? row : NV - 1;
        const double tx = ax[(cq ? A::tq + cc : A::tv + (cc - NV)) + rc * A::LD];
        acc[ti][r] = -tx * ((row < NV && col < NX) ? 1.0 : 0.0);
      }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][ks], bv[ks], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][ks], bv[ks], acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + l4 + 4 * r;
        if (row < NV && col < NX) K[row * NX + col] = acc[ti][r];
      }
  }
}

}  // namespace agx
