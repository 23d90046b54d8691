// agx_tiles.hpp -- what the kernels of every translation unit share about the solver state and the tiles: the per-instance
// state, the predicates of the derivative pass, the addressing of reference / QP / aux tiles and the tile layouts
// (documented where the tiles are produced, agx_kernels.hpp).
#pragma once

#include "agx_device.hpp"

// Per-instance solver state, device resident.
struct DevState {
  double kkt, cost, merit, gap;  // as agx_status
  double preg, dreg;             // crocoddyl regularisation (reg_min 1e-9)
  int iter, qp_iters, solved, flags;
  int done;                      // 1: instance finished (solved, or regularisation saturated)
  int gains_iter;  // SQP iteration whose tiles the reported gains (Kout) were swept from (-1: none)
  int dir_iter;    // SQP iteration of the last direction this instance computed
  double gains_preg, gains_dreg; // regularisation the last direction was computed with
  // constrained problems (ADMM, agx_admm.hpp)
  double rho_sparse;             // persists across solves (SolverCSQP reset_rho = false); 0 = not initialised
  double con;                    // l1 norm of the constraint violation at the last evaluation
  int admm_conv, admm_iter;      // QP converged in this SQP iteration / ADMM iterations done
  int ls_acc;                    // large models: the sigma sweep in front of k_gains_to_u_* took this instance (agx_big.hpp)
  int admm_refactor;             // ADMM: the Hessian part of the augmented tiles changed (first iteration / new rho)
  int dir_fail;                  // the last backward sweep met a non-positive / non-finite pivot (Quu not positive definite)
  // line search by derivative passes at the trial points (nv <= 7: k_sqp_head / k_sqp_accept)
  int searching;                 // the instance is inside the line search of the current SQP iteration
  int ls_n;                      // index of the trial in flight: step length 2^-ls_n
  int tiles_ok;                  // QP / aux tiles (and the constraint data) belong to the current (xs, us): the derivative pass skips it
  int carry;                     // this MPC step inherits the tiles of nodes 1 .. T-1 of the previous solve as its nodes 0 .. T-2 (k_mpc_prologue sets it,
                                 // the head of the first iteration clears it): the first derivative pass evaluates nodes 0, T-1 and T only
  double preg_trial;             // control regularisation the NEXT iteration runs with if the trial in flight is accepted (baked into its tiles)
  int carry_counted, pad_cc;     // this instance is counted in n_done[6] (instances whose tiles the next MPC step may inherit)
};
// which instances a derivative pass (K1, k_con_eval) works on: phase 0 = start of an SQP iteration (everyone whose tiles are
// stale), phase 1 = the trial points of the instances that are searching (their tiles are overwritten in place)
__device__ __forceinline__ bool k1_active(const DevState &S, int phase) { return phase ? (S.searching != 0) : (!S.done && !S.tiles_ok); }
// ... and which of their nodes: an instance that inherits tiles (DevState::carry) evaluates its running nodes 0 and T - 1 only.
// The one test of the eight-lane K1 and of the kernel that adds to the tiles K1 wrote (k_cost_pairs).
__device__ __forceinline__ bool k1_node_active(const DevState &S, int phase, bool term, int t, int T) {
  return k1_active(S, phase) && (term || !S.carry || t == 0 || t == T - 1);
}
__device__ __forceinline__ double k1_preg(const DevState &S, int phase) { return phase ? S.preg_trial : S.preg; }
// Physical slot of node t in the per-instance arrays of QP / aux tiles (nv <= 7).  The running nodes form a ring whose origin
// advances by one node per carried MPC step (agx_ocp_mpc_step), so that the tiles of the old nodes 1 .. T-1 are the new nodes
// 0 .. T-2 without a copy; the terminal tile keeps slot T.  head == 0 (always, where tiles are not carried): the identity.
__device__ __forceinline__ int tile_slot(const DevOcp &o, int t) {
  const int s = t + o.head;
  return t >= o.T ? t : (s >= o.T ? s - o.T : s);
}

// Addressing of the reference tiles (host tile or a window of the resident trajectory).
struct RefView {
  const double *base;
  long long bstride;  // doubles between instances
  long long tstride;  // doubles between nodes
  long long term_off; // extra offset of the terminal node's tile
  const int *frames;  // [B][T+1][AGX_MAX_ROWS] or null
};
__device__ __forceinline__ const double *ref_at(const RefView &rv, int b, int t, int T) {
  return rv.base + (long long)b * rv.bstride + (long long)t * rv.tstride + (t == T ? rv.term_off : 0);
}
__device__ __forceinline__ const int *frames_at(const RefView &rv, int b, int t, int T) {
  return rv.frames ? rv.frames + ((long long)b * (T + 1) + t) * AGX_MAX_ROWS : nullptr;
}

namespace agx {

constexpr int kPairsToQp = 0, kPairsToCanonical = 1, kPairsDistance = 2, kPairsItems = 3;  // destinations of k_cost_pairs (agx_cost_pairs.hpp)

template <int NV>
struct QT {
  static constexpr int NX = 2 * NV, LD = (NV <= 8 ? 8 : 32), B2 = NV * LD;  // row stride: one (nv <= 8) or four 64-byte lines
  static constexpr int Hqq = 0, Hqv = B2, Hvv = 2 * B2, Hqw = 3 * B2, Hvw = 4 * B2, Hww = 5 * B2, gx = 6 * B2, gw = gx + 2 * LD,
                       f = gw + LD, cost = f + 2 * LD, SIZE = cost + 8;
};
template <int NV>
struct AUX {
  static constexpr int LD = (NV <= 8 ? 8 : 32), B2 = NV * LD;
  static constexpr int M = 0, tq = B2, tv = 2 * B2, Lqq = 3 * B2, Lvv = 4 * B2, Luu = Lvv + LD, Lu = Luu + LD, SIZE = Lu + LD;
};

}  // namespace agx
