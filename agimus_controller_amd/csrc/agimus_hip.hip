// agimus_hip.hip -- C ABI of libagimus_hip.so (see include/agimus_hip.h).
// Host-side orchestration of the gfx950 kernels in agx_kernels.hpp: device-resident
// horizon buffers, the SQP iteration loop, warm-start shift, resident reference
// trajectories.  No CPU fallback: every compute entry point needs a HIP device.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "agx_kernels.hpp"

// launchers of the wide-cost-set kernels, compiled in a translation unit of their own (agx_cost_pairs.hip)
extern "C" int agx_cost_pairs_launch(int dest, void *stream, long long nodes, const DevModel *m, const DevOcp *o, const DevCostWide *w,
                                     const double *dts, const double *xs, const RefView *rv, double *out, double *auxs, const DevState *st,
                                     int phase, int sel, int which, const void *obs);
extern "C" int agx_cost_pairs_fill_launch(void *stream, const DevCostWide *w, const double *gw_item, double *traj, long long units, int stride);
extern "C" int agx_cost_pairs_fill_ring_launch(void *stream, const DevCostWide *w, const double *gw_item, double *traj, int B, int m_new, int end,
                                               int cap, int mirror, int stride);
// launchers of the diagnostics kernels, likewise (agx_diag.hip)
extern "C" int agx_diag_iter_log_launch(void *stream, const DevState *st, int B, int it, int phase, agx_iter_record *rec, int *n, int capacity);
extern "C" int agx_diag_item_costs_launch(void *stream, int nv, int chain, const DevModel *m, const DevRows *rows2, int B, int T, const double *xs,
                                          const double *us, const RefView *rv, int R, double *cost, double *Lx, double *Lu, const void *obs);
extern "C" int agx_diag_clearance_chunks(int m_samples);
extern "C" int agx_diag_clearance_launch(void *stream, const DevModel *mp, int nv, int B, int n_pairs, const int *fa, const int *fb, const double *q,
                                         long long qb, int qs, int m_samples, double *dist, double *witness, double *cmin, int *cidx,
                                         double *min_dist, int *min_where, const void *obs);

// launchers of the general-cost-row kernels of large models, likewise (agx_general_rows.hip; dest: the constants below)
extern "C" int agx_general_rows_launch(int dest, void *stream, int nv, int prismatic, long long units, const DevModel *m, const DevOcp *o,
                                       const double *dts, const double *xs, const double *us, const RefView *rv, double *out0, double *out1,
                                       double *out2, const DevState *st, int phase, int only, int R);
extern "C" int agx_general_kkt_launch(void *stream, int nv, long long nodes, const DevOcp *o, const double *qts, const double *auxs, const double *auxg,
                                      const double *dxs, const double *wss, double *dus, double *nodestat, const DevState *st);
constexpr int kGenToQp = 0, kGenToCanonical = 1, kGenItems = 2;  // agx_general_rows.hpp
// -DAGX_NO_GENERAL_ROWS compiles the launch sites of these kernels out (and K1 of large models reads d_ocp, as it did before
// they existed): the second library of backend.build(), against which a test compares a handle without general rows bit for bit.
#ifdef AGX_NO_GENERAL_ROWS
constexpr bool kGeneralRowsWg = false;
#else
constexpr bool kGeneralRowsWg = true;
#endif

#include "agx_host_handle.hpp"

namespace {

void fill_rows(const agx_cost_row *rows, int n, int nv, int nvu, DevRows &d) {
  std::memset(&d, 0, sizeof(d));
  d.n = n;
  d.nvu = nvu;
  int off = 0;
  for (int r = 0; r < n; ++r) {
    d.kind[r] = rows[r].kind;
    d.act[r] = rows[r].activation;
    d.active[r] = rows[r].active;
    d.frame[r] = rows[r].frame;
    d.frame_b[r] = rows[r].frame_b;
    d.alpha[r] = rows[r].alpha;
    d.weight[r] = rows[r].weight;
    d.nref[r] = agx_row_nref(rows[r].kind, nv);
    d.nr[r] = agx_row_nr(rows[r].kind, nv);
    d.off[r] = off;
    off += 1 + d.nref[r] + d.nr[r];
    if (rows[r].active && (rows[r].kind == AGX_RES_CONTROL_GRAV || rows[r].kind == AGX_RES_FRAME_VELOCITY)) d.general = 1;
  }
}

// A cost-row table as a wide cost set sees it (include/agimus_hip.h): `n_prefix` rows in front of the trailing block of collision
// rows; `offender` is the first collision row that is not part of that block (-1: the collision rows are trailing).
struct CostSplit { int n_other = 0, n_pairs = 0, n_prefix = 0, offender = -1; };
CostSplit split_cost_rows(const agx_cost_row *rows, int n) {
  CostSplit s;
  for (int r = 0; r < n; ++r) (rows[r].kind == AGX_RES_COLLISION ? s.n_pairs : s.n_other)++;
  s.n_prefix = n;
  while (s.n_prefix > 0 && rows[s.n_prefix - 1].kind == AGX_RES_COLLISION) --s.n_prefix;
  for (int r = 0; r < s.n_prefix && s.offender < 0; ++r)
    if (rows[r].kind == AGX_RES_COLLISION) s.offender = r;
  return s;
}
void fill_cost_pairs(const agx_cost_row *rows, int n, const CostSplit &cs, int nv, DevCostPairs &P) {
  std::memset(&P, 0, sizeof(P));
  P.n = n - cs.n_prefix;
  P.first = cs.n_prefix;
  for (int r = 0; r < cs.n_prefix; ++r) P.prefix += 1 + agx_row_nref(rows[r].kind, nv) + agx_row_nr(rows[r].kind, nv);
  for (int p = 0; p < P.n; ++p) {
    const agx_cost_row &c = rows[cs.n_prefix + p];
    P.fa[p] = c.frame; P.fb[p] = c.frame_b; P.act[p] = c.activation; P.active[p] = c.active; P.alpha[p] = c.alpha; P.weight[p] = c.weight;
  }
}

// component k of a residual of `kind` over nv (capacity) joints -> the caller's component over nvu joints, -1 for a pad joint
int user_component(int kind, int k, int nv, int nvu, bool is_ref) {
  const bool joint_blocks = kind == AGX_RES_STATE || kind == AGX_RES_CONTROL || (kind == AGX_RES_CONTROL_GRAV && !is_ref);
  if (!joint_blocks || nv == nvu) return k;
  const int blk = k / nv, i = k % nv;
  return i < nvu ? blk * nvu + i : -1;
}

// Constraint rows a node type leaves out: inactive rows and, at the terminal node, which has no control, the residuals on u
// (crocoddyl evaluates them with nu = 0).  The one rule of fill_cons, wide_class and fill_cons_wide.
bool cons_row_skipped(const agx_constraint_row &c, bool terminal) {
  return !c.active || (terminal && (c.kind == AGX_RES_CONTROL || c.kind == AGX_RES_CONTROL_GRAV));
}

int fill_cons(const agx_constraint_row *rows, int n, int nv, int nvu, const DevModel &m, DevCons &d, bool terminal) {
  std::memset(&d, 0, sizeof(d));
  int off = 0;
  for (int r = 0; r < n; ++r) {
    const agx_constraint_row &c = rows[r];
    if (cons_row_skipped(c, terminal)) continue;
    if (d.n >= AGX_MAX_CONS) return fail("agx_ocp_create: at most 4 active constraint rows per node type");
    if (c.kind != AGX_RES_STATE && c.kind != AGX_RES_CONTROL && !agx::cons_has_dense_rows(c.kind))
      return fail("agx_ocp_create: unknown constraint residual kind");
    const int nr = agx_row_nr(c.kind, nv), nref = agx_row_nref(c.kind, nv);
    if (off + nr > AGX_MAX_NC) return fail("agx_ocp_create: more than " + std::to_string(AGX_MAX_NC) + " constraint components per node");
    if (!c.lower || !c.upper) return fail("agx_ocp_create: constraint bounds missing");
    const int i = d.n++;
    d.kind[i] = c.kind; d.frame[i] = c.frame; d.frame_b[i] = c.frame_b; d.off[i] = off; d.nr[i] = nr;
    for (int k = 0; k < nref; ++k) {
      const int ku = user_component(c.kind, k, nv, nvu, true);
      d.ref[i][k] = (c.ref && ku >= 0) ? c.ref[ku] : 0.0;
    }
    for (int k = 0; k < nr; ++k) {
      const int ku = user_component(c.kind, k, nv, nvu, false);  // pad joints: unbounded components
      d.lb[off + k] = ku >= 0 ? c.lower[ku] : -INFINITY; d.ub[off + k] = ku >= 0 ? c.upper[ku] : INFINITY;
      if (!(d.lb[off + k] <= d.ub[off + k])) return fail("agx_ocp_create: constraint with lower > upper");
    }
    if (c.kind == AGX_RES_COLLISION) {
      if (c.frame < 0 || c.frame >= m.nframes || c.frame_b < 0 || c.frame_b >= m.nframes || !agx::frame_has_geometry(m, c.frame) ||
          !agx::frame_has_geometry(m, c.frame_b))
        return fail("agx_ocp_create: collision constraint refers to a frame without geometry");
      if (agx::frame_is_box(m, c.frame) && agx::frame_is_box(m, c.frame_b))
        return fail("agx_ocp_create: box / box collision pairs are not supported");
      d.coll_slot[i] = d.ncoll++;
    }
    if (c.kind != AGX_RES_COLLISION && agx::cons_has_dense_rows(c.kind)) {  // nr scalar rows with dense gradients in q: nr Jacobian slots
      if (c.frame < 0 || c.frame >= m.nframes) return fail("agx_ocp_create: constraint frame id out of range");
      d.coll_slot[i] = d.ncoll;
      d.ncoll += nr;
    }
    if (c.kind == AGX_RES_FRAME_VELOCITY && (c.frame_b < 0 || c.frame_b > 2)) return fail("agx_ocp_create: FrameVelocity constraint: reference frame must be 0 (WORLD), 1 (LOCAL) or 2 (LOCAL_WORLD_ALIGNED)");
    if (d.ncoll > AGX_MAX_DENSE) return fail("agx_ocp_create: at most 8 constraint components with a dense Jacobian (collision pairs, frame residuals, ControlGrav) per node type");
    off += nr;
  }
  d.nc = off;
  return 0;
}

// Wide constraint sets (DevCons): collision-distance rows next to at most one State and one Control row.  Class of the active rows
// of one node type: 0 they qualify, 1 they do not (another kind, a second State / Control row), 2 more than AGX_MAX_PAIRS pairs.
int wide_class(const agx_constraint_row *rows, int n, bool terminal) {
  int ns = 0, nc = 0, np = 0;
  for (int r = 0; r < n; ++r) {
    const agx_constraint_row &c = rows[r];
    if (cons_row_skipped(c, terminal)) continue;
    if (c.kind == AGX_RES_STATE) ++ns;
    else if (c.kind == AGX_RES_CONTROL) ++nc;
    else if (c.kind == AGX_RES_COLLISION) ++np;
    else return 1;
  }
  if (ns > 1 || nc > 1) return 1;
  return np > AGX_MAX_PAIRS ? 2 : 0;
}

// The wide layout of a set wide_class accepts: State / Control rows in the row table (components first), then the pairs in the
// caller's order at pair_off + p.  The strides are set by the caller (the same for both node types).
int fill_cons_wide(const agx_constraint_row *rows, int n, int nv, int nvu, const DevModel &m, DevCons &d, bool terminal) {
  std::memset(&d, 0, sizeof(d));
  int off = 0;
  for (int r = 0; r < n; ++r) {
    const agx_constraint_row &c = rows[r];
    if (cons_row_skipped(c, terminal) || c.kind == AGX_RES_COLLISION) continue;
    // the kernels of the wide layout know State / Control rows and the pair table only (wide_class admits nothing else)
    if ((c.kind != AGX_RES_STATE && c.kind != AGX_RES_CONTROL) || d.n >= 2)
      return fail("agx_ocp_create: a wide constraint set holds collision pairs, at most one State and one Control row");
    if (!c.lower || !c.upper) return fail("agx_ocp_create: constraint bounds missing");
    const int nr = agx_row_nr(c.kind, nv), nref = agx_row_nref(c.kind, nv);
    const int i = d.n++;
    d.kind[i] = c.kind; d.frame[i] = c.frame; d.frame_b[i] = c.frame_b; d.off[i] = off; d.nr[i] = nr;
    for (int k = 0; k < nref; ++k) {
      const int ku = user_component(c.kind, k, nv, nvu, true);
      d.ref[i][k] = (c.ref && ku >= 0) ? c.ref[ku] : 0.0;
    }
    for (int k = 0; k < nr; ++k) {
      const int ku = user_component(c.kind, k, nv, nvu, false);  // pad joints: unbounded components
      d.lb[off + k] = ku >= 0 ? c.lower[ku] : -INFINITY; d.ub[off + k] = ku >= 0 ? c.upper[ku] : INFINITY;
      if (!(d.lb[off + k] <= d.ub[off + k])) return fail("agx_ocp_create: constraint with lower > upper");
    }
    off += nr;
  }
  d.pair_off = off;
  for (int r = 0; r < n; ++r) {
    const agx_constraint_row &c = rows[r];
    if (cons_row_skipped(c, terminal) || c.kind != AGX_RES_COLLISION) continue;
    if (d.npairs >= AGX_MAX_PAIRS) return fail("agx_ocp_create: at most " + std::to_string(AGX_MAX_PAIRS) + " collision-pair constraints per node type");
    if (!c.lower || !c.upper) return fail("agx_ocp_create: constraint bounds missing");
    if (c.frame < 0 || c.frame >= m.nframes || c.frame_b < 0 || c.frame_b >= m.nframes || !agx::frame_has_geometry(m, c.frame) ||
        !agx::frame_has_geometry(m, c.frame_b))
      return fail("agx_ocp_create: collision constraint refers to a frame without geometry");
    if (agx::frame_is_box(m, c.frame) && agx::frame_is_box(m, c.frame_b))
      return fail("agx_ocp_create: box / box collision pairs are not supported");
    if (!(c.lower[0] <= c.upper[0])) return fail("agx_ocp_create: constraint with lower > upper");
    const int p = d.npairs++;
    d.pa[p] = c.frame; d.pb[p] = c.frame_b; d.plb[p] = c.lower[0]; d.pub[p] = c.upper[0];
  }
  d.nc = off + d.npairs;
  return 0;
}

// ---- dispatch over the compiled (NV, CHAIN) instantiations --------------------
// The library is built as one translation unit per group of capacities (AGX_GROUP = 0: 7 joints, 1: 16, 30 and 32, compiled in
// parallel by backend.build(), namespace and entry points suffixed per group, csrc/agx_front.py
// generates the forwarding entry points) or, without AGX_GROUP, as a single translation unit.
#if defined(AGX_ONLY_NV7) || (defined(AGX_GROUP) && AGX_GROUP == 0)  // AGX_ONLY_NV7: development builds, short compile
#define AGX_FOR_NV(MACRO) MACRO(7)
#elif defined(AGX_ONLY_NV30) || (defined(AGX_GROUP) && AGX_GROUP == 1)
#define AGX_FOR_NV(MACRO) MACRO(16) MACRO(30) MACRO(32)
#else
#define AGX_FOR_NV(MACRO) MACRO(7) MACRO(16) MACRO(30) MACRO(32)
#endif

// capacity a model of nv joints runs at: the smallest compiled size that holds it (0: none)
int pad_capacity(int nv) {
  int best = 0;
#define AGX_CAP(N) if (N >= nv && (best == 0 || N < best)) best = N;
  AGX_FOR_NV(AGX_CAP)
#undef AGX_CAP
  return best;
}

// The workgroup-per-node kernels are instantiated with and without the prismatic-joint code (agx_big_k1.hpp: PRISM): a model
// without a prismatic joint runs the instruction stream of the revolute-only kernels.  f(std::bool_constant<PRISM>) launches.
template <typename F>
void launch_wg(const agx_ocp *o, F &&f) {
  if (o->hm.prismatic) f(std::true_type());
  else f(std::false_type());
}

template <typename F>
int dispatch(int nv, bool chain, F &&f) {
  switch (nv) {
#define AGX_CASE(N)                                                  \
  case N:                                                            \
    if constexpr (N <= 8) { if (chain) return f(std::integral_constant<int, N>(), std::true_type()); } \
    return f(std::integral_constant<int, N>(), std::false_type());  /* large models: the tree code path serves chains too */
    AGX_FOR_NV(AGX_CASE)
#undef AGX_CASE
  }
#define AGX_NAME(N) " " #N
  return fail("no kernel instantiation for nv = " + std::to_string(nv) + " (compiled capacities:" AGX_FOR_NV(AGX_NAME) ")");
#undef AGX_NAME
}

// Per-instance sources.  The 7-joint kernels that evaluate dynamics or a collision distance end in a template pack: empty,
// InstanceInertials<NV> (agx_ocp_set_model_inertials), ObstaclePlacements (agx_ocp_set_obstacle_placements) or both in that order,
// one more argument each (agx_device.hpp: pack_has, pack_ptr, world_of).  with_sources calls f(sources...) with the trailing
// arguments of the instantiation a launch takes: the inertials where the kernel evaluates dynamics (INERT: running nodes) and the
// handle has them, the table where it evaluates a collision distance (OBS) and the handle has one.  A handle with neither reaches
// f(): the kernel on the model's own tables, as do the larger capacities, whose setters refuse.  src_t names the pack from the
// arguments.  Every launch of such a kernel goes through here once; DESIGN.md has the table of flags per kernel.
template <class P>
using src_t = std::remove_const_t<std::remove_pointer_t<P>>;
template <int NV, bool INERT, bool OBS, class F>
void with_sources(agx_ocp *o, F &&f) {
  if constexpr (NV <= 7) {
    [[maybe_unused]] const auto *inst = (const agx::InstanceInertials<NV> *)o->d_minert;
    [[maybe_unused]] const auto *obs = (const agx::ObstaclePlacements *)o->d_obs;
    if constexpr (INERT && OBS) if (o->minert_set && o->obs_set) return f(inst, obs);
    if constexpr (INERT) if (o->minert_set) return f(inst);
    if constexpr (OBS) if (o->obs_set) return f(obs);
  }
  f();
}

int launch_calc_diff_rows(agx_ocp *o, bool masked, bool running_only) {
  if (!o->d_tiles) HIPCHK(o->own.device(&o->d_tiles, (size_t)o->B * (o->T + 1) * o->tile));  // the canonical tiles: on first use
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    const long long units = (long long)o->B * o->T;
    const DevState *stm = masked ? o->d_state : nullptr;
    auto both = [&](auto GENc) {
      constexpr bool GEN = decltype(GENc)::value;
      with_sources<NV, true, true>(o, [&](auto... src) {
        hipLaunchKernelGGL((agx::k_calc_diff<NV, CH, GEN, src_t<decltype(src)>...>), dim3((int)((units + 63) / 64)), dim3(64), 0, o->stream, o->d_model,
                           o->d_ocp, o->d_dt, o->d_xs, o->d_us, o->rv, o->d_tiles, stm, src...);
      });
      if (!running_only)
        with_sources<NV, false, true>(o, [&](auto... src) {
          hipLaunchKernelGGL((agx::k_calc_diff_term<NV, CH, GEN, src_t<decltype(src)>...>), dim3((o->B + 63) / 64), dim3(64), 0, o->stream, o->d_model,
                             o->d_ocp, o->d_xs, o->rv, o->d_tiles, stm, src...);
        });
    };
    if constexpr (NV <= 7) { if (o->general) both(std::true_type()); else both(std::false_type()); }  // (GEN: 7 joints only)
    else both(std::false_type());
    HIPCHK(hipGetLastError());
    return 0;
  });
}

// K1 production: QP tiles in acceleration-input form.  Serial chains use the 8-lanes-per-node
// kernel (agx_k1_lanes.hpp); trees fall back to one lane per node.
// phase 1: the pass runs at the trial iterates (staging halves of xs / us) of the instances in the line search and leaves
// their tiles in place of the current ones (k_sqp_head / k_sqp_accept, agx_kernels.hpp); every model size.
// compact (phase 0, eight-lane kernel): every instance inherits its tiles (DevState::carry): a grid over nodes 0, T - 1 and T only.
int launch_k1(agx_ocp *o, bool running_only, bool term_only, int phase, bool compact) {
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    const long long units = (long long)o->B * o->T;
    const double *xs_in = phase ? o->d_xs + (size_t)o->B * (o->T + 1) * o->nx : o->d_xs;
    const double *us_in = phase ? o->d_us + (size_t)o->B * o->T * o->nu : o->d_us;
    if constexpr (NV > 8) {
      // large models: one workgroup per node, running and terminal nodes in one launch (agx_big_k1.hpp)
      if (term_only) return 0;  // the launch of the running nodes (profiled path) already covered the terminal ones
      launch_wg(o, [&](auto PRc) {
        hipLaunchKernelGGL((agx::k_calc_qp_wg<NV, decltype(PRc)::value>), dim3((int)(units + o->B)), dim3(256), 0, o->stream, o->d_model, kGeneralRowsWg ? o->d_ocp_k1 : o->d_ocp, o->d_dt, xs_in,
                         us_in, o->rv, o->d_qt, o->d_aux, o->d_state, phase);
      });
    } else if (NV <= 7 && !o->general && CH && o->k1_lanes && o->lanes_ok) {
      const long long run_nodes = compact ? (long long)o->B * (o->T > 1 ? 2 : 1) : units;
      const int n_run = (int)((run_nodes * 8 + 63) / 64), n_term = (int)(((long long)o->B * 8 + 63) / 64), cp = compact ? 1 : 0;
      auto lanes8 = [&](auto COLLc) {
        // OBS = COLL: without a collision row the kernel evaluates no distance and never takes the table, even when one is set
        constexpr bool COLL = decltype(COLLc)::value;
        if (o->k1_fused && !term_only && !running_only) {  // both node types in one launch
          with_sources<NV, true, COLL>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_calc_qp_lj_all<NV, COLL, src_t<decltype(src)>...>), dim3(n_run + n_term), dim3(64), 0, o->stream, o->d_model,
                               o->d_ocp_k1, o->d_dt, xs_in, us_in, o->rv, o->d_qt, o->d_aux, o->d_state, n_run, phase, cp, src...);
          });
          return;
        }
        if (!term_only)
          with_sources<NV, true, COLL>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_calc_qp_lj<NV, false, COLL, src_t<decltype(src)>...>), dim3(n_run), dim3(64), 0, o->stream, o->d_model,
                               o->d_ocp_k1, o->d_dt, xs_in, us_in, o->rv, o->d_qt, o->d_aux, o->d_state, phase, cp, src...);
          });
        if (!running_only)
          with_sources<NV, false, COLL>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_calc_qp_lj<NV, true, COLL, src_t<decltype(src)>...>), dim3(n_term), dim3(64), 0, o->stream, o->d_model,
                               o->d_ocp_k1, o->d_dt, xs_in, us_in, o->rv, o->d_qt, o->d_aux, o->d_state, phase, cp, src...);
          });
      };
      if constexpr (NV <= 7) { if (o->lanes_coll) lanes8(std::true_type()); else lanes8(std::false_type()); }
    } else {  // one lane per node
      auto both = [&](auto GENc) {
        constexpr bool GEN = decltype(GENc)::value;
        double *auxg = GEN ? o->d_auxg : nullptr;
        if (!term_only)
          with_sources<NV, true, true>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_calc_qp<NV, CH, GEN, src_t<decltype(src)>...>), dim3((int)((units + 63) / 64)), dim3(64), 0, o->stream,
                               o->d_model, o->d_ocp, o->d_dt, xs_in, us_in, o->rv, o->d_qt, o->d_aux, o->d_state, auxg, phase, src...);
          });
        if (!running_only)
          with_sources<NV, false, true>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_calc_qp_term<NV, CH, GEN, src_t<decltype(src)>...>), dim3((o->B + 63) / 64), dim3(64), 0, o->stream, o->d_model,
                               o->d_ocp, xs_in, o->rv, o->d_qt, o->d_aux, o->d_state, auxg, phase, src...);
          });
      };
      if constexpr (NV <= 7) { if (o->general) both(std::true_type()); else both(std::false_type()); }  // (GEN: 7 joints only)
      else both(std::false_type());
    }
    HIPCHK(hipGetLastError());
    return 0;
  });
}

// The trailing collision rows of a wide cost set (agx_cost_pairs.hpp) on the node grid of the K1 launch in front of it.
// dest: agx::kPairsToQp (QP / aux tiles, nodes chosen by K1's predicate), kPairsToCanonical (o->d_tiles), kPairsDistance
// (pair `which` at the running nodes into `dist` [B][T]).  sel: 0 every node, 1 running, 2 terminal.
int launch_cost_pairs(agx_ocp *o, int dest, int sel, int phase, bool masked = false, int which = 0, double *dist = nullptr);

int launch_calc_diff(agx_ocp *o, bool masked, bool running_only = false) {
  if (launch_calc_diff_rows(o, masked, running_only)) return -1;
  if (kGeneralRowsWg && o->general && o->nv > 7) {  // large models: k_general_rows_wg adds the ControlGrav / FrameVelocity rows (Lxu, dense Lxx) behind k_calc_diff
    const long long units = (long long)o->B * o->T + (running_only ? 0 : o->B);
    HIPCHK((hipError_t)agx_general_rows_launch(kGenToCanonical, (void *)o->stream, o->nv, o->hm.prismatic ? 1 : 0, units, o->d_model, o->d_ocp, o->d_dt,
                                               o->d_xs, o->d_us, &o->rv, o->d_tiles, nullptr, nullptr, masked ? o->d_state : nullptr, 0, -1, 0));
  }
  return o->cost_wide ? launch_cost_pairs(o, agx::kPairsToCanonical, running_only ? 1 : 0, 0, masked) : 0;
}

// The derivative pass every caller launches: K1 on the row table, then -- wide cost sets -- k_cost_pairs on the same iterate,
// phase and nodes.
int launch_calc_qp(agx_ocp *o, bool running_only = false, bool term_only = false, int phase = 0, bool compact = false) {
  if (launch_k1(o, running_only, term_only, phase, compact)) return -1;
  if (kGeneralRowsWg && o->general && o->nv > 7 && !term_only) {
    // large models: k_general_rows_wg adds the ControlGrav / FrameVelocity rows into the tiles of the K1 launch in front of it,
    // which covers every node (launch_k1), at the same iterate (phase 1: the trial points) and by the same predicate
    const double *xs_in = phase ? o->d_xs + (size_t)o->B * (o->T + 1) * o->nx : o->d_xs;
    const double *us_in = phase ? o->d_us + (size_t)o->B * o->T * o->nu : o->d_us;
    HIPCHK((hipError_t)agx_general_rows_launch(kGenToQp, (void *)o->stream, o->nv, o->hm.prismatic ? 1 : 0, (long long)o->B * (o->T + 1), o->d_model,
                                               o->d_ocp, o->d_dt, xs_in, us_in, &o->rv, o->d_qt, o->d_aux, o->d_auxg, o->d_state, phase, -1, 0));
  }
  return o->cost_wide ? launch_cost_pairs(o, agx::kPairsToQp, running_only ? 1 : (term_only ? 2 : 0), phase) : 0;
}

// K2 of large models on `tiles` (k_riccati_blk, agx_big_k2.hpp, which documents forward / gains_pass)
template <int NV>
void launch_riccati_blk(agx_ocp *o, const double *tiles, int forward, int gains_pass) {
  hipLaunchKernelGGL((agx::k_riccati_blk<NV>), dim3(o->B), dim3(256), 0, o->stream, o->d_ocp, o->d_dt, tiles, o->d_Kws, o->d_kws, o->d_dx,
                     o->d_w, o->d_state, forward, gains_pass);
}

// K2: direction sweep; with `pair` the speculative gains sweep of SQP iteration `iter` rides in the same launch
int launch_riccati(agx_ocp *o, int forward, bool pair = false, int iter = 0, const double *tiles = nullptr) {
  if (o->nv <= 7 && o->T + 1 > 512) return fail("the sweeps stage the step lengths of up to 511 nodes in LDS: horizon too long");
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    const double *qt = tiles ? tiles : o->d_qt;
    if constexpr (NV <= 7) if (o->mx2_S >= 2 && o->riccati_mx && !tiles) {
      // small batches: segments in parallel, exact boundary value functions (agx_riccati_mx2.hpp)
      const int S = o->mx2_S, P2 = pair ? 2 : 1;
      if (!o->d_mx2_elem) {
        HIPCHK(o->own.device(&o->d_mx2_elem, 2 * (size_t)o->B * S * 768));
        HIPCHK(o->own.device(&o->d_mx2_bnd, 2 * (size_t)o->B * S * 256));
        HIPCHK(o->own.device(&o->d_mx2_cl, (size_t)o->B * S * 256));
      }
      hipLaunchKernelGGL((agx::k_riccati_mx2_elem<NV>), dim3(P2 * o->B * S), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux,
                         o->d_Kws, o->d_kws, o->d_Kout, o->d_state, o->d_mx2_elem, o->d_mx2_bnd, o->d_mx2_cl, S, pair ? 1 : 0, 0, 1, iter);
      hipLaunchKernelGGL((agx::k_riccati_mx2_sweep<NV>), dim3(P2 * o->B * (S - 1)), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux,
                         o->d_Kws, o->d_kws, o->d_Kout, o->d_state, o->d_mx2_elem, o->d_mx2_bnd, o->d_mx2_cl, S, pair ? 1 : 0, 0, 1);
      if (forward)
        hipLaunchKernelGGL((agx::k_riccati_mx2_fwd<NV>), dim3(o->B * S), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_Kws, o->d_kws,
                           o->d_dx, o->d_w, o->d_state, o->d_mx2_cl, S);
      HIPCHK(hipGetLastError());
      return 0;
    }
    if constexpr (NV <= 7) {
      // `forward` is honoured by the one-wave MFMA-layout pair only (solve_resident with the step tail: the forward pass runs in
      // k_step_tail); k_riccati_pair and the segmented pair above run their forward pass whatever it says, as they always did
      if (pair && o->riccati_mx && !forward)
        hipLaunchKernelGGL((agx::k_riccati_mx_pair_sweeps<NV>), dim3(16 * ((o->B + 7) / 8)), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt,
                           o->d_aux, o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_Kout, o->d_state, iter);
      else if (pair && o->riccati_mx)
        hipLaunchKernelGGL((agx::k_riccati_mx_pair<NV>), dim3(16 * ((o->B + 7) / 8)), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux,
                           o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_Kout, o->d_state, iter);
      else if (pair)
        hipLaunchKernelGGL((agx::k_riccati_pair<NV>), dim3(2 * o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux,
                           o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_du, o->d_Kout, o->d_state, iter);
      else if (o->riccati_mx)
        hipLaunchKernelGGL((agx::k_riccati_mx<NV, false>), dim3(o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, qt, o->d_aux,
                           o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_Kout, o->d_state, forward, 0);
      else
        hipLaunchKernelGGL((agx::k_riccati<NV, false>), dim3(o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, qt, o->d_aux,
                           o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_du, o->d_Kout, o->d_state, forward, 0);
    } else {
      (void)pair; (void)iter;
      launch_riccati_blk<NV>(o, qt, forward, 0);
    }
    HIPCHK(hipGetLastError());
    return 0;
  });
}

// K3 (node shares of the KKT residual, cost, gaps; du) and the head of the step: instance totals, convergence test and the
// first trial iterate of the line search (the caller runs the trial rounds: line_search_rounds).
agx::HostWords host_words(agx_ocp *o, bool line_search_counters, unsigned long long seq) {
  agx::HostWords hw{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  if (!o->poll || !o->fold_publish || seq == 0) return hw;
  hw.done = o->h_ndone_dev + 0;
  if (line_search_counters) { hw.handed = o->h_ndone_dev + 6; hw.stale = o->h_ndone_dev + 7; }
  hw.carry = o->h_ndone_dev + 8;
  hw.packed = o->h_ndone_dev + 9;
  hw.seq = o->h_ndone_dev + 1;
  hw.stamp = seq;
  return hw;
}

// the block the head of the step packs first-node records into: the mapped block of agx_ocp_first_packed once it exists
double *first_block(const agx_ocp *o) {
  return (o->first_in_solve && o->poll && o->first_stride == o->nu + o->nu * o->nx + o->nx + 8) ? o->d_first : nullptr;
}

// `seq` != 0 (small batches): the head's last workgroup hands the finished-instance count to the host under that stamp.
// `pack` (solve_resident): converging instances pack their first-node record (first_block).
int launch_step(agx_ocp *o, int iter, int max_iter, int mode, bool with_node_kkt = true, bool with_step = true, unsigned long long seq = 0,
                bool pack = false) {
  if (o->T + 1 > 512) return fail("step kernel supports horizons up to 511 nodes");
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    (void)CH;
    const long long nodes = (long long)o->B * (o->T + 1);
    double *xs_t = o->d_xs + (size_t)o->B * (o->T + 1) * o->nx, *us_t = o->d_us + (size_t)o->B * o->T * o->nu;
    if (with_node_kkt) {
      if constexpr (NV <= 7) {
        if (o->general)
          hipLaunchKernelGGL((agx::k_node_kkt_gen<NV>), dim3((int)((nodes + 63) / 64)), dim3(64), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux,
                             o->d_auxg, o->d_dx, o->d_w, o->d_du, o->d_nodestat, o->d_state);
        else if (o->node_kkt_wide)
          hipLaunchKernelGGL((agx::k_node_kkt_ahead<NV>), dim3((int)((nodes + 7) / 8)), dim3(64), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux,
                             o->d_dx, o->d_w, o->d_du, o->d_nodestat, o->d_state);
        else
          hipLaunchKernelGGL((agx::k_node_kkt<NV>), dim3((int)((nodes * 8 + 255) / 256)), dim3(256), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux,
                             o->d_dx, o->d_w, o->d_du, o->d_nodestat, o->d_state);
      } else if (kGeneralRowsWg && o->general)  // every block of the identities (k_node_kkt_big_gen, agx_general_rows.hpp)
        HIPCHK((hipError_t)agx_general_kkt_launch((void *)o->stream, NV, nodes, o->d_ocp, o->d_qt, o->d_aux, o->d_auxg, o->d_dx, o->d_w, o->d_du,
                                                  o->d_nodestat, o->d_state));
      else
        hipLaunchKernelGGL((agx::k_node_kkt_big<NV>), dim3((int)((nodes + 1) / 2)), dim3(64), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux,
                           o->d_dx, o->d_w, o->d_du, o->d_nodestat, o->d_state);
    }
    if (with_step)
      hipLaunchKernelGGL((agx::k_sqp_head<NV>), dim3(o->B), dim3(128), 0, o->stream, o->d_ocp, o->d_xs, o->d_us, o->d_dx, o->d_du, xs_t, us_t,
                         o->d_nodestat, o->d_state, iter, max_iter, mode, o->d_ndone, host_words(o, false, seq), o->d_Kout,
                         pack ? first_block(o) : nullptr, o->first_stride);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

// Forward pass, K3 and the head of the step in one launch, one workgroup per instance (k_step_tail, agx_step_tail.hpp), behind a
// sweep launched with forward = 0: the 7-joint capacity, unconstrained, no general rows, one-wave MFMA-layout sweeps.
bool step_tail_path(const agx_ocp *o) {
  return o->step_tail && o->nv <= 7 && !o->has_con && !o->general && o->riccati_mx && o->node_kkt_wide && o->mx2_S < 2;
}
int launch_step_tail(agx_ocp *o, int iter, int max_iter, unsigned long long seq, bool pack) {
  if (o->T + 1 > 512) return fail("step kernel supports horizons up to 511 nodes");
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    (void)CHc;
    if constexpr (NV <= 7) {
      double *xs_t = o->d_xs + (size_t)o->B * (o->T + 1) * o->nx, *us_t = o->d_us + (size_t)o->B * o->T * o->nu;
      hipLaunchKernelGGL((agx::k_step_tail<NV>), dim3(o->B), dim3(agx::kTailThreads), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux,
                         o->d_Kws, o->d_kws, o->d_xs, o->d_us, o->d_dx, o->d_w, o->d_du, xs_t, us_t, o->d_nodestat, o->d_state, iter,
                         max_iter, o->d_ndone, host_words(o, false, seq), o->d_Kout, pack ? first_block(o) : nullptr, o->first_stride);
      HIPCHK(hipGetLastError());
      o->step_tail_launches += 1;
      return 0;
    } else {
      (void)iter; (void)max_iter; (void)seq; (void)pack;
      return fail("the step tail serves the 7-joint capacity");
    }
  });
}

// exit path: the sigma (proximal) Riccati sweep that yields the gains the solver reports, one kernel.
// gmode 0: every instance; 2: only instances whose last direction has no (speculative) sweep yet.
int launch_gains(agx_ocp *o, int gmode = 0) {
  if (o->nv <= 7 && o->T + 1 > 512) return fail("the sweeps stage the step lengths of up to 511 nodes in LDS: horizon too long");
  if (o->nv > 7 && !o->d_qt2) HIPCHK(o->own.device(&o->d_qt2, (size_t)o->B * (o->T + 1) * o->qt_size));
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    if constexpr (NV <= 7) {
      if (o->riccati_mx)
        hipLaunchKernelGGL((agx::k_riccati_mx<NV, true>), dim3(o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux, o->d_Kws,
                           o->d_kws, o->d_dx, o->d_w, o->d_Kout, o->d_state, 0, gmode);
      else
      hipLaunchKernelGGL((agx::k_riccati<NV, true>), dim3(o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_aux, o->d_Kws,
                         o->d_kws, o->d_dx, o->d_w, o->d_du, o->d_Kout, o->d_state, 0, gmode);
    } else {
      // large models: sigma-augmented tiles, sweep (instances selected by gmode, as riccati_body), gains to u-space for
      // the instances the sweep took
      const long long nodes = (long long)o->B * (o->T + 1);
      const int gsel = gmode == 0 ? 1 : gmode;
      hipLaunchKernelGGL((agx::k_sigma_tile_big<NV>), dim3((int)nodes), dim3(256), 0, o->stream, o->d_ocp, o->d_qt, o->d_qt2, o->d_aux);
      launch_riccati_blk<NV>(o, o->d_qt2, 0, gsel);
      if constexpr (NV > 16) {
        if (o->gains_mfma) {  // the dense feedback-gain GEMM on the matrix cores
          hipLaunchKernelGGL((agx::k_gains_to_u_mfma<NV>), dim3(o->B * o->T), dim3(64), 0, o->stream, o->d_ocp, o->d_aux, o->d_Kws, o->d_Kout,
                             o->d_state);
          HIPCHK(hipGetLastError());
          return 0;
        }
      }
      const long long units = (long long)o->B * o->T * 64;
      hipLaunchKernelGGL((agx::k_gains_to_u_big<NV>), dim3((int)((units + 255) / 256)), dim3(256), 0, o->stream, o->d_ocp, o->d_aux,
                         o->d_Kws, o->d_Kout, o->d_state);
    }
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int reset_state(agx_ocp *o) {
  hipLaunchKernelGGL(agx::k_reset_state, dim3((o->B + 255) / 256), dim3(256), 0, o->stream, o->d_state, o->B, o->d_ndone);
  HIPCHK(hipGetLastError());
  return 0;
}

// the rollout the handle's plant asks for: k_plant_rollout on the plant's inertials once a plant is set; otherwise the
// controller's model is its own plant: k_plant_rollout on its per-instance inertials if it has them, else k_feedback_rollout
int launch_rollout(agx_ocp *o, int n_substeps, double dt_sub, const double *d_dist) {
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    if (o->plant_set || o->minert_set)
      hipLaunchKernelGGL((agx::k_plant_rollout<NV, CH>), dim3((o->B + 63) / 64), dim3(64), 0, o->stream, o->d_model,
                         (const agx::PlantInertials<NV> *)(o->plant_set ? o->d_plant : o->d_minert), o->d_us, o->d_Kout, o->d_x0, d_dist, o->B, o->T,
                         n_substeps, dt_sub);
    else
      hipLaunchKernelGGL((agx::k_feedback_rollout<NV, CH>), dim3((o->B + 63) / 64), dim3(64), 0, o->stream, o->d_model, o->d_us, o->d_Kout, o->d_x0,
                         d_dist, o->B, o->T, n_substeps, dt_sub);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int prof_mark(agx_ocp *o, int kind, bool start) {
  if (!o->prof) return 0;
  if (o->prof_used == o->prof_ev.size()) {  // events are created once and reused by every later solve
    o->prof_ev.push_back(nullptr);
    HIPCHK(o->own.event(&o->prof_ev.back()));
  }
  HIPCHK(hipEventRecord(o->prof_ev[o->prof_used++], o->stream));
  if (start) o->prof_kind.push_back(kind);
  return 0;
}
int prof_collect(agx_ocp *o) {
  if (!o->prof || o->prof_used == 0) return 0;
  HIPCHK(hipStreamSynchronize(o->stream));
  for (size_t k = 0; k < o->prof_kind.size(); ++k) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, o->prof_ev[2 * k], o->prof_ev[2 * k + 1]));
    o->prof_ms[o->prof_kind[k]] += ms;
    o->prof_n[o->prof_kind[k]] += 1;
  }
  o->prof_used = 0;
  o->prof_kind.clear();
  return 0;
}

// Hand-off of one word from the stream to the host without a copy or a synchronize: a one-thread
// kernel stores value and sequence stamp into mapped pinned memory, the host spins on the stamp.
int publish(agx_ocp *o, int slot_value, int slot_seq, const int *d_value, unsigned long long seq) {
  hipLaunchKernelGGL(agx::k_publish, dim3(1), dim3(1), 0, o->stream, d_value, o->h_ndone_dev + slot_value, o->h_ndone_dev + slot_seq, seq);
  HIPCHK(hipGetLastError());
  return 0;
}
int wait_stamp(agx_ocp *o, int slot_seq, unsigned long long seq) {
  volatile unsigned long long *w = o->h_ndone + slot_seq;
  const auto t_begin = std::chrono::steady_clock::now();
  for (unsigned long spins = 1;; ++spins) {
    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return 0;
    if ((spins & 0x3FFF) == 0) {  // every so often make sure the stream is still alive and not stuck
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count() > 120.0)
        return fail("timed out after 120 s waiting for the device (stamp never published)");
      const hipError_t e = hipStreamQuery(o->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == seq) return 0;
        return fail("stream drained without publishing its stamp");
      }
      if (e != hipErrorNotReady) return fail(std::string("stream error while waiting: ") + hipGetErrorString(e));
    }
    __builtin_ia32_pause();
  }
}

// stream-ordered read of one device int (polled stamp or copy + synchronize)
int read_int(agx_ocp *o, const int *d_value, int slot_value, int slot_seq, int *out) {
  const unsigned long long seq = ++o->seq;
  if (o->poll) {
    if (publish(o, slot_value, slot_seq, d_value, seq)) return -1;
    if (wait_stamp(o, slot_seq, seq)) return -1;
  } else {
    o->h_ndone[slot_value] = 0;  // the 4-byte copy below fills the low half (little endian)
    HIPCHK(hipMemcpyAsync(o->h_ndone + slot_value, d_value, sizeof(int), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
  }
  *out = (int)__atomic_load_n(o->h_ndone + slot_value, __ATOMIC_ACQUIRE);
  return 0;
}

int quorum_count(int B, double q) {
  if (!(q < 1.0)) return B;
  const int n = (int)std::ceil(q * B - 1e-9);
  return n < 1 ? 1 : (n > B ? B : n);
}

// Constraint values / Jacobian rows / violation of every node at (xs, us): 8 lanes per node for serial chains whose rows are
// control limits, state bounds and collision distances (k_con_eval_lj, wide sets: k_con_eval_pairs), else one lane per node
// (k_con_eval).
template <int NV, bool CH>
void launch_con_eval(agx_ocp *o, const double *xs, const double *us, int phase) {
  if constexpr (NV <= 7) {
    const long long nodes = (long long)o->B * (o->T + 1);
    with_sources<NV, false, true>(o, [&](auto... src) {
      if (o->con_wide)
        hipLaunchKernelGGL((agx::k_con_eval_pairs<NV, src_t<decltype(src)>...>), dim3((int)((nodes * 8 + 63) / 64)), dim3(64), 0, o->stream, o->d_model,
                           o->d_ocp, xs, us, o->d_cg, o->d_cjac, o->d_nodestat, o->d_state, phase, src...);
      else if (CH && o->con_lanes)
        hipLaunchKernelGGL((agx::k_con_eval_lj<NV, src_t<decltype(src)>...>), dim3((int)((nodes * 8 + 63) / 64)), dim3(64), 0, o->stream, o->d_model,
                           o->d_ocp, xs, us, o->d_cg, o->d_cjac, o->d_nodestat, o->d_state, phase, src...);
      else
        hipLaunchKernelGGL((agx::k_con_eval<NV, CH, src_t<decltype(src)>...>), dim3((int)((nodes + 63) / 64)), dim3(64), 0, o->stream, o->d_model,
                           o->d_ocp, xs, us, o->d_cg, o->d_cjac, o->d_nodestat, o->d_state, phase, src...);
    });
  }
}

// The ADMM loop of admm_direction for the 7-joint capacity; W: wide constraint sets (DevCons), the WIDE instances of the node kernels.
template <int NV, bool CH, bool W>
int admm_direction_nv7(agx_ocp *o, bool prefactor) {
  const long long nodes = (long long)o->B * (o->T + 1);
  const int g8 = (int)((nodes * 8 + 255) / 256), g8b = (int)((nodes * 8 + 127) / 128), g1 = (int)((nodes + 255) / 256);
  if (prefactor) {
    if (!o->d_Kws_lqr) {
      HIPCHK(o->own.device(&o->d_Kws_lqr, (size_t)o->B * o->T * o->nu * o->nx));
      HIPCHK(o->own.device(&o->d_kws_lqr, (size_t)o->B * o->T * o->nu));
    }
    // constraint data and the augmented Hessians need only (xs, us) and rho: before the LQR pass
    launch_con_eval<NV, CH>(o, o->d_xs, o->d_us, 0);
    hipLaunchKernelGGL(agx::k_admm_pre, dim3((o->B + 255) / 256), dim3(256), 0, o->stream, o->d_ocp, o->d_state);
    hipLaunchKernelGGL((agx::k_admm_tile<NV, W>), dim3(g8b), dim3(128), 0, o->stream, o->d_ocp, o->d_qt, o->d_qt2, o->d_aux, o->d_cx,
                       o->d_du, o->d_cjac, o->d_y, o->d_z, o->d_state, 0);  // its gradient part is rewritten below
    hipLaunchKernelGGL((agx::k_riccati_lqr_prefactor<NV>), dim3(2 * o->B), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_qt2,
                       o->d_aux, o->d_Kws, o->d_kws, o->d_Kws_lqr, o->d_kws_lqr, o->d_dx, o->d_w, o->d_du, o->d_Kout, o->d_state, o->d_fac);
    if (o->admm_segments)
      hipLaunchKernelGGL((agx::k_seg_products<NV>), dim3(o->B * agx::kSeg), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_Kws, o->d_segP,
                         o->d_state);
    HIPCHK(hipGetLastError());
  }
  if (launch_step(o, 0, 0, 0, true, false)) return -1;  // du of the initial guess (k_node_kkt)
  HIPCHK(hipMemsetAsync(o->d_ndone + 1, 0, sizeof(int), o->stream));
  hipLaunchKernelGGL((agx::k_admm_init<NV, W>), dim3(g1), dim3(256), 0, o->stream, o->d_ocp, o->d_dx, o->d_cx, o->d_z, o->d_state,
                     o->d_ndone + 1);
  if (!prefactor)
    launch_con_eval<NV, CH>(o, o->d_xs, o->d_us, 0);
  HIPCHK(hipGetLastError());
  const int max_qp = o->ho.max_qp;
  // Polls the count of converged QPs; true when the loop ends here (quorum reached: the others are capped at `iter`)
  auto quorum_reached = [&](int iter, bool *stop) -> int {
    int n_conv = 0;
    *stop = false;
    if (read_int(o, o->d_ndone + 1, 4, 5, &n_conv)) return -1;
    if (n_conv >= quorum_count(o->B, o->quorum_qp)) {
      if (n_conv < o->B && iter < max_qp) {  // quorum reached: the others stop here with the iterations they ran
        hipLaunchKernelGGL(agx::k_admm_cap, dim3((o->B + 255) / 256), dim3(256), 0, o->stream, o->d_state, o->B, iter);
        HIPCHK(hipGetLastError());
      }
      *stop = true;
    }
    return 0;
  };
  for (int iter = 1; iter <= max_qp;) {
    // augmented Hessians change at the first iteration and after a rho update (k_admm_reduce decides at
    // multiples of kRhoInterval); in between k_admm_update leaves the next gradient behind
    const bool boundary = iter == 1 || (iter > 2 && (iter - 1) % agx::kRhoInterval == 0);
    if (!boundary && o->admm_loop && o->admm_segments && (o->admm_loop_always || 4 * o->n_unfinished <= o->B)) {
      // gradient-only iterations up to the next rho check in one launch per instance (k_admm_loop); with a quorum < 1 in the
      // chunks of the host's polling schedule, so that which instances are cut does not depend on the workgroups' progress
      int last = ((iter - 1) / agx::kRhoInterval + 1) * agx::kRhoInterval;
      if (o->quorum_qp < 1.0) last = std::min(last, ((iter + 3) / 4) * 4);
      last = std::min(last, max_qp);
      hipLaunchKernelGGL((agx::k_admm_loop<NV, W>), dim3(o->B), dim3(64 * agx::kSeg), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt, o->d_qt2, o->d_aux,
                         o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_du, o->d_cx, o->d_cg, o->d_cjac, o->d_y, o->d_z, o->d_nodestat,
                         o->d_admmstat, o->d_state, o->d_fac, o->d_segP, iter, last, o->d_ndone + 1,
                         o->general ? (const double *)o->d_auxg : (const double *)nullptr);
      HIPCHK(hipGetLastError());
      iter = last + 1;
      bool stop;
      if (quorum_reached(last, &stop)) return -1;
      if (stop) break;
      continue;
    }
    const bool pre = prefactor && iter == 1;  // Hessian and factors of this iteration exist: gradient only
    if (boundary)
      hipLaunchKernelGGL((agx::k_admm_tile<NV, W>), dim3(g8b), dim3(128), 0, o->stream, o->d_ocp, o->d_qt, o->d_qt2, o->d_aux, o->d_cx,
                         o->d_du, o->d_cjac, o->d_y, o->d_z, o->d_state, pre ? 1 : 0);
    const bool may_refactor = !pre && boundary;
    hipLaunchKernelGGL((agx::k_riccati_admm<NV>), dim3(o->B), dim3(64 * agx::kSeg), 0, o->stream, o->d_ocp, o->d_dt, o->d_qt2, o->d_aux,
                       o->d_Kws, o->d_kws, o->d_dx, o->d_w, o->d_du, o->d_Kout, o->d_state, o->d_fac,
                       o->admm_segments ? (const double *)o->d_segP : (const double *)nullptr, pre ? 1 : 0);
    if (may_refactor && o->admm_segments)  // new gains: the segments' closed-loop products for the gradient-only sweeps that follow
      hipLaunchKernelGGL((agx::k_seg_products<NV>), dim3(o->B * agx::kSeg), dim3(64), 0, o->stream, o->d_ocp, o->d_dt, o->d_Kws, o->d_segP,
                         o->d_state);
    hipLaunchKernelGGL((agx::k_admm_update<NV, W>), dim3(g8), dim3(256), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux, o->d_dx, o->d_w,
                       o->d_du, o->d_cx, o->d_cg, o->d_cjac, o->d_y, o->d_z, o->d_nodestat, o->d_admmstat, o->d_qt2, o->d_state,
                       o->general ? (const double *)o->d_auxg : (const double *)nullptr);
    hipLaunchKernelGGL(agx::k_admm_reduce, dim3(o->B), dim3(128), 0, o->stream, o->d_ocp, o->d_admmstat, o->d_state, iter,
                       o->d_ndone + 1);
    HIPCHK(hipGetLastError());
    if (iter % 4 == 0 || iter == max_qp) {
      bool stop;
      if (quorum_reached(iter, &stop)) return -1;
      if (stop) break;
    }
    ++iter;
  }
  // the gains the solver reports: those of the last ADMM backward pass, in u-space
  const long long units = (long long)o->B * o->T * 16;
  hipLaunchKernelGGL((agx::k_gains_to_u<NV>), dim3((int)((units + 255) / 256)), dim3(256), 0, o->stream, o->d_ocp, o->d_aux, o->d_Kws,
                     o->d_Kout, o->d_state);
  HIPCHK(hipGetLastError());
  return 0;
}

// Constrained direction of one SQP iteration (SolverCSQP::computeDirection): the plain LQR pass has
// run (equality-QP initial guess: dx, w); now du, the constraint data and the ADMM loop.
// prefactor: the plain LQR pass has NOT run yet -- it is launched here, in one kernel with the factorisation of the
// augmented Hessians of the first ADMM iteration (k_riccati_lqr_prefactor).
int admm_direction(agx_ocp *o, bool prefactor = false) {
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    if constexpr (NV > 7) {
      // Large models: control-limit rows only (agx_ocp_create), every ADMM iteration factorises (k_riccati_blk on the
      // augmented tile); the node kernels are k_admm_tile_big / k_admm_update_big (agx_big.hpp), norms and rho schedule
      // as for the 7-joint path (k_admm_reduce).
      (void)CH; (void)prefactor;
      const long long nodes = (long long)o->B * (o->T + 1);
      const int g1 = (int)((nodes + 255) / 256);
      if (launch_step(o, 0, 0, 0, true, false)) return -1;  // du of the initial guess (k_node_kkt_big)
      HIPCHK(hipMemsetAsync(o->d_ndone + 1, 0, sizeof(int), o->stream));
      hipLaunchKernelGGL((agx::k_admm_init<NV>), dim3(g1), dim3(256), 0, o->stream, o->d_ocp, o->d_dx, o->d_cx, o->d_z, o->d_state, o->d_ndone + 1);
      launch_wg(o, [&](auto PRc) {
        hipLaunchKernelGGL((agx::k_con_eval_wg<NV, decltype(PRc)::value>), dim3((int)nodes), dim3(256), 0, o->stream, o->d_model, o->d_ocp, o->d_xs, o->d_us, o->d_cg, o->d_cjac,
                         o->d_nodestat, o->d_state, 0);
      });
      HIPCHK(hipGetLastError());
      const int max_qp = o->ho.max_qp;
      for (int iter = 1; iter <= max_qp; ++iter) {
        if (iter == 1 || (iter > 2 && (iter - 1) % agx::kRhoInterval == 0))  // Hessian part: first iteration and after a rho update
          hipLaunchKernelGGL((agx::k_admm_tile_big<NV>), dim3((int)nodes), dim3(256), 0, o->stream, o->d_ocp, o->d_qt, o->d_qt2, o->d_aux, o->d_cx,
                             o->d_du, o->d_cjac, o->d_y, o->d_z, o->d_state);
        launch_riccati_blk<NV>(o, o->d_qt2, 1, 0);
        hipLaunchKernelGGL((agx::k_admm_update_big<NV>), dim3((int)((nodes + 1) / 2)), dim3(64), 0, o->stream, o->d_ocp, o->d_qt, o->d_aux, o->d_dx,
                           o->d_w, o->d_du, o->d_cx, o->d_cg, o->d_cjac, o->d_y, o->d_z, o->d_nodestat, o->d_admmstat, o->d_qt2, o->d_state);
        hipLaunchKernelGGL(agx::k_admm_reduce, dim3(o->B), dim3(128), 0, o->stream, o->d_ocp, o->d_admmstat, o->d_state, iter, o->d_ndone + 1);
        HIPCHK(hipGetLastError());
        if (iter % 4 == 0 || iter == max_qp) {
          int n_conv = 0;
          if (read_int(o, o->d_ndone + 1, 4, 5, &n_conv)) return -1;
          if (n_conv >= quorum_count(o->B, o->quorum_qp)) {
            if (n_conv < o->B && iter < max_qp) {
              hipLaunchKernelGGL(agx::k_admm_cap, dim3((o->B + 255) / 256), dim3(256), 0, o->stream, o->d_state, o->B, iter);
              HIPCHK(hipGetLastError());
            }
            break;
          }
        }
      }
      // the gains the solver reports: those of the last ADMM backward pass, in u-space
      const long long units = (long long)o->B * o->T * 64;
      hipLaunchKernelGGL((agx::k_gains_to_u_big<NV>), dim3((int)((units + 255) / 256)), dim3(256), 0, o->stream, o->d_ocp, o->d_aux, o->d_Kws,
                         o->d_Kout, (const DevState *)nullptr);
      HIPCHK(hipGetLastError());
      return 0;
    } else {
      if constexpr (CH) if (o->con_wide) return admm_direction_nv7<NV, CH, true>(o, prefactor);
      return admm_direction_nv7<NV, CH, false>(o, prefactor);
    }
  });
}

// Every entry point that changes an input of the derivative pass, the iterate or the tiles outside agx_ocp_mpc_step: the next
// step runs the full pass, with the tiles back in node order.  The same calls may change what the first-node block was packed
// from during the last solve (iterate, gains, state): the next agx_ocp_first_packed packs again.
int carry_invalidate(agx_ocp *o) {
  o->carry_armed = false;
  o->first_fresh = false;
  if (o->head != 0) {
    o->head = 0;
    HIPCHK(hipMemsetAsync((char *)o->d_ocp + offsetof(DevOcp, head), 0, sizeof(int), o->stream));
  }
  return 0;
}

// agx_ocp_refs_activate: the tile staged by agx_ocp_set_refs_async becomes the solver's tile -- the solver's stream waits
// for the copy (no host wait) and the two device tiles swap roles.
int adopt_pending_refs(agx_ocp *o) {
  if (!o->refs_pending) return 0;
  if (carry_invalidate(o)) return -1;
  if (o->refs_pending_frames) o->frames_uniform = false;
  HIPCHK(hipStreamWaitEvent(o->stream, o->ev_refs, 0));
  std::swap(o->d_ref, o->d_ref_back);  // (both fields stay registered with the owner, which reads them when it frees)
  if (o->refs_pending_frames) std::swap(o->d_frames, o->d_frames_back);
  rv_own_tile(o, o->refs_pending_frames ? o->d_frames : nullptr);
  o->refs_pending = false;
  return 0;
}
int ensure_copy_stream(agx_ocp *o) {
  if (o->copy_stream) return 0;
  HIPCHK(hipStreamCreateWithFlags(&o->copy_stream, hipStreamNonBlocking));
  HIPCHK(o->own.event(&o->ev_refs, hipEventDisableTiming));
  HIPCHK(o->own.event(&o->ev_snap, hipEventDisableTiming));
  HIPCHK(o->own.event(&o->ev_dl, hipEventDisableTiming));
  return 0;
}

// Trial rounds of the line search of SQP iteration `it` (nv <= 7; k_sqp_head has written the first trial iterate):
// derivative pass (+ constraint evaluation) at the trial points, k_sqp_accept, and -- only while the counter of handed-on
// trials grows, i.e. when somebody rejected a step length -- the same again.  The finished-instance count comes back
// under the same stamp, and so does the counter of iterations that ended with every trial rejected: only then does the
// next iteration need a derivative pass of its own (`need_k1`); after an accepted trial the tiles are already there.
// `head_seq` != 0 (large batches, from the second iteration on): the counters the head left were published right behind it under
// that stamp (slots 10 .. 13).  The first round is queued without asking, as ever; then the host looks at the head's words, and
// when they say that every instance has finished it leaves without waiting for the round: its launches find nobody searching,
// change no counter, and stay queued ahead of whatever the stream gets next.
int line_search_rounds(agx_ocp *o, int it, int max_iter, bool *need_k1, int *n_done_out, unsigned long long head_seq = 0) {
  double *xs_t = o->d_xs + (size_t)o->B * (o->T + 1) * o->nx, *us_t = o->d_us + (size_t)o->B * o->T * o->nu;
  for (int round = 0; round < 10; ++round) {
    if (o->prof && round == 0 && it == 0) {  // the kernel the roofline is quoted on, timed alone: running nodes of the trial pass of the first
                                             // iteration (every unfinished instance searches; later iterations serve a few stragglers: not the launch the bytes are counted for)
      if (prof_mark(o, 0, true)) return -1;
      if (launch_calc_qp(o, true, false, 1)) return -1;
      if (prof_mark(o, 0, false)) return -1;
      if (launch_calc_qp(o, false, true, 1)) return -1;
    } else if (launch_calc_qp(o, false, false, 1)) return -1;
    const unsigned long long seq = ++o->seq;
    int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
      constexpr int NV = decltype(NVc)::value;
      constexpr bool CH = decltype(CHc)::value;
      (void)CH;
      if constexpr (NV <= 7) if (o->has_con) {
        launch_con_eval<NV, CH>(o, xs_t, us_t, 1);
      }
      if constexpr (NV > 7) if (o->has_con) {
        const long long nodes = (long long)o->B * (o->T + 1);
        launch_wg(o, [&](auto PRc) {
        hipLaunchKernelGGL((agx::k_con_eval_wg<NV, decltype(PRc)::value>), dim3((int)nodes), dim3(256), 0, o->stream, o->d_model, o->d_ocp, xs_t, us_t, o->d_cg, o->d_cjac,
                           o->d_nodestat, o->d_state, 1);
      });
      }
      if (prof_mark(o, 2, true)) return -1;
      hipLaunchKernelGGL((agx::k_sqp_accept<NV>), dim3(o->B), dim3(128), 0, o->stream, o->d_ocp, o->d_xs, o->d_us, o->d_dx, o->d_du, xs_t, us_t,
                         o->d_qt, o->d_nodestat, o->d_state, it, max_iter, o->d_ndone, host_words(o, true, seq));
      HIPCHK(hipGetLastError());
      return prof_mark(o, 2, false);
    });
    if (rc) return rc;
    if (o->poll && o->fold_publish) {
      if (wait_stamp(o, 1, seq)) return -1;  // stored by the last workgroup of k_sqp_accept
    } else if (o->poll) {
      hipLaunchKernelGGL(agx::k_publish3, dim3(1), dim3(1), 0, o->stream, o->d_ndone, o->h_ndone_dev + 0, o->h_ndone_dev + 6, o->h_ndone_dev + 7,
                         o->h_ndone_dev + 8, o->h_ndone_dev + 9, o->h_ndone_dev + 1, seq);
      HIPCHK(hipGetLastError());
      if (round == 0 && head_seq != 0) {
        if (wait_stamp(o, 10, head_seq)) return -1;
        const int done_at_head = (int)__atomic_load_n(o->h_ndone + 11, __ATOMIC_ACQUIRE);
        if (done_at_head >= o->B) {
          *n_done_out = done_at_head;
          o->n_carriable = (int)__atomic_load_n(o->h_ndone + 12, __ATOMIC_ACQUIRE);
          o->n_packed = (int)__atomic_load_n(o->h_ndone + 13, __ATOMIC_ACQUIRE);
          o->early_exits += 1;
          return 0;
        }
      }
      if (wait_stamp(o, 1, seq)) return -1;
    } else {
      o->h_ndone[0] = 0; o->h_ndone[6] = 0; o->h_ndone[7] = 0; o->h_ndone[8] = 0; o->h_ndone[9] = 0;  // (no mapped block on this path: nothing is packed in the solve)
      HIPCHK(hipMemcpyAsync(o->h_ndone + 8, o->d_ndone + 6, sizeof(int), hipMemcpyDeviceToHost, o->stream));
      HIPCHK(hipMemcpyAsync(o->h_ndone, o->d_ndone, sizeof(int), hipMemcpyDeviceToHost, o->stream));
      HIPCHK(hipMemcpyAsync(o->h_ndone + 6, o->d_ndone + 3, sizeof(int), hipMemcpyDeviceToHost, o->stream));
      HIPCHK(hipMemcpyAsync(o->h_ndone + 7, o->d_ndone + 4, sizeof(int), hipMemcpyDeviceToHost, o->stream));
      HIPCHK(hipStreamSynchronize(o->stream));
    }
    *n_done_out = (int)__atomic_load_n(o->h_ndone, __ATOMIC_ACQUIRE);
    const unsigned handed = (unsigned)__atomic_load_n(o->h_ndone + 6, __ATOMIC_ACQUIRE);
    const unsigned stale = (unsigned)__atomic_load_n(o->h_ndone + 7, __ATOMIC_ACQUIRE);
    o->n_carriable = (int)__atomic_load_n(o->h_ndone + 8, __ATOMIC_ACQUIRE);
    o->n_packed = (int)__atomic_load_n(o->h_ndone + 9, __ATOMIC_ACQUIRE);
    const bool more = handed != o->ls_handed;
    if (stale != o->ls_stale) *need_k1 = true;
    o->ls_handed = handed;
    o->ls_stale = stale;
    if (!more) break;
  }
  return 0;
}

// Per-iteration solver log: k_iter_log (agx_diag.hip) behind the head (phase 0) and behind the trial rounds (phase 1) of SQP
// iteration `it`.  Off: nothing is launched.
int iter_log_mark(agx_ocp *o, int it, int phase) {
  if (o->log_cap <= 0) return 0;
  HIPCHK((hipError_t)agx_diag_iter_log_launch((void *)o->stream, o->d_state, o->B, it, phase, o->d_log, o->d_log_n, o->log_cap));
  return 0;
}

// The SQP loop of SolverCSQP::solve on the resident buffers.
// carry_mode (agx_ocp_mpc_step): 0 no instance inherits tiles, 1 some do (k_mpc_prologue has decided: DevState::carry), 2 all do.
int solve_resident(agx_ocp *o, int max_iter, double max_time, bool prologue_done = false, int carry_mode = 0) {
  if (max_iter <= 0) max_iter = 1000;
  o->last_max_iter = max_iter;
  o->n_carriable = -1;
  o->first_fresh = false;
  o->n_packed = 0;
  const bool packing = first_block(o) != nullptr;
  bool cut = false;  // the loop ended on a quorum or the time limit with instances unfinished
  auto t0 = std::chrono::steady_clock::now();
  if (!prologue_done) {  // k_mpc_prologue has reset the state and pinned x0 already
    if (reset_state(o)) return -1;
    hipLaunchKernelGGL(agx::k_pin_x0, dim3((o->B * o->nx + 255) / 256), dim3(256), 0, o->stream, o->d_xs, o->d_x0, o->B, o->T, o->nx);
  }
  if (o->log_cap > 0) HIPCHK(hipMemsetAsync(o->d_log_n, 0, sizeof(int) * (size_t)o->B, o->stream));  // every solve starts the log afresh
  // Every iteration after the first finds its tiles already there (the accepted trial of the line search left them); a
  // derivative pass of its own is needed at the start and after an iteration that ended with every step length rejected.
  bool need_k1 = true;
  const bool tail = step_tail_path(o);  // the sweep leaves its forward pass to the launch that also holds K3 and the head
  // the exit fix-up of the gains is launched only if an instance can have finished (or the loop can
  // have ended) in an iteration whose direction sweep was not paired with the gains sweep
  bool need_fixup = false;
  int prev_done = 0;
  for (int it = 0; it < max_iter; ++it) {
    const bool pair = o->speculate && it >= 1 && !o->has_con && o->nv <= 7;  // large models: gains only on exit
    o->n_unfinished = o->B - prev_done;
    // derivative pass: running and terminal nodes in one launch; under agx_ocp_profile the running
    // nodes get their own launch so that the kernel the roofline is quoted on is timed alone
    if (need_k1) {
      if (it == 0 && carry_mode != 0) {
        // inherited tiles: nodes 0, T - 1 and T of every carrying instance -- on a grid of just those when everybody carries.
        // Never the launch the roofline is quoted on (prof_mark 0 stands for a pass over all B T running nodes).
        if (launch_calc_qp(o, false, false, 0, carry_mode == 2)) return -1;
      } else if (o->prof && it == 0) {
        if (prof_mark(o, 0, true)) return -1;
        if (launch_calc_qp(o, true, false)) return -1;
        if (prof_mark(o, 0, false)) return -1;
        if (launch_calc_qp(o, false, true)) return -1;
      } else if (launch_calc_qp(o, false, false)) return -1;
    }
    need_k1 = false;
    if (prof_mark(o, 1, true)) return -1;
    // from the second iteration on (where warm-started MPC steps converge) the gains sweep rides along
    if (o->has_con && o->admm_prefactor && o->riccati_mx && o->nv <= 7 && !o->general) {
      if (admm_direction(o, true)) return -1;  // LQR pass inside, next to the ADMM factorisation
    } else {
      if (launch_riccati(o, tail ? 0 : 1, pair, it)) return -1;
      if (o->has_con && admm_direction(o)) return -1;
    }
    if (prof_mark(o, 1, false)) return -1;
    const bool last = it + 1 == max_iter;
    if (prof_mark(o, 2, true)) return -1;
    const unsigned long long seq_head = ++o->seq;
    if (tail ? launch_step_tail(o, it, max_iter, seq_head, pair && packing)
             : launch_step(o, it, max_iter, 1, !o->has_con, true, seq_head, pair && packing)) return -1;
    if (prof_mark(o, 2, false)) return -1;
    if (iter_log_mark(o, it, 0)) return -1;  // the evaluation and how the head left every instance, before a trial round moves on
    // Large batches, from the second iteration on (where warm-started MPC steps converge): what the head left, to the host
    // under a stamp of its own right behind it -- the trial round below is still queued without asking, but the host no longer
    // waits for it when the head has finished everyone (line_search_rounds).
    unsigned long long seq_early = 0;
    if (o->poll && !o->fold_publish && !o->prof && !o->no_empty && it >= 1) {
      seq_early = ++o->seq;
      hipLaunchKernelGGL(agx::k_publish3, dim3(1), dim3(1), 0, o->stream, o->d_ndone, o->h_ndone_dev + 11, (unsigned long long *)nullptr, (unsigned long long *)nullptr, o->h_ndone_dev + 12,
                         o->h_ndone_dev + 13, o->h_ndone_dev + 10, seq_early);
      HIPCHK(hipGetLastError());
    }
    int n_done = 0;
    // The trial passes overwrite the tiles of this iterate.  Where the loop may end right after this iteration without a
    // paired gains sweep (iteration cap, time limit, quorum), the sweep that yields the reported gains runs first --
    // for the instances the head has not finished (those keep their tiles for the fix-up on exit).
    if (!pair && !o->has_con && (last || max_time > 0.0 || o->quorum_sqp < 1.0)) {
      if (launch_gains(o, 4)) return -1;
    }
    // Small batches: from the second iteration on a warm-started step usually ends at the head, whose last workgroup has
    // handed the finished count over: the host asks before it launches trial passes that would find nobody searching (in the
    // first iteration it does not wait: somebody nearly always searches, and the trial pass starts right behind the head).
    bool searching = true;
    if (o->poll && o->fold_publish && it >= 1) {
      if (wait_stamp(o, 1, seq_head)) return -1;
      n_done = (int)__atomic_load_n(o->h_ndone, __ATOMIC_ACQUIRE);
      o->n_carriable = (int)__atomic_load_n(o->h_ndone + 8, __ATOMIC_ACQUIRE);
      o->n_packed = (int)__atomic_load_n(o->h_ndone + 9, __ATOMIC_ACQUIRE);
      searching = n_done < o->B;
    } else if (o->prof || o->no_empty) {  // timing / profiling runs: no launches that find nothing to do
      if (read_int(o, o->d_ndone, 0, 1, &n_done)) return -1;
      searching = n_done < o->B;
      if (!searching && read_int(o, o->d_ndone + 6, 8, 1, &o->n_carriable)) return -1;  // (the line search would have brought it)
      if (!searching && pair && packing && read_int(o, o->d_ndone + 7, 9, 1, &o->n_packed)) return -1;  // (likewise)
    }
    if (searching && line_search_rounds(o, it, max_iter, &need_k1, &n_done, seq_early)) return -1;
    if (iter_log_mark(o, it, 1)) return -1;  // the outcome of the search (queued behind the trial round where the host left it early)
    if (last) { need_fixup = need_fixup || !pair; break; }
    if (!pair && n_done > prev_done) need_fixup = true;
    prev_done = n_done;
    if (n_done >= quorum_count(o->B, o->quorum_sqp)) {
      if (n_done < o->B) { o->last_max_iter = it + 1; cut = true; }  // the stragglers stop here: iterations that really ran
      break;
    }
    if (max_time > 0.0) {
      // SolverCSQP max_solve_time (ocp_base_croco.py:70-71): checked once per SQP iteration; unfinished instances
      // report the iterations that really ran
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > max_time) { need_fixup = need_fixup || !pair; o->last_max_iter = it + 1; cut = true; break; }
    }
  }
  if (!o->has_con && need_fixup && launch_gains(o, 2)) return -1;  // instances whose last direction has no gains sweep yet
  // every instance packed its first-node record where it converged, and nothing has been launched on the gains since
  o->first_fresh = packing && o->n_packed == o->B && !need_fixup && !cut;
  return prof_collect(o);
}

int launch_cost_pairs(agx_ocp *o, int dest, int sel, int phase, bool masked, int which, double *dist) {
  if (!o->cost_wide || o->nv != 7 || !o->chain) return fail("wide cost sets run on serial chains of revolute joints, at most 7 of them");  // agx_ocp_create admits nothing else
  const long long nodes = (long long)o->B * (o->T + 1);
  const double *xs_in = phase ? o->d_xs + (size_t)o->B * (o->T + 1) * o->nx : o->d_xs;
  double *out = dest == agx::kPairsToQp ? o->d_qt : (dest == agx::kPairsToCanonical ? o->d_tiles : dist);
  const DevState *st = dest == agx::kPairsToQp ? o->d_state : ((dest == agx::kPairsToCanonical && masked) ? o->d_state : nullptr);
  HIPCHK((hipError_t)agx_cost_pairs_launch(dest, (void *)o->stream, nodes, o->d_model, o->d_ocp, o->d_cw, o->d_dt, xs_in, &o->rv, out,
                                           dest == agx::kPairsToQp ? o->d_aux : nullptr, st, dest == agx::kPairsToQp ? phase : 0,
                                           dest == agx::kPairsDistance ? 1 : sel, which, o->obs_set ? o->d_obs : nullptr));
  return 0;
}

}  // namespace

#include "agx_host_traj.hpp"

extern "C" {

const char *agx_last_error(void) { return g_err.c_str(); }

int agx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int agx_row_nref(int kind, int nv) {
  switch (kind) {
    case AGX_RES_STATE: return 2 * nv;
    case AGX_RES_CONTROL: return nv;
    case AGX_RES_CONTROL_GRAV: return 0;
    case AGX_RES_FRAME_PLACEMENT: return 12;
    case AGX_RES_FRAME_TRANSLATION: return 3;
    case AGX_RES_FRAME_ROTATION: return 9;
    case AGX_RES_FRAME_VELOCITY: return 6;
    case AGX_RES_COLLISION: return 0;
  }
  return -1;
}
int agx_row_nr(int kind, int nv) {
  switch (kind) {
    case AGX_RES_STATE: return 2 * nv;
    case AGX_RES_CONTROL: return nv;
    case AGX_RES_CONTROL_GRAV: return nv;
    case AGX_RES_FRAME_PLACEMENT: return 6;
    case AGX_RES_FRAME_TRANSLATION: return 3;
    case AGX_RES_FRAME_ROTATION: return 3;
    case AGX_RES_FRAME_VELOCITY: return 6;
    case AGX_RES_COLLISION: return 1;
  }
  return -1;
}
int agx_ref_stride(const agx_ocp_desc *d, int nv) {
  int s0 = 0, s1 = 0;
  for (int r = 0; r < d->n_running_rows; ++r) s0 += 1 + agx_row_nref(d->running_rows[r].kind, nv) + agx_row_nr(d->running_rows[r].kind, nv);
  for (int r = 0; r < d->n_terminal_rows; ++r) s1 += 1 + agx_row_nref(d->terminal_rows[r].kind, nv) + agx_row_nr(d->terminal_rows[r].kind, nv);
  return std::max(std::max(s0, s1), 1);
}

int agx_model_create(const agx_model_desc *d, agx_model **out) {
  if (!d || !out) return fail("agx_model_create: null argument");
  if (d->nv < 1 || d->nv > AGX_MAX_NV) return fail("agx_model_create: nv out of range");
  if (d->nframes < 0 || d->nframes > AGX_MAX_FRAMES) return fail("agx_model_create: too many frames");
  const int cap = pad_capacity(d->nv);
  if (cap == 0) return fail("agx_model_create: no compiled capacity holds nv = " + std::to_string(d->nv));
  agx_model *m = new agx_model();
  m->nvu = d->nv;
  DevModel &h = m->h;
  std::memset(&h, 0, sizeof(h));
  h.nv = cap;
  h.nframes = d->nframes;
  h.is_chain = 1;
  for (int i = 0; i < d->nv; ++i) {
    h.parent[i] = d->parent[i];
    if (d->parent[i] >= i || d->parent[i] < -1) { delete m; return fail("agx_model_create: parents must precede children"); }
    if (d->parent[i] != i - 1) h.is_chain = 0;
    h.anc[i] = (1u << i) | (d->parent[i] >= 0 ? h.anc[d->parent[i]] : 0u);
    for (int j = 0; j <= i; ++j)
      if ((h.anc[i] >> j) & 1u) h.desc[j] |= (1u << i);
    std::memcpy(h.placement[i], d->placement + 12 * i, sizeof(double) * 12);
    std::memcpy(h.axis[i], d->axis + 3 * i, sizeof(double) * 3);
    h.mass[i] = d->mass[i];
    std::memcpy(h.com[i], d->com + 3 * i, sizeof(double) * 3);
    std::memcpy(h.inertia[i], d->inertia + 9 * i, sizeof(double) * 9);
    h.armature[i] = d->armature ? d->armature[i] : 0.0;
    const int jt = d->joint_type ? d->joint_type[i] : AGX_JOINT_REVOLUTE;
    if (jt != AGX_JOINT_REVOLUTE && jt != AGX_JOINT_PRISMATIC) {
      delete m;
      return fail("agx_model_create: joint " + std::to_string(i) + " has joint_type " + std::to_string(jt) + ": 0 (revolute) and 1 (prismatic) are supported");
    }
    if (jt == AGX_JOINT_PRISMATIC) h.prismatic |= 1u << i;
  }
  // The eight-lane kernels, wide cost / constraint sets and the tile carry are written for serial chains of revolute joints: a model
  // with a prismatic joint takes the kernels (and the padding) of a tree of its size, which know both joint types.
  if (h.prismatic) h.is_chain = 0;
  // pad joints (robot_model.py:231-257 takes any URDF and any set of locked joints; the kernels come in a few capacities): massless,
  // unit armature, identity placement, revolute -- appended to a serial chain of revolute joints (the eight-lane kernel needs one), children
  // of the universe otherwise
  for (int i = d->nv; i < cap; ++i) {
    h.parent[i] = h.is_chain ? i - 1 : -1;
    h.anc[i] = (1u << i) | (h.parent[i] >= 0 ? h.anc[h.parent[i]] : 0u);
    for (int j = 0; j <= i; ++j)
      if ((h.anc[i] >> j) & 1u) h.desc[j] |= (1u << i);
    h.placement[i][0] = h.placement[i][4] = h.placement[i][8] = 1.0;
    h.axis[i][2] = 1.0;
    h.armature[i] = 1.0;
  }
  h.gravity[0] = d->gravity ? d->gravity[0] : 0.0;
  h.gravity[1] = d->gravity ? d->gravity[1] : 0.0;
  h.gravity[2] = d->gravity ? d->gravity[2] : -9.81;
  for (int f = 0; f < d->nframes; ++f) {
    h.frame_parent[f] = d->frame_parent[f];
    if (d->frame_parent[f] >= d->nv) { delete m; return fail("agx_model_create: bad frame parent"); }
    std::memcpy(h.frame_placement[f], d->frame_placement + 12 * f, sizeof(double) * 12);
    h.frame_radius[f] = d->frame_radius ? d->frame_radius[f] : 0.0;
    h.frame_halflen[f] = d->frame_halflen ? d->frame_halflen[f] : 0.0;
    for (int e = 0; e < 3; ++e) h.frame_box[f][e] = d->frame_box ? d->frame_box[3 * f + e] : 0.0;
    if (h.frame_box[f][0] > 0.0 && !(h.frame_box[f][1] > 0.0 && h.frame_box[f][2] > 0.0)) {
      delete m;
      return fail("agx_model_create: box half extents must all be positive");
    }
  }
  *out = m;
  return 0;
}
void agx_model_destroy(agx_model *m) { delete m; }

int agx_ocp_create(const agx_model *m, const agx_ocp_desc *d, int batch, int device, agx_ocp **out) {
  if (!m || !d || !out) return fail("agx_ocp_create: null argument");
  if (batch < 1) return fail("agx_ocp_create: batch must be positive");
  if (d->horizon < 1) return fail("agx_ocp_create: horizon must be positive");
  if (d->n_running_rows < 0 || d->n_terminal_rows < 0) return fail("agx_ocp_create: negative row count");
  // Up to AGX_MAX_ROWS rows per node type keep the row table; more make a wide cost set: at most AGX_MAX_ROWS rows that are not
  // collision rows in front of at most AGX_MAX_COST_PAIRS trailing collision rows, on a serial chain of the 7-joint capacity.
  // AGX_COST_WIDE=1 gives every set with a collision cost row that layout where it meets these conditions.
  const CostSplit csplit[2] = {split_cost_rows(d->running_rows, d->n_running_rows), split_cost_rows(d->terminal_rows, d->n_terminal_rows)};
  bool cost_wide = false;
  {
    const bool wide_model = m->h.is_chain && m->h.nv <= 7;
    if (d->n_running_rows > AGX_MAX_ROWS || d->n_terminal_rows > AGX_MAX_ROWS) {
      for (int lay = 0; lay < 2; ++lay) {
        const char *which = lay ? "terminal" : "running";
        if (csplit[lay].n_other > AGX_MAX_ROWS)
          return fail(std::string("agx_ocp_create: too many cost rows: at most ") + std::to_string(AGX_MAX_ROWS) + " " + which +
                      " rows that are not collision rows (AGX_MAX_ROWS)");
        if (csplit[lay].n_pairs > AGX_MAX_COST_PAIRS)
          return fail(std::string("agx_ocp_create: too many cost rows: at most ") + std::to_string(AGX_MAX_COST_PAIRS) + " " + which +
                      " collision-pair cost rows (AGX_MAX_COST_PAIRS)");
        if (csplit[lay].offender >= 0)
          return fail(std::string("agx_ocp_create: the collision rows of a wide cost set (more than ") + std::to_string(AGX_MAX_ROWS) +
                      " cost rows) must be the trailing rows of the table: " + which + " row " + std::to_string(csplit[lay].offender) +
                      " has other rows behind it");
      }
      if (!m->h.is_chain) return fail("agx_ocp_create: a wide cost set (more than " + std::to_string(AGX_MAX_ROWS) + " cost rows per node type) needs a serial chain of revolute joints: trees and models with prismatic joints are not supported");
      if (m->h.nv > 7) return fail("agx_ocp_create: a wide cost set (more than " + std::to_string(AGX_MAX_ROWS) + " cost rows per node type) is implemented for models of at most 7 joints after padding");
      cost_wide = true;
    } else if (const char *e = getenv("AGX_COST_WIDE")) {
      cost_wide = e[0] == '1' && wide_model && csplit[0].n_pairs + csplit[1].n_pairs > 0 && csplit[0].offender < 0 && csplit[1].offender < 0;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("agx_ocp_create: no HIP device available (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail("agx_ocp_create: bad device index");
  for (int r = 0; r < d->n_running_rows + d->n_terminal_rows; ++r) {
    const agx_cost_row &row = r < d->n_running_rows ? d->running_rows[r] : d->terminal_rows[r - d->n_running_rows];
    switch (row.kind) {
      case AGX_RES_STATE: case AGX_RES_CONTROL: case AGX_RES_FRAME_PLACEMENT: case AGX_RES_FRAME_TRANSLATION: case AGX_RES_FRAME_ROTATION:
      case AGX_RES_COLLISION: break;
      case AGX_RES_CONTROL_GRAV: case AGX_RES_FRAME_VELOCITY:
        if (row.kind == AGX_RES_FRAME_VELOCITY && (row.frame < 0 || row.frame >= m->h.nframes || row.frame_b < 0 || row.frame_b > 2))
          return fail("agx_ocp_create: FrameVelocity row needs a valid frame and a reference frame 0 (WORLD), 1 (LOCAL) or 2 (LOCAL_WORLD_ALIGNED)");
        break;
      default: return fail("agx_ocp_create: residual kind " + std::to_string(row.kind) + " is not implemented on the HIP path yet");
    }
    if (row.activation != AGX_ACT_WEIGHTED_QUAD && (row.kind == AGX_RES_CONTROL_GRAV || row.kind == AGX_RES_FRAME_VELOCITY))
      return fail("agx_ocp_create: ActivationModelExp / QuadExp are not implemented for ControlGrav / FrameVelocity residuals");
    if (row.activation != AGX_ACT_WEIGHTED_QUAD && !(row.alpha > 0.0)) return fail("agx_ocp_create: activation alpha must be positive");
    if ((row.kind == AGX_RES_FRAME_PLACEMENT || row.kind == AGX_RES_FRAME_TRANSLATION || row.kind == AGX_RES_FRAME_ROTATION) &&
        (row.frame < 0 || row.frame >= m->h.nframes))
      return fail("agx_ocp_create: frame id out of range");
    if (row.kind == AGX_RES_COLLISION) {
      if (row.frame < 0 || row.frame >= m->h.nframes || row.frame_b < 0 || row.frame_b >= m->h.nframes)
        return fail("agx_ocp_create: collision pair refers to a geometry frame out of range");
      if (!agx::frame_has_geometry(m->h, row.frame) || !agx::frame_has_geometry(m->h, row.frame_b))
        return fail("agx_ocp_create: collision pair refers to a frame without geometry (radius 0, no box)");
      if (agx::frame_is_box(m->h, row.frame) && agx::frame_is_box(m->h, row.frame_b))
        return fail("agx_ocp_create: box / box collision pairs are not supported");
    }
  }
  agx_ocp *o = new agx_ocp();
  o->device = device;
  // every failure from here on leaves through agx_ocp_destroy (`bail` with a message, or after a callee has set one)
  auto bail = [o](const std::string &msg) {
    agx_ocp_destroy(o);
    return fail(msg);
  };
  o->hm = m->h;
  o->nv = m->h.nv; o->nx = 2 * o->nv; o->nu = o->nv;
  o->chain = m->h.is_chain != 0;
  if (const char *e = getenv("AGX_K1_LANES")) o->k1_lanes = (e[0] != '0');
  if (const char *e = getenv("AGX_SPECULATE_GAINS")) o->speculate = (e[0] != '0');
  if (const char *e = getenv("AGX_GAINS_MFMA")) o->gains_mfma = (e[0] != '0');
  if (const char *e = getenv("AGX_RICCATI_MX")) o->riccati_mx = (e[0] != '0');
  if (const char *e = getenv("AGX_NO_EMPTY_LAUNCHES")) o->no_empty = (e[0] != '0');
  o->fold_publish = batch <= 204;
  if (const char *e = getenv("AGX_FOLD_PUBLISH")) o->fold_publish = (e[0] != '0');
  if (const char *e = getenv("AGX_ADMM_LOOP")) { o->admm_loop = (e[0] != '0'); o->admm_loop_always = (e[0] == '2'); }
  if (const char *e = getenv("AGX_K1_FUSED")) o->k1_fused = (e[0] != '0');
  if (const char *e = getenv("AGX_NODE_KKT_WIDE")) o->node_kkt_wide = (e[0] != '0');
  if (const char *e = getenv("AGX_TILE_CARRY")) o->tile_carry = (e[0] != '0');
  o->T = d->horizon; o->B = batch;
  {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) o->n_cu = n;
  }
  o->tile = AGX_TILE_DOUBLES(o->nv);
  const int ld = o->nv <= 8 ? 8 : 32;
  o->qt_size = 6 * o->nv * ld + 5 * ld + 8;  // QT<NV>::SIZE
  o->aux_size = 4 * o->nv * ld + 3 * ld;     // AUX<NV>::SIZE
  o->stride = agx_ref_stride(d, o->nv);
  o->dt.assign(d->dt, d->dt + d->horizon);
  std::memset(&o->ho, 0, sizeof(o->ho));
  o->ho.T = o->T; o->ho.B = o->B; o->ho.stride = o->stride;
  o->cost_wide = cost_wide;
  o->n_rows_all[0] = d->n_running_rows; o->n_rows_all[1] = d->n_terminal_rows;
  // wide cost sets: the row table holds the prefix, the pair table the trailing collision rows
  fill_rows(d->running_rows, cost_wide ? csplit[0].n_prefix : d->n_running_rows, o->nv, m->nvu, o->ho.rows[0]);
  fill_rows(d->terminal_rows, cost_wide ? csplit[1].n_prefix : d->n_terminal_rows, o->nv, m->nvu, o->ho.rows[1]);
  if (cost_wide) {
    fill_cost_pairs(d->running_rows, d->n_running_rows, csplit[0], o->nv, o->hw.lay[0]);
    fill_cost_pairs(d->terminal_rows, d->n_terminal_rows, csplit[1], o->nv, o->hw.lay[1]);
  }
  o->ho.tol = d->termination_tolerance;
  o->ho.mu_dyn = d->mu_dynamic;
  o->ho.mu_con = d->mu_constraint;
  o->nvu = m->nvu;
  o->padded = o->nvu != o->nv;
  o->stride_u = agx_ref_stride(d, o->nvu);
  if (o->padded) {
    // reference-tile maps: row r of a layout sits at off_u[r] in the caller's tile, at off[r] in the internal one; the joint
    // blocks of State / Control references and activation weights grow from nvu to nv entries (pad weights 1: the pad
    // residuals are identically zero, the weight only keeps the pad block of the Hessians well conditioned)
    for (int lay = 0; lay < 2; ++lay) {
      const agx_cost_row *rows = lay ? d->terminal_rows : d->running_rows;  // every row of the table, the pairs of a wide set included
      o->refmap[lay].assign(o->stride, -1);
      o->reffill[lay].assign(o->stride, 0.0);
      int off_u = 0, off = 0;
      for (int r = 0; r < o->n_rows_all[lay]; ++r) {
        const int kind = rows[r].kind, nref_u = agx_row_nref(kind, o->nvu), nr_u = agx_row_nr(kind, o->nvu);
        const int nref = agx_row_nref(kind, o->nv), nr = agx_row_nr(kind, o->nv);
        o->refmap[lay][off] = off_u;
        for (int k = 0; k < nref; ++k) {
          const int ku = user_component(kind, k, o->nv, o->nvu, true);
          o->refmap[lay][off + 1 + k] = ku >= 0 ? off_u + 1 + ku : -1;
        }
        for (int k = 0; k < nr; ++k) {
          const int ku = user_component(kind, k, o->nv, o->nvu, false);
          o->refmap[lay][off + 1 + nref + k] = ku >= 0 ? off_u + 1 + nref_u + ku : -1;
          if (ku < 0) o->reffill[lay][off + 1 + nref + k] = 1.0;
        }
        off_u += 1 + nref_u + nr_u;
        off += 1 + nref + nr;
      }
    }
  }
  {
    // Sets within the fixed limits keep the fixed layout; a set over them whose rows are collision pairs (at most AGX_MAX_PAIRS) with
    // at most one State and one Control row takes the wide layout on serial chains of the 7-joint capacity; AGX_CON_WIDE=1 gives
    // every such set the wide layout.  Everything else is refused by fill_cons.
    const int wc_r = wide_class(d->running_constraints, d->n_running_constraints, false),
              wc_t = wide_class(d->terminal_constraints, d->n_terminal_constraints, true);
    const bool wide_model = o->nv <= 7 && o->chain, wide_ok = wide_model && wc_r == 0 && wc_t == 0;
    bool wide = false;
    if (const char *e = getenv("AGX_CON_WIDE")) wide = wide_ok && e[0] == '1';
    if (!wide && (fill_cons(d->running_constraints, d->n_running_constraints, o->nv, o->nvu, m->h, o->ho.cons[0], false) ||
                  fill_cons(d->terminal_constraints, d->n_terminal_constraints, o->nv, o->nvu, m->h, o->ho.cons[1], true))) {
      if (wide_model && (wc_r == 2 || wc_t == 2)) return bail("agx_ocp_create: at most " + std::to_string(AGX_MAX_PAIRS) + " collision-pair constraints per node type");
      if (!wide_ok) { agx_ocp_destroy(o); return -1; }
      wide = true;
    }
    if (wide) {
      if (fill_cons_wide(d->running_constraints, d->n_running_constraints, o->nv, o->nvu, m->h, o->ho.cons[0], false) ||
          fill_cons_wide(d->terminal_constraints, d->n_terminal_constraints, o->nv, o->nvu, m->h, o->ho.cons[1], true)) { agx_ocp_destroy(o); return -1; }
      const int cs = std::max(1, std::max(o->ho.cons[0].nc, o->ho.cons[1].nc)), js = std::max(1, std::max(o->ho.cons[0].npairs, o->ho.cons[1].npairs));
      for (int lay = 0; lay < 2; ++lay) { o->ho.cons[lay].cstride = cs; o->ho.cons[lay].jstride = js; }
      o->con_wide = o->ho.cons[0].nc + o->ho.cons[1].nc > 0;
      if (o->con_wide) o->con_cs = cs;
    }
  }
  for (int lay = 0; lay < 2; ++lay)
    for (int r = 0; r < o->ho.cons[lay].n; ++r) {
      const int k = o->ho.cons[lay].kind[r];
      if (k != AGX_RES_CONTROL && k != AGX_RES_STATE && k != AGX_RES_COLLISION) o->con_lanes = false;
    }
  if (const char *e = getenv("AGX_CON_LANES")) o->con_lanes = o->con_lanes && (e[0] != '0');
  o->has_con = o->ho.cons[0].nc + o->ho.cons[1].nc > 0;
  o->general = o->ho.rows[0].general || o->ho.rows[1].general;
  o->ho.has_con = o->has_con ? 1 : 0;
  o->ho.max_qp = d->max_qp_iters > 0 ? d->max_qp_iters : 1000;
  o->ho.eps_abs = d->eps_abs;
  o->ho.eps_rel = d->eps_rel;
  o->ho.use_filter = d->use_filter_line_search ? 1 : 0;
  // (the filter test lives in k_sqp_accept, which serves every model size and every kind of cost row)
  if (!kGeneralRowsWg && o->general && o->nv > 7)
    return bail("agx_ocp_create: this build has the ControlGrav / FrameVelocity kernels of models above 7 joints compiled out (AGX_NO_GENERAL_ROWS)");
  if (o->has_con && o->nv > 7) {  // large models: ConstraintModelControlLimit only (agx_big.hpp)
    for (int lay = 0; lay < 2; ++lay)
      for (int r = 0; r < o->ho.cons[lay].n; ++r)
        if (o->ho.cons[lay].kind[r] == AGX_RES_FRAME_VELOCITY || o->ho.cons[lay].kind[r] == AGX_RES_CONTROL_GRAV)
          return bail("agx_ocp_create: FrameVelocity / ControlGrav constraints are implemented for models of at most 7 joints (after padding)");
    // general cost rows next to constraints: k_admm_update_big does not carry the blocks Lqv | Lvvd | Lqu
    for (int lay = 0; lay < 2; ++lay)
      for (int r = 0; r < o->ho.rows[lay].n; ++r)
        if (o->ho.rows[lay].active[r] && (o->ho.rows[lay].kind[r] == AGX_RES_CONTROL_GRAV || o->ho.rows[lay].kind[r] == AGX_RES_FRAME_VELOCITY))
          return bail(std::string("agx_ocp_create: a ") + (o->ho.rows[lay].kind[r] == AGX_RES_CONTROL_GRAV ? "ControlGrav" : "FrameVelocity") +
                      " cost row together with constraints is implemented for models of at most 7 joints (after padding)");
  }
  {
    auto n_frame_rows = [](const DevRows &r) {
      int n = 0;
      for (int i = 0; i < r.n; ++i)
        n += (r.kind[i] == AGX_RES_FRAME_PLACEMENT || r.kind[i] == AGX_RES_FRAME_TRANSLATION || r.kind[i] == AGX_RES_FRAME_ROTATION);
      return n;
    };
    auto n_collision_rows = [](const DevRows &r) {
      int n = 0;
      for (int i = 0; i < r.n; ++i) n += (r.kind[i] == AGX_RES_COLLISION);
      return n;
    };
    // Exp / QuadExp activations on vector residuals (ocp_croco_generic.py:118-131) are evaluated by the one-lane-per-node kernel
    auto n_vector_exp_rows = [&]() {
      int n = 0;
      for (int lay = 0; lay < 2; ++lay)
        for (int i = 0; i < o->ho.rows[lay].n; ++i)
          if (o->ho.rows[lay].active[i] && o->ho.rows[lay].act[i] != AGX_ACT_WEIGHTED_QUAD && o->ho.rows[lay].kind[i] != AGX_RES_COLLISION) ++n;
      return n;
    };
    // at most one collision cost row per node type, capsule / sphere / box pair, serial chain: the COLL variant
    o->lanes_coll = n_collision_rows(o->ho.rows[0]) + n_collision_rows(o->ho.rows[1]) > 0;
    // (a wide cost set: K1 stages the prefix of the tile only, the pairs are k_cost_pairs' business)
    const int k1_stride = cost_wide ? std::max(1, std::max(o->hw.lay[0].prefix, o->hw.lay[1].prefix)) : o->stride;
    o->lanes_ok = k1_stride <= agx::kLjRef && n_frame_rows(o->ho.rows[0]) <= 2 && n_frame_rows(o->ho.rows[1]) <= 2 &&
                  n_collision_rows(o->ho.rows[0]) <= 1 && n_collision_rows(o->ho.rows[1]) <= 1 && !o->general && !n_vector_exp_rows();
  }
  int wg_k1_stride = 0;  // large models with general rows: the tile doubles K1 stages
  if (o->nv > 8) {
    // the workgroup-per-node kernels stage the reference tile and the dense residual rows of a node in LDS
    auto n_dense = [](const DevRows &r) {
      int n = 0;
      for (int i = 0; i < r.n; ++i)
        if (r.active[i])
          n += r.kind[i] == AGX_RES_FRAME_PLACEMENT ? 6 : ((r.kind[i] == AGX_RES_FRAME_TRANSLATION || r.kind[i] == AGX_RES_FRAME_ROTATION) ? 3 : (r.kind[i] == AGX_RES_COLLISION ? 1 : 0));
      return n;
    };
    // A handle with general rows: K1 stages the tile up to the end of its last row that is not a general row (it skips the two
    // kinds), k_general_rows_wg from the first general row on (agx_general_rows.hpp: general_ref_lo); the limit applies to the
    // caller's tile and to either piece.  A padded 31-joint model keeps the five-row set of a torque-controlled arm that way.
    // (wg_costs of K1 still forms the tile pointer of every active row and loads its item weight before it looks at the kind:
    // for a general row that is a load from LDS K1 has not staged -- at most 258 doubles into WgNode's ref | J region, inside
    // the structure -- whose value is never used.  K1 uses nothing of a general row's tile; it does touch that one address.)
    int gen_lo = o->stride;
    if (o->general) {
      wg_k1_stride = 1;
      for (int lay = 0; lay < 2; ++lay)
        for (int r = 0; r < o->ho.rows[lay].n; ++r) {
          const DevRows &R = o->ho.rows[lay];
          if (R.kind[r] == AGX_RES_CONTROL_GRAV || R.kind[r] == AGX_RES_FRAME_VELOCITY) gen_lo = std::min(gen_lo, R.off[r]);
          else wg_k1_stride = std::max(wg_k1_stride, R.off[r] + 1 + R.nref[r] + R.nr[r]);
        }
    }
    const int widest = o->general ? std::max(o->stride_u, std::max(wg_k1_stride, o->stride - gen_lo)) : o->stride;
    if (widest > agx::kWgRef) return bail("agx_ocp_create: reference tile of " + std::to_string(widest) + " doubles per node exceeds the large-model limit of " + std::to_string(agx::kWgRef));
    if (n_dense(o->ho.rows[0]) > agx::kWgJ || n_dense(o->ho.rows[1]) > agx::kWgJ) return bail("agx_ocp_create: more than 16 frame / collision residual components per node (large models)");
  }
  // two-level sweep for small batches of unconstrained problems on the MFMA-layout kernel.  Only with Gauss-Newton Hessians of
  // quadratic activations: then Hww = M (Luu + preg) M is positive definite at every node and no sweep -- neither the ordinary one
  // nor a segment's zero-terminal one, whose pivots are the smaller ones -- can meet a non-positive pivot.  An Exp / QuadExp cost
  // row has negative curvature inside its bell: such problems keep the one-wave sweep and its breakdown handling.
  bool convex_rows = true;
  for (int lay = 0; lay < 2; ++lay) {
    for (int r = 0; r < o->ho.rows[lay].n; ++r)
      if (o->ho.rows[lay].active[r] && o->ho.rows[lay].act[r] != AGX_ACT_WEIGHTED_QUAD) convex_rows = false;
    for (int p = 0; p < o->hw.lay[lay].n; ++p)  // (wide cost sets: the pairs)
      if (o->hw.lay[lay].active[p] && o->hw.lay[lay].act[p] != AGX_ACT_WEIGHTED_QUAD) convex_rows = false;
  }
  if (o->nv <= 7 && o->riccati_mx && !o->has_con && convex_rows) {
    // ten segments while the two sweeps of a paired launch (2 B S waves of 254 VGPRs) fit the 2 048 wave slots of the chip
    // at two per SIMD; fewer above that; below five segments the 2.4 x arithmetic is not paid back (measured, B = 256: none)
    int S = std::min(10, 1024 / o->B);
    if (S < 5) S = 0;
    if (const char *e = getenv("AGX_MX2_SEGMENTS")) S = atoi(e);
    if (S > agx::kMx2MaxSeg) S = agx::kMx2MaxSeg;
    while (S >= 2 && o->T / S < 4) --S;  // segments of at least four nodes
    o->mx2_S = S >= 2 ? S : 0;
  }
  {
    bool one_dt = true;  // nodes with dt_i != dt_0 are re-integrated by the warm-start shift: not the old node's inputs
    for (int t = 0; t < o->T; ++t) one_dt = one_dt && o->dt[t] == o->dt[0];
    o->carry_static = o->tile_carry && o->nv <= 7 && o->chain && o->k1_lanes && o->lanes_ok && o->riccati_mx && !o->has_con && !o->general && one_dt &&
                      !o->cost_wide;  // (a wide cost set does not carry tiles: k_cost_pairs adds to the tiles of the pass in front of it)
  }
  // probe that a kernel instantiation exists
  if (dispatch(o->nv, o->chain, [](auto, auto) -> int { return 0; }) || set_device(o)) { agx_ocp_destroy(o); return -1; }
  const size_t B = o->B, T = o->T, nx = o->nx, nu = o->nu;
  // every buffer the handle has from the start, zero-filled; the first allocation that fails ends the list
  hipError_t bad = hipSuccess;
  auto alloc = [&](auto **field, size_t count) { if (bad == hipSuccess) bad = o->own.device(field, count, true); };
  alloc(&o->d_model, 1);
  alloc(&o->d_ocp, (o->cost_wide || wg_k1_stride) ? 2 : 1);  // wide cost sets, general rows of large models: [1] the copy K1 reads
  if (o->cost_wide) alloc(&o->d_cw, 1);
  alloc(&o->d_dt, T);
  alloc(&o->d_xs, 2 * B * (T + 1) * nx);  // second half: shift staging
  alloc(&o->d_us, 2 * B * T * nu);
  alloc(&o->d_x0, B * nx);
  alloc(&o->d_Kws, B * T * nu * nx);
  alloc(&o->d_kws, B * T * nu);
  alloc(&o->d_Kout, B * T * nu * nx);
  alloc(&o->d_dx, B * (T + 1) * nx);
  alloc(&o->d_du, B * T * nu);
  alloc(&o->d_w, B * T * nu);
  alloc(&o->d_nodestat, B * (T + 1) * 4);
  alloc(&o->d_qt, B * (T + 1) * (size_t)o->qt_size);
  alloc(&o->d_aux, B * (T + 1) * (size_t)o->aux_size);
  alloc(&o->d_ref, B * (T + 1) * (size_t)o->stride);
  alloc(&o->d_frames, B * (T + 1) * AGX_MAX_ROWS);
  alloc(&o->d_state, B);
  alloc(&o->d_ndone, 8);  // [0] finished instances, [1] instances whose ADMM loop has ended, [2] instances in the split line search
  if (o->nv > 8) {
    for (int t = 0; t < o->T; ++t)
      if (o->dt[t] != o->dt[0]) o->shift_nodes.push_back(t);
    if (!o->shift_nodes.empty()) alloc(&o->d_shift_nodes, o->shift_nodes.size());
  }
  if (o->general) alloc(&o->d_auxg, B * (T + 1) * (size_t)(3 * o->nv * ld));  // 3 A::B2 of the capacity
  if (o->has_con) {
    alloc(&o->d_qt2, B * (T + 1) * (size_t)o->qt_size);
    const size_t cs = (size_t)o->con_cs;  // AGX_MAX_NC, wide sets: their own stride
    alloc(&o->d_cg, B * (T + 1) * cs);
    if (o->con_wide) alloc(&o->d_cjac, B * (T + 1) * (size_t)o->ho.cons[0].jstride * 8);  // distance gradients, d/dq only
    else alloc(&o->d_cjac, B * (T + 1) * AGX_MAX_DENSE * 32);  // 24 per row up to 7 joints (q | v | u, 8 each), 32 above (q only)
    alloc(&o->d_y, B * (T + 1) * cs);
    alloc(&o->d_z, B * (T + 1) * cs);
    alloc(&o->d_cx, B * (T + 1) * nx);
    alloc(&o->d_admmstat, B * (T + 1) * 4);
    alloc(&o->d_fac, B * T * 192);
    alloc(&o->d_segP, B * agx::kSeg * 256);
    if (const char *e = getenv("AGX_ADMM_SEGMENTS")) o->admm_segments = (e[0] != '0');
    if (const char *e = getenv("AGX_ADMM_PREFACTOR")) o->admm_prefactor = (e[0] != '0');
  }
  if (bad != hipSuccess) return bail(std::string("agx_ocp_create: hipMalloc: ") + hipGetErrorString(bad));
  o->d_ocp_k1 = o->d_ocp;
  if (o->d_shift_nodes) (void)hipMemcpy(o->d_shift_nodes, o->shift_nodes.data(), sizeof(int) * o->shift_nodes.size(), hipMemcpyHostToDevice);
  if (pinned_polled(o, &o->h_ndone, 16 * sizeof(unsigned long long))) return bail("hipHostMalloc failed");
  std::memset(o->h_ndone, 0xff, 16 * sizeof(unsigned long long));
  if (o->poll && hipHostGetDevicePointer((void **)&o->h_ndone_dev, o->h_ndone, 0) != hipSuccess) o->poll = false;
  if (const char *e = getenv("AGX_HOST_POLL")) o->poll = o->poll && (e[0] != '0');
  if (hipMemcpy(o->d_model, &o->hm, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(o->d_ocp, &o->ho, sizeof(DevOcp), hipMemcpyHostToDevice) != hipSuccess ||
      (o->cost_wide && hipMemcpy(o->d_cw, &o->hw, sizeof(DevCostWide), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(o->d_dt, o->dt.data(), sizeof(double) * T, hipMemcpyHostToDevice) != hipSuccess)
    return bail("agx_ocp_create: upload of the problem description failed");
  if (o->cost_wide || wg_k1_stride) {
    DevOcp k1 = o->ho;
    k1.stride = wg_k1_stride ? wg_k1_stride : std::max(1, std::max(o->hw.lay[0].prefix, o->hw.lay[1].prefix));
    o->d_ocp_k1 = o->d_ocp + 1;
    if (hipMemcpy(o->d_ocp_k1, &k1, sizeof(DevOcp), hipMemcpyHostToDevice) != hipSuccess) return bail("agx_ocp_create: upload of the problem description failed");
  }
  if (hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking) != hipSuccess) return bail("hipStreamCreate failed");
  o->own_stream = true;
  (void)o->own.event(&o->ev0);
  (void)o->own.event(&o->ev1);
  (void)o->own.event(&o->ev_done, hipEventDisableTiming);
  rv_own_tile(o, nullptr);
  if (reset_state(o) || hipStreamSynchronize(o->stream) != hipSuccess) return bail("agx_ocp_create: state reset failed");
  *out = o;
  return 0;
}

void agx_ocp_destroy(agx_ocp *o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  if (o->stream) (void)hipStreamSynchronize(o->stream);
  if (o->copy_stream) { (void)hipStreamSynchronize(o->copy_stream); (void)hipStreamDestroy(o->copy_stream); }
  if (o->own_stream && o->stream) (void)hipStreamDestroy(o->stream);
  delete o;  // (the owner frees what the handle still holds)
}

int agx_ocp_set_stream(agx_ocp *o, void *hip_stream) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (o->stream) HIPCHK(hipStreamSynchronize(o->stream));
  if (hip_stream) {
    if (o->own_stream && o->stream) (void)hipStreamDestroy(o->stream);
    o->stream = (hipStream_t)hip_stream;
    o->own_stream = false;
  } else if (!o->own_stream) {
    HIPCHK(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
    o->own_stream = true;
  }
  return 0;
}

int agx_ocp_sync(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_set_quorum(agx_ocp *o, double sqp_fraction, double qp_fraction) {
  if (!o) return fail("null handle");
  if (!(sqp_fraction > 0.0 && sqp_fraction <= 1.0) || !(qp_fraction > 0.0 && qp_fraction <= 1.0))
    return fail("agx_ocp_set_quorum: fractions must be in (0, 1]");
  o->quorum_sqp = sqp_fraction;
  o->quorum_qp = qp_fraction;
  return 0;
}

int agx_ocp_reset_duals(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  o->first_fresh = false;  // (the state changes)
  if (o->has_con) HIPCHK(hipMemsetAsync(o->d_y, 0, sizeof(double) * (size_t)o->B * (o->T + 1) * o->con_cs, o->stream));
  hipLaunchKernelGGL(agx::k_reset_rho, dim3((o->B + 255) / 256), dim3(256), 0, o->stream, o->d_state, o->B);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_set_geom_placement(agx_ocp *o, int frame, const double *se3) {
  if (!o || !se3) return fail("agx_ocp_set_geom_placement: null argument");
  if (frame < 0 || frame >= o->hm.nframes) return fail("agx_ocp_set_geom_placement: frame out of range");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  std::memcpy(o->hm.frame_placement[frame], se3, sizeof(double) * 12);
  // in-stream update of the one placement inside the resident model
  HIPCHK(hipMemcpyAsync((char *)o->d_model + offsetof(DevModel, frame_placement) + sizeof(double) * 12 * frame, o->hm.frame_placement[frame],
                        sizeof(double) * 12, hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_general_rows(agx_ocp *o) {
  if (!o) return fail("null handle");
  return o->general ? 1 : 0;
}

int agx_ocp_cost_wide(agx_ocp *o) {
  if (!o) return fail("null handle");
  return o->cost_wide ? 1 : 0;
}

int agx_ocp_set_refs(agx_ocp *o, const double *ref_tile, const int32_t *frame_ids) {
  if (!o || !ref_tile) return fail("agx_ocp_set_refs: null argument");
  if (frame_ids && o->cost_wide) return fail("agx_ocp_set_refs: a wide cost set takes no frame-id table (rows from AGX_MAX_ROWS on have no column in it)");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  if (frame_ids) o->frames_uniform = false;
  if (o->refs_pending) { HIPCHK(hipEventSynchronize(o->ev_refs)); o->refs_pending = false; }  // superseded
  const size_t n = (size_t)o->B * (o->T + 1);
  if (o->padded) {  // the caller's tile is laid out for nvu joints
    o->stage.resize(n * o->stride);
    pad_ref_tile(o, o->stage.data(), ref_tile, o->B, o->T);
    ref_tile = o->stage.data();
  }
  HIPCHK(hipMemcpyAsync(o->d_ref, ref_tile, sizeof(double) * n * o->stride, hipMemcpyHostToDevice, o->stream));
  if (frame_ids) HIPCHK(hipMemcpyAsync(o->d_frames, frame_ids, sizeof(int) * n * AGX_MAX_ROWS, hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));  // the caller may reuse its buffers
  rv_own_tile(o, frame_ids ? o->d_frames : nullptr);
  return 0;
}

int agx_ocp_set_refs_device(agx_ocp *o, const double *d_ref_tile, const int32_t *d_frame_ids, int adopt) {
  if (!o || !d_ref_tile) return fail("agx_ocp_set_refs_device: null argument");
  if (d_frame_ids && o->cost_wide) return fail("agx_ocp_set_refs_device: a wide cost set takes no frame-id table (rows from AGX_MAX_ROWS on have no column in it)");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  if (d_frame_ids) o->frames_uniform = false;
  const size_t n = (size_t)o->B * (o->T + 1);
  if (o->padded) {  // a device tile in the caller's layout: through the host (padded models are not the fast path)
    std::vector<double> tmp(n * o->stride_u);
    HIPCHK(hipMemcpyAsync(tmp.data(), d_ref_tile, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    o->stage.resize(n * o->stride);
    pad_ref_tile(o, o->stage.data(), tmp.data(), o->B, o->T);
    HIPCHK(hipMemcpyAsync(o->d_ref, o->stage.data(), sizeof(double) * n * o->stride, hipMemcpyHostToDevice, o->stream));
    if (d_frame_ids) HIPCHK(hipMemcpyAsync(o->d_frames, d_frame_ids, sizeof(int) * n * AGX_MAX_ROWS, hipMemcpyDeviceToDevice, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    rv_own_tile(o, d_frame_ids ? o->d_frames : nullptr);
  } else if (adopt) {  // the caller's memory, in the layout of the handle's own tile: the owner never sees it
    rv_own_tile(o, d_frame_ids);
    o->rv.base = d_ref_tile;
  } else {
    HIPCHK(hipMemcpyAsync(o->d_ref, d_ref_tile, sizeof(double) * n * o->stride, hipMemcpyDeviceToDevice, o->stream));
    if (d_frame_ids) HIPCHK(hipMemcpyAsync(o->d_frames, d_frame_ids, sizeof(int) * n * AGX_MAX_ROWS, hipMemcpyDeviceToDevice, o->stream));
    rv_own_tile(o, d_frame_ids ? o->d_frames : nullptr);
  }
  return 0;
}

int agx_host_alloc(size_t bytes, void **out) {
  if (!out || bytes == 0) return fail("agx_host_alloc: bad argument");
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return 0;
}
int agx_host_free(void *p) {
  if (p) HIPCHK(hipHostFree(p));
  return 0;
}

int agx_ocp_set_refs_async(agx_ocp *o, const double *ref_tile, const int32_t *frame_ids) {
  if (!o || !ref_tile) return fail("agx_ocp_set_refs_async: null argument");
  if (frame_ids && o->cost_wide) return fail("agx_ocp_set_refs_async: a wide cost set takes no frame-id table (rows from AGX_MAX_ROWS on have no column in it)");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  if (ensure_copy_stream(o)) return -1;
  const size_t n = (size_t)o->B * (o->T + 1);
  if (!o->d_ref_back) HIPCHK(o->own.device(&o->d_ref_back, n * o->stride));
  if (frame_ids && !o->d_frames_back) HIPCHK(o->own.device(&o->d_frames_back, n * AGX_MAX_ROWS));
  if (o->refs_pending) HIPCHK(hipEventSynchronize(o->ev_refs));  // a second upload before any solve: replaces the first
  // the back tile is free: the solve that read it has returned (solves are synchronous to the host)
  if (o->padded) {  // repacked through the handle's staging vector: the copy has to finish before this call returns
    o->stage.resize(n * o->stride);
    pad_ref_tile(o, o->stage.data(), ref_tile, o->B, o->T);
    ref_tile = o->stage.data();
  }
  HIPCHK(hipMemcpyAsync(o->d_ref_back, ref_tile, sizeof(double) * n * o->stride, hipMemcpyHostToDevice, o->copy_stream));
  if (frame_ids) HIPCHK(hipMemcpyAsync(o->d_frames_back, frame_ids, sizeof(int) * n * AGX_MAX_ROWS, hipMemcpyHostToDevice, o->copy_stream));
  HIPCHK(hipEventRecord(o->ev_refs, o->copy_stream));
  if (o->padded) HIPCHK(hipStreamSynchronize(o->copy_stream));
  o->refs_pending = true;
  o->refs_pending_frames = frame_ids != nullptr;
  return 0;
}
int agx_ocp_refs_wait(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (o->refs_pending) HIPCHK(hipEventSynchronize(o->ev_refs));
  return 0;
}
int agx_ocp_refs_activate(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (!o->refs_pending) return fail("agx_ocp_refs_activate: no staged reference tile (agx_ocp_set_refs_async)");
  if (set_device(o)) return -1;
  return adopt_pending_refs(o);
}

int agx_ocp_download_async(agx_ocp *o, double *xs, double *us, double *K) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (ensure_copy_stream(o)) return -1;
  const size_t B = o->B, T = o->T, nx = o->nx, nu = o->nu;
  if (o->padded) {  // repacked on the host: the synchronous route
    if (xs && down(o, xs, o->d_xs, B * (T + 1), 2)) return -1;
    if (us && down(o, us, o->d_us, B * T, 1)) return -1;
    if (K && down_gains(o, K, o->d_Kout, B * T)) return -1;
    HIPCHK(hipStreamSynchronize(o->stream));
    return 0;
  }
  const size_t n_xs = B * (T + 1) * nx, n_us = B * T * nu, n_K = B * T * nu * nx;
  if (!o->d_snap) HIPCHK(o->own.device(&o->d_snap, n_xs + n_us + n_K));
  if (o->dl_pending) HIPCHK(hipEventSynchronize(o->ev_dl));  // the previous download still reads the snapshot
  // snapshot in the solver's stream (device to device, ~0.1 ms for 100 MB), then the copy engine drains it while the
  // solver goes on with the next step
  if (xs) HIPCHK(hipMemcpyAsync(o->d_snap, o->d_xs, sizeof(double) * n_xs, hipMemcpyDeviceToDevice, o->stream));
  if (us) HIPCHK(hipMemcpyAsync(o->d_snap + n_xs, o->d_us, sizeof(double) * n_us, hipMemcpyDeviceToDevice, o->stream));
  if (K) HIPCHK(hipMemcpyAsync(o->d_snap + n_xs + n_us, o->d_Kout, sizeof(double) * n_K, hipMemcpyDeviceToDevice, o->stream));
  HIPCHK(hipEventRecord(o->ev_snap, o->stream));
  HIPCHK(hipStreamWaitEvent(o->copy_stream, o->ev_snap, 0));
  if (xs && us && K && us == xs + n_xs && K == us + n_us) {  // one contiguous destination (xs | us | K): one transfer
    HIPCHK(hipMemcpyAsync(xs, o->d_snap, sizeof(double) * (n_xs + n_us + n_K), hipMemcpyDeviceToHost, o->copy_stream));
  } else {
    if (xs) HIPCHK(hipMemcpyAsync(xs, o->d_snap, sizeof(double) * n_xs, hipMemcpyDeviceToHost, o->copy_stream));
    if (us) HIPCHK(hipMemcpyAsync(us, o->d_snap + n_xs, sizeof(double) * n_us, hipMemcpyDeviceToHost, o->copy_stream));
    if (K) HIPCHK(hipMemcpyAsync(K, o->d_snap + n_xs + n_us, sizeof(double) * n_K, hipMemcpyDeviceToHost, o->copy_stream));
  }
  HIPCHK(hipEventRecord(o->ev_dl, o->copy_stream));
  o->dl_pending = true;
  return 0;
}
int agx_ocp_download_wait(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (o->dl_pending) HIPCHK(hipEventSynchronize(o->ev_dl));
  o->dl_pending = false;
  return 0;
}

int agx_ocp_upload_x0(agx_ocp *o, const double *x0) {
  if (!o || !x0) return fail("agx_ocp_upload_x0: null argument");
  if (set_device(o)) return -1;
  if (up(o, o->d_x0, x0, o->B, 2)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_upload_warmstart(agx_ocp *o, const double *xs_ws, const double *us_ws) {
  if (!o || !xs_ws || !us_ws) return fail("agx_ocp_upload_warmstart: null argument");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  if (up(o, o->d_xs, xs_ws, (size_t)o->B * (o->T + 1), 2)) return -1;
  if (up(o, o->d_us, us_ws, (size_t)o->B * o->T, 1)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_solve_resident(agx_ocp *o, int max_iter, double max_time) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  return solve_resident(o, max_iter, max_time);
}

int agx_ocp_download(agx_ocp *o, double *xs, double *us, double *K, agx_status *st) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  const size_t B = o->B, T = o->T, nx = o->nx, nu = o->nu;
  (void)nx; (void)nu;
  if (xs && down(o, xs, o->d_xs, B * (T + 1), 2)) return -1;
  if (us && down(o, us, o->d_us, B * T, 1)) return -1;
  if (K && down_gains(o, K, o->d_Kout, B * T)) return -1;
  std::vector<DevState> hs;
  if (st) {
    hs.resize(B);
    HIPCHK(hipMemcpyAsync(hs.data(), o->d_state, sizeof(DevState) * B, hipMemcpyDeviceToHost, o->stream));
  }
  HIPCHK(hipStreamSynchronize(o->stream));
  if (st)
    for (size_t b = 0; b < B; ++b) {
      st[b].kkt = hs[b].kkt; st[b].cost = hs[b].cost; st[b].merit = hs[b].merit; st[b].gap_norm = hs[b].gap;
      st[b].iter = hs[b].done ? hs[b].iter : o->last_max_iter;
      st[b].qp_iters = hs[b].qp_iters; st[b].solved = hs[b].solved; st[b].flags = hs[b].flags;
    }
  return 0;
}

// What a controller consumes per cycle, packed on the device and copied with ONE transfer into a
// pinned host buffer owned by the handle: per instance
//   [ us0 (nu) | K0 (nu x ndx, row major) | x1 (nx) | kkt cost merit gap iter qp_iters solved flags ].
int agx_ocp_first_packed(agx_ocp *o, const double **host, int *stride) {
  if (!o || !host) return fail("agx_ocp_first_packed: null argument");
  if (set_device(o)) return -1;
  const int FS = o->nu + o->nu * o->nx + o->nx + 8;
  if (!o->h_first) {
    if (pinned_polled(o, &o->h_first, sizeof(double) * (size_t)o->B * FS)) return -1;
    if (o->poll) HIPCHK(hipHostGetDevicePointer((void **)&o->d_first, o->h_first, 0));  // the pack kernel writes host memory directly: a view, not registered
    else HIPCHK(o->own.device(&o->d_first, (size_t)o->B * FS));
    o->first_stride = FS;
  }
  const long long n = (long long)o->B * FS;
  if (o->first_fresh && first_block(o)) {
    // every instance packed its record where it converged (k_sqp_head), and the host has seen the stamp behind those stores
    o->first_served[0] += 1;
  } else {
    o->first_served[1] += 1;
    hipLaunchKernelGGL(agx::k_pack_first, dim3((int)((n + 255) / 256)), dim3(256), 0, o->stream, o->d_us, o->d_Kout, o->d_xs, o->d_state,
                       o->d_first, o->B, o->T, o->nx, o->nu, o->last_max_iter);
    HIPCHK(hipGetLastError());
    if (o->poll) {
      const unsigned long long seq = ++o->seq;
      if (publish(o, 3, 2, o->d_ndone, seq)) return -1;
      if (wait_stamp(o, 2, seq)) return -1;
    } else {
      HIPCHK(hipMemcpyAsync(o->h_first, o->d_first, sizeof(double) * n, hipMemcpyDeviceToHost, o->stream));
      HIPCHK(hipStreamSynchronize(o->stream));
    }
  }
  if (o->padded) {  // [us0 | K0 | x1 | status] of the caller's nvu joints
    const int nv = o->nv, nvu = o->nvu, FSu = nvu + nvu * 2 * nvu + 2 * nvu + 8;
    o->h_first_u.resize((size_t)o->B * FSu);
    for (int b = 0; b < o->B; ++b) {
      const double *r = o->h_first + (size_t)b * FS;
      double *w = o->h_first_u.data() + (size_t)b * FSu;
      unpad_rows(w, r, 1, 1, nvu, nv);
      for (int i = 0; i < nvu; ++i) unpad_rows(w + nvu + (size_t)i * 2 * nvu, r + nv + (size_t)i * 2 * nv, 1, 2, nvu, nv);
      unpad_rows(w + nvu + nvu * 2 * nvu, r + nv + nv * 2 * nv, 1, 2, nvu, nv);
      std::memcpy(w + nvu + nvu * 2 * nvu + 2 * nvu, r + nv + nv * 2 * nv + 2 * nv, sizeof(double) * 8);
    }
    *host = o->h_first_u.data();
    if (stride) *stride = FSu;
    return 0;
  }
  *host = o->h_first;
  if (stride) *stride = FS;
  return 0;
}

int agx_ocp_download_first(agx_ocp *o, double *us0, double *K0, double *x1, agx_status *st) {
  const double *h = nullptr;
  int FS = 0;
  if (agx_ocp_first_packed(o, &h, &FS)) return -1;
  const int nu = o->nvu, nx = 2 * o->nvu, nk = nu * nx;
  for (int b = 0; b < o->B; ++b) {
    const double *r = h + (size_t)b * FS;
    if (us0) std::memcpy(us0 + (size_t)b * nu, r, sizeof(double) * nu);
    if (K0) std::memcpy(K0 + (size_t)b * nk, r + nu, sizeof(double) * nk);
    if (x1) std::memcpy(x1 + (size_t)b * nx, r + nu + nk, sizeof(double) * nx);
    if (st) {
      const double *q = r + nu + nk + nx;
      st[b].kkt = q[0]; st[b].cost = q[1]; st[b].merit = q[2]; st[b].gap_norm = q[3];
      st[b].iter = (int)q[4]; st[b].qp_iters = (int)q[5]; st[b].solved = (int)q[6]; st[b].flags = (int)q[7];
    }
  }
  return 0;
}

int agx_ocp_set_first_pack(agx_ocp *o, int in_solve) {
  if (!o) return fail("null handle");
  o->first_in_solve = in_solve != 0;
  return 0;
}

int agx_ocp_first_pack_counts(agx_ocp *o, long long *served_in_solve, long long *served_by_launch) {
  if (!o) return fail("null handle");
  if (served_in_solve) *served_in_solve = o->first_served[0];
  if (served_by_launch) *served_by_launch = o->first_served[1];
  return 0;
}

int agx_ocp_handoff_counts(agx_ocp *o, long long *early_exits, int *n_carriable) {
  if (!o) return fail("null handle");
  if (early_exits) *early_exits = o->early_exits;
  if (n_carriable) *n_carriable = o->n_carriable;
  return 0;
}

int agx_ocp_carry_counts(agx_ocp *o, long long *steps_carried, long long *steps_full) {
  if (!o) return fail("null handle");
  if (steps_carried) *steps_carried = o->steps_carried;
  if (steps_full) *steps_full = o->steps_full;
  return 0;
}

int agx_ocp_solve(agx_ocp *o, const double *x0, const double *xs_ws, const double *us_ws, int max_iter, double max_time,
                  double *xs, double *us, double *K, agx_status *st) {
  if (!o || !x0 || !xs_ws || !us_ws) return fail("agx_ocp_solve: null argument");
  o->first_fresh = false;
  if (agx_ocp_upload_x0(o, x0)) return -1;
  if (agx_ocp_upload_warmstart(o, xs_ws, us_ws)) return -1;  // (ends the tile carry: carry_invalidate)
  if (solve_resident(o, max_iter, max_time)) return -1;
  return agx_ocp_download(o, xs, us, K, st);
}

int agx_ocp_shift_warmstart(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    const long long units = (long long)o->B * o->T;
    const long long n = (long long)o->B * (o->T + 1) * o->nx;
    if constexpr (NV > 8) {
      // large models: plain copies for the nodes with dt_i == dt_0, one workgroup per node that has to be integrated
      (void)units;
      hipLaunchKernelGGL(agx::k_shift_copy, dim3((int)((n + 255) / 256)), dim3(256), 0, o->stream, o->d_dt, o->d_xs, o->d_us, o->B, o->T, o->nx, o->nu);
      if (!o->shift_nodes.empty())
        launch_wg(o, [&](auto PRc) {
        hipLaunchKernelGGL((agx::k_integrate_wg<NV, decltype(PRc)::value>), dim3(o->B * (int)o->shift_nodes.size()), dim3(256), 0, o->stream, o->d_model, o->dt[0], o->d_xs,
                           o->d_us, o->d_xs + n, o->d_shift_nodes, (int)o->shift_nodes.size(), o->T);
      });
    } else
      with_sources<NV, true, false>(o, [&](auto... src) {
        hipLaunchKernelGGL((agx::k_shift<NV, CH, src_t<decltype(src)>...>), dim3((int)((units + 63) / 64)), dim3(64), 0, o->stream, o->d_model, o->d_ocp,
                           o->d_dt, o->d_xs, o->d_us, src...);
      });
    hipLaunchKernelGGL(agx::k_shift_commit, dim3((int)((n + 255) / 256)), dim3(256), 0, o->stream, o->d_xs, o->d_us, o->B, o->T, o->nx, o->nu);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int agx_ocp_x0_from_prediction(agx_ocp *o) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  hipLaunchKernelGGL(agx::k_x0_from_pred, dim3((o->B * o->nx + 255) / 256), dim3(256), 0, o->stream, o->d_x0, o->d_xs, o->B, o->T, o->nx);
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_ocp_integrate(agx_ocp *o, int n, const double *x, const double *u, double *xnext) {
  if (!o || !x || !u || !xnext || n < 1) return fail("agx_ocp_integrate: bad argument");
  if (set_device(o)) return -1;
  const size_t bytes = sizeof(double) * n * (2 * o->nx + o->nu);
  if (ensure_scratch(o, bytes)) return -1;
  double *dx = o->d_scratch, *du = dx + (size_t)n * o->nx, *dn = du + (size_t)n * o->nu;
  if (up(o, dx, x, n, 2) || up(o, du, u, n, 1)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    if constexpr (NV > 8)
      launch_wg(o, [&](auto PRc) {
        hipLaunchKernelGGL((agx::k_integrate_wg<NV, decltype(PRc)::value>), dim3(n), dim3(256), 0, o->stream, o->d_model, o->dt[0], dx, du, dn, (const int *)nullptr, 0, 0);
      });
    else
      hipLaunchKernelGGL((agx::k_integrate<NV, CH>), dim3((n + 63) / 64), dim3(64), 0, o->stream, o->d_model, o->dt[0], n, dx, du, dn);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  if (down(o, xnext, dn, n, 2)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_model_rnea(agx_ocp *o, int n, const double *q, const double *v, const double *a, double *tau) {
  if (!o || !q || !v || !a || !tau || n < 1) return fail("agx_model_rnea: bad argument");
  if (set_device(o)) return -1;
  const size_t cnt = (size_t)n * o->nv;
  if (ensure_scratch(o, sizeof(double) * 4 * cnt)) return -1;
  double *dq = o->d_scratch, *dv = dq + cnt, *da = dv + cnt, *dt = da + cnt;
  if (up(o, dq, q, n, 1) || up(o, dv, v, n, 1) || up(o, da, a, n, 1)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    hipLaunchKernelGGL((agx::k_rnea<NV, CH>), dim3((n + 63) / 64), dim3(64), 0, o->stream, o->d_model, n, dq, dv, da, dt);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  if (down(o, tau, dt, n, 1)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_model_frame_placement(agx_ocp *o, int n, int frame, const double *q, double *out) {
  if (!o || !q || !out || n < 1) return fail("agx_model_frame_placement: bad argument");
  if (frame < 0 || frame >= o->hm.nframes) return fail("agx_model_frame_placement: frame id out of range");
  if (set_device(o)) return -1;
  const size_t cnt = (size_t)n * o->nv;
  if (ensure_scratch(o, sizeof(double) * (cnt + (size_t)n * 12))) return -1;
  double *dq = o->d_scratch, *dout = dq + cnt;
  if (up(o, dq, q, n, 1)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    hipLaunchKernelGGL((agx::k_frame<NV, CH>), dim3((n + 63) / 64), dim3(64), 0, o->stream, o->d_model, n, frame, dq, dout);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * n * 12, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_model_frame_jacobian(agx_ocp *o, int n, int frame, int local, const double *q, double *J) {
  if (!o || !q || !J || n < 1) return fail("agx_model_frame_jacobian: bad argument");
  if (frame < 0 || frame >= o->hm.nframes) return fail("agx_model_frame_jacobian: frame id out of range");
  if (set_device(o)) return -1;
  const size_t cnt = (size_t)n * o->nv;
  if (ensure_scratch(o, sizeof(double) * (cnt + 6 * cnt))) return -1;
  double *dq = o->d_scratch, *dout = dq + cnt;
  if (up(o, dq, q, n, 1)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    hipLaunchKernelGGL((agx::k_frame_jacobian<NV, CH>), dim3((n + 63) / 64), dim3(64), 0, o->stream, o->d_model, n, frame, local, dq, dout);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  if (down(o, J, dout, (size_t)n * 6, 1)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_get_residuals(agx_ocp *o, int row, double *out) {
  if (!o || !out) return fail("agx_ocp_get_residuals: null argument");
  if (row < 0 || row >= o->n_rows_all[0]) return fail("agx_ocp_get_residuals: row out of range");
  if (set_device(o)) return -1;
  if (row >= o->ho.rows[0].n) {  // a pair row of a wide cost set: its distance, one component
    const size_t cnt = (size_t)o->B * o->T;
    if (ensure_scratch(o, sizeof(double) * cnt)) return -1;
    HIPCHK(hipMemsetAsync(o->d_scratch, 0, sizeof(double) * cnt, o->stream));  // (an inactive row is not evaluated)
    if (launch_cost_pairs(o, agx::kPairsDistance, 1, 0, false, row - o->hw.lay[0].first, o->d_scratch)) return -1;
    HIPCHK(hipMemcpyAsync(out, o->d_scratch, sizeof(double) * cnt, hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    return 0;
  }
  const int nr = o->ho.rows[0].nr[row];
  const size_t cnt = (size_t)o->B * o->T * nr;
  if (ensure_scratch(o, sizeof(double) * cnt)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    const long long units = (long long)o->B * o->T;
    with_sources<NV, false, true>(o, [&](auto... src) {
      hipLaunchKernelGGL((agx::k_residuals<NV, CH, src_t<decltype(src)>...>), dim3((int)((units + 63) / 64)), dim3(64), 0, o->stream, o->d_model, o->d_ocp,
                         o->d_xs, o->d_us, o->rv, row, o->d_scratch, src...);
    });
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  {
    const int kind = o->ho.rows[0].kind[row];
    const bool joint_blocks = kind == AGX_RES_STATE || kind == AGX_RES_CONTROL || kind == AGX_RES_CONTROL_GRAV;
    if (o->padded && joint_blocks) { if (down(o, out, o->d_scratch, (size_t)o->B * o->T, nr / o->nv)) return -1; }
    else HIPCHK(hipMemcpyAsync(out, o->d_scratch, sizeof(double) * cnt, hipMemcpyDeviceToHost, o->stream));
  }
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_iter_log(agx_ocp *o, int capacity) {
  if (!o) return fail("null handle");
  if (capacity < 0) return fail("agx_ocp_iter_log: negative capacity");
  if (set_device(o)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));  // (a queued log launch may still write the old arrays)
  o->own.release(&o->d_log);
  o->own.release(&o->d_log_n);
  o->log_cap = 0;
  if (capacity == 0) return 0;
  HIPCHK(o->own.device(&o->d_log, (size_t)o->B * capacity));
  HIPCHK(o->own.device(&o->d_log_n, (size_t)o->B));
  HIPCHK(hipMemsetAsync(o->d_log, 0, sizeof(agx_iter_record) * (size_t)o->B * capacity, o->stream));
  HIPCHK(hipMemsetAsync(o->d_log_n, 0, sizeof(int) * (size_t)o->B, o->stream));
  o->log_cap = capacity;
  return 0;
}

int agx_ocp_iter_log_read(agx_ocp *o, agx_iter_record *out, int32_t *n) {
  if (!o) return fail("null handle");
  if (o->log_cap <= 0) return fail("agx_ocp_iter_log_read: the log is off (agx_ocp_iter_log)");
  if (set_device(o)) return -1;
  if (out) HIPCHK(hipMemcpyAsync(out, o->d_log, sizeof(agx_iter_record) * (size_t)o->B * o->log_cap, hipMemcpyDeviceToHost, o->stream));
  if (n) HIPCHK(hipMemcpyAsync(n, o->d_log_n, sizeof(int) * (size_t)o->B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

// Every cost item of every node on its own, at the resident (xs, us) with the references the solver would read (o->rv).  Reads
// only: the iterate, the tiles, the solver state and the tile carry are left as they are (a staging buffer of its own).
int agx_ocp_item_costs(agx_ocp *o, double *cost_r, double *Lx_r, double *Lu_r, double *cost_t, double *Lx_t) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  const int B = o->B, T = o->T, NV = o->nv, NX = o->nx, NU = o->nu, nvu = o->nvu;
  const int Rr = o->n_rows_all[0], Rt = o->n_rows_all[1], R = std::max(std::max(Rr, Rt), 1);
  const size_t units = (size_t)B * (T + 1) * R, total = units * (1 + NX + NU);
  if (sizeof(double) * total > o->items_bytes) {
    if (o->d_items) HIPCHK(hipStreamSynchronize(o->stream));  // (a queued launch may still write the old block)
    HIPCHK(o->own.device(&o->d_items, total));
    o->items_bytes = sizeof(double) * total;
  }
  double *d_cost = o->d_items, *d_Lx = d_cost + units, *d_Lu = d_Lx + units * NX;
  HIPCHK(hipMemsetAsync(o->d_items, 0, sizeof(double) * total, o->stream));  // inactive rows, rows a node type lacks, the terminal Lu
  const DevRows *rows2 = (const DevRows *)((const char *)o->d_ocp + offsetof(DevOcp, rows));
  const int rc = agx_diag_item_costs_launch((void *)o->stream, NV, o->chain ? 1 : 0, o->d_model, rows2, B, T, o->d_xs, o->d_us, &o->rv, R, d_cost, d_Lx,
                                            d_Lu, o->obs_set ? o->d_obs : nullptr);
  if (rc < 0) return fail("agx_ocp_item_costs: no kernel instantiation for nv = " + std::to_string(NV));
  HIPCHK((hipError_t)rc);
  if (kGeneralRowsWg && o->general && NV > 7)  // large models: the ControlGrav / FrameVelocity rows, one launch each (k_item_costs leaves them out)
    for (int lay = 0; lay < 2; ++lay)
      for (int r = 0; r < o->ho.rows[lay].n; ++r) {
        const int kind = o->ho.rows[lay].kind[r];
        if (!o->ho.rows[lay].active[r] || (kind != AGX_RES_CONTROL_GRAV && kind != AGX_RES_FRAME_VELOCITY)) continue;
        bool other = false;  // the other table's row r is evaluated by the same launch
        if (lay == 1 && r < o->ho.rows[0].n && o->ho.rows[0].active[r]) other = o->ho.rows[0].kind[r] == AGX_RES_CONTROL_GRAV || o->ho.rows[0].kind[r] == AGX_RES_FRAME_VELOCITY;
        if (other) continue;
        HIPCHK((hipError_t)agx_general_rows_launch(kGenItems, (void *)o->stream, NV, o->hm.prismatic ? 1 : 0, (long long)B * (T + 1), o->d_model, o->d_ocp,
                                                   o->d_dt, o->d_xs, o->d_us, &o->rv, d_cost, d_Lx, d_Lu, nullptr, 0, r, R));
      }
  if (o->cost_wide)  // the pair rows of a wide cost set: each pair's own value and gradient row
    HIPCHK((hipError_t)agx_cost_pairs_launch(agx::kPairsItems, (void *)o->stream, (long long)B * (T + 1), o->d_model, o->d_ocp, o->d_cw, o->d_dt, o->d_xs,
                                             &o->rv, d_cost, d_Lx, nullptr, 0, 0, R, o->obs_set ? o->d_obs : nullptr));
  std::vector<double> h(total);
  HIPCHK(hipMemcpyAsync(h.data(), o->d_items, sizeof(double) * total, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  const double *h_cost = h.data(), *h_Lx = h_cost + units, *h_Lu = h_Lx + units * NX;
  const int nxu = 2 * nvu;
  for (int b = 0; b < B; ++b)
    for (int t = 0; t <= T; ++t) {
      const bool term = t == T;
      const int Rn = term ? Rt : Rr;
      double *c_out = term ? cost_t : cost_r, *x_out = term ? Lx_t : Lx_r;
      const size_t node_out = term ? (size_t)b : (size_t)b * T + t;
      for (int r = 0; r < Rn; ++r) {
        const size_t u = ((size_t)b * (T + 1) + t) * R + r, w = node_out * Rn + r;
        if (c_out) c_out[w] = h_cost[u];
        if (x_out)
          for (int i = 0; i < nvu; ++i) { x_out[w * nxu + i] = h_Lx[u * NX + i]; x_out[w * nxu + nvu + i] = h_Lx[u * NX + NV + i]; }
        if (!term && Lu_r)
          for (int i = 0; i < nvu; ++i) Lu_r[w * nvu + i] = h_Lu[u * NU + i];
      }
    }
  return 0;
}

// Distances (and witness points, and the minimum) of the caller's pair list at the caller's configurations or at the iterate.
// Reads only, as agx_ocp_item_costs: everything it writes on the device lies in d_clear, a block of its own.
int agx_ocp_clearance(agx_ocp *o, int n_pairs, const int32_t *frame_a, const int32_t *frame_b, const double *q, int m, double *dist,
                      double *witness, double *min_dist, int32_t *min_where) {
  if (!o) return fail("agx_ocp_clearance: null handle");
  if (!frame_a || !frame_b) return fail("agx_ocp_clearance: null pair arrays");
  if (!dist) return fail("agx_ocp_clearance: null dist");
  if (n_pairs < 1) return fail("agx_ocp_clearance: n_pairs must be at least 1");
  if (m < 1) return fail("agx_ocp_clearance: m must be at least 1");
  if (!q && m != o->T + 1) return fail("agx_ocp_clearance: q == NULL evaluates the iterate, m must be T + 1 = " + std::to_string(o->T + 1));
  if ((long long)m * n_pairs > (long long)INT32_MAX) return fail("agx_ocp_clearance: m x n_pairs exceeds 2^31 - 1");
  for (int p = 0; p < n_pairs; ++p) {
    const std::string where = "agx_ocp_clearance: pair " + std::to_string(p) + ": ";
    for (const int f : {(int)frame_a[p], (int)frame_b[p]}) {
      if (f < 0 || f >= o->hm.nframes) return fail(where + "frame " + std::to_string(f) + " out of range");
      if (!agx::frame_has_geometry(o->hm, f)) return fail(where + "frame " + std::to_string(f) + " carries no collision geometry");
    }
    if (agx::frame_is_box(o->hm, frame_a[p]) && agx::frame_is_box(o->hm, frame_b[p])) return fail(where + "box / box collision pairs are not supported");
  }
  if (set_device(o)) return -1;
  const size_t B = o->B, NV = o->nv, items = B * m * n_pairs;
  const int chunks = agx_diag_clearance_chunks(m);
  // d_clear: dist | witness | chunk minima | min_dist | q (padded to the capacity) | then the ints: pairs a | pairs b | chunk items | min_where
  const size_t n_wit = witness ? items * 9 : 0, n_q = q ? B * m * NV : 0;
  const size_t n_dbl = items + n_wit + B * chunks + B + n_q, n_int = 2 * (size_t)n_pairs + B * chunks + 2 * B;
  const size_t bytes = sizeof(double) * n_dbl + sizeof(int) * n_int;
  if (bytes > o->clear_bytes) {  // (nothing queued uses the old block: every call ends with a wait for the stream)
    HIPCHK(o->own.device_bytes(&o->d_clear, bytes));
    o->clear_bytes = bytes;
  }
  double *d_dist = (double *)o->d_clear, *d_wit = d_dist + items, *d_cmin = d_wit + n_wit, *d_min = d_cmin + B * chunks, *d_q = d_min + B;
  int *d_fa = (int *)(d_q + n_q), *d_fb = d_fa + n_pairs, *d_cidx = d_fb + n_pairs, *d_where = d_cidx + B * chunks;
  std::vector<int> h_pairs(2 * (size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) { h_pairs[p] = frame_a[p]; h_pairs[n_pairs + p] = frame_b[p]; }
  HIPCHK(hipMemcpyAsync(d_fa, h_pairs.data(), sizeof(int) * h_pairs.size(), hipMemcpyHostToDevice, o->stream));
  std::vector<double> h_q;  // (alive until the wait below)
  if (q) {
    const double *src = q;
    if (o->padded) {
      h_q.assign(n_q, 0.0);
      pad_rows(h_q.data(), q, B * m, 1, o->nvu, o->nv, 0.0);
      src = h_q.data();
    }
    HIPCHK(hipMemcpyAsync(d_q, src, sizeof(double) * n_q, hipMemcpyHostToDevice, o->stream));
  }
  const bool want_min = min_dist || min_where;
  HIPCHK((hipError_t)agx_diag_clearance_launch((void *)o->stream, o->d_model, o->nv, o->B, n_pairs, d_fa, d_fb, q ? d_q : o->d_xs,
                                               q ? (long long)m * o->nv : (long long)(o->T + 1) * o->nx, q ? o->nv : o->nx, m, d_dist,
                                               witness ? d_wit : nullptr, d_cmin, d_cidx, want_min ? d_min : nullptr, d_where,
                                               o->obs_set ? o->d_obs : nullptr));
  HIPCHK(hipMemcpyAsync(dist, d_dist, sizeof(double) * items, hipMemcpyDeviceToHost, o->stream));
  if (witness) HIPCHK(hipMemcpyAsync(witness, d_wit, sizeof(double) * n_wit, hipMemcpyDeviceToHost, o->stream));
  if (min_dist) HIPCHK(hipMemcpyAsync(min_dist, d_min, sizeof(double) * B, hipMemcpyDeviceToHost, o->stream));
  if (min_where) HIPCHK(hipMemcpyAsync(min_where, d_where, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_calc_diff(agx_ocp *o, double *tiles) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (launch_calc_diff(o, false)) return -1;
  if (tiles && o->padded) {
    // canonical tiles Fx | Fu | f | Lx | Lu | Lxx | Lxu | Luu | cost of the caller's nvu joints out of the capacity-sized ones
    const size_t nodes = (size_t)o->B * (o->T + 1);
    const int nv = o->nv, nvu = o->nvu, NX = 2 * nv, NU = nv, nxu = 2 * nvu, nuu = nvu, TU = AGX_TILE_DOUBLES(nvu);
    o->stage.resize(nodes * o->tile);
    HIPCHK(hipMemcpyAsync(o->stage.data(), o->d_tiles, sizeof(double) * o->stage.size(), hipMemcpyDeviceToHost, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
    auto xm = [&](int i) { return i < nvu ? i : nv + (i - nvu); };
    for (size_t n = 0; n < nodes; ++n) {
      const double *c = o->stage.data() + n * o->tile;
      double *u = tiles + n * TU;
      const double *cFx = c, *cFu = cFx + NX * NX, *cf = cFu + NX * NU, *cLx = cf + NX, *cLu = cLx + NX, *cLxx = cLu + NU,
                   *cLxu = cLxx + NX * NX, *cLuu = cLxu + NX * NU, *ccost = cLuu + NU * NU;
      double *uFx = u, *uFu = uFx + nxu * nxu, *uf = uFu + nxu * nuu, *uLx = uf + nxu, *uLu = uLx + nxu, *uLxx = uLu + nuu,
             *uLxu = uLxx + nxu * nxu, *uLuu = uLxu + nxu * nuu, *ucost = uLuu + nuu * nuu;
      for (int i = 0; i < nxu; ++i) {
        for (int j = 0; j < nxu; ++j) { uFx[i * nxu + j] = cFx[xm(i) * NX + xm(j)]; uLxx[i * nxu + j] = cLxx[xm(i) * NX + xm(j)]; }
        for (int j = 0; j < nuu; ++j) { uFu[i * nuu + j] = cFu[xm(i) * NU + j]; uLxu[i * nuu + j] = cLxu[xm(i) * NU + j]; }
        uf[i] = cf[xm(i)]; uLx[i] = cLx[xm(i)];
      }
      for (int i = 0; i < nuu; ++i) {
        uLu[i] = cLu[i];
        for (int j = 0; j < nuu; ++j) uLuu[i * nuu + j] = cLuu[i * NU + j];
      }
      *ucost = *ccost;
    }
    return 0;
  }
  if (tiles) HIPCHK(hipMemcpyAsync(tiles, o->d_tiles, sizeof(double) * o->B * (o->T + 1) * (size_t)o->tile, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

// One QP direction at the resident (xs, us) through the production kernels: K1 (QP tiles),
// K2 (Riccati + forward), the prologue of K4 (du, KKT) and the exit path (reported gains).
int agx_ocp_direction(agx_ocp *o, double *K, double *k, double *dx, double *du, double *kkt) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (carry_invalidate(o)) return -1;
  if (reset_state(o)) return -1;
  if (launch_calc_qp(o)) return -1;
  if (launch_riccati(o, 1, 0)) return -1;
  if (launch_step(o, 0, 1, 0)) return -1;
  if (launch_gains(o)) return -1;
  const size_t B = o->B, T = o->T, nx = o->nx, nu = o->nu;
  (void)nx; (void)nu;
  if (K && down_gains(o, K, o->d_Kout, B * T)) return -1;
  if (k && down(o, k, o->d_kws, B * T, 1)) return -1;
  if (dx && down(o, dx, o->d_dx, B * (T + 1), 2)) return -1;
  if (du && down(o, du, o->d_du, B * T, 1)) return -1;
  std::vector<DevState> hs(B);
  HIPCHK(hipMemcpyAsync(hs.data(), o->d_state, sizeof(DevState) * B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  if (kkt) for (size_t b = 0; b < B; ++b) kkt[b] = hs[b].kkt;
  return 0;
}

int agx_ocp_set_step_tail(agx_ocp *o, int on, long long *launches) {
  if (!o) return fail("null handle");
  if (on >= 0) o->step_tail = on != 0;  // (read at every solve: step_tail_path)
  if (launches) *launches = o->step_tail_launches;
  return 0;
}

int agx_ocp_last_direction(agx_ocp *o, double *dx, double *du, double *nodestat) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  const size_t B = o->B, T = o->T;
  if (dx && down(o, dx, o->d_dx, B * (T + 1), 2)) return -1;
  if (du && down(o, du, o->d_du, B * T, 1)) return -1;
  if (nodestat) HIPCHK(hipMemcpyAsync(nodestat, o->d_nodestat, sizeof(double) * B * (T + 1) * 4, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_qp_tiles(agx_ocp *o, double *qt, double *aux, int *qt_size, int *aux_size) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (qt_size) *qt_size = o->qt_size;
  if (aux_size) *aux_size = o->aux_size;
  if (!qt && !aux) return 0;
  if (carry_invalidate(o)) return -1;
  if (reset_state(o)) return -1;  // (and with the ring back at its origin the tiles below come out in node order)
  if (launch_calc_qp(o)) return -1;
  const size_t n = (size_t)o->B * (o->T + 1);
  if (qt) HIPCHK(hipMemcpyAsync(qt, o->d_qt, sizeof(double) * n * o->qt_size, hipMemcpyDeviceToHost, o->stream));
  if (aux) HIPCHK(hipMemcpyAsync(aux, o->d_aux, sizeof(double) * n * o->aux_size, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

#ifdef AGX_WG_PROFILE
// development only: cycle stamps of one workgroup of the large-model derivative pass (not part of the ABI)
int agx_dev_wg_stamps(long long *out, int *n) {
  int zero = 0;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(agx::g_wg_ts), sizeof(long long) * 64) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(n, HIP_SYMBOL(agx::g_wg_n), sizeof(int)) != hipSuccess) return -1;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(agx::g_wg_n), &zero, sizeof(int));
  return 0;
}
#endif

int agx_ocp_time_kernel(agx_ocp *o, int which, int reps, double *avg_ms) {
  if (!o || !avg_ms || reps < 1) return fail("agx_ocp_time_kernel: bad argument");
  if (set_device(o)) return -1;
  if (which == 10) {  // the device work of the last stream append again (same chunk, same slots, same values), on the copy stream
    if (!o->streamed || o->st_last.buf < 0) return fail("agx_ocp_time_kernel: which = 10 needs a streamed trajectory with an append");
    HIPCHK(hipStreamSynchronize(o->stream));
    HIPCHK(hipStreamSynchronize(o->copy_stream));
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) HIPCHK(hipEventRecord(o->ev0, o->copy_stream));
      for (int r = 0; r < (pass == 0 ? 1 : reps); ++r)
        if (stream_enqueue_last(o, false)) return -1;
    }
    HIPCHK(hipEventRecord(o->ev1, o->copy_stream));
    HIPCHK(hipEventSynchronize(o->ev1));
    float ms10 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms10, o->ev0, o->ev1));
    *avg_ms = (double)ms10 / reps;
    return 0;
  }
  // state for the timed kernel: fresh solver state, QP tiles and a direction at the resident point
  if (carry_invalidate(o)) return -1;
  if (reset_state(o)) return -1;
  if (which == 1 || which == 2 || which == 5 || which == 6 || which == 7 || which == 9) { if (launch_calc_qp(o)) return -1; }
  if (which == 2) { if (launch_riccati(o, 1, 0)) return -1; }
  double *d_x0_keep = nullptr;
  if (which == 8) {  // every rollout moves x0: the timed ones start from where the last one ended, the caller's x0 comes back afterwards
    if (ensure_scratch(o, sizeof(double) * o->B * o->nx)) return -1;
    d_x0_keep = o->d_scratch;
    HIPCHK(hipMemcpyAsync(d_x0_keep, o->d_x0, sizeof(double) * o->B * o->nx, hipMemcpyDeviceToDevice, o->stream));
  }
  // warm-up launch, then `reps` timed launches bracketed by events on the problem's stream
  for (int pass = 0; pass < 2; ++pass) {
    const int n = pass == 0 ? 1 : reps;
    if (pass == 1) HIPCHK(hipEventRecord(o->ev0, o->stream));
    for (int r = 0; r < n; ++r) {
      int rc = 0;
      if (which == 0) rc = launch_calc_qp(o, false);
      else if (which == 1) rc = launch_riccati(o, 1, 0);
      else if (which == 2) rc = launch_step(o, 0, 1 << 30, 1 | 4);
      else if (which == 3) rc = launch_calc_qp(o, true);
      else if (which == 4) rc = launch_calc_diff(o, false, true);
      else if (which == 5) rc = launch_riccati(o, 0, 0);
      else if (which == 6) rc = launch_gains(o);
      else if (which == 7) rc = launch_riccati(o, 1, true, 1);
      else if (which == 8) rc = launch_rollout(o, 10, 1e-3, nullptr);
      else if (which == 9) rc = o->cost_wide ? launch_cost_pairs(o, agx::kPairsToQp, 0, 0) : fail("agx_ocp_time_kernel: kernel 9 (k_cost_pairs) needs a wide cost set");
      else return fail("agx_ocp_time_kernel: unknown kernel");
      if (rc) return rc;
    }
    if (pass == 1) HIPCHK(hipEventRecord(o->ev1, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
  }
  if (d_x0_keep) {
    HIPCHK(hipMemcpyAsync(o->d_x0, d_x0_keep, sizeof(double) * o->B * o->nx, hipMemcpyDeviceToDevice, o->stream));
    HIPCHK(hipStreamSynchronize(o->stream));
  }
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, o->ev0, o->ev1));
  *avg_ms = (double)ms / reps;
  return 0;
}

int agx_ocp_profile(agx_ocp *o, int enable, double *ms_sum, long long *count) {
  if (!o) return fail("null handle");
  if (ms_sum && count)
    for (int k = 0; k < 3; ++k) { ms_sum[k] = o->prof_ms[k]; count[k] = o->prof_n[k]; }
  if (enable != (o->prof ? 1 : 0)) {
    o->prof = enable != 0;
    for (int k = 0; k < 3; ++k) { o->prof_ms[k] = 0.0; o->prof_n[k] = 0; }
  }
  return 0;
}

int agx_ocp_download_x0(agx_ocp *o, double *x0) {
  if (!o || !x0) return fail("agx_ocp_download_x0: null argument");
  if (set_device(o)) return -1;
  if (down(o, x0, o->d_x0, o->B, 2)) return -1;
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_feedback_rollout(agx_ocp *o, int n_substeps, double dt_sub, const double *disturbance) {
  if (!o) return fail("null handle");
  if (n_substeps < 1 || !(dt_sub > 0.0)) return fail("agx_ocp_feedback_rollout: bad sub-stepping");
  if (set_device(o)) return -1;
  double *d_dist = nullptr;
  if (disturbance) {
    if (ensure_scratch(o, sizeof(double) * o->B * o->nu)) return -1;
    d_dist = o->d_scratch;
    if (up(o, d_dist, disturbance, o->B, 1)) return -1;
  }
  if (launch_rollout(o, n_substeps, dt_sub, d_dist)) return -1;
  if (disturbance) HIPCHK(hipStreamSynchronize(o->stream));  // the caller may reuse its buffer
  return 0;
}

// The body of the two per-instance inertial setters: checks the caller's arrays (at nvu joints), builds the host image of
// agx::InstanceInertials<nv>[B] in `stage` and uploads it to *d_buf (allocated on first use).  `fn` prefixes the messages.
// Nothing of the handle changes unless every check has passed.
static int upload_inertials(agx_ocp *o, const std::string &fn, const double *mass, const double *com, const double *inertia, const double *armature,
                            std::vector<double> &stage, double **d_buf) {
  const size_t B = o->B, nv = o->nv, nvu = o->nvu, w = 14 * nv;  // mass nv | com 3 nv | inertia 9 nv | armature nv
  for (size_t k = 0; k < B * nvu; ++k) {
    if (!std::isfinite(mass[k]) || (armature && !std::isfinite(armature[k])))
      return fail(fn + ": non-finite mass or armature (instance " + std::to_string(k / nvu) + ", joint " + std::to_string(k % nvu) + ")");
    if (mass[k] < 0.0) return fail(fn + ": negative mass (instance " + std::to_string(k / nvu) + ", joint " + std::to_string(k % nvu) + ")");
    if (armature && armature[k] < 0.0)
      return fail(fn + ": negative armature (instance " + std::to_string(k / nvu) + ", joint " + std::to_string(k % nvu) + ")");
  }
  for (size_t k = 0; k < B * nvu * 3; ++k)
    if (!std::isfinite(com[k])) return fail(fn + ": non-finite com (instance " + std::to_string(k / (3 * nvu)) + ")");
  for (size_t k = 0; k < B * nvu * 9; ++k)
    if (!std::isfinite(inertia[k])) return fail(fn + ": non-finite inertia (instance " + std::to_string(k / (9 * nvu)) + ")");
  if (set_device(o)) return -1;
  if (!*d_buf) HIPCHK(o->own.device(d_buf, B * w));
  // a kernel queued earlier may still read the buffer, and the copy below reads the image: both are the handle's own, so the
  // host waits for the stream before it rewrites the image, then uploads IN the solver's stream, behind everything queued
  HIPCHK(hipStreamSynchronize(o->stream));
  stage.assign(B * w, 0.0);
  for (size_t b = 0; b < B; ++b) {
    double *p = stage.data() + b * w, *pc = p + nv, *pi = pc + 3 * nv, *pa = pi + 9 * nv;
    for (size_t i = 0; i < nvu; ++i) {
      p[i] = mass[b * nvu + i];
      std::memcpy(pc + 3 * i, com + (b * nvu + i) * 3, sizeof(double) * 3);
      std::memcpy(pi + 9 * i, inertia + (b * nvu + i) * 9, sizeof(double) * 9);
      pa[i] = armature ? armature[b * nvu + i] : o->hm.armature[i];
    }
    for (size_t i = nvu; i < nv; ++i) pa[i] = o->hm.armature[i];  // pad joints: massless, the armature of the padding
  }
  HIPCHK(hipMemcpyAsync(*d_buf, stage.data(), sizeof(double) * B * w, hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_set_plant_inertials(agx_ocp *o, const double *mass, const double *com, const double *inertia, const double *armature) {
  if (!o) return fail("null handle");
  if (!mass && !com && !inertia && !armature) {  // back to the controller's own model; d_plant stays allocated for the next plant
    o->plant_set = false;
    return 0;
  }
  if (!mass || !com || !inertia) return fail("agx_ocp_set_plant_inertials: mass, com and inertia go together (all NULL clears the plant)");
  if (upload_inertials(o, "agx_ocp_set_plant_inertials", mass, com, inertia, armature, o->plant_stage, &o->d_plant)) return -1;
  o->plant_set = true;
  return 0;
}

int agx_ocp_set_model_inertials(agx_ocp *o, const double *mass, const double *com, const double *inertia, const double *armature) {
  if (!o) return fail("null handle");
  if (!mass && !com && !inertia && !armature) {  // back to the nominal table; d_minert stays allocated for the next upload
    if (!o->minert_set) return 0;
    if (set_device(o)) return -1;
    if (carry_invalidate(o)) return -1;
    o->minert_set = false;
    return 0;
  }
  if (!mass || !com || !inertia) return fail("agx_ocp_set_model_inertials: mass, com and inertia go together (all NULL goes back to the model's table)");
  if (o->nv > 7)
    return fail("agx_ocp_set_model_inertials: per-instance controller inertials are implemented for models of at most 7 joints after padding (this handle runs at " +
                std::to_string(o->nv) + ")");
  // g(q) of a ControlGrav row depends on the inertials and is evaluated on the model's table: refused, never silently nominal
  // (whether the row is active or not: rows are switched on and off after creation)
  for (int lay = 0; lay < 2; ++lay) {
    for (int r = 0; r < o->ho.rows[lay].n; ++r)
      if (o->ho.rows[lay].kind[r] == AGX_RES_CONTROL_GRAV)
        return fail("agx_ocp_set_model_inertials: the problem has a ControlGrav cost item (" + std::string(lay ? "terminal" : "running") + " row " + std::to_string(r) +
                    "), whose gravity torque is evaluated on the model's own table");
    for (int r = 0; r < o->ho.cons[lay].n; ++r)
      if (o->ho.cons[lay].kind[r] == AGX_RES_CONTROL_GRAV)
        return fail("agx_ocp_set_model_inertials: the problem has a ControlGrav constraint item (" + std::string(lay ? "terminal" : "running") + " row " +
                    std::to_string(r) + "), whose gravity torque is evaluated on the model's own table");
  }
  if (upload_inertials(o, "agx_ocp_set_model_inertials", mass, com, inertia, armature, o->minert_stage, &o->d_minert)) return -1;
  if (carry_invalidate(o)) return -1;  // every tile depends on the inertials; they are constant across steps, so the carry resumes
  o->minert_set = true;
  return 0;
}

int agx_ocp_set_obstacle_placements(agx_ocp *o, int n_frames, const int32_t *frames, const double *se3) {
  static const std::string fn = "agx_ocp_set_obstacle_placements";
  if (!o) return fail(fn + ": null handle");
  if (n_frames == 0 && !frames && !se3) {  // back to the model's placements; the buffer stays allocated for the next table
    if (!o->obs_set) return 0;
    if (set_device(o)) return -1;
    if (carry_invalidate(o)) return -1;
    o->obs_set = false;
    return 0;
  }
  if (n_frames < 1 || !frames || !se3)
    return fail(fn + ": n_frames, frames and se3 go together (0, NULL, NULL goes back to the model's placements), got n_frames = " + std::to_string(n_frames));
  if (o->nv > 7)
    return fail(fn + ": per-instance obstacle placements are implemented for models of at most 7 joints after padding (this handle runs at " +
                std::to_string(o->nv) + ")");
  // every check first: nothing of the handle changes unless all of them pass
  int slot[AGX_MAX_FRAMES];
  for (int f = 0; f < AGX_MAX_FRAMES; ++f) slot[f] = -1;
  for (int s = 0; s < n_frames; ++s) {
    const int f = frames[s];
    const std::string at = " (entry " + std::to_string(s) + ", frame " + std::to_string(f) + ")";
    if (f < 0 || f >= o->hm.nframes) return fail(fn + ": frame out of range" + at);
    if (o->hm.frame_parent[f] >= 0)
      return fail(fn + ": the frame is attached to joint " + std::to_string(o->hm.frame_parent[f]) +
                  " and moves with the robot: its placement is relative to that joint and stays the model's" + at);
    if (!(o->hm.frame_radius[f] > 0.0) && !(o->hm.frame_box[f][0] > 0.0 || o->hm.frame_box[f][1] > 0.0 || o->hm.frame_box[f][2] > 0.0))
      return fail(fn + ": the frame carries no geometry" + at);
    if (slot[f] >= 0) return fail(fn + ": frame listed twice" + at);
    slot[f] = s;
  }
  const size_t B = o->B, n = (size_t)n_frames;
  for (size_t k = 0; k < B * n * 12; ++k)
    if (!std::isfinite(se3[k]))
      return fail(fn + ": non-finite entry (instance " + std::to_string(k / (12 * n)) + ", frame " + std::to_string(frames[(k / 12) % n]) + ")");
  if (set_device(o)) return -1;
  static_assert(sizeof(agx::ObstaclePlacements) % sizeof(double) == 0, "the placements follow the header as doubles");
  const size_t hd = sizeof(agx::ObstaclePlacements) / sizeof(double), bytes = sizeof(double) * (hd + B * n * 12);
  // a kernel queued earlier may still read the buffer, and the copy below reads the image: the host waits for the solver's
  // stream before it touches either, then uploads IN that stream (as upload_inertials)
  HIPCHK(hipStreamSynchronize(o->stream));
  if (bytes > o->obs_bytes) {
    HIPCHK(o->own.device_bytes(&o->d_obs, bytes));
    o->obs_bytes = bytes;
  }
  o->obs_stage.assign(hd + B * n * 12, 0.0);
  agx::ObstaclePlacements head{};
  head.n = n_frames;
  std::memcpy(head.slot, slot, sizeof(slot));
  std::memcpy(o->obs_stage.data(), &head, sizeof(head));
  std::memcpy(o->obs_stage.data() + hd, se3, sizeof(double) * B * n * 12);
  HIPCHK(hipMemcpyAsync(o->d_obs, o->obs_stage.data(), bytes, hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  if (carry_invalidate(o)) return -1;  // the tiles of the collision rows depend on the placements; constant across steps, so the carry resumes
  o->obs_set = true;
  return 0;
}

int agx_model_sensitivity(agx_ocp *o, int n, double dt, const double *x, const double *u, double delta_inertia, double delta_com,
                          double delta_mass, double *out) {
  if (!o || !x || !u || !out) return fail("agx_model_sensitivity: null argument");
  if (n < 1) return fail("agx_model_sensitivity: n must be positive");
  if (!(dt > 0.0) || !std::isfinite(dt)) return fail("agx_model_sensitivity: dt must be positive");
  for (double d : {delta_inertia, delta_com, delta_mass})
    if (d == 0.0 || !std::isfinite(d)) return fail("agx_model_sensitivity: the deltas must be finite and not zero");
  if (set_device(o)) return -1;
  const size_t n_out = (size_t)n * 2 * o->nvu * 10 * o->nvu;
  if (ensure_scratch(o, sizeof(double) * ((size_t)n * (o->nx + o->nu) + n_out))) return -1;
  double *dx = o->d_scratch, *du = dx + (size_t)n * o->nx, *dout = du + (size_t)n * o->nu;
  if (up(o, dx, x, n, 2) || up(o, du, u, n, 1)) return -1;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    hipLaunchKernelGGL((agx::k_model_sensitivity<NV, CH>), dim3(n), dim3(agx::kSensitivityLanes<NV>), 0, o->stream, o->d_model, o->nvu, dt, dx, du,
                       delta_inertia, delta_com, delta_mass, dout);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, dout, sizeof(double) * n_out, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_ocp_mpc_step(agx_ocp *o, int k0, int max_iter, int first) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  o->first_fresh = false;  // (the prologue moves the iterate; solve_resident decides anew)
  if (agx_traj_set_window(o, k0)) return -1;
  bool prologue_done = false;
  // Tile carry: this step follows the previous one by one sample on the resident trajectory, so after the shift below node t
  // has bit for bit the inputs node t + 1 had (iterate, reference sample, dt) for t = 0 .. T - 2; x0 may differ: node 0 is
  // always evaluated.  Instances decide for themselves in the prologue (tiles of their final iterate, starting regularisation).
  const size_t lds = sizeof(double) * (size_t)o->T * (o->nx + o->nu);
  const bool one_launch = o->nv <= 8 && lds <= 60 * 1024;
  const bool carry = o->carry_static && o->carry_armed && first != 1 && k0 == o->carry_k0 + 1 && one_launch && o->hidx.empty() && o->frames_uniform;
  const int carry_mode = !carry ? 0 : (o->n_carriable == o->B ? 2 : 1);
  if (!carry && carry_invalidate(o)) return -1;
  o->carry_armed = false;  // until this step has gone through
  if (first == 1) {
    if (ws_from_ref(o, o->win_k0, 1)) return -1;  // (the physical window start: k0 itself unless the trajectory is a streamed ring)
  } else {
    // x0 <- xs[1] (first == 0; first == 2: x0 was set by the caller / the feedback rollout), warm-start
    // shift, x0 pin and state reset: one launch when the shifted nodes of an instance fit in LDS
    if (one_launch) {
      if (carry) o->head = (o->head + 1) % o->T;
      int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
        constexpr int NV = decltype(NVc)::value;
        constexpr bool CH = decltype(CHc)::value;
        if constexpr (NV <= 8) {
          with_sources<NV, true, false>(o, [&](auto... src) {
            hipLaunchKernelGGL((agx::k_mpc_prologue<NV, CH, src_t<decltype(src)>...>), dim3(o->B), dim3(128), lds, o->stream, o->d_model, o->d_ocp,
                               o->d_dt, o->d_xs, o->d_us, o->d_x0, o->d_state, o->d_ndone, first == 0 ? 1 : 0, carry ? 1 : 0, o->head,
                               (int *)((char *)o->d_ocp + offsetof(DevOcp, head)), src...);
          });
          HIPCHK(hipGetLastError());
        }
        return 0;
      });
      if (rc) return rc;
      prologue_done = true;
    } else {
      if (first == 0 && agx_ocp_x0_from_prediction(o)) return -1;
      if (agx_ocp_shift_warmstart(o)) return -1;
    }
  }
  if (solve_resident(o, max_iter, 0.0, prologue_done, carry_mode)) return -1;
  (carry_mode != 0 ? o->steps_carried : o->steps_full) += 1;
  o->carry_armed = o->carry_static;
  o->carry_k0 = k0;
  return 0;
}

}  // extern "C"
