// agx_host_handle.hpp -- the handle types of libagimus_hip.so and what every host function needs around them: the error
// channel (fail / HIPCHK), the owner of a handle's device resources and the repacking between the caller's layout and the
// capacity.  Host code only; included by agimus_hip.hip (one translation unit per capacity group).
#pragma once

#include <deque>

namespace {

thread_local std::string g_err;
int fail(const std::string &msg) {
  g_err = msg;
  return -1;
}
#define HIPCHK(expr)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));                \
  } while (0)

// Owner of what a handle allocates: device memory, page-locked host memory and events, each registered under the address of the
// agx_ocp field (or container element) that holds it.  The fields stay raw pointers, launches read them as ever, and two registered
// fields may swap their values: the owner looks at a field only when it frees.  What is still registered when the handle is deleted
// is freed then.  Nothing here waits for a stream: callers keep their waits in front of a release.  Views of something else are
// never registered (the declarations of d_first, d_ocp_k1, h_ndone_dev and rv say whose), nor are streams (agx_ocp_destroy).
class DeviceOwner {
 public:
  DeviceOwner() = default;
  DeviceOwner(const DeviceOwner &) = delete;
  ~DeviceOwner() { for (const Held &h : held_) free_value(*h.field, h.kind); }
  // `count` elements of T into *field (zero: cleared before this returns).  What the field held is freed once the new block
  // exists: a failed allocation leaves the field as it was, and a regrow (scratch, item staging, obstacle table) holds old and new
  // block for a moment.  A caller that wants the room of the old block first releases it first (traj_drop, agx_ocp_iter_log).
  template <class T> hipError_t device(T **field, size_t count, bool zero = false) { return device_bytes((void **)field, sizeof(T) * count, zero); }
  hipError_t device_bytes(void **field, size_t bytes, bool zero = false) {
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && zero) (void)hipMemset(p, 0, bytes);
    return adopt(field, p, kDevice, e);
  }
  template <class T> hipError_t pinned(T **field, size_t bytes, unsigned flags) {
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    return adopt((void **)field, p, kPinned, e);
  }
  hipError_t event(hipEvent_t *field, unsigned flags = hipEventDefault) {
    hipEvent_t ev = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&ev, flags);
    return adopt((void **)field, (void *)ev, kEvent, e);
  }
  // frees what a registered field holds and sets it to null; a field the owner does not know is left alone
  template <class T> void release(T *field) {
    for (Held &h : held_)
      if (h.field == (void **)field) {
        free_value(*h.field, h.kind);
        *h.field = nullptr;
        h = held_.back();
        held_.pop_back();
        return;
      }
  }

 private:
  enum Kind { kDevice, kPinned, kEvent };
  struct Held { void **field; Kind kind; };
  static void free_value(void *p, Kind kind) {
    if (p) (void)(kind == kDevice ? hipFree(p) : (kind == kPinned ? hipHostFree(p) : hipEventDestroy((hipEvent_t)p)));
  }
  hipError_t adopt(void **field, void *p, Kind kind, hipError_t e) {
    if (e != hipSuccess) return e;
    release(field);
    *field = p;
    held_.push_back({field, kind});
    return hipSuccess;
  }
  std::vector<Held> held_;
};

}  // namespace

struct agx_model {
  DevModel h;   // padded to the compiled capacity (see pad_capacity)
  int nvu = 0;  // joints of the caller's model
};

struct agx_ocp {
  DevModel hm;
  DevOcp ho;
  int nv = 0, nx = 0, nu = 0, T = 0, B = 0, tile = 0, stride = 0, device = 0;
  // Model sizes at run time: the kernels exist for a few CAPACITIES (7 joints: eight lanes per node; 30 / 32: a workgroup per
  // node).  A model with fewer joints is padded with massless, unit-armature joints that couple to nothing (pad_model): every
  // cross term with a real joint is an exact zero, the pad block of each QP is an independent problem with zero data, so the
  // real entries of xs, us, K, the costs and KKT residuals are what the exact-size recursion gives.  nv / nx / nu / stride above
  // are the internal (capacity) sizes; nvu / stride_u the caller's.  Arrays crossing the C ABI are repacked on the host.
  int nvu = 0, stride_u = 0;
  bool padded = false;
  std::vector<int> refmap[2];        // internal reference-tile element -> element of the caller's tile (-1: pad), running / terminal layout
  std::vector<double> reffill[2];    // value of the pad elements
  std::vector<double> stage;         // host staging of repacked arrays
  std::vector<double> h_first_u;     // first-node results in the caller's layout
  bool chain = false;
  std::vector<double> dt;
  hipStream_t stream = nullptr;  // created by the handle (own_stream) or the caller's (agx_ocp_set_stream): agx_ocp_destroy destroys its own only
  bool own_stream = false;
  // device buffers (registered with `own`, the last member, unless the declaration says whose view a pointer is)
  DevModel *d_model = nullptr;
  DevOcp *d_ocp = nullptr;
  double *d_dt = nullptr, *d_xs = nullptr, *d_us = nullptr, *d_x0 = nullptr, *d_tiles = nullptr;
  double *d_Kws = nullptr, *d_kws = nullptr, *d_Kout = nullptr, *d_dx = nullptr, *d_du = nullptr;
  double *d_Kws_lqr = nullptr, *d_kws_lqr = nullptr;  // gains of the plain LQR pass when it runs next to the ADMM factorisation
  bool admm_prefactor = true;  // AGX_ADMM_PREFACTOR=0: LQR pass, then the factorisation inside the first ADMM iteration
  double *d_qt = nullptr, *d_aux = nullptr, *d_w = nullptr, *d_nodestat = nullptr;  // QP tiles, aux tiles, acceleration steps
  // constrained problems (agx_admm.hpp): augmented tiles, constraint values / collision Jacobians,
  // multipliers y (persistent across solves), slack z, prox centre, per-node residual norms
  bool has_con = false;
  std::vector<int> shift_nodes;  // large models: nodes with dt_i != dt_0 (integrated by the warm-start shift)
  int *d_shift_nodes = nullptr;
  bool general = false;       // ControlGrav / FrameVelocity cost rows: one-lane GEN kernels (agx_general.hpp) up to 7 joints,
                              // k_general_rows_wg / k_node_kkt_big_gen behind the workgroup kernels above (agx_general_rows.hpp)
  double *d_auxg = nullptr;   // [B][T+1][3 nv LD]: Lqv | Lvvd | Lqu of every node (general problems; LD: the tiles' row stride)
  double *d_qt2 = nullptr, *d_cg = nullptr, *d_cjac = nullptr, *d_y = nullptr, *d_z = nullptr, *d_cx = nullptr, *d_admmstat = nullptr,
         *d_fac = nullptr,  // Riccati factors of every node for the gradient-only ADMM sweeps [B][T][192]
         *d_segP = nullptr;  // closed-loop transition products of the horizon segments [B][kSeg][4][64] (agx_admm.hpp)
  bool admm_segments = true;  // AGX_ADMM_SEGMENTS=0: gradient-only sweeps on one wave per instance
  int qt_size = 0, aux_size = 0;
  bool k1_lanes = true;  // AGX_K1_LANES=0 selects the one-lane-per-node derivative kernel
  bool lanes_ok = true;  // problem fits the LDS staging of the 8-lanes-per-node kernel
  bool lanes_coll = false;  // ... in its variant with one collision cost row
  // Wide cost set (agx_cost_pairs.hpp): ho.rows hold the non-collision prefix of the caller's row tables, the trailing collision
  // rows live in hw (k_cost_pairs adds them to the tiles behind every K1 launch).  K1 reads d_ocp_k1, a copy of the description
  // whose `stride` is the length of the prefix (what it stages in LDS); everybody else d_ocp with the stride of the tile.
  bool cost_wide = false;
  DevCostWide hw{};
  DevCostWide *d_cw = nullptr;
  DevOcp *d_ocp_k1 = nullptr;  // == d_ocp unless cost_wide (or general rows on a large model: K1 stages the tile up to its last
                               // row that is not a general row), then d_ocp + 1: a view, never registered
  int n_rows_all[2] = {0, 0};  // rows of the caller's tables, running / terminal (ho.rows[l].n + hw.lay[l].n)
  bool speculate = true;  // AGX_SPECULATE_GAINS=0: gains sweep only on exit
  bool gains_mfma = true; // AGX_GAINS_MFMA=0: scalar K = M Kw - taux for large models
  bool riccati_mx = true;    // AGX_RICCATI_MX=0: nv <= 7 sweeps on the 8 x 8 lane grid (k_riccati) instead of the MFMA operand layout (k_riccati_mx)
  // Exact two-level sweep (agx_riccati_mx2.hpp): the horizon in mx2_S segments swept in parallel; 0 = the one-wave sweep.
  // Chosen from the batch at creation (small batches leave most of the chip idle), AGX_MX2_SEGMENTS=n overrides (0: off).
  int mx2_S = 0;
  double *d_mx2_elem = nullptr, *d_mx2_bnd = nullptr, *d_mx2_cl = nullptr;  // [2][B][S][3][256] segment elements, [2][B][S][256] boundary value functions, [B][S][256] transitions under the gains
  bool k1_fused = true;     // AGX_K1_FUSED=0: running and terminal nodes of the derivative pass as two launches (profiling)
  bool node_kkt_wide = true;  // AGX_NODE_KKT_WIDE=0: nv <= 7 node shares by k_node_kkt (a wait per group of loads) instead of k_node_kkt_ahead
  long long step_tail_launches = 0;  // k_step_tail launches of this handle so far (agx_ocp_set_step_tail reports it)
  bool step_tail = true;      // agx_ocp_set_step_tail(0): forward pass in the sweep, K3 and the head of the step as three launches instead of k_step_tail
  // Tile carry across MPC steps: the running-node tiles live in a ring (tile_slot, agx_kernels.hpp) whose
  // origin advances with every carried agx_ocp_mpc_step, so that the first derivative pass of a step evaluates nodes 0, T - 1
  // and T only.  7-joint capacity, eight-lane derivative kernel, unconstrained, MFMA-layout sweeps, one dt for every node.
  bool tile_carry = true;       // AGX_TILE_CARRY=0: the full pass every step
  bool carry_static = false;    // the problem qualifies (agx_ocp_create)
  bool carry_armed = false;     // the last call that touched the iterate, the references or the tiles was an agx_ocp_mpc_step
  int carry_k0 = 0;             // ... with this window
  int head = 0;                 // DevOcp::head as the stream will see it
  int n_carriable = -1;         // instances whose tiles the next step may inherit, as the last solve published it (-1: not known)
  bool frames_uniform = true;   // the resident frame table holds one frame per row for every node (no per-node override uploaded)
  // Batch policy (agx_ocp_set_quorum): the SQP loop of a batch step ends once this fraction of the instances has
  // finished, the ADMM loop of an SQP iteration once this fraction of the QPs has converged; the others keep their
  // iterate (solved = 0 / qp_iters = max_qp_iters) and continue from it at the next MPC step, as a lone controller
  // that ran into max_solve_time would.  1.0 = wait for everyone (the default).
  double quorum_sqp = 1.0, quorum_qp = 1.0;
  bool con_lanes = true;          // constraint rows are control limits / state bounds / collision distances: k_con_eval_lj (AGX_CON_LANES=0: one lane per node)
  bool con_wide = false;          // wide constraint set (DevCons: up to AGX_MAX_PAIRS collision pairs): k_con_eval_pairs, WIDE ADMM kernels (AGX_CON_WIDE=1 forces it where it applies)
  int con_cs = AGX_MAX_NC;        // stride of g / y / z per node (wide sets: DevCons::cstride)
  bool admm_loop_always = false;  // AGX_ADMM_LOOP=2 (tests): k_admm_loop whatever the number of unfinished instances
  bool admm_loop = true;      // AGX_ADMM_LOOP=0: every ADMM iteration as three launches (sweep, update, reduce) instead of k_admm_loop
  int n_unfinished = 1 << 30; // instances the SQP loop still works on (host's last count): k_admm_loop serves the tail of a step, when
                              // few instances are left (with the whole batch active the node-parallel update across the chip is faster)
  bool fold_publish = false;  // small batches (B <= 204, polled hand-off): the head / accept kernels hand the counters to the host themselves (last workgroup to arrive) and the host asks after the head from the second iteration on; AGX_FOLD_PUBLISH=0/1 overrides
  int n_cu = 256;         // compute units of the device (grid of the persistent kernels)
  bool no_empty = false;  // AGX_NO_EMPTY_LAUNCHES=1 (profiling): the host asks after the head of the step whether anybody searches and skips the trial launches otherwise, so that per-kernel averages are those of working launches
  double *d_ref = nullptr;  // owned tile [B][T+1][stride]
  // asynchronous reference upload (agx_ocp_set_refs_async): second tile / frame table filled by the copy stream while the
  // solver works on the first; the next solve waits for the copy's event and swaps the two
  double *d_ref_back = nullptr;
  int *d_frames_back = nullptr;
  bool refs_pending = false, refs_pending_frames = false;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_refs = nullptr, ev_snap = nullptr, ev_dl = nullptr;
  // asynchronous result download (agx_ocp_download_async): device-side snapshot of xs | us | K taken in the solver's stream
  double *d_snap = nullptr;
  bool dl_pending = false;
  int *d_frames = nullptr;  // owned [B][T+1][AGX_MAX_ROWS]
  bool frames_set = false;
  DevState *d_state = nullptr;
  int *d_ndone = nullptr;
  // pinned, fine-grained (coherent) mapped host words, 64 bit each: [0] finished-instance count, [1] its sequence
  // stamp, [2] stamp of the packed results, [3] scratch value, [4] ADMM converged count, [5] its stamp, [6] / [7] line-search
  // trials handed on / iterations ended with stale tiles, [8] instances with tiles the next MPC step may inherit, [9] instances
  // whose first-node record k_sqp_head has packed, [10] stamp of the hand-off right behind the head of large batches and
  // [11] / [12] / [13] its finished / inheritable / packed counts.
  // Stamps are 64-bit and only ever grow (no wrap in practice); slots start at ~0, which no stamp takes.
  unsigned long long *h_ndone = nullptr;
  unsigned long long *h_ndone_dev = nullptr;  // the same words as the device sees them (mapped host memory): a view of h_ndone
  unsigned long long seq = 0;
  unsigned ls_handed = 0, ls_stale = 0;  // last values seen of the device counters of handed-on line-search trials / iterations ended with stale tiles (d_ndone[3], [4]; never reset)
  bool poll = true;  // AGX_HOST_POLL=0: stream-ordered copies + synchronize instead of polled mapped words
  double *d_first = nullptr, *h_first = nullptr;  // packed first-node results [B][first_stride], device / pinned host; while `poll` is on d_first is the mapped view of h_first, never registered
  int first_stride = 0;
  // First-node records packed during the solve (k_sqp_head, agx_ocp_set_first_pack): once the block exists the head gets it, and
  // a solve that every instance ended by packing its record leaves it fresh -- agx_ocp_first_packed then returns it as it is.
  bool first_in_solve = true;
  bool first_fresh = false;  // the block holds the results of the last solve and nothing has touched xs / us / K / the state since
  int n_packed = 0;          // records packed in the running solve, as last published
  long long first_served[2] = {0, 0};  // agx_ocp_first_packed calls served from the fresh block / by k_pack_first
  long long steps_carried = 0, steps_full = 0;  // agx_ocp_mpc_step calls whose first derivative pass inherited tiles (carry_mode != 0) / ran in full (agx_ocp_carry_counts)
  long long early_exits = 0;  // SQP loops that ended on the hand-off right behind the head, without waiting for the trial round (agx_ocp_handoff_counts)
  double *d_scratch = nullptr;
  size_t scratch_bytes = 0;
  // plant of the closed loop (agx_ocp_set_plant_inertials): agx::PlantInertials<nv>[B], read by k_plant_rollout only
  double *d_plant = nullptr;
  bool plant_set = false;
  std::vector<double> plant_stage;  // host image of d_plant (the upload reads it after the setter has returned the caller's arrays)
  // per-instance controller model (agx_ocp_set_model_inertials, 7-joint capacity): agx::InstanceInertials<nv>[B].  While set,
  // every launch that evaluates dynamics goes to the instantiation that reads it (with_sources), as does the plant-less rollout.
  double *d_minert = nullptr;
  bool minert_set = false;
  std::vector<double> minert_stage;
  // per-instance obstacle placements (agx_ocp_set_obstacle_placements, 7-joint capacity): one buffer, agx::ObstaclePlacements (the
  // frame -> slot map) followed by se3 [B][n][12].  While set, every launch that evaluates a collision distance goes to the
  // instantiation that reads it (with_sources); unset, nothing of a launch differs from a handle that never had a table.
  void *d_obs = nullptr;
  size_t obs_bytes = 0;  // allocated
  bool obs_set = false;
  std::vector<double> obs_stage;  // host image of d_obs
  RefView rv{};  // base / frames: views into d_ref, d_traj, d_frames -- or the caller's memory (agx_ocp_set_refs_device, adopt = 1); never registered
  // resident trajectory
  double *d_traj = nullptr, *d_pts = nullptr;
  double *d_sine = nullptr;  // q0, amp, puls, scale, t0
  int n_points = 0;
  // non-uniform horizon indexes (TrajectoryBuffer): empty = node t looks at sample k0 + t
  std::vector<int> hidx;
  int *d_hidx = nullptr;
  int win_logical = -1;  // streamed ring: logical start of the last window set (-1: none since the ring was created)
  int win_k0 = 0;  // physical start sample of the window (a streamed ring: slot k0 mod capacity)
  // Streamed resident trajectory (agx_traj_stream_*): d_traj / d_pts hold a ring of st_cap sample slots per
  // instance followed by st_span - 1 mirror slots (n_points = their sum); logical samples [st_first, st_end) are retained,
  // sample k in slot k mod st_cap.  An append stages its chunk in one of two page-locked buffers, copies it to the device twin and
  // fills the slots on the copy stream; ev_st[i] is recorded behind the fill.  st_pending[i]: the solver stream has not been made
  // to wait for that append yet (done when a window or a reader reaches a sample >= st_lo[i]).
  bool streamed = false;
  int st_cap = 0, st_span = 0, st_first = 0, st_end = 0;
  int st_chunk = 0;  // samples per instance a staging buffer holds (longer appends go in pieces)
  double *st_host[2] = {nullptr, nullptr}, *d_st_stage[2] = {nullptr, nullptr};
  hipEvent_t ev_st[2] = {nullptr, nullptr}, ev_st_solver = nullptr;
  bool st_used[2] = {false, false}, st_pending[2] = {false, false};
  int st_lo[2] = {0, 0};
  int st_next = 0;
  // agx_traj_stream_timing: while on, every join is bracketed by two events on the solver stream ([0]: how long that stream sat
  // waiting for a fill) and every appended piece by two on the copy stream ([1]: transfer + fill); pairs are kept until read
  bool st_timing = false;
  std::deque<hipEvent_t> st_tev[2];  // [kind][2 * k] start, [2 * k + 1] stop (a deque: the owner keeps the address of every element)
  size_t st_tev_used[2] = {0, 0};
  double st_tms[2] = {0.0, 0.0};
  long long st_tn[2] = {0, 0};
  long long st_joins = 0;  // times the solver stream was made to wait for an append (agx_traj_stream_joins)
  agx::SineParams st_sp{};  // weights and frame given at create
  // the device work of the last appended piece (agx_ocp_time_kernel(10) repeats it): staging buffer, samples, logical start,
  // doubles copied, kernel parameters
  struct { int buf = -1, m = 0, end = 0; size_t used = 0; agx::SineParams sp{}; } st_last;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
  int last_max_iter = 0;
  // per-iteration solver log (agx_ocp_iter_log): records [B][log_cap] and counts [B] on the device; log_cap == 0: off, and a solve
  // launches nothing for it
  int log_cap = 0;
  agx_iter_record *d_log = nullptr;
  int *d_log_n = nullptr;
  // staging of agx_ocp_item_costs (cost | Lx | Lu of every node and row at the capacity), grown on demand
  double *d_items = nullptr;
  size_t items_bytes = 0;
  // block of agx_ocp_clearance (the call's pair table, its padded configurations and its results), grown on demand
  void *d_clear = nullptr;
  size_t clear_bytes = 0;
  // in-situ kernel timing (agx_ocp_profile): event pairs around the launches of the SQP loop
  bool prof = false;
  std::deque<hipEvent_t> prof_ev;  // [2 * k] start, [2 * k + 1] stop (a deque, as st_tev); the first prof_used are recorded in the running solve
  size_t prof_used = 0;
  std::vector<int> prof_kind;
  double prof_ms[3] = {0, 0, 0};
  long long prof_n[3] = {0, 0, 0};
  // owner of the allocations and events above.  The last member: it is destroyed first, while every field it reads is still there
  DeviceOwner own;
};

namespace {

int set_device(agx_ocp *o) {
  HIPCHK(hipSetDevice(o->device));
  return 0;
}

// the solver reads its references from the handle's own tile d_ref [B][T + 1][stride]; `frames`: d_frames, or null for the rows' own frames
void rv_own_tile(agx_ocp *o, const int *frames) {
  o->rv.base = o->d_ref;
  o->rv.bstride = (long long)(o->T + 1) * o->stride;
  o->rv.tstride = o->stride;
  o->rv.term_off = 0;
  o->rv.frames = frames;
}

// ---- repacking between the caller's layout (nvu joints) and the internal one (nv = capacity) -----------------------------
// rows of `blocks` blocks of nvu doubles  <->  rows of `blocks` blocks of nv doubles
void pad_rows(double *dst, const double *src, size_t rows, int blocks, int nvu, int nv, double fill) {
  for (size_t r = 0; r < rows; ++r)
    for (int b = 0; b < blocks; ++b) {
      double *d = dst + (r * blocks + b) * nv;
      const double *q = src + (r * blocks + b) * nvu;
      for (int i = 0; i < nvu; ++i) d[i] = q[i];
      for (int i = nvu; i < nv; ++i) d[i] = fill;
    }
}
void unpad_rows(double *dst, const double *src, size_t rows, int blocks, int nvu, int nv) {
  for (size_t r = 0; r < rows; ++r)
    for (int b = 0; b < blocks; ++b) {
      double *d = dst + (r * blocks + b) * nvu;
      const double *q = src + (r * blocks + b) * nv;
      for (int i = 0; i < nvu; ++i) d[i] = q[i];
    }
}
// host -> device of [rows][blocks][nvu] into [rows][blocks][nv]; synchronous for padded handles (staging is reused)
int up(agx_ocp *o, double *d_dst, const double *h_src, size_t rows, int blocks, double fill = 0.0) {
  if (!o->padded) {
    HIPCHK(hipMemcpyAsync(d_dst, h_src, sizeof(double) * rows * blocks * o->nv, hipMemcpyHostToDevice, o->stream));
    return 0;
  }
  o->stage.resize(rows * blocks * o->nv);
  pad_rows(o->stage.data(), h_src, rows, blocks, o->nvu, o->nv, fill);
  HIPCHK(hipMemcpyAsync(d_dst, o->stage.data(), sizeof(double) * o->stage.size(), hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}
// device -> host of [rows][blocks][nv] into [rows][blocks][nvu]; padded handles synchronize inside
int down(agx_ocp *o, double *h_dst, const double *d_src, size_t rows, int blocks) {
  if (!o->padded) {
    HIPCHK(hipMemcpyAsync(h_dst, d_src, sizeof(double) * rows * blocks * o->nv, hipMemcpyDeviceToHost, o->stream));
    return 0;
  }
  o->stage.resize(rows * blocks * o->nv);
  HIPCHK(hipMemcpyAsync(o->stage.data(), d_src, sizeof(double) * o->stage.size(), hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  unpad_rows(h_dst, o->stage.data(), rows, blocks, o->nvu, o->nv);
  return 0;
}
// gains: [n][nv][2 nv] on the device -> [n][nvu][2 nvu]
int down_gains(agx_ocp *o, double *h_dst, const double *d_src, size_t n) {
  if (!o->padded) {
    HIPCHK(hipMemcpyAsync(h_dst, d_src, sizeof(double) * n * o->nu * o->nx, hipMemcpyDeviceToHost, o->stream));
    return 0;
  }
  const int nv = o->nv, nvu = o->nvu;
  o->stage.resize(n * nv * 2 * nv);
  HIPCHK(hipMemcpyAsync(o->stage.data(), d_src, sizeof(double) * o->stage.size(), hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  for (size_t r = 0; r < n; ++r)
    for (int i = 0; i < nvu; ++i)
      unpad_rows(h_dst + (r * nvu + i) * 2 * nvu, o->stage.data() + (r * nv + i) * 2 * nv, 1, 2, nvu, nv);
  return 0;
}
// reference tile [nodes][stride_u] (running layout, `term_every` > 0: every term_every-th node in the terminal layout)
void pad_ref_tile(const agx_ocp *o, double *dst, const double *src, size_t B, int T) {
  for (size_t b = 0; b < B; ++b)
    for (int t = 0; t <= T; ++t) {
      const int lay = t == T ? 1 : 0;
      const double *q = src + (b * (T + 1) + t) * o->stride_u;
      double *d = dst + (b * (T + 1) + t) * o->stride;
      const int *map = o->refmap[lay].data();
      const double *fill = o->reffill[lay].data();
      for (int e = 0; e < o->stride; ++e) d[e] = map[e] >= 0 ? q[map[e]] : fill[e];
    }
}

// Page-locked block the device writes and the host polls: that needs FINE-GRAINED memory (the stamp must not overtake the data it
// guards), asked for explicitly.  When the runtime cannot give it: plain pinned memory, and stream-ordered copies + synchronize from here on.
template <class T>
int pinned_polled(agx_ocp *o, T **field, size_t bytes) {
  if (o->poll && o->own.pinned(field, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); o->poll = false; }
  if (!o->poll) HIPCHK(o->own.pinned(field, bytes, hipHostMallocDefault));
  return 0;
}

int ensure_scratch(agx_ocp *o, size_t bytes) {
  if (bytes <= o->scratch_bytes) return 0;
  HIPCHK(o->own.device_bytes((void **)&o->d_scratch, bytes));
  o->scratch_bytes = bytes;
  return 0;
}

}  // namespace
