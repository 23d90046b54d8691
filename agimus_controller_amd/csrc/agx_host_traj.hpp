// agx_host_traj.hpp -- the resident reference trajectories (agx_traj_*): the generators, the window, the readers and the
// streamed ring.  Host code only; included by agimus_hip.hip behind its launch helpers (dispatch, carry_invalidate,
// ensure_copy_stream), in front of the entry points that use ws_from_ref / stream_enqueue_last.
#pragma once

namespace {

// The handle stops being a streamed ring (another trajectory is created, or a new ring): fills still queued on the copy stream
// write d_traj / d_pts, so the host waits for them before those are freed.  The staging buffers go too: a new ring sizes its own.
int stream_end(agx_ocp *o) {
  if (!o->streamed) return 0;
  HIPCHK(hipStreamSynchronize(o->copy_stream));
  for (int i = 0; i < 2; ++i) {
    o->own.release(&o->d_st_stage[i]);
    o->own.release(&o->st_host[i]);
    o->st_used[i] = o->st_pending[i] = false;
  }
  o->streamed = false;
  o->st_last.buf = -1;
  o->st_cap = o->st_span = o->st_first = o->st_end = o->st_chunk = 0;
  return 0;
}
// next event of the timing pairs of `kind`, recorded on `s` (events are created once and reused after every read-out)
int stream_time_mark(agx_ocp *o, int kind, hipStream_t s) {
  if (!o->st_timing) return 0;
  if (o->st_tev_used[kind] == o->st_tev[kind].size()) {
    o->st_tev[kind].push_back(nullptr);
    HIPCHK(o->own.event(&o->st_tev[kind].back()));
  }
  HIPCHK(hipEventRecord(o->st_tev[kind][o->st_tev_used[kind]++], s));
  return 0;
}
// Transfer of the staged piece o->st_last and fill of its slots, on the copy stream.  behind_solver: the fill waits for what the
// solver stream holds at this moment, which may still read the slots released since (the transfer need not wait: the device
// half of a staging buffer is read by fills of the copy stream only).
int stream_enqueue_last(agx_ocp *o, bool behind_solver) {
  const auto &L = o->st_last;
  if (behind_solver && stream_time_mark(o, 1, o->copy_stream)) return -1;
  HIPCHK(hipMemcpyAsync(o->d_st_stage[L.buf], o->st_host[L.buf], sizeof(double) * L.used, hipMemcpyHostToDevice, o->copy_stream));
  if (behind_solver) {
    HIPCHK(hipEventRecord(o->ev_st_solver, o->stream));
    HIPCHK(hipStreamWaitEvent(o->copy_stream, o->ev_st_solver, 0));
  }
  const long long units = (long long)o->B * L.m;
  int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    hipLaunchKernelGGL((agx::k_traj_append<NV, CH>), dim3((unsigned)((units + 63) / 64)), dim3(64), 0, o->copy_stream, o->d_model, o->d_ocp, L.sp, o->d_traj,
                       o->d_pts, L.m, L.end, o->st_cap, o->st_span - 1);
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  if (o->cost_wide)
    HIPCHK((hipError_t)agx_cost_pairs_fill_ring_launch((void *)o->copy_stream, o->d_cw, L.sp.gw_item, o->d_traj, o->B, L.m, L.end, o->st_cap, o->st_span - 1,
                                                       o->stride));
  if (behind_solver && stream_time_mark(o, 1, o->copy_stream)) return -1;
  return 0;
}
// The solver stream waits (the host does not) for every append not yet joined that wrote a sample below `upto`.
int stream_join(agx_ocp *o, int upto) {
  for (int n = 0; n < 2; ++n) {
    const int i = (o->st_next + n) % 2;  // the older buffer first
    if (o->st_pending[i] && o->st_lo[i] < upto) {
      if (stream_time_mark(o, 0, o->stream)) return -1;
      HIPCHK(hipStreamWaitEvent(o->stream, o->ev_st[i], 0));
      if (stream_time_mark(o, 0, o->stream)) return -1;
      o->st_pending[i] = false;
      ++o->st_joins;
    }
  }
  return 0;
}
// Sample index of a resident trajectory as the kernels and copies address it: `k` itself, or on a streamed ring the slot of
// logical sample k, with the samples [k, k + span) required inside [first, end) and their appends joined.
int traj_locate(agx_ocp *o, const char *fn, const char *what, int k, int span, int *phys) {
  if (!o->streamed) {
    if (k < 0 || (long long)k + span > o->n_points) return fail(std::string(fn) + ": " + what);
    *phys = k;
    return 0;
  }
  if (k < o->st_first || (long long)k + span > o->st_end)
    return fail(std::string(fn) + ": samples [" + std::to_string(k) + ", " + std::to_string((long long)k + span) + ") are not inside the retained range [first, end) = [" +
                std::to_string(o->st_first) + ", " + std::to_string(o->st_end) + ") of the streamed trajectory");
  if (stream_join(o, k + span)) return -1;
  *phys = k % o->st_cap;
  return 0;
}

}  // namespace

extern "C" {

// Wide cost sets: k_sine_fill has written the rows of the prefix; the pair rows of every sample get [row.weight (or the scheduled
// item weight gw_item [B][n_points], device) | 1].
static int traj_fill_pairs(agx_ocp *o, int n_points, const double *d_gw_item) {
  if (!o->cost_wide) return 0;
  const long long units = (long long)o->B * n_points;
  HIPCHK((hipError_t)agx_cost_pairs_fill_launch((void *)o->stream, o->d_cw, d_gw_item, o->d_traj, units, o->stride));
  return 0;
}

// The resident generators track ONE end-effector frame: frame-based cost rows look at it on every node
// (what the host path does per node with `obj.id = ...`, ocp_croco_generic.py:208).
static int traj_frames(agx_ocp *o, int frame) {
  std::vector<int> fr((size_t)o->B * (o->T + 1) * AGX_MAX_ROWS, -1);
  for (int b = 0; b < o->B; ++b)
    for (int t = 0; t <= o->T; ++t) {
      const DevRows &rows = o->ho.rows[t == o->T ? 1 : 0];
      for (int r = 0; r < rows.n; ++r)
        if (rows.kind[r] == AGX_RES_FRAME_PLACEMENT || rows.kind[r] == AGX_RES_FRAME_TRANSLATION || rows.kind[r] == AGX_RES_FRAME_ROTATION)
          fr[((size_t)b * (o->T + 1) + t) * AGX_MAX_ROWS + r] = frame;
    }
  HIPCHK(hipMemcpyAsync(o->d_frames, fr.data(), sizeof(int) * fr.size(), hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  o->frames_set = true;
  o->frames_uniform = true;
  return 0;
}

// ---- the steps every creator of a resident trajectory goes through -----------------------------------------------------------
// The checks the generators share, in this order (`too_short`: what a trajectory below T + 1 samples is told).
static int traj_check(const agx_ocp *o, const std::string &name, int n_points, int frame, const char *too_short = "trajectory shorter than the horizon") {
  if (n_points < o->T + 1) return fail(name + ": " + too_short);
  if (frame < 0 || frame >= o->hm.nframes) return fail(name + ": frame id out of range");
  return 0;
}

// Nothing of a resident trajectory stays behind: agx_traj_set_window / agx_ocp_mpc_step refuse the handle until a creator succeeds.
static void traj_drop(agx_ocp *o) {
  o->own.release(&o->d_traj);
  o->own.release(&o->d_pts);
  o->own.release(&o->d_sine);
  o->n_points = 0;
}

// Behind a creator's checks: the handle leaves the tile carry and the streamed ring (stream_end waits for the fills that still
// write the old arrays), drops the trajectory it has and gets d_traj / d_pts for n_slots samples.  n_points stays 0 until the
// trajectory is complete, and the solver looks at the handle's own tile until a window is set.
static int traj_begin(agx_ocp *o, size_t n_slots) {
  if (set_device(o) || carry_invalidate(o) || stream_end(o)) return -1;
  traj_drop(o);
  rv_own_tile(o, nullptr);
  const size_t B = o->B, nv = o->nv;
  hipError_t e = o->own.device(&o->d_traj, B * n_slots * 2 * o->stride);
  if (e == hipSuccess) e = o->own.device(&o->d_pts, B * n_slots * (4 * nv + 12));
  if (e == hipSuccess) return 0;
  traj_drop(o);
  return fail(std::string("hipMalloc of the resident trajectory: ") + hipGetErrorString(e));
}

// A build between traj_begin and its last step: whatever way a creator leaves before that, the half-built trajectory is dropped.
struct TrajBuild {
  agx_ocp *o; bool complete = false;
  ~TrajBuild() { if (!complete) traj_drop(o); }
  // Last step of the generators, behind k_sine_fill: pair rows, frame table, then the trajectory exists and window 0 is set.
  int finish(const agx::SineParams &sp) {
    if (traj_fill_pairs(o, sp.n_points, sp.gw_item)) return -1;
    HIPCHK(hipStreamSynchronize(o->stream));
    if (traj_frames(o, sp.frame)) return -1;
    o->n_points = sp.n_points;
    complete = true;  // the trajectory stands, whatever the window says (horizon indexes set earlier may reach past it)
    return agx_traj_set_window(o, 0);
  }
};

// Weights, frame and length of the samples a creator fills (everything else zero; w_pose may be null: per-sample pose weights).
static agx::SineParams traj_params(const agx_ocp *o, const double *w_q, const double *w_qdot, const double *w_effort, const double *w_pose, int frame,
                                   int n_points) {
  agx::SineParams sp;
  std::memset(&sp, 0, sizeof(sp));
  for (int i = 0; i < o->nv; ++i) {  // pad joints: weight 1 on an identically zero residual
    const bool real = i < o->nvu;
    sp.w_q[i] = real ? w_q[i] : 1.0; sp.w_qdot[i] = real ? w_qdot[i] : 1.0; sp.w_effort[i] = real ? w_effort[i] : 1.0;
  }
  if (w_pose)
    for (int i = 0; i < 6; ++i) sp.w_pose[i] = w_pose[i];
  sp.n_points = n_points; sp.frame = frame;
  return sp;
}

// k_sine_fill over the sp.n_points samples of every instance: reference tiles into d_traj, samples into d_pts
static int traj_fill(agx_ocp *o, const agx::SineParams &sp) {
  return dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    const long long units = (long long)o->B * sp.n_points;
    hipLaunchKernelGGL((agx::k_sine_fill<NV, CH>), dim3((int)((units + 63) / 64)), dim3(64), 0, o->stream, o->d_model, o->d_ocp, sp, o->d_traj, o->d_pts);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

int agx_traj_sine_create(agx_ocp *o, int n_points, double dt, const double *q0, const double *amp, const double *pulsation,
                         const double *scale_duration, const double *t0, const double *w_q, const double *w_qdot,
                         const double *w_effort, const double *w_pose, int frame) {
  if (!o || !q0 || !amp || !pulsation || !scale_duration || !t0 || !w_q || !w_qdot || !w_effort || !w_pose)
    return fail("agx_traj_sine_create: null argument");
  if (traj_check(o, "agx_traj_sine_create", n_points, frame, "need at least T+1 samples")) return -1;
  if (traj_begin(o, n_points)) return -1;
  TrajBuild build{o};
  const size_t B = o->B, nv = o->nv;
  HIPCHK(o->own.device(&o->d_sine, 4 * B * nv + B));
  double *d = o->d_sine;
  // pad joints: amplitude 0 (they stay at rest), scale duration 1 (it divides)
  if (up(o, d, q0, B, 1) || up(o, d + B * nv, amp, B, 1) || up(o, d + 2 * B * nv, pulsation, B, 1) || up(o, d + 3 * B * nv, scale_duration, B, 1, 1.0)) return -1;
  HIPCHK(hipMemcpyAsync(d + 4 * B * nv, t0, sizeof(double) * B, hipMemcpyHostToDevice, o->stream));
  agx::SineParams sp = traj_params(o, w_q, w_qdot, w_effort, w_pose, frame, n_points);
  sp.q0 = d; sp.amp = d + B * nv; sp.puls = d + 2 * B * nv; sp.scale = d + 3 * B * nv; sp.t0 = d + 4 * B * nv;
  sp.dt = dt;
  if (traj_fill(o, sp)) return -1;
  return build.finish(sp);
}

// The caller-fed resident trajectory behind agx_traj_generic_create / agx_traj_generic_create_weighted (`fn`: the entry point, for
// the messages).  pose / gw_pose / gw_item: optional per-sample arrays [B][n_points][12] / [6] / [1] (host); w_pose: the constant
// pose weights used without gw_pose.
static int traj_generic_build(agx_ocp *o, const char *fn, int n_points, const double *q, const double *dq, const double *ddq,
                              const double *w_q, const double *w_qdot, const double *w_effort, const double *w_pose, int frame,
                              const double *pose, const double *gw_pose, const double *gw_item) {
  if (traj_check(o, fn, n_points, frame)) return -1;
  if (traj_begin(o, n_points)) return -1;
  TrajBuild build{o};
  const size_t B = o->B, nv = o->nv, np = B * (size_t)n_points, n = np * nv;
  // q | dq | ddq samples, then the optional per-sample poses, pose weights and collision item weights
  HIPCHK(o->own.device(&o->d_sine, 3 * n + (pose ? 12 * np : 0) + (gw_pose ? 6 * np : 0) + (gw_item ? np : 0)));
  double *d = o->d_sine;
  if (up(o, d, q, np, 1) || up(o, d + n, dq, np, 1) || up(o, d + 2 * n, ddq, np, 1)) return -1;
  agx::SineParams sp = traj_params(o, w_q, w_qdot, w_effort, w_pose, frame, n_points);
  sp.gq = d; sp.gdq = d + n; sp.gddq = d + 2 * n;
  double *extra = d + 3 * n;
  if (pose) {
    HIPCHK(hipMemcpyAsync(extra, pose, sizeof(double) * 12 * np, hipMemcpyHostToDevice, o->stream));
    sp.gpose = extra; extra += 12 * np;
  }
  if (gw_pose) {
    HIPCHK(hipMemcpyAsync(extra, gw_pose, sizeof(double) * 6 * np, hipMemcpyHostToDevice, o->stream));
    sp.gw_pose = extra; extra += 6 * np;
  }
  if (gw_item) {
    HIPCHK(hipMemcpyAsync(extra, gw_item, sizeof(double) * np, hipMemcpyHostToDevice, o->stream));
    sp.gw_item = extra;
  }
  if (traj_fill(o, sp)) return -1;
  return build.finish(sp);
}

int agx_traj_generic_create(agx_ocp *o, int n_points, const double *q, const double *dq, const double *ddq, const double *w_q,
                            const double *w_qdot, const double *w_effort, const double *w_pose, int frame) {
  if (!o || !q || !dq || !ddq || !w_q || !w_qdot || !w_effort || !w_pose) return fail("agx_traj_generic_create: null argument");
  return traj_generic_build(o, "agx_traj_generic_create", n_points, q, dq, ddq, w_q, w_qdot, w_effort, w_pose, frame, nullptr, nullptr, nullptr);
}

int agx_traj_generic_create_weighted(agx_ocp *o, int n_points, const double *q, const double *dq, const double *ddq, const double *w_q,
                                     const double *w_qdot, const double *w_effort, int frame, const double *pose, const double *w_pose,
                                     const double *w_collision) {
  if (!o || !q || !dq || !ddq || !w_q || !w_qdot || !w_effort || !w_pose) return fail("agx_traj_generic_create_weighted: null argument");
  return traj_generic_build(o, "agx_traj_generic_create_weighted", n_points, q, dq, ddq, w_q, w_qdot, w_effort, nullptr, frame, pose, w_pose,
                            w_collision);
}

// The Cartesian sine generators: `period` null = agx_traj_cartesian_sine_create, set = the weight-increasing variant (`fn`: the entry
// point, for the messages).
static int traj_cartesian_build(agx_ocp *o, const char *fn, int n_points, double dt, const double *q0, const double *amp, const double *pulsation,
                                double scale_duration, double precision, int it_max, const double *w_q, const double *w_qdot,
                                const double *w_effort, const double *w_pose, int frame, const double *period, double max_weight, double rate) {
  const std::string name(fn);
  if (traj_check(o, name, n_points, frame)) return -1;
  if (!(scale_duration > 0.0) || !(precision > 0.0) || it_max < 1) return fail(name + ": scale_duration, precision, it_max must be positive");
  if (o->nv > 7) return fail(name + ": nv <= 7");
  if (period) {
    for (size_t i = 0; i < (size_t)o->B * 3; ++i)
      if (!(period[i] > 0.0) || !std::isfinite(period[i])) return fail(name + ": periods must be positive");
    if (!std::isfinite(max_weight) || !std::isfinite(rate)) return fail(name + ": max_weight and rate must be finite");
  }
  if (traj_begin(o, n_points)) return -1;
  TrajBuild build{o};
  const size_t B = o->B, nv = o->nv, n = B * (size_t)n_points * nv;
  // q | dq | ddq samples, then the per-instance parameters q0 | amp | pulsation | period, the poses, the scheduled pose weights
  // (weight-increasing variant) and the failure flags
  const size_t npar = B * (nv + 9), npose = B * (size_t)n_points * 12, nw = period ? B * (size_t)n_points * 6 : 0;
  HIPCHK(o->own.device_bytes((void **)&o->d_sine, sizeof(double) * (3 * n + npar + npose + nw) + sizeof(int) * B));
  double *d = o->d_sine, *dpar = d + 3 * n, *dpose = dpar + npar, *dw = dpose + npose;
  int *dfail = reinterpret_cast<int *>(dw + nw);
  HIPCHK(hipMemsetAsync(d + 2 * n, 0, sizeof(double) * n, o->stream));  // ddq = 0
  if (up(o, dpar, q0, B, 1)) return -1;
  HIPCHK(hipMemcpyAsync(dpar + B * nv, amp, sizeof(double) * B * 3, hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipMemcpyAsync(dpar + B * nv + B * 3, pulsation, sizeof(double) * B * 3, hipMemcpyHostToDevice, o->stream));
  if (period) HIPCHK(hipMemcpyAsync(dpar + B * nv + B * 6, period, sizeof(double) * B * 3, hipMemcpyHostToDevice, o->stream));
  agx::CartSineParams cp;
  std::memset(&cp, 0, sizeof(cp));
  cp.q0 = dpar; cp.amp = dpar + B * nv; cp.puls = dpar + B * nv + B * 3;
  cp.dt = dt; cp.scale = scale_duration; cp.precision = precision;
  cp.n_points = n_points; cp.frame = frame; cp.it_max = it_max;
  cp.q = d; cp.dq = d + n; cp.pose = dpose; cp.fail = dfail;
  if (period) {
    cp.period = dpar + B * nv + B * 6; cp.max_weight = max_weight; cp.rate = rate; cp.wpose = dw;
    for (int i = 0; i < 3; ++i) cp.w_rot[i] = w_pose[3 + i];
  }
  agx::SineParams sp = traj_params(o, w_q, w_qdot, w_effort, w_pose, frame, n_points);
  sp.gq = d; sp.gdq = d + n; sp.gddq = d + 2 * n;
  sp.gpose = dpose;
  if (period) sp.gw_pose = dw;
  const int rc = dispatch(o->nv, o->chain, [&](auto NVc, auto CHc) -> int {
    constexpr int NV = decltype(NVc)::value;
    constexpr bool CH = decltype(CHc)::value;
    if constexpr (NV <= 7) {
      if (period) hipLaunchKernelGGL((agx::k_cartesian_sine_ik<NV, CH, true>), dim3((int)((B + 63) / 64)), dim3(64), 0, o->stream, o->d_model, (int)B, cp);
      else hipLaunchKernelGGL((agx::k_cartesian_sine_ik<NV, CH>), dim3((int)((B + 63) / 64)), dim3(64), 0, o->stream, o->d_model, (int)B, cp);
    }
    HIPCHK(hipGetLastError());
    return 0;
  });
  if (rc || traj_fill(o, sp)) return -1;
  std::vector<int> failed(B);
  HIPCHK(hipMemcpyAsync(failed.data(), dfail, sizeof(int) * B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  for (size_t b = 0; b < B; ++b)
    if (failed[b]) {  // (the build ends here: nothing half-built stays behind)
      char msg[160];
      std::snprintf(msg, sizeof(msg), "inverse kinematics failed to converge: instance %zu at point %d (it_max %d)", b, failed[b] - 1, it_max);
      return fail(msg);
    }
  return build.finish(sp);
}

int agx_traj_cartesian_sine_create(agx_ocp *o, int n_points, double dt, const double *q0, const double *amp, const double *pulsation,
                                   double scale_duration, double precision, int it_max, const double *w_q, const double *w_qdot,
                                   const double *w_effort, const double *w_pose, int frame) {
  if (!o || !q0 || !amp || !pulsation || !w_q || !w_qdot || !w_effort || !w_pose) return fail("agx_traj_cartesian_sine_create: null argument");
  return traj_cartesian_build(o, "agx_traj_cartesian_sine_create", n_points, dt, q0, amp, pulsation, scale_duration, precision, it_max, w_q, w_qdot,
                              w_effort, w_pose, frame, nullptr, 0.0, 0.0);
}

int agx_traj_cartesian_sine_wi_create(agx_ocp *o, int n_points, double dt, const double *q0, const double *amp, const double *pulsation,
                                      double scale_duration, double precision, int it_max, const double *w_q, const double *w_qdot,
                                      const double *w_effort, const double *w_pose, int frame, const double *period, double max_weight,
                                      double rate) {
  if (!o || !q0 || !amp || !pulsation || !w_q || !w_qdot || !w_effort || !w_pose || !period)
    return fail("agx_traj_cartesian_sine_wi_create: null argument");
  return traj_cartesian_build(o, "agx_traj_cartesian_sine_wi_create", n_points, dt, q0, amp, pulsation, scale_duration, precision, it_max, w_q,
                              w_qdot, w_effort, w_pose, frame, period, max_weight, rate);
}

int agx_traj_set_horizon_indexes(agx_ocp *o, const int32_t *idx) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  if (o->streamed && idx && idx[o->T] >= 0 && idx[o->T] + 1 > o->st_span)
    return fail("agx_traj_set_horizon_indexes: the window covers idx[T] + 1 = " + std::to_string(idx[o->T] + 1) + " samples, the streamed trajectory was created with max_span " +
                std::to_string(o->st_span));
  if (carry_invalidate(o)) return -1;
  o->hidx.clear();
  if (!idx) return 0;  // back to uniform
  bool uniform = true;
  for (int t = 0; t <= o->T; ++t) {
    if (idx[t] < 0 || (t > 0 && idx[t] <= idx[t - 1])) return fail("agx_traj_set_horizon_indexes: indexes must be non-negative and increasing");
    uniform = uniform && idx[t] == t;
  }
  if (uniform) return 0;
  o->hidx.assign(idx, idx + o->T + 1);
  if (!o->d_hidx) HIPCHK(o->own.device(&o->d_hidx, (size_t)o->T + 1));
  HIPCHK(hipMemcpyAsync(o->d_hidx, o->hidx.data(), sizeof(int) * (o->T + 1), hipMemcpyHostToDevice, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  return 0;
}

int agx_traj_set_window(agx_ocp *o, int k0) {
  if (!o) return fail("null handle");
  if (!o->d_traj) return fail("agx_traj_set_window: no resident trajectory");
  const int last = o->hidx.empty() ? o->T : o->hidx[o->T];
  if (o->streamed && set_device(o)) return -1;
  const int k0_logical = k0;
  if (traj_locate(o, "agx_traj_set_window", "window leaves the trajectory", k0_logical, last + 1, &k0)) return -1;
  o->win_logical = k0_logical;
  o->win_k0 = k0;
  o->rv.frames = o->d_frames;
  if (o->hidx.empty()) {
    o->rv.base = o->d_traj + (long long)k0 * 2 * o->stride;
    o->rv.bstride = (long long)o->n_points * 2 * o->stride;
    o->rv.tstride = 2 * o->stride;
    o->rv.term_off = o->stride;
    return 0;
  }
  if (set_device(o)) return -1;
  const long long n = (long long)o->B * (o->T + 1) * o->stride;
  hipLaunchKernelGGL(agx::k_gather_window, dim3((int)((n + 255) / 256)), dim3(256), 0, o->stream, o->d_traj, o->d_ref, o->d_hidx, o->B, o->T,
                     o->stride, o->n_points, k0);
  HIPCHK(hipGetLastError());
  rv_own_tile(o, o->d_frames);
  return 0;
}

int agx_traj_get_point(agx_ocp *o, int k, double *q, double *v, double *a, double *u, double *pose) {
  if (!o || !o->d_pts) return fail("agx_traj_get_point: no resident trajectory");
  if (set_device(o)) return -1;
  if (traj_locate(o, "agx_traj_get_point", "sample out of range", k, 1, &k)) return -1;
  const size_t B = o->B, nv = o->nv, w = 4 * nv + 12;
  std::vector<double> h(B * w);
  HIPCHK(hipMemcpy2DAsync(h.data(), sizeof(double) * w, o->d_pts + (size_t)k * w, sizeof(double) * o->n_points * w, sizeof(double) * w, B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  for (size_t b = 0; b < B; ++b) {
    const double *p = &h[b * w];
    const size_t nvu = o->nvu;  // the sample's joint blocks hold nv (capacity) entries, the caller's nvu
    if (q) std::memcpy(q + b * nvu, p, sizeof(double) * nvu);
    if (v) std::memcpy(v + b * nvu, p + nv, sizeof(double) * nvu);
    if (a) std::memcpy(a + b * nvu, p + 2 * nv, sizeof(double) * nvu);
    if (u) std::memcpy(u + b * nvu, p + 3 * nv, sizeof(double) * nvu);
    if (pose) std::memcpy(pose + b * 12, p + 4 * nv, sizeof(double) * 12);
  }
  return 0;
}

int agx_traj_get_tile(agx_ocp *o, int k, int terminal, double *out) {
  if (!o || !out) return fail("agx_traj_get_tile: null argument");
  if (!o->d_traj) return fail("agx_traj_get_tile: no resident trajectory");
  if (set_device(o)) return -1;
  if (traj_locate(o, "agx_traj_get_tile", "sample out of range", k, 1, &k)) return -1;
  if (carry_invalidate(o)) return -1;
  const size_t B = o->B, st = o->stride, su = o->stride_u;
  const int lay = terminal ? 1 : 0;
  std::vector<double> h(B * st);
  HIPCHK(hipMemcpy2DAsync(h.data(), sizeof(double) * st, o->d_traj + ((size_t)k * 2 + lay) * st, sizeof(double) * o->n_points * 2 * st,
                          sizeof(double) * st, B, hipMemcpyDeviceToHost, o->stream));
  HIPCHK(hipStreamSynchronize(o->stream));
  // the generators write the rows of the layout; what lies behind them in a slot of `stride` doubles is returned as zeros
  const DevRows &R = o->ho.rows[lay];
  const size_t used = (R.n ? (size_t)R.off[R.n - 1] + 1 + R.nref[R.n - 1] + R.nr[R.n - 1] : 0) + 2 * (size_t)o->hw.lay[lay].n;  // + the pair rows of a wide cost set
  std::memset(out, 0, sizeof(double) * B * su);
  for (size_t b = 0; b < B; ++b)
    for (size_t e = 0; e < used; ++e) {
      const int eu = o->padded ? o->refmap[lay][e] : (int)e;  // pad joints have no place in the caller's tile
      if (eu >= 0) out[b * su + eu] = h[b * st + e];
    }
  return 0;
}

static int ws_from_ref(agx_ocp *o, int k0, int set_x0) {
  const long long units = (long long)o->B * (o->T + 1);
  hipLaunchKernelGGL(agx::k_ws_from_ref, dim3((int)((units + 255) / 256)), dim3(256), 0, o->stream, o->d_xs, o->d_us, o->d_x0, o->d_pts,
                     o->B, o->T, o->nv, o->n_points, k0, set_x0, o->hidx.empty() ? nullptr : o->d_hidx);
  HIPCHK(hipGetLastError());
  return 0;
}

int agx_traj_warmstart_from_reference(agx_ocp *o) {
  if (!o || !o->d_pts) return fail("agx_traj_warmstart_from_reference: no resident trajectory");
  if (set_device(o)) return -1;
  if (o->streamed) {  // the window may have been released, or never set
    int phys = 0;
    if (o->win_logical < 0) return fail("agx_traj_warmstart_from_reference: no window set on the streamed trajectory");
    if (traj_locate(o, "agx_traj_warmstart_from_reference", "", o->win_logical, (o->hidx.empty() ? o->T : o->hidx[o->T]) + 1, &phys)) return -1;
  }
  if (carry_invalidate(o)) return -1;
  return ws_from_ref(o, o->win_k0, 1);
}

// ---- streamed resident trajectory ---------------------------------------------------------------------------------------------
// doubles one (instance, sample) of a staged chunk takes: q | dq | ddq at the capacity nv, pose 12, pose weights 6, collision weight 1
static size_t stream_sample_doubles(const agx_ocp *o) { return 3 * (size_t)o->nv + 19; }

int agx_traj_stream_create(agx_ocp *o, int capacity, int max_span, const double *w_q, const double *w_qdot, const double *w_effort,
                           const double *w_pose, int frame) {
  if (!o || !w_q || !w_qdot || !w_effort || !w_pose) return fail("agx_traj_stream_create: null argument");
  if (max_span < o->T + 1) return fail("agx_traj_stream_create: max_span " + std::to_string(max_span) + " is below the T + 1 = " + std::to_string(o->T + 1) + " samples of a window");
  if (capacity < max_span) return fail("agx_traj_stream_create: capacity " + std::to_string(capacity) + " is below max_span " + std::to_string(max_span));
  if (frame < 0 || frame >= o->hm.nframes) return fail("agx_traj_stream_create: frame id out of range");
  if ((long long)capacity + max_span - 1 > INT_MAX) return fail("agx_traj_stream_create: capacity + max_span - 1 does not fit an int");
  // horizon indexes set earlier stay with the handle: their window must fit the mirror too (agx_traj_set_horizon_indexes checks later ones)
  if (!o->hidx.empty() && o->hidx[o->T] + 1 > max_span)
    return fail("agx_traj_stream_create: the horizon indexes of the handle cover idx[T] + 1 = " + std::to_string(o->hidx[o->T] + 1) +
                " samples, max_span is " + std::to_string(max_span));
  // no window yet: the solver looks at the handle's own tile until agx_traj_set_window / agx_ocp_mpc_step finds one in the ring
  const size_t n_slots = (size_t)capacity + max_span - 1;
  if (traj_begin(o, n_slots)) return -1;
  TrajBuild build{o};
  if (ensure_copy_stream(o)) return -1;
  const size_t B = o->B, nv = o->nv;
  HIPCHK(hipMemsetAsync(o->d_traj, 0, sizeof(double) * B * n_slots * 2 * o->stride, o->stream));
  HIPCHK(hipMemsetAsync(o->d_pts, 0, sizeof(double) * B * n_slots * (4 * nv + 12), o->stream));
  o->st_chunk = max_span;
  const size_t stage = sizeof(double) * B * (size_t)o->st_chunk * stream_sample_doubles(o);
  for (int i = 0; i < 2; ++i) {
    HIPCHK(o->own.pinned(&o->st_host[i], stage, hipHostMallocDefault));
    HIPCHK(o->own.device_bytes((void **)&o->d_st_stage[i], stage));
    if (!o->ev_st[i]) HIPCHK(o->own.event(&o->ev_st[i], hipEventDisableTiming));
  }
  if (!o->ev_st_solver) HIPCHK(o->own.event(&o->ev_st_solver, hipEventDisableTiming));
  o->st_sp = traj_params(o, w_q, w_qdot, w_effort, w_pose, frame, (int)n_slots);
  o->st_cap = capacity; o->st_span = max_span; o->st_first = o->st_end = 0; o->st_next = 0;
  o->win_logical = -1;
  if (traj_frames(o, frame)) return -1;  // (waits for the solver stream: the ring is zeroed when this returns)
  o->n_points = (int)n_slots;
  o->streamed = true;
  build.complete = true;
  return 0;
}

int agx_traj_stream_timing(agx_ocp *o, int enable, double *ms_sum, long long *count) {
  if (!o) return fail("null handle");
  if (set_device(o)) return -1;
  // read out what has been recorded: both streams have to be through with it
  if (o->st_tev_used[0] || o->st_tev_used[1]) {
    HIPCHK(hipStreamSynchronize(o->stream));
    if (o->copy_stream) HIPCHK(hipStreamSynchronize(o->copy_stream));
    for (int kind = 0; kind < 2; ++kind) {
      for (size_t k = 0; k + 1 < o->st_tev_used[kind]; k += 2) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, o->st_tev[kind][k], o->st_tev[kind][k + 1]));
        o->st_tms[kind] += ms;
        o->st_tn[kind] += 1;
      }
      o->st_tev_used[kind] = 0;
    }
  }
  if (ms_sum && count)
    for (int kind = 0; kind < 2; ++kind) { ms_sum[kind] = o->st_tms[kind]; count[kind] = o->st_tn[kind]; }
  if ((enable != 0) != o->st_timing) {
    o->st_timing = enable != 0;
    for (int kind = 0; kind < 2; ++kind) { o->st_tms[kind] = 0.0; o->st_tn[kind] = 0; }
  }
  return 0;
}

int agx_traj_stream_append(agx_ocp *o, int m, const double *q, const double *dq, const double *ddq, const double *pose, const double *w_pose,
                           const double *w_collision) {
  if (!o || !q || !dq || !ddq) return fail("agx_traj_stream_append: null argument");
  if (!o->streamed) return fail("agx_traj_stream_append: the handle has no streamed trajectory (agx_traj_stream_create)");
  if (m < 1) return fail("agx_traj_stream_append: m must be at least 1");
  if (m > INT_MAX - o->st_end) return fail("agx_traj_stream_append: end + m does not fit an int (logical sample indexes are int)");
  if ((long long)o->st_end + m - o->st_first > o->st_cap)
    return fail("agx_traj_stream_append: " + std::to_string(m) + " more samples overflow the ring, release the past first (first " + std::to_string(o->st_first) +
                ", end " + std::to_string(o->st_end) + ", capacity " + std::to_string(o->st_cap) + ")");
  const size_t B = o->B, nv = o->nv, nvu = o->nvu, np = B * (size_t)m;
  struct { const double *a; size_t n; const char *name; } in[] = {{q, np * nvu, "q"}, {dq, np * nvu, "dq"}, {ddq, np * nvu, "ddq"}, {pose, np * 12, "pose"},
                                                               {w_pose, np * 6, "w_pose"}, {w_collision, np, "w_collision"}};
  for (const auto &c : in)
    if (c.a)
      for (size_t i = 0; i < c.n; ++i)
        if (!std::isfinite(c.a[i])) return fail(std::string("agx_traj_stream_append: non-finite value in ") + c.name + " (element " + std::to_string(i) + ")");
  if (set_device(o)) return -1;
  // pieces of at most st_chunk samples, one staging buffer each
  for (int j0 = 0; j0 < m; j0 += o->st_chunk) {
    const int mp = std::min(o->st_chunk, m - j0);
    const int i = o->st_next;
    // the buffer's previous piece: its copy and its fill have to be over before the host rewrites the page-locked half and the
    // copy stream the device half.  The fill is then complete for everybody: nothing is left to join.
    if (o->st_used[i]) {
      HIPCHK(hipEventSynchronize(o->ev_st[i]));
      o->st_pending[i] = false;
    }
    const size_t npp = B * (size_t)mp, n = npp * nv;
    double *h = o->st_host[i], *d = o->d_st_stage[i];
    const double *src3[3] = {q, dq, ddq};
    const bool whole = mp == m;  // one piece: the caller's [B][m] arrays have the layout of the chunk
    for (int a = 0; a < 3; ++a) {
      if (whole && !o->padded) { std::memcpy(h + a * n, src3[a], sizeof(double) * n); continue; }
      for (size_t b = 0; b < B; ++b)
        pad_rows(h + a * n + b * mp * nv, src3[a] + (b * m + j0) * nvu, (size_t)mp, 1, (int)nvu, (int)nv, 0.0);
    }
    size_t used = 3 * n;
    agx::SineParams sp = o->st_sp;
    sp.gq = d; sp.gdq = d + n; sp.gddq = d + 2 * n;
    struct { const double *a; size_t w; const double **dst; } opt[] = {{pose, 12, &sp.gpose}, {w_pose, 6, &sp.gw_pose}, {w_collision, 1, &sp.gw_item}};
    for (const auto &c : opt)
      if (c.a) {
        if (whole) std::memcpy(h + used, c.a, sizeof(double) * npp * c.w);
        else
          for (size_t b = 0; b < B; ++b) std::memcpy(h + used + b * mp * c.w, c.a + (b * m + j0) * c.w, sizeof(double) * mp * c.w);
        *c.dst = d + used;
        used += npp * c.w;
      }
    const int end = o->st_end;
    o->st_last.buf = i; o->st_last.m = mp; o->st_last.end = end; o->st_last.used = used; o->st_last.sp = sp;
    if (stream_enqueue_last(o, true)) return -1;
    HIPCHK(hipEventRecord(o->ev_st[i], o->copy_stream));
    o->st_used[i] = o->st_pending[i] = true;
    o->st_lo[i] = end;
    o->st_end = end + mp;
    o->st_next = 1 - i;
  }
  return 0;
}

int agx_traj_stream_release(agx_ocp *o, int k) {
  if (!o) return fail("null handle");
  if (!o->streamed) return fail("agx_traj_stream_release: the handle has no streamed trajectory (agx_traj_stream_create)");
  if (k < o->st_first || k > o->st_end)
    return fail("agx_traj_stream_release: " + std::to_string(k) + " is outside [first, end] = [" + std::to_string(o->st_first) + ", " + std::to_string(o->st_end) + "]");
  o->st_first = k;
  return 0;
}

int agx_traj_stream_joins(agx_ocp *o, long long *joins, int *pending) {
  if (!o) return fail("null handle");
  if (!o->streamed) return fail("agx_traj_stream_joins: the handle has no streamed trajectory (agx_traj_stream_create)");
  if (joins) *joins = o->st_joins;
  if (pending) *pending = (o->st_pending[0] ? 1 : 0) + (o->st_pending[1] ? 1 : 0);
  return 0;
}

int agx_traj_stream_range(agx_ocp *o, int *first, int *end) {
  if (!o) return fail("null handle");
  if (!o->streamed) return fail("agx_traj_stream_range: the handle has no streamed trajectory (agx_traj_stream_create)");
  if (first) *first = o->st_first;
  if (end) *end = o->st_end;
  return 0;
}

}  // extern "C"
