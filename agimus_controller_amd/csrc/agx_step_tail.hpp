// agx_step_tail.hpp -- forward pass, node KKT pass (K3) and head of the step of one SQP iteration in ONE launch, one workgroup
// of four waves per instance (7-joint capacity, unconstrained, one-wave sweeps; agx_ocp_set_step_tail, default on).
//
// The three phases are bound by three different things -- the forward pass is a dependent chain on one wave, K3 streams the
// aux tiles from HBM, the head is a latency chain per instance -- and as three launches each leaves idle what the others need.
// Here, per instance:
//   wave 0       riccati_forward as it is (same loads, arithmetic and stores); next to its stores it leaves (w[t], dx[t + 1]) in
//                LDS and publishes how many nodes are complete (an LDS word, workgroup-scope release) after every group of its
//                pipelined loop.  It never waits for the other waves.
//   waves 1 .. 3 the body of k_node_kkt_ahead on groups of eight consecutive nodes (wave w: groups w - 1, w + 2, ...): the 30 aux
//                rows, f and cost of the group -- none of which depends on the direction -- are issued first, then the wave
//                waits (s_sleep; the producer is resident by construction) until the forward pass covers the group, takes dx and
//                w from LDS and runs the products, row sums and butterflies unchanged.  du and the nodestat words go to global
//                memory as before (k_sqp_accept, k_iter_log and the trial rounds read them) and to LDS.
//   barrier; threads 0 .. 127 run k_sqp_head: same strided sums over t (stride 128), same wave_max / wave_sum, same red[]
//                combination, decision, counters, record packing and trial iterate at alpha = 1 -- with the shares, dx and du
//                out of LDS instead of a round trip through HBM.
// No operand, product or summation order changes: a solve hands out the same bits as with the three launches.
//
// LDS holds the first kTailCap nodes of an instance (36 KB, four workgroups per CU); whatever a longer horizon has beyond them is
// read back from the global arrays this very workgroup has written (visible to its own waves at workgroup scope).
#pragma once

namespace agx {

constexpr int kTailCap = 128;      // nodes of an instance whose dx / w / du / shares have an LDS copy
constexpr int kTailThreads = 256;  // wave 0: forward pass, waves 1 .. 3: K3
constexpr int kHeadThreads = 128;  // the head's part keeps the thread count (and with it the summation order) of k_sqp_head

// what wave 0 leaves in LDS (riccati_forward's TAP)
template <int NV>
struct FwdTailTap {
  double *s_dx, *s_w;
  int *s_prog;
  __device__ __forceinline__ void start(int lane) const {
    if (lane < NV) { s_dx[lane] = 0.0; s_dx[NV + lane] = 0.0; }
  }
  __device__ __forceinline__ void node(int t, int r, double wv, double nq, double nv2) const {
    if (t < kTailCap) {
      s_w[t * NV + r] = wv;
      s_dx[(t + 1) * 2 * NV + r] = nq;
      s_dx[(t + 1) * 2 * NV + NV + r] = nv2;
    }
  }
  // nodes 0 .. n - 1 are complete.  Release at workgroup scope by the whole wave: the LDS stores above (and the global ones,
  // for the nodes beyond kTailCap) are ordered before the word by the wait the fence stands for, not by a barrier.
  __device__ __forceinline__ void done_to(int n) const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (threadIdx.x == 0) __hip_atomic_store(s_prog, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

template <int NV>
__global__ void __launch_bounds__(kTailThreads, 4) k_step_tail(const DevOcp *__restrict__ op, const double *__restrict__ dts,
                                                               const double *__restrict__ qts, const double *__restrict__ auxs,
                                                               const double *__restrict__ Kws, const double *__restrict__ kws,
                                                               const double *__restrict__ xs, const double *__restrict__ us,
                                                               double *dxs, double *wss, double *dus,
                                                               double *__restrict__ xs_t, double *__restrict__ us_t,
                                                               double *nodestat, DevState *__restrict__ st, int iter, int max_iter,
                                                               int *__restrict__ n_done, HostWords hw, const double *__restrict__ Kout,
                                                               double *__restrict__ first, int first_stride) {
  static_assert(NV <= 7, "one 8 x 8 lane grid per instance, eight lanes per node");
  constexpr int NX = 2 * NV, NU = NV;
  typedef QT<NV> Q;
  typedef AUX<NV> A;
  __shared__ double s_dt[kMaxHorizon];
  __shared__ double s_dx[(kTailCap + 1) * NX];
  __shared__ double s_w[kTailCap * NV];
  __shared__ double s_du[kTailCap * NV];
  __shared__ double s_ns[(kTailCap + 1) * 3];  // kkt, cost, gap shares (the violation share of an unconstrained node is zero)
  __shared__ int s_prog;
  __shared__ double red[8];
  __shared__ double s_words[8];  // status words of a record packed here
  __shared__ int flag;
  const DevOcp &o = *op;
  const int T = o.T, b = blockIdx.x, tid = threadIdx.x;
  DevState &S = st[b];
  if (S.done) {  // (uniform over the workgroup) as the sweep, K3 and the head leave a finished instance
    if (tid == 0) arrive_and_publish(n_done, hw);
    return;
  }
  if (tid == 0) s_prog = 0;
  __syncthreads();
  const int nxs = (T + 1) * NX, nus = T * NU;
  const long long ox = (long long)b * nxs, ou = (long long)b * nus;
  double *dxb = dxs + ox, *wb = wss + ou, *dub = dus + ou, *nsb = nodestat + (long long)b * (T + 1) * 4;
  if (tid < 64) {
    stage_dts(s_dt, dts, T);
    const double *qb = qts + (long long)b * (T + 1) * Q::SIZE;
    riccati_forward<NV>(o, b, T, dts, qb, Kws + (long long)b * T * NV * NX, kws + (long long)b * T * NV, dxs, wss, s_dt,
                        FwdTailTap<NV>{s_dx, s_w, &s_prog});
  } else {
    const int l8 = tid & 7, wave = tid >> 6;
    const double preg = S.preg, dreg = S.dreg;
    const bool jl = l8 < NV;
    const int jj = jl ? l8 : 0;
    const int n_groups = (T + 8) >> 3;  // of the T + 1 nodes
    for (int g = wave - 1; g < n_groups; g += 3) {
      const int t_lane = 8 * g + ((tid & 63) >> 3);
      const bool act = t_lane <= T;  // (the lanes behind the terminal node work on node 0 and store nothing)
      const int t = act ? t_lane : 0;
      const long long sid = (long long)b * (T + 1) + tile_slot(o, t);
      const double *qt = qts + sid * Q::SIZE;
      const double *ax = auxs + sid * A::SIZE;
      // what does not depend on the direction: in flight before the wait
      const double fq_l = qt[Q::f + jj], fv_l = qt[Q::f + NV + jj];  // (the terminal tile carries zeros there)
      const double cost = qt[Q::cost];
      double rM[8] = {}, rtq[8] = {}, rtv[8] = {}, rLqq[8] = {}, rLuu = 0.0, rLvv = 0.0;
      if (t < T) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          rM[i] = ax[A::M + i * A::LD + l8]; rtq[i] = ax[A::tq + i * A::LD + l8]; rtv[i] = ax[A::tv + i * A::LD + l8];
        }
        rLuu = ax[A::Luu + l8];
      }
      if (t > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) rLqq[i] = ax[A::Lqq + i * A::LD + l8];
        rLvv = ax[A::Lvv + l8];
      }
      // the group needs dx[t] of its nodes and w[t] of its running ones: the forward pass complete up to its last node
      const int need = 8 * g + 8 < T ? 8 * g + 8 : T;
      while (__hip_atomic_load(&s_prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(2);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      double dq_l, dv_l, wj_l = 0.0;
      if (t <= kTailCap) { dq_l = s_dx[t * NX + jj]; dv_l = s_dx[t * NX + NV + jj]; }
      else { dq_l = dxb[t * NX + jj]; dv_l = dxb[t * NX + NV + jj]; }
      if (t < T) wj_l = t < kTailCap ? s_w[t * NV + jj] : wb[t * NV + jj];
      // from here on the arithmetic of k_node_kkt_ahead
      const double dq = jl ? dq_l : 0.0, dv = jl ? dv_l : 0.0;
      double kkt = 0.0, gap = 0.0;
      if (t < T) {
        const double wj = jl ? wj_l : 0.0;
        const double fq = jl ? fq_l : 0.0, fv = jl ? fv_l : 0.0;
        kkt = fmax(fabs(fq), fabs(fv));
        gap = fabs(fq) + fabs(fv);
        double pr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) pr[i] = (i < NV) ? rM[i] * wj + rtq[i] * dq + rtv[i] * dv : 0.0;
        const double du = transpose_reduce8(pr, l8);
        if (jl) {
          if (act) {
            dub[t * NV + l8] = du;
            if (t < kTailCap) s_du[t * NV + l8] = du;
          }
          kkt = fmax(kkt, fabs((rLuu + preg) * du));
        }
      }
      if (t > 0) {
        double pr[8];
AGX_UNROLL_NV
        for (int i = 0; i < 8; ++i) pr[i] = (i < NV) ? rLqq[i] * dq : 0.0;
        const double hq = transpose_reduce8(pr, l8);
        if (jl) kkt = fmax(kkt, fmax(fabs(hq + dreg * dq), fabs((rLvv + dreg) * dv)));
      }
      // group max / sum (fixed order: deterministic)
      kkt = fmax(kkt, dpp_xor4(kkt)); kkt = fmax(kkt, dpp_xor2(kkt)); kkt = fmax(kkt, dpp_xor1(kkt));
      gap += dpp_xor4(gap); gap += dpp_xor2(gap); gap += dpp_xor1(gap);
      if (act && l8 == 0) {
        double *ns = nsb + t * 4;
        ns[0] = kkt; ns[1] = cost; ns[2] = gap; ns[3] = 0.0;
        if (t <= kTailCap) { s_ns[t * 3 + 0] = kkt; s_ns[t * 3 + 1] = cost; s_ns[t * 3 + 2] = gap; }
      }
    }
  }
  __syncthreads();  // every share, du and dx of the instance is there (LDS, and global memory at workgroup scope)

  // ---- the head of the step (k_sqp_head with the line search on), on threads 0 .. kHeadThreads - 1; the other two waves only
  // keep the barriers company
  const bool hd = tid < kHeadThreads;
  // operands of the first trial iterate that are not in LDS, in flight during the reduction and the decision
  double px[kPrefX], pu[kPrefU];
#pragma unroll
  for (int k = 0; k < kPrefX; ++k) {
    const int e = tid + k * kHeadThreads;
    px[k] = (hd && e < nxs) ? xs[ox + e] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < kPrefU; ++k) {
    const int e = tid + k * kHeadThreads;
    pu[k] = (hd && e < nus) ? us[ou + e] : 0.0;
  }
  auto dx_at = [&](int e) -> double { return e < (kTailCap + 1) * NX ? s_dx[e] : dxb[e]; };
  auto du_at = [&](int e) -> double { return e < kTailCap * NV ? s_du[e] : dub[e]; };
  // likewise the first workgroup stride of the record [us0 | K0 | x1 | words] this instance packs if it converges (all of it)
  constexpr int NK = NU * NX, FS = NU + NK + NX + 8;  // (FS == first_stride: the host passes the block only then)
  static_assert(FS <= kHeadThreads, "the record of the 7-joint capacity fits one stride of the head");
  const bool may_pack = first != nullptr && S.gains_iter == iter;  // (uniform over the workgroup)
  auto record_element = [&](int e) -> double {  // e < FS - 8
    if (e < NU) return us[ou + e];
    if (e < NU + NK) return Kout[(long long)b * T * NK + (e - NU)];
    return xs[ox + NX + (e - NU - NK)];
  };
  double prec = 0.0;
  if (may_pack && tid < FS - 8) prec = record_element(tid);
  if (hd) {
    double kkt = 0.0, csum = 0.0, gsum = 0.0, vsum = 0.0;
    for (int t = tid; t <= T; t += kHeadThreads) {
      if (t <= kTailCap) {
        kkt = fmax(kkt, s_ns[t * 3 + 0]);
        csum += s_ns[t * 3 + 1];
        gsum += s_ns[t * 3 + 2];
      } else {
        const double *ns = nsb + t * 4;
        kkt = fmax(kkt, ns[0]);
        csum += ns[1];
        gsum += ns[2];
      }
    }
    kkt = wave_max(kkt);
    csum = wave_sum(csum);
    gsum = wave_sum(gsum);
    vsum = wave_sum(vsum);
    if ((tid & 63) == 0) { red[tid >> 6] = kkt; red[2 + (tid >> 6)] = csum; red[4 + (tid >> 6)] = gsum; red[6 + (tid >> 6)] = vsum; }
  }
  __syncthreads();
  if (tid == 0) {
    double kk = fmax(red[0], red[1]);
    const double cc = red[2] + red[3], gg = red[4] + red[5], vv = red[6] + red[7];
    kk = fmax(kk, vv);  // checkKKTConditions: KKT = max(KKT, constraint_norm)
    const int dir_fail = S.dir_fail;
    S.carry = 0;  // inherited tiles served the first derivative pass of the solve only
    if (dir_fail) kk = __builtin_nan("");  // discarded direction: its KKT residual is undefined (never "converged")
    S.kkt = kk; S.cost = cc; S.gap = gg; S.con = vv; S.merit = cc + o.mu_dyn * gg + o.mu_con * vv;
    S.qp_iters = 1;
    S.admm_conv = 0;
    S.dir_iter = iter;
    if (!(kk == kk)) S.flags |= 1;
    const bool conv = kk <= o.tol;
    int what = 0;  // 0: nothing more, 1: line search starts, 2: first-node record packed here
    if (conv) {
      S.solved = 1; S.done = 1; S.iter = iter; S.tiles_ok = 1; atomicAdd(n_done, 1);  // (the tiles are those of the final iterate)
      if (may_pack) {
        what = 2;
        s_words[0] = kk; s_words[1] = cc; s_words[2] = S.merit; s_words[3] = gg;
        s_words[4] = iter; s_words[5] = S.qp_iters; s_words[6] = 1; s_words[7] = S.flags;
      }
    } else {
      S.tiles_ok = 0;
      if (dir_fail) { S.flags |= 4; sqp_iteration_end(S, false, 1.0 / 512.0, iter, max_iter, n_done); }
      else {
        what = 1;
        S.searching = 1;
        S.ls_n = 0;
        double pr = S.preg, dr = S.dreg;
        bool stop;
        reg_schedule(1.0, pr, dr, stop);
        S.preg_trial = pr;
      }
    }
    flag = what;
    count_carriable(S, n_done);
    if (what != 2) arrive_and_publish(n_done, hw);  // (the host wants the finished count; the trial iterate below is for the next kernel of the stream)
  }
  __syncthreads();
  if (flag == 2) {
    double *rec = first + (long long)b * first_stride;
    if (tid < FS) rec[tid] = tid < FS - 8 ? prec : s_words[tid - (FS - 8)];
    __syncthreads();
    if (tid == 0) {
      // as k_sqp_head: fenced at system scope only where the stamp that lets the host read comes out of this kernel
      if (hw.seq) __threadfence_system();
      atomicAdd(n_done + 7, 1);
      arrive_and_publish(n_done, hw);
    }
    return;
  }
  if (!flag || !hd) return;
  // write_trial_iterate at alpha = 1
#pragma unroll
  for (int k = 0; k < kPrefX; ++k) {
    const int e = tid + k * kHeadThreads;
    if (e < nxs) xs_t[ox + e] = px[k] + 1.0 * dx_at(e);
  }
  for (int e = tid + kPrefX * kHeadThreads; e < nxs; e += kHeadThreads) xs_t[ox + e] = xs[ox + e] + 1.0 * dx_at(e);
#pragma unroll
  for (int k = 0; k < kPrefU; ++k) {
    const int e = tid + k * kHeadThreads;
    if (e < nus) us_t[ou + e] = pu[k] + 1.0 * du_at(e);
  }
  for (int e = tid + kPrefU * kHeadThreads; e < nus; e += kHeadThreads) us_t[ou + e] = us[ou + e] + 1.0 * du_at(e);
}

// the paired sweeps of k_riccati_mx_pair with the direction wave's forward pass left to k_step_tail
template <int NV>
__global__ void __launch_bounds__(64, 2) k_riccati_mx_pair_sweeps(const DevOcp *__restrict__ op, const double *__restrict__ dts,
                                                                  const double *__restrict__ qts, const double *__restrict__ auxs,
                                                                  double *__restrict__ Kws, double *__restrict__ kws,
                                                                  double *__restrict__ dxs, double *__restrict__ wss,
                                                                  double *__restrict__ Kout, DevState *__restrict__ st, int iter) {
  const int grp = blockIdx.x >> 4, w16 = blockIdx.x & 15;  // placement: as k_riccati_mx_pair
  const int b = grp * 8 + (w16 & 7);
  if (b >= op->B) return;
  if (w16 >> 3)
    riccati_mx_body<NV, true>(b, op, dts, qts, auxs, Kws, kws, dxs, wss, Kout, st, 0, 1, iter);
  else
    riccati_mx_body<NV, false>(b, op, dts, qts, auxs, Kws, kws, dxs, wss, Kout, st, 0, 0, iter);
}

}  // namespace agx
