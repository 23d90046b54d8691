/*
 * agimus_hip.h -- C ABI of the MI355X-native OCP solve path (libagimus_hip.so).
 *
 * This is the drop-in boundary for the one hot path of agimus_controller:
 * OCPCrocoGeneric.solve() + warm-start shift + reference update.  Every entry
 * point cites the reference interface it replaces (paths are relative to the
 * upstream agimus_controller repository).  Plain pointers and sizes only: no
 * C++ types, no torch types.  All floating point is IEEE fp64, row-major.
 *
 * The same structures are consumed by oracle/ (the CPU checker), which is test
 * infrastructure and never part of the product path.
 *
 * Conventions
 *   nv = nq = nu        number of 1-DoF revolute joints (full actuation)
 *   nx = ndx = 2*nv     state x = [q; v]
 *   T                   number of controls (running nodes); T+1 states
 *   B                   batch: independent MPC instances resident on one GPU
 *   spatial vectors     [linear(3); angular(3)] (Pinocchio ordering)
 *   SE3 as 12 doubles   R row-major (9) then p (3)
 *
 * Status codes: 0 = ok, negative = error (message via agx_last_error()).
 * Handles are thread-compatible, not thread-safe.
 */
#ifndef AGIMUS_HIP_H
#define AGIMUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_MAX_ROWS 8   /* cost rows per node type (running / terminal) that are not collision rows of a wide cost set */
/* Wide cost sets (serial chains of revolute joints, at most 7 joints after padding): a node type may carry up to AGX_MAX_ROWS rows of any kind
 * followed by up to AGX_MAX_COST_PAIRS AGX_RES_COLLISION rows (soft collision avoidance, one row per collision pair).  The
 * rows stay plain agx_cost_row entries in table order and every collision row owns [item weight | activation weight] at its
 * table offset of the reference tile.  A set is wide when a node type has more than AGX_MAX_ROWS rows (AGX_COST_WIDE=1: any
 * set with a collision cost row that meets the conditions); its collision rows must be the trailing rows of the table, and
 * the handle takes no frame-id table (rows >= AGX_MAX_ROWS have no column in it).  Kernel: k_cost_pairs.                  */
#define AGX_MAX_COST_PAIRS 64
#define AGX_MAX_NV 32    /* joints a model table may have; kernels are compiled for nv in {1,2,3,4,6,7} (register-resident
                            path) and 30 (LDS path for large models); other sizes are refused by agx_ocp_create */
#define AGX_JOINT_REVOLUTE 0   /* agx_model_desc.joint_type */
#define AGX_JOINT_PRISMATIC 1

/* Residual kinds: class names of the YAML schema,
 * agimus_controller/agimus_controller/ocp/ocp_croco_generic.py:147-550.        */
enum agx_residual_kind {
  AGX_RES_STATE = 0,             /* ResidualModelState            :154 */
  AGX_RES_CONTROL = 1,           /* ResidualModelControl          :170 */
  AGX_RES_CONTROL_GRAV = 2,      /* ResidualModelControlGrav      :186 */
  AGX_RES_FRAME_PLACEMENT = 3,   /* ResidualModelFramePlacement   :198 (+Static :223, VisualServoing :436) */
  AGX_RES_FRAME_TRANSLATION = 4, /* ResidualModelFrameTranslation :252 (+Static :277) */
  AGX_RES_FRAME_ROTATION = 5,    /* ResidualModelFrameRotation    :306 (+Static :331) */
  AGX_RES_FRAME_VELOCITY = 6,    /* ResidualModelFrameVelocity    :360 (+Static :396) */
  AGX_RES_COLLISION = 7          /* ResidualDistanceCollision     :524 */
};

/* Activation kinds, ocp_croco_generic.py:93-143.                               */
enum agx_activation_kind {
  AGX_ACT_WEIGHTED_QUAD = 0, /* a = 1/2 sum w_j r_j^2 (also the default quad, w = 1) */
  AGX_ACT_EXP = 1,           /* colmpc ActivationModelExp(nr, alpha):     a = exp(-|r| / alpha)   */
  AGX_ACT_QUAD_EXP = 2       /* colmpc ActivationModelQuadExp(nr, alpha): a = exp(-|r|^2 / alpha) */
};
/* Exp / QuadExp: any residual but ControlGrav / FrameVelocity; |r| over the nr components of the row, diagonal second
 * derivative; the activation weights of the row's tile are ignored.  Forms recalled, parity against colmpc unpinned. */
/* ControlGrav / FrameVelocity cost rows (the rows with Lxu and dense Lxx blocks) are accepted at every capacity.  Up to 7
 * joints the one-lane-per-node kernels evaluate them; above (capacities 16 / 30 / 32) k_general_rows_wg adds them into the
 * tiles of the workgroup-per-node derivative pass and k_node_kkt_big_gen forms the KKT shares (agx_ocp_general_rows tells).
 * Above 7 joints such a cost row is refused together with any constraint.                                                 */

/* One CostModelSumItem (ocp_croco_generic.py:578-585) lowered to a table row.
 * Per-node data of the row lives in the reference tile (agx_ocp_set_refs):
 *   [ item weight (1) | reference (agx_row_nref) | activation weights (agx_row_nr) ]
 * rows are laid out back to back in table order.                               */
typedef struct agx_cost_row {
  int32_t kind;       /* agx_residual_kind                                      */
  int32_t activation; /* agx_activation_kind                                    */
  int32_t active;     /* CostModelSumItem.active                                */
  int32_t frame;      /* default frame id (may be overridden per node); collision: first geometry frame */
  int32_t frame_b;    /* collision: second geometry frame of the pair (:499-533);
                         FrameVelocity: reference frame 0 WORLD / 1 LOCAL / 2 LOCAL_WORLD_ALIGNED (:360-432) */
  int32_t pad_;
  double alpha;       /* Exp / QuadExp parameter                                */
  double weight;      /* CostModelSumItem.weight of the YAML: the item weight the device-resident
                         reference generators write (host tiles carry their own per node) */
} agx_cost_row;

/* One ConstraintListItem (ocp_croco_generic.py:554-647) lowered to a row:
 *   lower <= r(x, u) <= upper   with r one of the residual kinds above.
 * ConstraintModelControlLimit (:624-640) is the AGX_RES_CONTROL row with zero
 * reference and -/+ effort limit.  Constraints are not updated per node
 * (:720-721), so reference and bounds are static.  Every residual kind is
 * implemented (references laid out like the cost rows'; FrameVelocity: frame_b =
 * reference frame 0 WORLD / 1 LOCAL / 2 LOCAL_WORLD_ALIGNED); at most 4 rows and 8
 * components with a dense Jacobian (collision 1, translation / rotation 3,
 * placement / velocity 6, ControlGrav nv) per node type; residuals on u are
 * dropped at the terminal node.  Models above 7 joints (after padding to the compiled
 * capacity): State, Control, collision and frame translation / rotation / placement
 * rows, up to 104 components per node; FrameVelocity / ControlGrav constraint rows are refused, and so is any constraint
 * next to a FrameVelocity / ControlGrav cost row. */
typedef struct agx_constraint_row {
  int32_t kind;        /* agx_residual_kind                                     */
  int32_t active;      /* ConstraintListItem.active                             */
  int32_t frame;
  int32_t frame_b;     /* as in agx_cost_row                                    */
  const double *ref;   /* [agx_row_nref(kind)] or NULL = zeros                  */
  const double *lower; /* [agx_row_nr(kind)], -inf allowed                      */
  const double *upper; /* [agx_row_nr(kind)], +inf allowed                      */
} agx_constraint_row;

/* Robot description: what factory/robot_model.py:88-351 extracts from the URDF
 * (reduced model, armature :346-351), as a flat table.                         */
typedef struct agx_model_desc {
  int32_t nv;
  int32_t nframes;
  const int32_t *parent;         /* [nv]   parent joint, -1 = world            */
  const double *placement;       /* [nv][12] joint frame in parent joint frame  */
  const double *axis;            /* [nv][3]  unit axis, joint frame: of rotation (revolute), of translation (prismatic) */
  const double *mass;            /* [nv]                                        */
  const double *com;             /* [nv][3]  joint frame                        */
  const double *inertia;         /* [nv][9]  about com, joint frame             */
  const double *armature;        /* [nv]                                        */
  const double *effort_limit;    /* [nv]                                        */
  const double *gravity;         /* [3]      linear gravity, world              */
  const int32_t *frame_parent;   /* [nframes] parent joint, -1 = world          */
  const double *frame_placement; /* [nframes][12] in parent joint frame         */
  /* Collision geometry (factory/robot_model.py:261-302: cylinders become coal.Capsule(radius,
   * halfLength)): a geometry object is a frame (parent joint + placement) whose local z axis
   * carries the capsule segment; halflen = 0 is a sphere.  NULL = no geometry.  */
  const double *frame_radius;    /* [nframes]                                   */
  const double *frame_halflen;   /* [nframes]                                   */
  /* Box geometry (coal.Box is kept as is by factory/robot_model.py:296-302): half extents along the
   * frame's axes, all 0 = not a box.  Pairs box / capsule and box / sphere are supported, box / box
   * is refused by agx_ocp_create.  NULL = no boxes.                              */
  const double *frame_box;       /* [nframes][3]                                */
  /* Joint types.  A prismatic joint translates its frame by q along `axis`; its model takes the kernels of a tree of the same size
   * (the eight-lane kernels, wide cost / constraint sets and the tile carry need a serial chain of revolute joints).  Any other
   * value is refused by agx_model_create.                                        */
  const int32_t *joint_type;     /* [nv] 0 = revolute, 1 = prismatic (axis = unit direction of translation, joint frame); NULL = all revolute */
} agx_model_desc;

/* Shooting problem + solver knobs:
 * OCPCrocoGeneric.create_running_model_list/create_terminal_model
 * (ocp_croco_generic.py:798-812) and OCPBaseCroco.__init__
 * (ocp_base_croco.py:55-80), OCPParamsBaseCroco (ocp_param_base.py:31-85).     */
typedef struct agx_ocp_desc {
  int32_t horizon;                  /* T = n_controls                           */
  const double *dt;                 /* [T] timesteps; terminal node has dt = 0  */
  int32_t n_running_rows;
  const agx_cost_row *running_rows; /* [n_running_rows]                         */
  int32_t n_terminal_rows;
  const agx_cost_row *terminal_rows;
  double termination_tolerance;     /* KKT tolerance, ocp_param_base.py:54      */
  int32_t max_qp_iters;             /* ocp_param_base.py:53                     */
  double eps_abs, eps_rel;          /* ocp_param_base.py:60-61                  */
  double mu_dynamic, mu_constraint; /* merit penalties (mim_solvers defaults)   */
  int32_t use_filter_line_search;   /* ocp_param_base.py:64                     */
  int32_t n_running_constraints;
  const agx_constraint_row *running_constraints;
  int32_t n_terminal_constraints;
  const agx_constraint_row *terminal_constraints;
} agx_ocp_desc;

/* Per-instance solver report: OCPDebugData fields filled by
 * OCPBaseCroco.fill_debug_data (ocp_base_croco.py:134-140).                    */
typedef struct agx_status {
  double kkt;       /* solver.KKT                                               */
  double cost;      /* total cost at the returned point's last evaluation       */
  double merit;     /* merit at that evaluation                                 */
  double gap_norm;  /* l1 norm of the dynamics gaps at that evaluation          */
  int32_t iter;     /* solver.iter                                              */
  int32_t qp_iters; /* solver.qp_iters                                          */
  int32_t solved;   /* return value of solver.solve()                           */
  int32_t flags;    /* bit0: non-finite result / discarded direction, bit1: a line search failed (all ten step lengths), bit2: a step length was rejected (the search backtracked) */
} agx_status;

/* One SQP iteration of one instance, as the per-iteration solver log keeps it (agx_ocp_iter_log): the line mim_solvers'
 * CallbackVerbose prints per iteration (ocp_base_croco.py:77-80) minus ||(dx,du)||, which is not kept on the device, plus what
 * only this solver knows: the regularisation, discarded directions and rejected step lengths.                              */
typedef struct agx_iter_record {      /* 80 bytes */
  double kkt, cost, merit, gap_norm, constraint_norm; /* evaluation at the start of the iteration:
                                         what agx_status reports if the solve ends here */
  double step;        /* accepted step length 2^-n; 0 = the iteration took no step */
  double preg, dreg;  /* regularisation this iteration's direction was computed with */
  int32_t iter, qp_iters, trials, flags;
  /* trials: step lengths tried (1 .. 10; 0: no search).
     flags bit0: converged in this iteration; bit1: direction discarded (failed factorisation);
     bit2: all ten step lengths rejected; bit3: ended by cap / time limit / quorum before a search (the SQP loop as it stands
     finishes the search of every iteration it starts, so the bit is never set at present) */
} agx_iter_record;

/* Doubles per node in the derivative tile written by the node-parallel pass:
 * Fx ndx^2 | Fu ndx*nu | f ndx | Lx ndx | Lu nu | Lxx ndx^2 | Lxu ndx*nu | Luu nu^2 | cost 1 */
#define AGX_TILE_DOUBLES(nv) (4 * (nv) * (nv) + 2 * (nv) * (nv) + 2 * (nv) + 2 * (nv) + (nv) + 4 * (nv) * (nv) + 2 * (nv) * (nv) + (nv) * (nv) + 1)

typedef struct agx_model agx_model;
typedef struct agx_ocp agx_ocp;

const char *agx_last_error(void);
/* Number of visible HIP devices (0 when none); never throws.                   */
int agx_device_count(void);

/* Layout helpers shared by host code and kernels.                              */
int agx_row_nref(int kind, int nv); /* reference doubles of a row               */
int agx_row_nr(int kind, int nv);   /* residual dimension of a row              */
/* doubles per node of the reference tile for this problem (max of running and
 * terminal tables)                                                             */
int agx_ref_stride(const agx_ocp_desc *desc, int nv);

/* ---- model ------------------------------------------------------------- */
int agx_model_create(const agx_model_desc *desc, agx_model **out);
void agx_model_destroy(agx_model *m);

/* ---- problem ----------------------------------------------------------- */
/* Replaces OCPBaseCroco.__init__ (ocp_base_croco.py:17-80): allocates the
 * device-resident horizon buffers for `batch` instances on HIP device `device`. */
int agx_ocp_create(const agx_model *m, const agx_ocp_desc *desc, int batch, int device, agx_ocp **out);
void agx_ocp_destroy(agx_ocp *ocp);
/* Run the kernels on a caller-provided hipStream_t (0 = library-owned stream). */
int agx_ocp_set_stream(agx_ocp *ocp, void *hip_stream);
int agx_ocp_sync(agx_ocp *ocp);
/* Replaces OCPBaseCroco.update_geometry_placement (ocp_base_croco.py:110-132): new placement
 * (R row major 9 | p 3, in the parent joint frame; world for parent -1) of a geometry frame,
 * e.g. a moving obstacle.  Applies to every instance of the handle.              */
int agx_ocp_set_geom_placement(agx_ocp *ocp, int frame, const double *se3);
/* Batch policy -- no counterpart upstream, where every controller is its own process (mpc.py:14-19) and a slow solve
 * delays only itself.  In a batch the SQP loop of one step runs until EVERY instance has finished; with a quorum
 * below 1 it ends as soon as that fraction has, and the ADMM loop of an SQP iteration as soon as that fraction of
 * the QPs has converged.  The remaining instances keep their current iterate and report solved = 0 with the SQP /
 * ADMM iterations they really ran (iter, qp_iters): what a lone controller returns when it runs into max_iter /
 * max_solve_time (ocp_base_croco.py:160-171); the next MPC step continues from that iterate through the warm-start shift.
 * Defaults 1.0 / 1.0: wait for everyone.                                            */
int agx_ocp_set_quorum(agx_ocp *ocp, double sqp_fraction, double qp_fraction);
/* Constrained problems keep the ADMM multipliers y and the penalty rho between solves, as the
 * reference's solver object does (SolverCSQP reset_y = reset_rho = false).  This forgets them:
 * the state of a freshly constructed solver.                                      */
int agx_ocp_reset_duals(agx_ocp *ocp);

/* Replaces OCPCrocoGeneric.set_reference_weighted_trajectory
 * (ocp_croco_generic.py:855-892): ref_tile [B][T+1][stride] host doubles,
 * frame_ids [B][T+1][AGX_MAX_ROWS] host int32 (NULL = row defaults).            */
int agx_ocp_set_refs(agx_ocp *ocp, const double *ref_tile, const int32_t *frame_ids);
/* 1 when the handle runs a wide cost set (more than AGX_MAX_ROWS cost rows in a node type, or AGX_COST_WIDE=1 on a set that
 * qualifies), 0 otherwise.  On such a handle agx_ocp_set_refs, agx_ocp_set_refs_async and agx_ocp_set_refs_device refuse a
 * non-NULL frame-id table: every frame row looks at the frame of its agx_cost_row on every node.                           */
int agx_ocp_cost_wide(agx_ocp *ocp);
/* 1 when an active cost row of the handle is a ControlGrav or FrameVelocity row (the kernels that carry Lxu and the dense Lxx
 * blocks run: the GEN one-lane kernels up to 7 joints, k_general_rows_wg / k_node_kkt_big_gen above), 0 otherwise.       */
int agx_ocp_general_rows(agx_ocp *ocp);
/* The same update without stalling the caller or the solver (the reference pays ~ T x #costs binding calls per step for it,
 * ocp_croco_generic.py:883-888), in two halves so that the tile of step k+1 can travel while step k is being solved:
 *   agx_ocp_set_refs_async  STAGES a tile: a second stream copies it into the handle's second device tile (the solver
 *                           keeps reading the first one); hand in page-locked memory (agx_host_alloc) and the copy runs
 *                           at the rate of the link, concurrently with kernels;
 *   agx_ocp_refs_activate   makes the staged tile the current one: the solver's stream waits for the copy (the host does
 *                           not) and the two device tiles swap roles.
 * Per step: activate (tile k, staged during step k-1), stage tile k+1, solve step k.  The host buffer of a staged tile must
 * stay untouched until agx_ocp_refs_wait returns or the solve after its activation has returned.                          */
int agx_ocp_set_refs_async(agx_ocp *ocp, const double *ref_tile, const int32_t *frame_ids);
int agx_ocp_refs_activate(agx_ocp *ocp);
int agx_ocp_refs_wait(agx_ocp *ocp);
/* Page-locked host memory for the tiles and results handed to this library (a plain allocation works everywhere, but its
 * transfers are staged by the runtime at a fraction of the link's rate).                                                */
int agx_host_alloc(size_t bytes, void **out);
int agx_host_free(void *p);
/* Same with device-resident tiles (no copy of the doubles is made when
 * `adopt` != 0: the solver then reads the caller's buffer directly).            */
int agx_ocp_set_refs_device(agx_ocp *ocp, const double *d_ref_tile, const int32_t *d_frame_ids, int adopt);

/* Replaces OCPBaseCroco.solve (ocp_base_croco.py:142-182) for B instances.
 * Host buffers: x0 [B][nx], xs_ws [B][T+1][nx], us_ws [B][T][nu];
 * outputs xs [B][T+1][nx], us [B][T][nu], K [B][T][nu][ndx], st [B].
 * max_iter <= 0 means 1000 (use_iteration_limits_and_timeout=False);
 * max_time <= 0 means no wall-clock cap.                                       */
int agx_ocp_solve(agx_ocp *ocp, const double *x0, const double *xs_ws, const double *us_ws,
                  int max_iter, double max_time, double *xs, double *us, double *K, agx_status *st);

/* Device-resident variant: the warm start is whatever currently sits in the
 * resident xs/us buffers (after agx_ocp_upload_warmstart or
 * agx_ocp_shift_warmstart); results stay on the device.                        */
int agx_ocp_upload_x0(agx_ocp *ocp, const double *x0);
int agx_ocp_upload_warmstart(agx_ocp *ocp, const double *xs_ws, const double *us_ws);
int agx_ocp_solve_resident(agx_ocp *ocp, int max_iter, double max_time);
int agx_ocp_download(agx_ocp *ocp, double *xs, double *us, double *K, agx_status *st);
/* The full OCPResults (ocp_base_croco.py:173-177: xs, K, us of every node) without holding up the next step: a device-side
 * snapshot is taken in the solver's stream and drained to the host by a second stream; the destination buffers (any may be
 * NULL; page-locked memory from agx_host_alloc for the rate of the link) are complete when agx_ocp_download_wait returns.  */
int agx_ocp_download_async(agx_ocp *ocp, double *xs, double *us, double *K);
int agx_ocp_download_wait(agx_ocp *ocp);
/* Only what the ROS node publishes (agimus_controller_ros/agimus_controller.py:418-426):
 * us0 [B][nu], K0 [B][nu][ndx], x1 [B][nx] (may be NULL).                      */
int agx_ocp_download_first(agx_ocp *ocp, double *us0, double *K0, double *x1, agx_status *st);
/* Same data without the host-side scatter: one device-side pack, one transfer into a pinned buffer
 * owned by the handle.  *host -> [B][*stride] doubles, per instance
 *   us0 (nu) | K0 (nu*ndx, row major) | x1 (nx) | kkt cost merit gap_norm iter qp_iters solved flags;
 * valid until the next call on this handle that solves (agx_ocp_solve, agx_ocp_solve_resident, agx_ocp_mpc_step) or packs
 * (this one, agx_ocp_download_first): instances that converge write their record into the same buffer while the solve runs.
 * When every instance of the last solve did -- each converged in an iteration whose gains sweep rode along, the usual end of a
 * warm-started MPC step -- and nothing has touched the iterate, the gains or the solver state since, the buffer is returned as
 * it is, without a launch and without a wait; otherwise one pack kernel fills it as before.                                    */
int agx_ocp_first_packed(agx_ocp *ocp, const double **host, int *stride);
/* in_solve = 0: no record is written during a solve, agx_ocp_first_packed always packs with its own launch.  Default 1.       */
int agx_ocp_set_first_pack(agx_ocp *ocp, int in_solve);
/* agx_ocp_first_packed / agx_ocp_download_first calls on this handle served from records written during the solve / by the
 * pack kernel (either pointer may be NULL).                                                                                    */
int agx_ocp_first_pack_counts(agx_ocp *ocp, long long *served_in_solve, long long *served_by_launch);
/* Introspection of the host loop (tests): solves of this handle whose SQP loop ended on the counters published right behind the
 * head of the step, without waiting for the queued trial round (batches above 204), and the number of instances whose derivative
 * tiles the next agx_ocp_mpc_step may inherit as the last solve published it (-1: not known).  Either pointer may be NULL.       */
int agx_ocp_handoff_counts(agx_ocp *ocp, long long *early_exits, int *n_carriable);
/* Introspection of the tile carry (tests): agx_ocp_mpc_step calls of this handle whose first derivative pass inherited the tiles
 * of the previous step (some or all instances: nodes 0, T - 1 and T only for those) and calls that ran the full pass.  A carried
 * and a full step hand out the same bits, so this is the only place the difference shows.  Either pointer may be NULL.         */
int agx_ocp_carry_counts(agx_ocp *ocp, long long *steps_carried, long long *steps_full);

/* Replaces WarmStartShiftPreviousSolution.shift
 * (warm_start_shift_previous_solution.py:85-109) on the resident solution.     */
int agx_ocp_shift_warmstart(agx_ocp *ocp);
/* x0 <- xs[1] of the resident solution (closed loop on the own prediction, as
 * agimus_controller_examples/scripts/dummy_mpc_test.py:127-129).               */
int agx_ocp_x0_from_prediction(agx_ocp *ocp);

/* Replaces OCPBaseCroco.integrate (ocp_base_croco.py:184-189): one Euler step
 * of the node-0 model for n states. Host buffers x [n][nx], u [n][nu].         */
int agx_ocp_integrate(agx_ocp *ocp, int n, const double *x, const double *u, double *xnext);

/* Replaces pin.rnea at warm_start_reference.py:78 and
 * trajectories/sine_wave_configuration_space.py:56 for n samples (host).       */
int agx_model_rnea(agx_ocp *ocp, int n, const double *q, const double *v, const double *a, double *tau);
/* Frame placement (pin.framesForwardKinematics,
 * trajectories/trajectory_base.py:38-41): out [n][12].                         */
int agx_model_frame_placement(agx_ocp *ocp, int n, int frame, const double *q, double *out);
/* pinocchio.getFrameJacobian: J [n][6][nv], rows linear | angular; local = 0 LOCAL_WORLD_ALIGNED,
 * 1 LOCAL (the inverse kinematics of trajectories/sine_wave_cartesian_space.py:62-111 uses both). */
int agx_model_frame_jacobian(agx_ocp *ocp, int n, int frame, int local, const double *q, double *J);

/* Sensitivity of the Euler node to the link inertials of the controller's model, the study of
 * agimus_controller_examples/main/model_sensibility/evaluate_model_sensibility.py:97-119, for n samples (host buffers
 * x [n][nx], u [n][nu]): out [n][2 nv][10 nv],
 *   out[s][r][10 l + k] = | xnext_r(model with entry k of link l moved) - xnext_r(model) | / delta ,
 * xnext = [q + v+ dt; v+], v+ = v + a dt.  Entries of a link as the script orders and perturbs them (:9-49):
 * k = 0..5 inertia (row, col) = (0,0) (1,0) (1,1) (2,0) (2,1) (2,2), delta_inertia added at [row][col] and at
 * [col][row] -- a diagonal entry moves by 2 delta_inertia and is still divided by delta_inertia; k = 6..8 centre of
 * mass x, y, z by delta_com; k = 9 mass by delta_mass.  A plant set on the handle plays no part.  Refuses n < 1,
 * dt <= 0 and a zero delta.                                                                       */
int agx_model_sensitivity(agx_ocp *ocp, int n, double dt, const double *x, const double *u,
                          double delta_inertia, double delta_com, double delta_mass, double *out);

/* Replaces the per-node residual copies of OCPCrocoGeneric.fill_debug_data
 * (ocp_croco_generic.py:840-853): residual of running row `row` at the resident
 * solution, out [B][T][nr] (a collision row, the pair rows of a wide cost set included: the distance). */
int agx_ocp_get_residuals(agx_ocp *ocp, int row, double *out);

/* ---- diagnostics -------------------------------------------------------- */
/* Per-iteration solver log, the counterpart of OCPParamsBaseCroco.callbacks (mim_solvers.CallbackVerbose / CallbackLogger,
 * ocp_base_croco.py:77-80).  agx_ocp_iter_log keeps room for `capacity` records per instance on the device (0 = off, the
 * default: a solve then launches exactly the kernels of a handle that never had a log); the call waits for the solver stream.
 * While on, every solving entry point (agx_ocp_solve, agx_ocp_solve_resident, agx_ocp_mpc_step) starts the log afresh and a
 * small kernel copies the record of SQP iteration j of instance b to out[b][j], behind the head of the iteration (evaluation,
 * regularisation) and behind its trial rounds (step, trials); the step kernels and the solver state are the same with the log
 * on or off, and so is every result.  n[b] counts the iterations instance b started: status.iter + 1 for an instance that
 * converged (the converging iteration has a record with step = 0 and flags bit0), status.iter otherwise (iteration cap,
 * max_time, quorum cut, saturated regularisation).  Records beyond `capacity` are dropped, n[b] still counts them.
 * agx_ocp_iter_log_read waits for the solver stream; out [B][capacity] (records j >= n[b] are stale or zero), n [B]; either
 * may be NULL.  Every model capacity, constrained problems, both sweep flavours.                                           */
int agx_ocp_iter_log(agx_ocp *ocp, int capacity);
int agx_ocp_iter_log_read(agx_ocp *ocp, agx_iter_record *out, int32_t *n);
/* What the MPC debugger reads out of Crocoddyl's data for every node and cost item (agimus_controller_ros
 * mpc_debugger_node.py:241-323: weight * cost, weight * Lx, weight * Lu), at the resident (xs, us) with the references the
 * solver would read (the handle's one reference view, whichever call set it: host tile, device tile, a window of a resident or
 * streamed trajectory), the frame-id table and per-instance obstacle placements (per-instance model inertials enter no cost row
 * a handle with them accepts):
 *   cost_r [B][T][Rr], Lx_r [B][T][Rr][nx], Lu_r [B][T][Rr][nu], cost_t [B][Rt], Lx_t [B][Rt][nx]   (any may be NULL)
 * with Rr / Rt ALL rows of the running / terminal table, the pair rows of a wide cost set included.  Values at the
 * differential level, as the debugger shows them: item weight x a(r) and item weight x R' a'(r) WITHOUT the Euler factor dt
 * (item x dt[t] summed over the items of a running node is the node's share in agx_ocp_calc_diff); the item weight is the
 * first entry of the row in that node's reference tile.  An inactive row gives zeros, and so does a Control / ControlGrav row
 * at the terminal node.  Gradients in the caller's joint layout [q | v].  Every row kind the handle accepts.
 * The call only reads: the iterate, the solver state, the multipliers and the tile carry of agx_ocp_mpc_step are untouched.
 * Kernels: k_item_costs (a lane per node and row), k_cost_pairs with the per-pair destination.  It waits for the solver stream.
 * A set-up-class call: it stages B (T + 1) R (1 + nx + nu) doubles at the capacity sizes (R: the larger row count of the two
 * node types) in a device buffer the handle keeps (grown on demand, never shrunk) and in a host buffer of the same size for the
 * duration of the call -- several hundred MB at a batch of 1024 with a wide cost set; probe a few instances' worth of batch.   */
int agx_ocp_item_costs(agx_ocp *ocp, double *cost_r, double *Lx_r, double *Lu_r, double *cost_t, double *Lx_t);
/* Clearance report: how far apart the geometries of a pair list are, at configurations of the caller's choice.
 *   frame_a[p], frame_b[p]  geometry frames of the handle's model, n_pairs >= 1 of them and no upper limit: any pairs, rows of the
 *                           problem or not, self pairs, a pair listed twice.  The table is uploaded with every call.
 *   q [B][m][nv]            the caller's joints (before padding, as agx_model_frame_placement takes them), m >= 1 samples per
 *                           instance; NULL: the handle's current iterate, m must be T + 1 and sample t is node t of xs, the
 *                           terminal node included.
 *   dist [B][m][n_pairs]    the signed distance, the function the collision cost rows and constraints evaluate
 *                           (collision_distance_placed: capsule, sphere and box; negative in penetration).
 *   witness [B][m][n_pairs][9]  optional: the point on geometry a, the point on geometry b and the unit normal n, world frame.
 *                           The points lie on the SURFACES (the device routine's points on a capsule's axis or at a sphere's
 *                           centre, moved by the radius along n), so pa - pb = dist n.  Coincident axis points leave n = 0.
 *   min_dist [B]            optional: the smallest distance of instance b over samples and pairs;
 *   min_where [B][2]        optional: its sample and pair; of equal distances the lowest sample, then the lowest pair.  A fixed-order
 *                           reduction without atomics: the same bits from run to run.  (-1, -1) and +inf where no distance is finite.
 * World-fixed frames are placed as the solve places them: by the latest agx_ocp_set_geom_placement and, for a listed frame on
 * the 7-joint capacity, by instance b's entry of agx_ocp_set_obstacle_placements.
 * The call only reads: it runs on the handle's stream in a device block of its own, waits for the stream and leaves the iterate,
 * the multipliers, the tiles and their carry, the first-node record and the resident trajectory as they are; a solve or MPC step
 * after it gives the bits it would have given without it.  Kernels: k_clearance (a workgroup per eight samples of an instance,
 * every model capacity), k_clearance_min.
 * Refused, naming the pair where there is one: null handle, pair arrays or dist; n_pairs < 1; m < 1; q == NULL with
 * m != T + 1; a frame out of range or without collision geometry; a box / box pair.                                        */
int agx_ocp_clearance(agx_ocp *ocp, int n_pairs, const int32_t *frame_a, const int32_t *frame_b, const double *q, int m, double *dist,
                      double *witness, double *min_dist, int32_t *min_where);

/* ---- kernel-level entry points (parity tests and bench instrumentation) - */
/* Node-parallel derivative pass at the resident (xs, us): writes the tiles to
 * the workspace and optionally copies them out, tiles [B][T+1][AGX_TILE_DOUBLES]. */
int agx_ocp_calc_diff(agx_ocp *ocp, double *tiles);
/* One QP direction at the resident (xs, us) exactly as the solver computes it (derivative pass,
 * Riccati backward + linear forward, KKT, reported gains): K [B][T][nu][ndx], k = acceleration-space
 * feed-forward [B][T][nu], dx [B][T+1][ndx], du [B][T][nu], kkt [B].                                */
int agx_ocp_direction(agx_ocp *ocp, double *K, double *k, double *dx, double *du, double *kkt);
/* What the last SQP iteration of the last solve left on the device, copied out as it stands (nothing is launched): the
 * direction dx [B][T+1][ndx], du [B][T][nu] and the node shares nodestat [B][T+1][4] = {kkt, cost, gap, violation} the head of
 * the step summed.  Any pointer may be NULL.  Entries of instances that had finished before that iteration are older.       */
int agx_ocp_last_direction(agx_ocp *ocp, double *dx, double *du, double *nodestat);
/* Forward pass, node KKT pass and head of the step of an SQP iteration as one launch per instance (k_step_tail; default on,
 * where it applies: 7-joint capacity, unconstrained, no general rows, one-wave sweeps) or, on = 0, as the three launches it
 * replaces; on < 0 leaves the choice as it is.  Same bits either way (tests/test_step_tail_gpu.py); takes effect from the next
 * solve.  *launches (may be NULL): k_step_tail launches of this handle so far -- whether its solves took the path at all.  */
int agx_ocp_set_step_tail(agx_ocp *ocp, int on, long long *launches);
/* The QP tiles of the node-parallel derivative pass at the resident (xs, us) exactly as the solver's sweep reads
 * them (acceleration-input form): qt [B][T+1][*qt_size], aux [B][T+1][*aux_size] (either may be
 * NULL; the sizes are always returned).  Layout per node, blocks nv x LD row major with LD = 8 (nv <= 8) or 32:
 *   qt  = Hqq | Hqv | Hvv | Hqw | Hvw | Hww | gx (2 nv of 2 LD) | gw (nv of LD) | f (2 nv of 2 LD) | cost (1 of 8)
 *   aux = M | dtau/dq | dtau/dqdot | Lqq | Lvv (LD) | Luu (LD) | Lu (LD)                                   */
int agx_ocp_qp_tiles(agx_ocp *ocp, double *qt, double *aux, int *qt_size, int *aux_size);
/* Average device time in milliseconds of `reps` launches of one kernel,
 * measured with hipEvents on the problem's stream.
 * which: 0 = derivative pass (running + terminal launches), 1 = Riccati backward + forward,
 * 2 = step kernel (du, KKT, line search; nothing committed), 3 = derivative pass over the running
 * nodes only (one launch), 4 = canonical-tile derivative pass (running nodes), 5 = Riccati backward
 * only, 6 = exit (gains) sweep alone, 7 = direction + speculative gains sweep in one launch,
 * 8 = the closed-loop rollout of agx_ocp_feedback_rollout as the handle would launch it (10 sub-steps of
 * 1 ms, no disturbance; with or without a plant), x0 restored afterwards, 9 = k_cost_pairs alone (wide cost sets; on
 * such a handle 0 and 3 time K1 and k_cost_pairs together, as every derivative pass launches them),
 * 10 = the device work of the last agx_traj_stream_append again (transfer of the staged chunk + fill of its slots with the
 * same values), on the COPY stream, after the host has waited for both streams; the handle's state is left as it is.  */
int agx_ocp_time_kernel(agx_ocp *ocp, int which, int reps, double *avg_ms);

/* In-situ kernel timing: while enabled, every solve brackets the launches of its SQP loop with
 * hipEvents on the problem's stream; ms_sum / count [3] return the accumulated device time and
 * launch count of {derivative pass over the running nodes, Riccati backward + forward, step
 * (per-node KKT + convergence test + line search)} since profiling was switched on.           */
int agx_ocp_profile(agx_ocp *ocp, int enable, double *ms_sum, long long *count);

/* ---- device-resident reference trajectory --------------- */
/* Sine wave in configuration space, trajectories/sine_wave_configuration_space.py:41-72,
 * for B instances and n_points time samples t_k = t0[b] + k*dt, written as
 * reference tiles [B][n_points][stride] directly in HBM for the goal-reaching
 * row table (control | state | frame placement).  Host parameter arrays:
 * q0 [B][nv], amp [B][nv], pulsation [B][nv], scale_duration [B][nv], t0 [B];
 * weights w_q, w_qdot, w_effort [nv], w_pose [6].                              */
int agx_traj_sine_create(agx_ocp *ocp, int n_points, double dt, const double *q0, const double *amp,
                         const double *pulsation, const double *scale_duration, const double *t0,
                         const double *w_q, const double *w_qdot, const double *w_effort,
                         const double *w_pose, int frame);
/* Same resident trajectory from caller-given samples q, dq, ddq [B][n_points][nv]
 * (GenericTrajectory.build_trajectory_from_q_dq_ddq_arrays, trajectories/generic_trajectory.py:37-70):
 * feed-forward effort by RNEA and end-effector pose by FK on the device.          */
int agx_traj_generic_create(agx_ocp *ocp, int n_points, const double *q, const double *dq, const double *ddq,
                            const double *w_q, const double *w_qdot, const double *w_effort, const double *w_pose, int frame);
/* Same resident trajectory from the Cartesian sine generator (SinusWaveCartesianSpace,
 * trajectories/sine_wave_cartesian_space.py:62-111): the end effector `frame` of instance b follows
 * p0_b + amp_b s(t) sin(pulsation_b t) with its initial orientation (s: the quintic of scale_duration);
 * q by the iterative inverse kinematics on the device (warm-started point to point, all six error components,
 * stop at |log6| < precision, error once more than it_max steps were taken -- upstream's `if i > it_max`, default 10000),
 * dq from the LOCAL_WORLD_ALIGNED Jacobian, ddq = 0.  The end-effector reference of a point is the DESIRED pose
 * (initial orientation, p0 + amp s sin), as upstream stores ee_des_pos.  On an inverse-kinematics failure the call
 * returns an error and the handle is left WITHOUT a resident trajectory.  q0 [B][nv], amp / pulsation [B][3].  nv <= 7. */
int agx_traj_cartesian_sine_create(agx_ocp *ocp, int n_points, double dt, const double *q0, const double *amp,
                                   const double *pulsation, double scale_duration, double precision, int it_max,
                                   const double *w_q, const double *w_qdot, const double *w_effort, const double *w_pose,
                                   int frame);
/* agx_traj_generic_create with a weight schedule: what the cost rows take from the weights of every point of a user-fed trajectory
 * (ocp_croco_generic.py:203-210, :257-264, :311-318 w_end_effector_poses; :713-719 w_collision_avoidance), resident on the device.  GenericVisualServoingTrajectory
 * (trajectories/generic_visual_servoing_trajectory.py:93-145) is the generator this serves: its pose weights ramp with
 * WeightIncreasing (trajectories/weight_increasing.py:17-20) and its collision weight changes with the visual-servoing state.
 *   pose        [B][n_points][12] or NULL: end-effector reference of every sample (R row major | p) instead of the forward
 *               kinematics of its q (:97-100: the pose re-expressed in the object frame);
 *   w_pose      [B][n_points][6]: activation weights of the frame placement / translation (first 3) / rotation (last 3) rows;
 *   w_collision [B][n_points] or NULL: item weight of the collision-distance rows (NULL: the row's YAML weight).
 * `frame` is the frame the rows look at; it need not be the frame whose poses are given (:57: the "_vs" frame).  Every model
 * size agx_traj_generic_create serves.                                                                                  */
int agx_traj_generic_create_weighted(agx_ocp *ocp, int n_points, const double *q, const double *dq, const double *ddq,
                                     const double *w_q, const double *w_qdot, const double *w_effort, int frame,
                                     const double *pose, const double *w_pose, const double *w_collision);
/* agx_traj_cartesian_sine_create with the schedule of SinusWaveCartesianSpaceWeightIncreasing
 * (trajectories/sine_wave_cartesian_space_weight_increasing.py:51-108): q, dq from the inverse kinematics of the sine as there; the
 * end-effector reference of a point has the initial orientation and, per axis, the extremum p0 + amp s(t) or p0 - amp s(t) the sine is
 * heading for (:51-61 get_targets_time with the cycle duration period[b][axis]: t1 = time since the cycle started, t2 = t1 +- period/2,
 * plus while t1 < t2); the translational pose weight of that axis is max_weight tanh(rate max(t1, t2)) (weight_increasing.py:17-20
 * with rate = arctanh(percent) / time_reach_percent).  w_pose [6]: its last three entries are the rotational weights, the first
 * three are replaced by the schedule.  t / period, its truncation and the remainder are rounded one by one as on the host, so a
 * sample on a half-cycle boundary takes the host's side.  period [B][3] > 0.  nv <= 7; failures as agx_traj_cartesian_sine_create. */
int agx_traj_cartesian_sine_wi_create(agx_ocp *ocp, int n_points, double dt, const double *q0, const double *amp,
                                      const double *pulsation, double scale_duration, double precision, int it_max,
                                      const double *w_q, const double *w_qdot, const double *w_effort, const double *w_pose,
                                      int frame, const double *period, double max_weight, double rate);
/* ---- streamed resident trajectory ---------------------------------------------------------------------------------------
 * The resident trajectory as TrajectoryBuffer uses it (trajectory.py:181-231: an unbounded list the planner appends to while
 * MPC.run pops one point per step with clear_past, mpc.py:30-41): a RING of `capacity` samples per instance in HBM that the
 * caller appends to and releases from while agx_ocp_mpc_step runs on it -- no allocation per step, no host wait for the solver,
 * and the tile carry goes on.  Samples have LOGICAL indexes 0, 1, 2, ... (int, as in agx_ocp_mpc_step); the handle retains
 * [first, end) with end - first <= capacity.  Logical sample k lives in slot k mod capacity and, when that slot is below
 * max_span - 1, a second time in the mirror slot capacity + (k mod capacity), so every window of up to max_span samples is
 * contiguous from slot k0 mod capacity and the window arithmetic, the gather of non-uniform horizons, the warm start and the
 * readers work as on a one-shot trajectory.  On a streamed handle agx_traj_set_window, agx_ocp_mpc_step,
 * agx_traj_warmstart_from_reference, agx_traj_get_point and agx_traj_get_tile take logical indexes and fail with a message
 * naming [first, end) when the window or sample is not inside it; agx_traj_set_horizon_indexes refuses idx[T] + 1 > max_span.
 *
 * agx_traj_stream_create: like the other create calls it frees any earlier trajectory, ends the tile carry and makes the
 * frame rows look at `frame`; it leaves an EMPTY ring (first = end = 0) and no window.  max_span: the most samples a window
 * may cover (idx[T] + 1, T + 1 for uniform indexes).  Refuses max_span < T + 1, capacity < max_span, a bad frame and horizon
 * indexes already set on the handle that are wider than max_span.  Every
 * model size agx_traj_generic_create serves; joint weights [nv], w_pose [6] (used by appends without a w_pose array).    */
int agx_traj_stream_create(agx_ocp *ocp, int capacity, int max_span, const double *w_q, const double *w_qdot,
                           const double *w_effort, const double *w_pose, int frame);
/* Appends logical samples end .. end + m - 1 of every instance: q, dq, ddq [B][m][nv]; pose [B][m][12], w_pose [B][m][6],
 * w_collision [B][m] optional, meaning what they mean in agx_traj_generic_create_weighted (NULL: forward kinematics of the
 * sample / the w_pose of create / the row's YAML weight).  Efforts by RNEA and poses by FK on the device, by the device
 * function the one-shot generators use: the tiles are bit for bit those of agx_traj_generic_create_weighted on the same samples.
 * Refuses m < 1, a ring that would overflow (release the past first), end + m beyond INT_MAX, non-finite input and a handle
 * without a stream; a refused call changes nothing.
 * Ordering contract.  The call copies the arrays into page-locked memory of the handle (the caller may reuse them on return)
 * and enqueues, on the handle's COPY stream (the one agx_ocp_set_refs_async uses), the transfer and the fill of the slots.  The
 * fill waits for an event recorded on the solver stream at the time of the call, so no work queued earlier can still be
 * reading a released slot it overwrites; the host does not wait.  A later agx_traj_set_window / agx_ocp_mpc_step (or reader)
 * that reaches a sample of an append not yet joined makes the SOLVER stream wait for that append's event -- again the host
 * does not wait.  The host blocks only when it reuses a staging buffer whose fill has not finished: there are two, used in
 * turn, each holding max_span samples per instance (a longer append goes in pieces).  Append and release do not end the tile
 * carry: they touch only samples no earlier window contained.                                                            */
int agx_traj_stream_append(agx_ocp *ocp, int m, const double *q, const double *dq, const double *ddq, const double *pose,
                           const double *w_pose, const double *w_collision);
/* Samples below k are no longer needed (TrajectoryBuffer.clear_past, several at once if wanted): first = k.  Refuses
 * k < first and k > end.  No device work.                                                                                */
int agx_traj_stream_release(agx_ocp *ocp, int k);
/* The retained logical range [first, end) (either pointer may be NULL).                                                  */
int agx_traj_stream_range(agx_ocp *ocp, int *first, int *end);
/* The ordering contract as the host keeps it (a debug reader for tests): *joins = how often the solver stream has been made
 * to wait for an append's event since the handle was created, *pending = appended pieces (0 .. 2) no window or reader has
 * reached and no staging-buffer reuse has completed yet (either pointer may be NULL).                                    */
int agx_traj_stream_joins(agx_ocp *ocp, long long *joins, int *pending);
/* In-situ timing of the two streams, in the manner of agx_ocp_profile: while enabled, every join is bracketed by two hipEvents on
 * the SOLVER stream -- ms_sum[0] / count[0]: how long that stream sat waiting for a fill, the event in front of the wait
 * completing as soon as the stream reaches it -- and every appended piece by two on the COPY stream -- ms_sum[1] / count[1]:
 * transfer + fill, the wait for the solver's event included.  Returns what has accumulated since timing was switched on (the
 * host waits for both streams to read the events out); switching on or off clears the sums.                              */
int agx_traj_stream_timing(agx_ocp *ocp, int enable, double *ms_sum, long long *count);
/* Point the solver at the horizon window starting at sample `k0` of the
 * resident trajectory (TrajectoryBuffer.horizon, trajectory.py:218-222, with
 * uniform horizon indexes).                                                    */
int agx_traj_set_window(agx_ocp *ocp, int k0);
/* Non-uniform horizon (TrajectoryBuffer.compute_horizon_indexes, trajectory.py:195-216: with
 * dt factors the node t looks at sample k0 + idx[t], pinned by tests/test_buffer.py:82-93 to
 * [0,1,2,4,6,9,12,16,20,25,30] for factors 1..4 x 2..3 steps).  idx [T+1], NULL = uniform.  */
int agx_traj_set_horizon_indexes(agx_ocp *ocp, const int32_t *idx);
/* Copy trajectory sample k of every instance to the host: q,v,a,u [B][nv], pose [B][12]. */
int agx_traj_get_point(agx_ocp *ocp, int k, double *q, double *v, double *a, double *u, double *pose);
/* Copy the reference tile of sample k to the host, out [B][stride]: [item weight | reference | activation weights] of every row
 * in the running (terminal = 0) or the terminal layout, what OCPCrocoGeneric.set_reference_weighted_trajectory
 * (ocp_croco_generic.py:855-892) would have written for that point; doubles behind the last row are zero.  A debug reader:
 * the next MPC step recomputes every derivative tile.                                       */
int agx_traj_get_tile(agx_ocp *ocp, int k, int terminal, double *out);
/* Warm start from the reference (WarmStartReference.generate,
 * warm_start_reference.py:33-96) on the device: xs <- [x0, ref[1:]], us <- ref efforts. */
int agx_traj_warmstart_from_reference(agx_ocp *ocp);

/* One receding-horizon step, MPC.run (mpc.py:32-66), fully device resident:
 * window k0, then by `first`: 1 = warm start and x0 from the reference (first step);
 * 0 = x0 <- previous xs[1] (closed loop on the own prediction) + warm-start shift;
 * 2 = x0 as it is (set by agx_ocp_upload_x0 / agx_ocp_feedback_rollout) + warm-start shift; then solve. */
int agx_ocp_mpc_step(agx_ocp *ocp, int k0, int max_iter, int first);
/* What consumes an MPC step: the linear feedback controller fed by
 * AgimusController.send_control_msg (agimus_controller_ros/agimus_controller.py:418-426) applies
 *   u = us[0] + K[0] (x0 - x_measured)
 * at the control rate.  Here the plant is the model -- instance b's own model where agx_ocp_set_model_inertials gave it
 * one -- or the model with the inertials of agx_ocp_set_plant_inertials: n_substeps semi-implicit Euler steps of dt_sub
 * from the resident x0 under that law (+ an optional constant torque disturbance [B][nu], host);
 * the end state replaces x0, ready for agx_ocp_mpc_step(..., first = 2).           */
int agx_ocp_feedback_rollout(agx_ocp *ocp, int n_substeps, double dt_sub, const double *disturbance);
/* The plant of that closed loop, per instance: link inertials that differ from the controller's model (unknown payload,
 * identified against nominal parameters, Monte-Carlo runs over parameter uncertainty).  Host arrays at the CALLER's nv:
 * mass [B][nv], com [B][nv][3] (joint frame), inertia [B][nv][9] (about the com, joint frame, row major), armature [B][nv]
 * (NULL: the model's).  Placements, axes, parents and gravity stay the model's, and so does everything the solver does:
 * only agx_ocp_feedback_rollout reads the plant.  All four NULL: back to the controller's own model, exactly the rollout
 * of a handle that never had a plant.  Non-finite values, a negative mass and a negative armature are refused (the handle
 * keeps what it had); the inertia is NOT tested for positive definiteness.
 * Ordering: the upload runs on the handle's solver stream (agx_ocp_set_stream), after the host has waited for the work
 * queued there; the call returns once the copy is complete, so the arrays may be reused at once and every rollout queued
 * before the call has used the old plant, every later one the new.                                                    */
int agx_ocp_set_plant_inertials(agx_ocp *ocp, const double *mass, const double *com, const double *inertia,
                                const double *armature);
/* The CONTROLLER's model, per instance: instance b solves its OCP on its own link inertials (one plant and many identified
 * models, a payload the controller knows about after a grasp, a fleet of arms with individually identified parameters).
 * Arrays, validation and ordering as agx_ocp_set_plant_inertials: host arrays at the CALLER's nv, mass [B][nv],
 * com [B][nv][3], inertia [B][nv][9], armature [B][nv] (NULL: the model's); pad joints of a model below the capacity are
 * massless with the padding's armature; non-finite values, a negative mass and a negative armature are refused and the
 * handle keeps what it had; the upload runs on the solver stream after the host has waited for it.  Placements, axes,
 * parents, gravity, frames and geometry stay the model's.  All four NULL: back to the model's own table, and from then on
 * exactly the launches of a handle that never had per-instance inertials.
 * READS the per-instance model -- everything that evaluates the controller's dynamics at a node of instance b: the
 * derivative pass of every solve and MPC step (eight-lane and one-lane kernels, wide cost and constraint sets, line-search
 * trial points included), agx_ocp_calc_diff / agx_ocp_direction / agx_ocp_qp_tiles, the re-integration of the warm-start
 * shift (agx_ocp_shift_warmstart, agx_ocp_mpc_step) and agx_ocp_feedback_rollout when no plant is set ("instance b's model
 * is its own plant"; a plant set with agx_ocp_set_plant_inertials still wins).
 * STAYS on the model's own table -- functions of the handle's table, or the planner, which has the nominal robot only:
 * agx_ocp_integrate, agx_model_rnea, agx_model_frame_*, agx_model_sensitivity, the trajectory generators and
 * agx_traj_stream_append (reference efforts by RNEA), agx_traj_warmstart_from_reference.
 * Scope: models of at most 7 joints after padding; a handle at the 16 / 30 / 32 capacities refuses the call.  A problem
 * with a ControlGrav cost or constraint item refuses it too (its g(q) would be evaluated on the model's table).
 * The call ends the tile carry of agx_ocp_mpc_step (the next step runs the full derivative pass); the carry resumes
 * afterwards, the inertials being constant across steps.                                                              */
int agx_ocp_set_model_inertials(agx_ocp *ocp, const double *mass, const double *com, const double *inertia,
                                const double *armature);
/* The OBSTACLES, per instance: instance b evaluates every collision-distance cost row and constraint row that names a listed
 * frame with that frame placed at se3[b][slot] (a Monte-Carlo study over obstacle poses, a fleet of cells with different
 * fixtures, a sweep of a moving obstacle's predicted pose, domain randomisation of the scene).
 * frames [n_frames]: ids of WORLD-FIXED geometry frames of the handle's model (frame_parent < 0, a radius or a box).
 * se3 [B][n_frames][12]: host memory in the layout of frame_placement (rotation row-major 9, then translation 3), one placement
 * per instance and listed frame.  Rotations are not checked for orthonormality, as in agx_ocp_set_geom_placement.
 * n_frames == 0 with both pointers NULL clears the table (accepted on a handle that has none): from then on exactly the
 * launches of a handle that never had one.
 * While set: frames that are not listed keep the model's placement, later agx_ocp_set_geom_placement calls on them included;
 * a listed frame ignores agx_ocp_set_geom_placement until the table is cleared -- that call still updates the model, and
 * after a clear the latest model placement applies.
 * READS the table -- everything that evaluates a collision distance of the problem, chains and trees: the derivative pass of
 * every solve and MPC step (eight-lane and one-lane kernels, running and terminal nodes, wide cost sets, line-search trial
 * points included), agx_ocp_calc_diff / agx_ocp_direction / agx_ocp_qp_tiles, the constraint evaluation of constrained
 * problems (narrow and wide sets) and the distance agx_ocp_get_residuals returns for a collision row.
 * STAYS on the model's table -- functions of the handle's table, or the planner, which knows the nominal scene only:
 * agx_model_frame_placement, agx_model_frame_jacobian and the trajectory generators.
 * Combines with agx_ocp_set_model_inertials (the running-node derivative kernels then read both tables) and with
 * agx_ocp_set_plant_inertials.
 * Refused, each with the entry point and the offending item in agx_last_error, the handle exactly as it was: null or
 * inconsistent arguments; a frame out of range; a frame attached to a joint (it moves with the robot: its placement is
 * relative to that joint and stays the model's); a frame that carries no geometry; a frame listed twice; a non-finite entry
 * (instance and frame are named).
 * Scope: models of at most 7 joints after padding; a handle at the 16 / 30 / 32 capacities refuses the call.
 * The upload waits for the solver stream, then runs in it.  The call ends the tile carry of agx_ocp_mpc_step (the next step
 * runs the full derivative pass); the carry resumes afterwards, the placements being constant across steps.  ADMM multipliers
 * are left alone (agx_ocp_reset_duals).                                                                                 */
int agx_ocp_set_obstacle_placements(agx_ocp *ocp, int n_frames, const int32_t *frames, const double *se3);
/* The resident initial state x0 [B][nx] (measured state of the next step).          */
int agx_ocp_download_x0(agx_ocp *ocp, double *x0);

#ifdef __cplusplus
}
#endif
#endif /* AGIMUS_HIP_H */
