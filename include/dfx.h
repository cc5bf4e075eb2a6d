/* dfx.h -- C ABI of libdfx, the MI355X engine for DifFlexMM's hot path.
 *
 * The library replaces, for one lattice, what the reference builds in Python/JAX:
 *
 *   dfx_create      <->  setup_dynamic_solver(...)            difflexmm/dynamics.py:60-136
 *                        (static data: connectivity, bond model, contact on/off, which DOFs are
 *                        constrained / loaded and by which time function)
 *   dfx_set_params  <->  the ControlParams pytree passed to solve_dynamics
 *                                                            difflexmm/utils.py:48-163
 *   dfx_forward     <->  solve_dynamics(state0, timepoints, control_params)
 *                                                            difflexmm/dynamics.py:138-184
 *                        (odeint call at dynamics.py:166 + reconstruction :169-182)
 *   dfx_adjoint     <->  the VJP jax.grad takes through solve_dynamics
 *                        (problems/quads_focusing.py:565; jax.experimental.ode._odeint_rev)
 *   dfx_rhs         <->  rhs(state, t, control_params, inertia)  difflexmm/dynamics.py:33-55
 *   dfx_rhs_vjp     <->  jax.vjp(rhs, ...)                     (test hook for the adjoint kernel)
 *
 * Conventions: every function returns 0 on success, non-zero on failure (message via
 * dfx_last_error).  All arrays are C-contiguous float64 / int32 HOST buffers owned by the
 * caller; the library copies what it needs and keeps no caller pointer after a call returns.
 * Device memory lives inside the handle.  A handle belongs to one (process, device) and is not
 * thread safe.  `batch` independent members (designs / inputs of one lattice) are integrated
 * side by side; every per-member array has a leading batch axis.
 *
 * DOF layout (geometry.py:174-175): dof = 3*block + {0:x, 1:y, 2:theta};  node = n_npb*block + local.
 */
#ifndef DFX_H
#define DFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_MAX_FNS 2         /* time functions per problem                                   */
#define DFX_FN_PARAMS 5       /* parameters per time function                                 */

enum { DFX_BOND_LINEARIZED = 0, DFX_BOND_NONLINEAR = 1,         /* energy.py:99 / energy.py:158 */
       DFX_BOND_SIMPLE_SPRING = 2,                              /* energy.py:30-48: k_stretch (|dU + l0| - |l0|)^2 / 2; k_bond[1..2] ignored */
       DFX_BOND_STRETCH_TORSION = 3 };                          /* energy.py:51-67: zero-length spring, k_stretch |dU|^2/2 + k_rot dtheta^2/2;
                                                                   k_bond[1] and reference_vector ignored (pass any non-zero vector) */
enum { DFX_CONTACT_NONE = 0, DFX_CONTACT_ANGLE = 1,            /* energy.py:364 (angle_based)  */
       DFX_CONTACT_DISTANCE = 2 };                              /* energy.py:222-330 (angle_based=False): void-edge distances;
                                                                   `contact` = (min, cutoff, k) are lengths, needs block_centroids */
enum { DFX_TABLEAU_DOPRI5 = 0, DFX_TABLEAU_RK4 = 1 };
/* time-function library; parameters p[] in this order */
enum {
  DFX_FN_ZERO = 0,
  DFX_FN_PULSE = 1,        /* (A, f, t_d)   problems/quads_focusing.py:211-222                   */
  DFX_FN_HARMONIC = 2,     /* (A, f, t_d)   problems/quads_spin.py:210-222                       */
  DFX_FN_RAMP = 3,         /* (A, r)        tests/test_difflexmm.py:85-86                        */
  DFX_FN_SECH2TANH = 4,    /* (A, s)        scripts/pulse_RS.py:49-50                            */
  DFX_FN_CONSTANT = 5,     /* (A)                                                                 */
  DFX_FN_RAMP_CAP = 6,     /* (L, r, cap): L min(t r, cap)  static compression, problems/quads_kinetic_energy_static_tuning.py:176-182;
                              the delayed pulse of :184-186 is DFX_FN_PULSE with t_d = cap / r + input_delay (host-side chain rule) */
  DFX_FN_TABLE = 7         /* (A, t_d): A * interp(t - t_d; table), piecewise linear, end values held (jnp.interp semantics):
                              a recorded input signal; the times are static data of dfx_problem, the values can be
                              set per member and differentiated (dfx_fn_table_values, dfx_fn_table_grads)          */
};

/* A block that has constrained and/or force-loaded DOFs.  u[dof] = sum_m con_coef[d][m] * g_m(t)
 * for constrained DOFs (kinematics.py:68-73); F_load[dof] = sum_m load_coef[d][m] * g_m(t)
 * (loading.py:36-45). */
typedef struct dfx_special {
  int32_t block;
  int32_t con_mask;                       /* bit d set: DOF d of the block is constrained       */
  double con_coef[3][DFX_MAX_FNS];
  double load_coef[3][DFX_MAX_FNS];
} dfx_special;

typedef struct dfx_problem {
  int32_t n_blocks;
  int32_t n_npb;                          /* nodes per block: 3 (kagome) or 4 (quads)           */
  int32_t n_bonds;
  const int32_t* bonds;                   /* (n_bonds, 2) node ids, geometry.bond_connectivity() */
  int32_t bond_model;                     /* DFX_BOND_*                                          */
  int32_t contact;                        /* DFX_CONTACT_*                                       */
  int32_t n_special;
  const dfx_special* special;
  int32_t n_fns;                          /* <= DFX_MAX_FNS                                      */
  int32_t fn_type[DFX_MAX_FNS];           /* DFX_FN_*                                            */
  int32_t batch;                          /* ensemble members integrated together                */
  int32_t tableau;                        /* DFX_TABLEAU_*                                       */
  int32_t device;                         /* HIP device ordinal (ignored by the CPU port)        */
  int32_t fn_table_n[DFX_MAX_FNS];        /* DFX_FN_TABLE: number of breakpoints (>= 2), else 0   */
  const double* fn_table[DFX_MAX_FNS];    /* DFX_FN_TABLE: fn_table_n increasing times, then fn_table_n values */
  int32_t streams;                        /* member groups advanced on their own HIP streams; 0 = choose (2 when the launches fill the
                                             chip, else 1).  Several engines driven concurrently (multi-input problems) run best with 1 */
} dfx_problem;

/* ControlParams, flattened (utils.py:48-163).  Leading axis of every array = batch. */
typedef struct dfx_params {
  const double* centroid_node_vectors;    /* (batch, n_blocks, n_npb, 2)                         */
  const double* reference_vector;         /* (batch, n_bonds, 2)                                 */
  const double* k_bond;                   /* (batch, n_bonds, 3) = k_stretch, k_shear, k_rot     */
  const double* inertia;                  /* (batch, n_blocks, 3)  [m, m, J]                     */
  const double* damping;                  /* (batch, n_blocks, 3)  per-DOF viscous coefficient   */
  const double* void_angle0;              /* (batch, n_bonds, 2) undeformed void angles or NULL  */
  const double* contact;                  /* (batch, 3) min_angle, cutoff_angle, k_contact / NULL */
  const double* fn_params;                /* (batch, n_fns, DFX_FN_PARAMS)                       */
  const double* block_centroids;          /* (batch, n_blocks, 2): DFX_CONTACT_DISTANCE only, else NULL */
} dfx_params;

/* Gradient of  L = sum(fields_bar * fields)  with respect to everything in dfx_params and the
 * initial state.  Any pointer may be NULL (that gradient is then not accumulated). */
typedef struct dfx_grads {
  double* centroid_node_vectors;          /* (batch, n_blocks, n_npb, 2)                         */
  double* reference_vector;               /* (batch, n_bonds, 2)                                 */
  double* k_bond;                         /* (batch, n_bonds, 3)                                 */
  double* inertia;                        /* (batch, n_blocks, 3)                                */
  double* damping;                        /* (batch, n_blocks, 3)                                */
  double* void_angle0;                    /* (batch, n_bonds, 2)                                 */
  double* contact;                        /* (batch, 3)                                          */
  double* fn_params;                      /* (batch, n_fns, DFX_FN_PARAMS)                       */
  double* state0;                         /* (batch, 2, n_blocks, 3)                             */
  double* block_centroids;                /* (batch, n_blocks, 2): non-zero with DFX_CONTACT_DISTANCE, and for DFX_OBJ_ANGULAR_MOMENTUM */
} dfx_grads;

typedef struct dfx_stats {
  int64_t steps;                          /* RK steps taken per member                           */
  int64_t rhs_evals;                      /* RHS evaluations per member (forward)                */
  int64_t launches;                       /* kernel launches issued                              */
  double kernel_ms;                       /* device time of the integration loop (HIP events)    */
  double stage_kernel_us;                 /* mean duration of one stage-kernel launch incl. gap  */
  int64_t streams;                        /* member groups integrated concurrently (one HIP stream each); reverse sweep at the segments level
                                             with the re-run of the next piece beside the reverse stages of this one: 2 */
  int64_t stage_checkpoint;               /* 1: the forward pass also kept the stage accelerations of every step, so the
                                             reverse sweep runs without recompute launches (chosen when it fits in HBM) */
  int64_t checkpoint_records;             /* 1: the forward pass kept EVERY stage record of every step (56 s B per unit and step): the
                                             reverse launches read them directly, nothing is rebuilt or recomputed (richest level,
                                             taken when it fits; then stage_checkpoint = 0);
                                             2: "segments": nothing but the outputs was kept, the reverse sweep re-runs one output
                                             interval at a time with the records of that interval only */
  int64_t tile_kernels;                   /* which builds of the stage kernels this call launched: 0 the generic slot kernels; 2 their
                                             per-stage builds (stage index and common parameter shape compiled in: launches that fill the
                                             chip; DFX_STAGE_BUILDS=0 switches them off); 1 the tile kernels (every
                                             ligament evaluated once on lattice tiles, DFX_TILE=1: opt-in); 3 the persistent stage
                                             loop (one launch per segment of <= 256 steps, stage records handed between neighbouring waves: solves
                                             whose launches do not fill the chip; DFX_PERSIST=0 switches it off) */
} dfx_stats;

typedef struct dfx_handle dfx_handle;

int dfx_create(const dfx_problem* problem, dfx_handle** out);
int dfx_destroy(dfx_handle* h);
const char* dfx_last_error(const dfx_handle* h);  /* h may be NULL: error of the last failed create */

int dfx_set_params(dfx_handle* h, const dfx_params* params);

/* Optional: pre-allocate device buffers for solves of up to `max_steps` RK steps and `max_timepoints`
 * outputs (trajectory checkpoint only when keep_trajectory != 0), so that later dfx_forward / dfx_adjoint
 * calls neither allocate nor re-instantiate their hipGraphs. */
int dfx_reserve(dfx_handle* h, int64_t max_steps, int32_t max_timepoints, int32_t keep_trajectory);

/* Let `h` keep its trajectory checkpoint in the buffers of `with` (same device) instead of its own: for handles whose solves never
 * overlap in time -- the engines of a multi-input objective (problems/quads_focusing_multi_input.py:66-86), each running forward +
 * reverse before the next starts.  One allocation instead of one per input, and room for a richer checkpoint level.  A reverse sweep
 * on a handle whose checkpoint has meanwhile been overwritten by another handle's forward pass fails with an error. */
int dfx_share_checkpoint(dfx_handle* h, dfx_handle* with);

/* Integrate from timepoints[0] with `steps_per_interval` equal RK steps between consecutive
 * timepoints.  state0: (batch, 2, n_blocks, 3), or NULL: every member starts at rest (the reference's problems all do,
 * problems/quads_focusing.py:300); fields: (batch, T, 2, n_blocks, 3) or NULL (they stay on the device), row 0 is the
 * reconstructed initial state.  keep_trajectory != 0 checkpoints every step state in HBM so that
 * dfx_adjoint can run afterwards. */
int dfx_forward(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                int32_t steps_per_interval, int32_t keep_trajectory, double* fields, dfx_stats* stats);

/* Same on a caller-chosen grid: steps_per_interval[k] steps between timepoints[k] and timepoints[k+1]
 * (n_timepoints - 1 entries); step_times == NULL: equal steps inside every interval; otherwise step_times holds the
 * sum(steps_per_interval) + 1 step boundaries, strictly increasing, with the boundary that starts interval k equal to
 * timepoints[k].  This is how the grid chosen by the adaptive controller (dfx_adaptive_step_counts /
 * dfx_adaptive_step_times) is made differentiable: dfx_adjoint is the exact reverse of this solve. */
int dfx_forward_grid(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                     const int32_t* steps_per_interval, const double* step_times, int32_t keep_trajectory,
                     double* fields, dfx_stats* stats);

/* The same with one time grid PER MEMBER: timepoints (batch, n_timepoints), step_times (batch, sum(steps_per_interval) + 1), required.
 * The step counts are shared (all members advance in the same launches), the times are not: forward inputs whose static phases differ
 * in length (problems/quads_kinetic_energy_static_tuning.py:246-259, mapped over devices with pmap at :473-478) are ensemble members
 * of one call.  dfx_adjoint reverses it like any other fixed-grid solve. */
int dfx_forward_grid_members(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                             const int32_t* steps_per_interval, const double* step_times, int32_t keep_trajectory,
                             double* fields, dfx_stats* stats);

/* The reference's own integrator semantics (jax.experimental.ode.odeint 0.4.8 called at dynamics.py:166): adaptive
 * Dormand-Prince 5(4), RMS error norm over the free (q, v) components with tolerance atol + rtol*max(|y0|,|y1|),
 * (state0 == NULL: every member starts at rest, as in dfx_forward / dfx_forward_grid)
 * step factor min(10, max(0.9 ratio^-1/5, 1 | 0.2)) applied on accept and reject, Hairer initial step, quartic dense
 * output at `timepoints` (steps are not clipped to output times).  Every member controls its own step.  Forward only:
 * the reverse sweep needs the fixed grid of dfx_forward.  stats->steps = accepted steps (max over members),
 * stats->rhs_evals = RHS evaluations (max over members). */
int dfx_forward_adaptive(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                         double rtol, double atol, int64_t max_attempts, double* fields, dfx_stats* stats);

/* The same solve, keeping what the reverse sweep needs (keep_trajectory != 0): the stage records of every ACCEPTED step (a rejected
 * attempt's records are overwritten in place), every member's own step boundaries, and for every output the step it was interpolated in.
 * dfx_adjoint / dfx_adjoint_kinetic / dfx_kinetic_value_and_grad[_device] then run the exact discrete adjoint of THIS solve with its step
 * sizes frozen -- the outputs' cotangents enter through the quartic dense output (an output at relative position r of step n adds g to
 * lambda_n and h_n B_j(r) g to the cotangent of stage slope j; the FSAL slope's share joins the first slope of the next step) -- so that
 * value_and_grad of the reference's default call, jit(value_and_grad(objective)) over odeint at dynamics.py:166, is ONE forward pass and
 * ONE reverse sweep here, and the gradient is the derivative of exactly the fields that were returned (neither the accept / reject
 * decisions nor the step sizes are differentiated; nor does the reference's continuous adjoint, jax.experimental.ode._odeint_rev).
 * fields may be NULL (they stay on the device).  keep_trajectory == 0: dfx_forward_adaptive. */
int dfx_forward_adaptive_keep(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                              double rtol, double atol, int64_t max_attempts, int32_t keep_trajectory, double* fields, dfx_stats* stats);

/* Failure isolation.  In the reference a member of an ensemble that diverges -- the list of forward problems of
 * problems/quads_focusing_multi_input.py:66-77, the pmap of quads_kinetic_energy_static_tuning.py:473-478 -- yields NaN for itself only.
 * dfx_member_status: status of every member after the last forward pass, (batch,): 0 ok, 1 non-finite state / error estimate, 2 step size
 * underflow, 3 step budget exceeded.  dfx_set_failure_policy(h, 1): such a member no longer fails the call (return 3 / 4) -- the call
 * returns 0, the member's outputs are NaN from the point of failure on (adaptive: from row 1 on), its status says why, the other members are
 * untouched, and a reverse sweep leaves NaN (fixed grid) or zeros (adaptive) in its gradients.  Default: 0, the call fails. */
int dfx_member_status(dfx_handle* h, int32_t* status);
int dfx_set_failure_policy(dfx_handle* h, int32_t isolate);

/* Accepted steps of the last dfx_forward_adaptive per member and output interval: counts (batch, n_timepoints - 1);
 * a step is counted in the interval that contains its start. */
int dfx_adaptive_step_counts(dfx_handle* h, int32_t* counts);

/* End times of the steps member `member` accepted in the last dfx_forward_adaptive: writes min(*n, capacity) values
 * into times and the number of accepted steps into *n (at most 2^20 steps per member are recorded). */
int dfx_adaptive_step_times(dfx_handle* h, int32_t member, double* times, int64_t capacity, int64_t* n);

/* Reverse sweep over the checkpointed trajectory of the last dfx_forward(keep_trajectory=1).
 * fields_bar: (batch, T, 2, n_blocks, 3) cotangent of `fields`. */
int dfx_adjoint(dfx_handle* h, const double* fields_bar, dfx_grads* grads, dfx_stats* stats);

/* ---- the samples of a DFX_FN_TABLE drive as a differentiable leaf (HIP library only) ----------------------------------------------------
 * g_f(t) = A interp(t - t_d; T, Y): the times T stay those of dfx_create (they are not differentiated), the values Y are a leaf like any
 * other.  `fn` names a time function of type DFX_FN_TABLE (anything else: return 1); n_tab = fn_table_n[fn].
 *
 * dfx_fn_table_values: new values for every member -- values (n_tab), or (batch, n_tab) with per_member != 0 -- without rebuilding the
 *   handle; they hold for every later call (dfx_set_params keeps them).  Like dfx_set_params it drops the kept trajectory.
 * dfx_fn_table_grads(h, 1): from now on every reverse sweep of the handle -- dfx_adjoint and every *_value_and_grad entry, on every
 *   checkpoint level and on the kept adaptive solve -- also keeps the cotangent gbar of the drive value g_f at every stage time (the
 *   "trace"; the sum over the member's DOFs of -(H w) con_coef on prescribed DOFs, w load_coef on loaded ones) and reduces it onto the
 *   samples: dL/dY[j] = A sum gbar hat_j(t - t_d), the end samples collecting everything at or beyond T[0] / T[n_tab - 1].  Such a sweep
 *   runs on stage launches in the build that also accumulates per-ligament gradients (dfx_stats.tile_kernels = 0), never on the
 *   persistent loops; it is refused (return 1) on lattices whose nodes carry more than one ligament.  Without the request every call
 *   launches what it launched before.  dfx_fn_table_grads(h, 0) switches it off.
 * dfx_fn_table_grad: the sample gradient (batch, n_tab) of the last such sweep.  The direct dependence of a prescribed OUTPUT row on its
 *   drive is not in it (as with fn_params): the caller adds fields_bar . hat weights for those rows.
 * dfx_drive_cotangent: the trace of one member, in the style of dfx_adaptive_step_times: *n = its number of stage evaluations (steps x
 *   stages in sweep order of time; the kept adaptive solve: the member's accepted steps and the evaluation at its final state),
 *   min(*n, capacity) stage times into `times` and, for function f, as many cotangents into gbar + f * capacity (either may be NULL).
 *   For any parameter p of function f the sweep's part of dL/dp is sum gbar[f] * dg_f/dp(times).
 * dfx_fn_table_tangents: per-direction sample tangents (n_dirs, batch, n_tab) for the forward-mode entries (dfx_forward_tangent*,
 *   dfx_rhs_jvp): direction k of a later call with the same n_dirs adds A interp(t - t_d; T, values_dots[k]) to the tangent of g_f.
 *   They stay until cleared (values_dots = NULL); a call with another number of directions is refused while they are set. */
int dfx_fn_table_values(dfx_handle* h, int32_t fn, const double* values, int32_t per_member);
int dfx_fn_table_grads(dfx_handle* h, int32_t enable);
int dfx_fn_table_grad(dfx_handle* h, int32_t fn, double* grad);
int dfx_drive_cotangent(dfx_handle* h, int32_t member, double* times, double* gbar, int64_t capacity, int64_t* n);
int dfx_fn_table_tangents(dfx_handle* h, int32_t fn, const double* values_dots, int32_t n_dirs);

/* Forward mode: the directional derivative of the fixed-grid solve (dfx_forward_grid, or dfx_forward_grid_members when
 * per_member_times != 0: timepoints (batch, n_timepoints), step_times (batch, sum(steps_per_interval) + 1) required) along
 * (state0_dot, params_dot), with its steps frozen.  fields (batch, T, 2, n_blocks, 3) is the primal history of the same call (equal to
 * dfx_forward_grid's to rounding); fields_dot = d fields / d(state0, params) . (state0_dot, params_dot).  On the same grid this is the
 * exact transpose of dfx_adjoint:  sum(fields_bar * fields_dot) == <dfx_adjoint(fields_bar), (state0_dot, params_dot)>.
 * params_dot has the shapes of dfx_params; a NULL array (or params_dot == NULL, state0_dot == NULL) is a zero tangent.  The primal
 * parameters are the ones dfx_set_params left on the handle; state0 == NULL: at rest.  The rows of PRESCRIBED DOFs in fields_dot hold the
 * tangent of c(t) in the position rows and 0 in the velocity rows (the caller assembles dc'/dp . dp if it needs them).
 * One stage launch per Runge-Kutta stage, primal and tangent in one pass (dual numbers).  This entry and dfx_forward_tangent_dense are
 * the _multi entries below with one direction ((batch, 1, ...) is (batch, ...)); supported: every bond model, no / angle-based /
 * distance-based contact, 3 and 4 nodes per block; nodes with more than one ligament return 1.  The call keeps its buffers to itself: the
 * trajectory checkpoint and the resident history of the last dfx_forward are left untouched, so a later dfx_adjoint still reverses THAT
 * solve.  Non-finite values in fields or fields_dot: return 3. */
int dfx_forward_tangent(dfx_handle* h, const double* state0, const double* state0_dot, const dfx_params* params_dot,
                        const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval,
                        const double* step_times, int32_t per_member_times,
                        double* fields, double* fields_dot, dfx_stats* stats);

/* Forward mode through the ADAPTIVE solve's dense output: the directional derivative of the map dfx_adjoint transposes after
 * dfx_forward_adaptive_keep.  Every member runs on its own accepted step boundaries, frozen: step_times (batch, stride), row m holds
 * t_0 .. t_{N_m} with N_m = n_steps[m] (dfx_adaptive_step_times gives t_1 .. t_{N_m}; t_0 = timepoints[0]); six Dopri5 stages per step,
 * output k taken from the step with t_n < timepoints[k] <= t_{n+1} by the quartic dense output the adaptive pass uses, which needs the
 * FSAL acceleration at y_{n+1} (after the last step: one extra evaluation at the final state, a step of size zero).  Output 0 is state0.
 * Neither the accept / reject decisions nor the step sizes are differentiated.  timepoints (n_timepoints), shared by the members.
 * Otherwise the contract of dfx_forward_tangent: fields / fields_dot (batch, T, 2, n_blocks, 3), buffers of its own (the checkpoint and
 * the resident history of the handle stay untouched: a dfx_adjoint after it still reverses the solve that was kept), every bond model
 * and contact model, one ligament per node; non-finite values, or a member the last forward pass flagged (dfx_member_status != 0):
 * return 3.  Return 1 (dfx_last_error says why) for a tableau other than dopri5, step times that do not increase,
 * t_0 != timepoints[0] or t_{N_m} < timepoints[n_timepoints - 1]. */
int dfx_forward_tangent_dense(dfx_handle* h, const double* state0, const double* state0_dot, const dfx_params* params_dot,
                              const double* timepoints, int32_t n_timepoints, const double* step_times, const int64_t* n_steps,
                              int64_t stride, double* fields, double* fields_dot, dfx_stats* stats);

/* The host half of dfx_forward_tangent_dense, on its own (no handle, no device): which outputs every frozen step holds and where.
 * out_ptr (batch, stride): outputs [out_ptr[m][n], out_ptr[m][n + 1]) lie in step n of member m (entries 0 .. N_m; out_ptr[m][0] = 1,
 * output 0 is the initial state); theta (batch, n_timepoints): (timepoints[k] - t_n) / (t_{n+1} - t_n), theta[m][0] = 0.  The rule and
 * the two IEEE operations are the adaptive controller's: timepoints[k] <= t_{n+1} puts an output on a step boundary into the step that
 * ends there.  Returns 0, or 1 step times not increasing, 2 t_0 != timepoints[0], 3 t_{N_m} < the last timepoint, 4 bad sizes. */
int dfx_dense_output_map(const double* step_times, const int64_t* n_steps, int64_t stride, int32_t batch,
                         const double* timepoints, int32_t n_timepoints, int32_t* out_ptr, double* theta);

/* Forward mode for SEVERAL directions per member: n_dirs directional derivatives of the same solve with the primal evaluated once per
 * stage (the stage kernel carries one value and KC epsilon parts; the library serves the n_dirs directions in ceil(n_dirs / KC) passes of
 * its compiled chunk widths, the spare directions of the last pass zero).  state0_dots (batch, n_dirs, 2, n_blocks, 3) or NULL;
 * params_dots: n_dirs entries, each with the shapes and the NULL rules of dfx_forward_tangent's params_dot (params_dots == NULL: every
 * parameter tangent zero).  fields (batch, T, 2, n_blocks, 3) comes from the first pass; fields_dots (batch, n_dirs, T, 2, n_blocks, 3),
 * column k = what dfx_forward_tangent / dfx_forward_tangent_dense return for direction k: the two single-direction entries are the
 * _multi entries with one direction.  Contracts, return codes and refusals are theirs; n_dirs < 1 returns 1.  The device
 * buffers of the call hold one pass (they do not grow with n_dirs) and are all allocated before the first pass: a failed allocation is
 * return 2 with nothing left behind.  stats->launches and kernel_ms cover all passes.  Where batch * n_blocks * n_dirs <= 65536 (too few
 * lanes to give every SIMD a wave) all directions run in ONE pass instead, spread over lanes at width 1, which is the cheaper form there;
 * the environment variable DFX_TANGENT_MULTI_FORM=chunked|spread forces either form (one direction is one pass of width 1 in both). */
int dfx_forward_tangent_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                              int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval,
                              const double* step_times, int32_t per_member_times,
                              double* fields, double* fields_dots, dfx_stats* stats);
int dfx_forward_tangent_dense_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                    int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const double* step_times,
                                    const int64_t* n_steps, int64_t stride, double* fields, double* fields_dots, dfx_stats* stats);

/* Forward-mode SIGNALS: the two _multi solves above with the history kept on the device.  Instead of fields / fields_dots the call
 * returns the signals of a term list (dfx_signal_values: terms (signal, block, component, coef), components 0..2 displacement, 3..5
 * velocity, 6..8 elastic force dE/d(x, y, theta) on the block, 9 + 3 node + dof the part of it one hinge carries) and their tangents: signals (batch, T, n_signals), from the first pass, and
 * signals_dots (batch, n_dirs, T, n_signals) -- the columns of the Jacobian of a least-squares fit of those signals.  At the end of every
 * pass the force channels and their tangents K(u) du + (d grad_u E / dp) dp are evaluated on the pass's own buffers (one dual-number
 * evaluation of the ligament gradient per listed slot and output time, with the pass's parameter tangents), the terms are added in list
 * order, and (batch, KT, T, n_signals) is downloaded; no atomics, every sum in a fixed order, so a repeated call returns the same bits.
 *   * column k of signals_dots is the derivative of dfx_signal_values along direction k of the same solve; on the same grid it is the
 *     transpose of dfx_signal_misfit_value_and_grad: sum_ks c_ks Sdot_ks == <gradient, direction> with c = tau omega (S - Starget);
 *   * prescribed DOFs: their position rows carry the exact tangent of c(t), so displacement terms on them and force terms on or beside a
 *     driven block are complete.  Their velocity rows are 0, as in dfx_forward_tangent: for a field term on the velocity of a prescribed
 *     DOF the column holds 0 and the caller adds coef * dc'/dp . dp;
 *   * contracts, return codes and refusals are those of dfx_forward_tangent_multi / dfx_forward_tangent_dense_multi, plus those of
 *     dfx_signal_values (return 1): a signal, block or component out of range, an empty signal, a non-finite coefficient, force
 *     components with the distance-based contact or on nodes with extra ligaments; signals or signals_dots NULL.  Non-finite fields or
 *     tangents anywhere in a member (also on blocks no term names): return 3 -- found by a pass over the history on the device, one
 *     flag per workgroup, ORed by the host;
 *   * the channels, signals, flags and term tables are allocated with the call's other buffers before the first pass and sized for the
 *     widest pass: a failed allocation is return 2 with nothing left behind.  Both pass forms serve it (DFX_TANGENT_MULTI_FORM keeps its
 *     meaning).  The trajectory checkpoint, the resident history and the signal tables of the handle are not touched: a dfx_adjoint or
 *     a dfx_signal_* call after it still sees the last dfx_forward. */
int dfx_forward_tangent_signals_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                      int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const int32_t* steps_per_interval,
                                      const double* step_times, int32_t per_member_times,
                                      int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                                      const double* term_coef, int32_t n_signals,
                                      double* signals, double* signals_dots, dfx_stats* stats);
int dfx_forward_tangent_signals_dense_multi(dfx_handle* h, const double* state0, const double* state0_dots, const dfx_params* params_dots,
                                            int32_t n_dirs, const double* timepoints, int32_t n_timepoints, const double* step_times,
                                            const int64_t* n_steps, int64_t stride,
                                            int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                            const int32_t* term_component, const double* term_coef, int32_t n_signals,
                                            double* signals, double* signals_dots, dfx_stats* stats);

/* Device-resident variants for benchmarking: the forward keeps the (T, ...) fields on the device and
 * the cotangent is the target-kinetic-energy objective  sum_t sum_{b in target} m_bd v_bd^2 / 2
 * (energy.py:494-499, problems/quads_focusing.py:447-467), evaluated on the device. */
int dfx_objective_kinetic(dfx_handle* h, const int32_t* target_blocks, int32_t n_target, double* objective);
int dfx_adjoint_kinetic(dfx_handle* h, const int32_t* target_blocks, int32_t n_target, dfx_grads* grads,
                        dfx_stats* stats);

/* The same objective and gradient in one call and without host-side copies: what jit(value_and_grad(objective)) returns at
 * problems/quads_focusing.py:565.  `objective` (batch,) may be NULL.  Non-NULL entries of `want` select the gradients; `views`
 * receives pointers to them in LIBRARY-OWNED (pinned) memory, laid out as in dfx_grads, valid until the next call on the handle.
 * The accumulators are re-laid-out on the device, so the host does no scatter work. */
int dfx_kinetic_value_and_grad(dfx_handle* h, const int32_t* target_blocks, int32_t n_target, double* objective,
                               const dfx_grads* want, dfx_grads* views, dfx_stats* stats);

/* The same call with the gradients left where the reverse sweep accumulated them: `device_views` receives DEVICE pointers (HBM of the
 * handle's GPU, dfx_grads layout, valid until the next call on the handle) -- what jit(value_and_grad(objective)) hands back in the
 * reference: device arrays, nothing crosses PCIe but the (batch,) objective.  Available for centroid_node_vectors, void_angle0,
 * inertia, damping, state0, block_centroids on lattices without extra ligaments; asking for an entry the library assembles on the host
 * (reference_vector, k_bond, contact, fn_params) returns 1.  dfx_download copies n doubles behind such a pointer to host memory
 * (through the pinned staging area).  A device-side consumer (the design map, an optimiser update, dfx_reduce_grads) reads them in place. */
int dfx_kinetic_value_and_grad_device(dfx_handle* h, const int32_t* target_blocks, int32_t n_target, double* objective,
                                      const dfx_grads* want, dfx_grads* device_views, dfx_stats* stats);
int dfx_download(dfx_handle* h, double* dst, const double* device_src, int64_t n);

/* Forward solve + objective + reverse sweep in ONE call -- jit(value_and_grad(objective))(design) at problems/quads_focusing.py:565 is one
 * XLA program too.  Equal to dfx_forward_grid(keep_trajectory = 1, fields = NULL) followed by dfx_kinetic_value_and_grad[_device]
 * (device_views != 0: `views` receives device pointers) bit for bit; the host does not wait for the forward pass before it enqueues the
 * sweep (one synchronisation and one round trip through the caller less: ~0.15 ms of a 5 ms job).  A non-finite forward state is
 * reported at the end (return 3, as dfx_forward; the sweep has then run on that state and its outputs are meaningless).
 * steps_per_interval: (n_timepoints - 1,); state0 NULL = at rest. */
int dfx_forward_kinetic_value_and_grad(dfx_handle* h, const double* state0, const double* timepoints, int32_t n_timepoints,
                                       const int32_t* steps_per_interval, const int32_t* target_blocks, int32_t n_target,
                                       double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views,
                                       dfx_stats* forward_stats, dfx_stats* adjoint_stats);

/* Weighted objectives on the device-resident history (HIP library only).  The other objectives of the reference's problems/ directory are
 * weighted sums over blocks and output times too, and get what the kinetic entries above give: the fields never leave HBM, the
 * objective rides along with the reverse sweep, and a list of designs runs as one ensemble.
 *   DFX_OBJ_KINETIC            J_m = sum_k tau_k sum_b w_mb sum_d p_mbd v_mkbd^2 / 2
 *                              (problems/quads_energy_splitting.py:66-88: w = the weights of the target regions, overlaps added)
 *   DFX_OBJ_ANGULAR_MOMENTUM   J_m = sum_k tau_k sum_b w_mb [ (a_x + u_x) m_y v_y - (a_y + u_y) m_x v_x + J omega ]
 *                              (problems/quads_spin.py:380-430 with energy.py:502-519)
 * p = (m_x, m_y, J) is the inertia of dfx_set_params, (u, v) the history of the last forward pass.
 * block_weights: (batch, n_blocks) when weights_per_member != 0, else (n_blocks,) shared by all members; blocks whose weight is zero in
 * every member cost nothing.  time_weights: NULL = all ones, else EXACTLY T = n_timepoints of the last forward pass doubles (the library
 * reads that many and cannot check the length of the caller's array).  lever0 (angular kind; ignored by the kinetic kind): a = block
 * centroid - spin centre, (batch, n_blocks, 2) when lever_per_member != 0, else (n_blocks, 2) -- passed by the caller, so the library
 * needs no centroid image on lattices without distance contact.  objective: (batch,), may be NULL in the gradient call.
 * dfx_objective_value needs a forward pass whose history is resident.  dfx_objective_value_and_grad equals dfx_adjoint on the
 * fields_bar of these formulas (position rows as well as velocity rows) PLUS the explicit terms d J / d inertia and, angular kind,
 * d J / d block_centroids = d J / d a (available on every lattice for this call; with distance contact it is added to what the sweep
 * accumulated) -- same cotangent buffer, same sweep, for every sweep form and checkpoint level, the kept steps of an adaptive solve
 * included.  Preconditions and refusals are those of dfx_kinetic_value_and_grad[_device]; want / views as there, device_views != 0:
 * `views` receives device pointers.  The value is a fixed-order two-level sum: two calls on the same history return the same bits.  With
 * 0/1 weights and time_weights == NULL the kinetic kind is dfx_kinetic_value_and_grad up to the order of that sum.
 * Return 1 (dfx_last_error says why): unknown kind, lever0 == NULL for the angular kind, non-finite weights or levers. */
enum { DFX_OBJ_KINETIC = 0, DFX_OBJ_ANGULAR_MOMENTUM = 1 };
int dfx_objective_value(dfx_handle* h, int32_t kind, const double* block_weights, int32_t weights_per_member,
                        const double* time_weights, const double* lever0, int32_t lever_per_member, double* objective);
int dfx_objective_value_and_grad(dfx_handle* h, int32_t kind, const double* block_weights, int32_t weights_per_member,
                                 const double* time_weights, const double* lever0, int32_t lever_per_member,
                                 double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats);

/* The elastic energy stored in the ligaments as an objective on the device-resident history (HIP library only): for member m, with bond
 * weights w_mb, output-time weights tau_k and four part coefficients c = parts4 = (c_stretch, c_shear, c_bend, c_contact),
 *   J_m = sum_k tau_k sum_bonds w_mb [ c_stretch E_stretch + c_shear E_shear + c_bend E_bend + c_contact E_contact ](bond; u_k, params_m)
 * E_stretch, E_shear, E_bend: the three terms of the handle's bond model (for nonlinear ligaments what dfx_response_data writes; a part a
 * model does not have contributes nothing), E_contact: the angle-contact penalty of the bond's two void angles, u_k the displacement part
 * of the history.  The energies are linear in the stiffnesses, so J is the plain energy with (c_stretch k_stretch, c_shear k_shear,
 * c_bend k_rot) and c_contact k_contact: one evaluation gives the value and every first derivative.
 * bond_weights: (batch, n_bonds) when weights_per_member != 0, else (n_bonds,), in the order of the problem's bond list; bonds whose weight
 * is zero in every member cost nothing.  time_weights: NULL = all ones, else EXACTLY T doubles.  objective: (batch,), may be NULL in the
 * gradient call.  dfx_strain_objective_value works after any forward pass; dfx_strain_objective_value_and_grad needs the kept trajectory
 * and equals dfx_adjoint on the fields_bar of this formula (the weighted ligament force on the position rows; velocity rows zero) PLUS the
 * explicit terms: d J / d centroid_node_vectors, d J / d void_angle0 and -- when want asks for them -- d J / d(reference_vector, k_bond,
 * contact).  As with dfx_adjoint, the direct dependence of a PRESCRIBED output DOF on the parameters of its time function is not part of
 * fn_params (the caller adds it from fields_bar; solve_dynamics.vjp does).  want / views / device_views / stats, the sweep forms, the
 * two-level fixed-order sum of the value and the refusals of a missing trajectory or a stale shared checkpoint are those of
 * dfx_objective_value_and_grad; without reference_vector / k_bond / contact in `want` the reverse sweep runs the same builds as for the
 * kinetic kinds.
 * Return 1 (dfx_last_error says why): a NULL bond_weights / parts4 (/ objective in the value call), a non-finite weight or part,
 * c_contact != 0 on a lattice without the angle contact (the distance-based contact energy is not part of this objective), nodes with
 * more than one ligament. */
int dfx_strain_objective_value(dfx_handle* h, const double* bond_weights, int32_t weights_per_member, const double* time_weights,
                               const double* parts4, double* objective);
int dfx_strain_objective_value_and_grad(dfx_handle* h, const double* bond_weights, int32_t weights_per_member, const double* time_weights,
                                        const double* parts4, double* objective, const dfx_grads* want, dfx_grads* views,
                                        int32_t device_views, dfx_stats* stats);

/* The peak ligament strain as an objective or constraint on the device-resident history (HIP library only): a smooth maximum over output
 * times and ligaments instead of a weighted sum.  For member m, output time k and every ligament b with a non-zero weight
 *   q_mkb = a_mb (l0 eps)^2 + s_mb (l0 gamma)^2 + r_mb kappa^2
 *         = 2 E_bond(b; u_mk) of the handle's bond model with (a_mb, s_mb, r_mb) = bond_coef in place of (k_stretch, k_shear, k_rot)
 *   W_mkb = tau_k omega_mb                       (tau = time_weights, omega = bond_weights, both >= 0; a zero weight excludes the pair)
 *   peak  q_hat_m = max over W > 0 of q_mkb at (k_hat, b_hat); on ties the lowest k, then the lowest bond
 *   DFX_PEAK_KS     J_m = q_hat_m + log( sum W exp(beta (q - q_hat_m)) ) / beta      pi = W exp(beta (q - J))          (sum pi = 1)
 *   DFX_PEAK_PNORM  J_m = q_hat_m ( sum W (q / q_hat_m)^p )^(1/p)                    pi = W q^(p-1) J^(1-p)            (J = 0: pi = 0)
 *   dJ_m = sum pi_mkb dq_mkb
 * (l0 eps, l0 gamma, kappa: the stretch elongation, the shear displacement and the bend angle of the ligament models; a part a model does
 * not have contributes nothing).  With a = 1 / (l0 eps_lim)^2, s = 1 / (l0 gamma_lim)^2, r = 1 / kappa_lim^2, q is the squared utilisation
 * of the ligament and J <= 1 a strain limit.  The coefficients are CONSTANTS of the call: the reference_vector gradient is that of q at
 * fixed (a, s, r) and does not see how a caller derived them from l0.
 * bond_coef: (batch, n_bonds, 3) when coef_per_member != 0, else (n_bonds, 3); bond_weights: (batch, n_bonds) when weights_per_member != 0,
 * else (n_bonds,), NULL = all ones; time_weights: NULL = all ones, else EXACTLY T doubles; sharpness: beta > 0 (KS) or p >= 1 (PNORM).
 * objective: (batch,), may be NULL in the gradient call; peak: (batch,) q_hat or NULL; peak_at: (batch, 2) int32 (output, bond) or NULL.
 * dfx_strain_peak_value works after any forward pass; dfx_strain_peak_value_and_grad needs the kept trajectory and equals dfx_adjoint on
 * the fields_bar of these formulas (sum_b pi dq/du on the position rows; velocity rows zero) PLUS the explicit terms d J /
 * d centroid_node_vectors and -- when want asks for it -- d J / d reference_vector.  q does not depend on the stiffnesses, the contact
 * constants or the void angles: k_bond, contact and void_angle0 receive what the sweep accumulates and nothing explicit.  The direct
 * dependence of a PRESCRIBED output DOF on its time function is not part of fn_params, as for the other device objectives.  want / views /
 * device_views / stats, the sweep forms and checkpoint levels, the kept steps of an adaptive solve and the refusals of a missing trajectory
 * or a stale shared checkpoint are those of dfx_strain_objective_value_and_grad.  Maximum and sum are fixed-order two-level reductions
 * without atomics: two calls on the same history return the same bits for J, peak, peak_at and every gradient.
 * A member whose history is not finite (every q NaN) gets peak = -inf, J = NaN and peak_at = (-1, -1).
 * Return 1 (dfx_last_error says why): no forward pass, a NULL bond_coef (/ objective in the value call), a non-finite or negative
 * coefficient or weight, all weights zero for some member, an unknown aggregate, sharpness not finite, beta <= 0 or p < 1, nodes with more
 * than one ligament. */
enum { DFX_PEAK_KS = 0, DFX_PEAK_PNORM = 1 };
int dfx_strain_peak_value(dfx_handle* h, const double* bond_coef, int32_t coef_per_member, const double* bond_weights,
                          int32_t weights_per_member, const double* time_weights, int32_t aggregate, double sharpness, double* objective,
                          double* peak, int32_t* peak_at);
int dfx_strain_peak_value_and_grad(dfx_handle* h, const double* bond_coef, int32_t coef_per_member, const double* bond_weights,
                                   int32_t weights_per_member, const double* time_weights, int32_t aggregate, double sharpness,
                                   double* objective, double* peak, int32_t* peak_at, const dfx_grads* want, dfx_grads* views,
                                   int32_t device_views, dfx_stats* stats);

/* Signal misfit on the device-resident history (HIP library only): a least-squares misfit between target histories and signals that are
 * linear combinations of displacement, velocity and elastic-force components of chosen blocks -- the objective of the hinge
 * characterisation (problems/hinge_characterization.py: the reaction force on the driven DOFs against a measured one), of a calibration
 * against tracked block motions and of waveform shaping.  For member m, output time k and signal s
 *   S_mks = sum over the terms of signal s: coef * channel(block, component; fields_mk, params_m)
 *   J_m   = 1/2 sum_k tau_k sum_s omega_s (S_mks - Starget_mks)^2
 * component 0..2: the displacement x, y, theta of the block; 3..5: its velocity; 6..8: the elastic force dE/d(x, y, theta) on it, E the
 * ligament plus angle-contact energy the handle was created with, at output configuration k with member m's parameters, prescribed DOFs at
 * the values the fields hold (no damping, no loading, no velocity: what dfx_rhs gives for a state at rest, times the inertia, with the sign
 * of an energy gradient).
 * component 9 + 3 n + d (n = 0 .. nodes per block - 1, d = 0, 1, 2): the HINGE force dE_h/d(x, y, theta)_block, E_h the energy of the one
 * ligament on node n of the block -- its bond energy and, with the angle contact, the penalty of its two void angles: the summand of
 * components 6..8, with their sign and units (the hinge pulls on the block with minus it; the hinge channels of a block add up to its
 * components 6..8; on the two ends of a ligament the x and y channels are opposite).  What one ligament carries, and -- summed over a line
 * of hinges -- what crosses a cut; paired with a velocity in dfx_signal_xcorr_value (DFX_XCORR_NORM_NONE, lag 0) the energy that crosses it.
 * Its cotangent is Hess(E_h) w_h on both end blocks, its explicit terms reach the parameters of that ligament alone.
 * The hinge components are OFF on a new handle -- component 9 and above are then out of range, as they were before these channels
 * existed -- and dfx_signal_hinge_channels(h, 1) switches them on for every entry that takes signal terms (these, the projections, the
 * cross-correlation, dfx_forward_tangent_signals_*), until dfx_signal_hinge_channels(h, 0).  Returns 0.
 * Terms are parallel arrays of n_terms entries (term_signal in 0..n_signals-1, term_block, term_component, term_coef); a signal adds its
 * terms in list order.  targets: (batch, T, n_signals) when targets_per_member != 0, else (T, n_signals); signal_weights omega: (n_signals,)
 * or NULL = ones; time_weights tau: EXACTLY T doubles or NULL = ones.
 * dfx_signal_values writes S (batch, T, n_signals) and dfx_signal_misfit_value J (batch,) after any forward pass.
 * dfx_signal_misfit_value_and_grad needs the kept trajectory and equals dfx_adjoint on the fields_bar of these formulas -- coef * c on the
 * row of a field term, c = tau omega (S - Starget), and for force terms the Hessian-vector product K(u_k) w on the position rows, w = sum
 * coef * c on the listed force DOFs -- PLUS the explicit terms of the force channels, the mixed derivatives d(w . grad E)/dp:
 * centroid_node_vectors, void_angle0 and, when `want` asks for them, reference_vector, k_bond, contact.  Both come from one dual-number
 * evaluation of the ligament gradient.  As with dfx_adjoint and the other device objectives, the direct dependence of a PRESCRIBED output
 * DOF on the parameters of its time function is not part of fn_params (the caller adds it from fields_bar; for a force term on or next to
 * a driven block that is (K w) on the driven DOF times d drive / d parameter).  want / views / device_views / stats, the sweep forms, the
 * fixed-order sum of the value (no atomics: the same history gives the same bits) and the refusals of a missing trajectory or a stale
 * shared checkpoint are those of dfx_strain_objective_value_and_grad; without reference_vector / k_bond / contact in `want` the reverse
 * sweep runs the same builds as for the kinetic kinds.  Signals of field components alone work for every physics the sweep serves.
 * Return 1 (dfx_last_error says why): no forward pass (no kept trajectory for the gradient call), a signal, block or component out of
 * range, a signal without terms, a NULL or non-finite argument, force or hinge components on a problem with the distance-based contact or
 * with nodes that carry more than one ligament, a hinge component while they are off, on a node the lattice's blocks do not have or on one
 * that carries no ligament. */
int dfx_signal_hinge_channels(dfx_handle* h, int32_t enable);
int dfx_signal_values(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                      const double* term_coef, int32_t n_signals, double* values);
int dfx_signal_misfit_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                            const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* targets,
                            int32_t targets_per_member, const double* signal_weights, const double* time_weights, double* objective);
int dfx_signal_misfit_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                     const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* targets,
                                     int32_t targets_per_member, const double* signal_weights, const double* time_weights,
                                     double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats);

/* Signal projections on the device-resident history (HIP library only): the signals S_mks of dfx_signal_values (the same term arrays, the
 * same components 0..20) projected on n_rows rows of a time basis, and a weighted quadratic form of the coefficients -- band power (a cos
 * and a sin row per frequency with equal weights), transmission at the drive frequency, harmonic generation, a matched filter (one row
 * holding the shifted template).  For member m, signal s and row j
 *   P_msj = sum_k B_jk S_mks                              k = 0 .. T-1
 *   J_m   = 1/2 sum_s sum_j W_sj (P_msj - Ptarget_msj)^2
 *   c_mks = sum_j W_sj (P_msj - Ptarget_msj) B_jk         the cotangent of J on the signals
 * basis B: (n_rows, T), shared by the members; the library does no trigonometry: quadrature weights and windows are baked into the rows.
 * row_weights W: (n_signals, n_rows), entries of any sign or zero.  targets Ptarget: (batch, n_signals, n_rows) when targets_per_member
 * != 0, else (n_signals, n_rows); NULL = zeros.  With B the identity, W_sk = tau_k omega_s and Ptarget = Starget this is the signal misfit.
 * basis must hold EXACTLY n_rows * T doubles, T the n_timepoints of the last forward pass, row_weights n_signals * n_rows and targets
 * n_signals * n_rows (times batch when per member): the library cannot check a length.
 * dfx_signal_projections writes P (batch, n_signals, n_rows) and dfx_signal_projection_value J (batch,) after any forward pass.
 * dfx_signal_projection_value_and_grad needs the kept trajectory and equals dfx_adjoint on the fields_bar of these formulas -- c takes
 * the place of tau omega (S - Starget) in dfx_signal_misfit_value_and_grad, all that follows it is that entry's: coef * c on the row of a
 * field term, K(u_k) w on the position rows for force terms, PLUS the explicit terms of the force channels.  want / views / device_views /
 * stats, the sweep forms, the checkpoint levels, the kept steps of an adaptive solve, what fn_params holds and the refusals of a missing
 * trajectory or a stale shared checkpoint are those of dfx_signal_misfit_value_and_grad.  Every sum has a fixed order (lane l of a wave
 * adds outputs l, l + 64, ... ascending, then the shuffle tree; rows ascending in c) and no atomics: the same history gives the same bits.
 * Return 1 (dfx_last_error says why): n_rows < 1, a NULL or non-finite basis or row_weights, non-finite targets, and everything the
 * signal entries refuse. */
int dfx_signal_projections(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                           const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows, double* values);
int dfx_signal_projection_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows,
                                const double* row_weights, const double* targets, int32_t targets_per_member, double* objective);
int dfx_signal_projection_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                         const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis,
                                         int32_t n_rows, const double* row_weights, const double* targets, int32_t targets_per_member,
                                         double* objective, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats);

/* Signal cross-correlation on the device-resident history (HIP library only): the normalised cross-correlation of pairs of the signals
 * S_mks of dfx_signal_values (the same term arrays, the same components 0..8) over time lags, its peak and the delay of the peak -- the
 * measures of difflexmm/objective.py (compute_xcorr*, compute_space_time_xcorr: pairs are the space rows at zero space shift) as an
 * objective: a pulse that keeps its shape at any delay, a chosen arrival time, a template at an unknown shift.
 * Pairs: n_pairs entries (pair_a[p], pair_b[p]); pair_a is a signal index; pair_b >= 0 a signal index, pair_b < 0 names column
 * -1 - pair_b of the fixed template array `templates`, (T, n_templates) shared by the members or (batch, T, n_templates) when
 * templates_per_member != 0 (EXACTLY that many doubles, T the n_timepoints of the last forward pass; NULL when no pair names a column).
 * A signal may stand on both sides of a pair and in several pairs.  With A_p[k], B_p[k] the two sides at output k, lags in OUTPUT
 * INDICES d = -max_lag .. max_lag, 0 <= max_lag <= T - 1, per member, all fp64:
 *   R[d]   = sum_p sum_{k : 0 <= k < T, 0 <= k + d < T} A_p[k] B_p[k + d]          d > 0: B lags A (the reference's `delay`)
 *   EA     = sum_p sum_k A_p[k]^2,   EB = sum_p sum_k B_p[k]^2
 *   rho[d] = R[d] / N     N = EA (DFX_XCORR_NORM_REFERENCE: the peak of A's auto-correlation, what compute_xcorr* divide by),
 *                         sqrt(EA EB) (DFX_XCORR_NORM_COEFFICIENT) or 1 (DFX_XCORR_NORM_NONE)
 * and a reduction over the lags to a peak M and a delay delta:
 *   DFX_XCORR_AT       M = rho[lag0], delta = lag0
 *   DFX_XCORR_MAX      M = max_d rho[d], delta its argmax; on ties the lowest d wins and takes the whole gradient (the subgradient
 *                      np.argmax implies; JAX's max splits a tie evenly -- ties are a set of measure zero)
 *   DFX_XCORR_SOFTMAX  M = (1 / beta) log sum_d exp(beta rho[d]) (the maximum subtracted first), pi = softmax(beta rho),
 *                      delta = sum_d d pi_d;  beta > 0
 *   J = w_peak M + 1/2 w_delay (delta - delay_target)^2          (w_peak < 0 maximises the correlation)
 * The cotangent of J: g_d = dJ/d rho[d] = w_peak at lag0 / at the argmax and zero elsewhere, or
 * w_peak pi_d + w_delay (delta - delay_target) beta pi_d (d - delta);  Rbar[d] = g_d / N, Nbar = - sum_d g_d rho[d] / N; on the energies
 * (eA, eB) = (Nbar, 0), (Nbar N / (2 EA), Nbar N / (2 EB)) or (0, 0) for the three normalisations; on the signals
 *   c[k, s] = sum_{p : a_p = s} ( sum_d Rbar[d] B_p[k + d] + 2 eA A_p[k] ) + sum_{p : b_p = s} ( sum_d Rbar[d] A_p[k - d] + 2 eB B_p[k] )
 * (outputs outside [0, T) contribute nothing; template columns receive nothing).  A member whose N is exactly 0 (a signal on a clamped
 * DOF) gets J = M = delta = rho = NaN and an all-zero cotangent: no division by zero reaches the sweep, the other members are unaffected.
 * dfx_signal_xcorr writes rho (batch, 2 max_lag + 1), lag d at index d + max_lag, and dfx_signal_xcorr_value J (batch,), M into `peak` and
 * delta into `delay` ((batch,) each, may be NULL) after any forward pass.  dfx_signal_xcorr_value_and_grad needs the kept trajectory and
 * equals dfx_adjoint on the fields_bar of these formulas -- c takes the place of tau omega (S - Starget) in
 * dfx_signal_misfit_value_and_grad, all that follows is that entry's, as for dfx_signal_projection_value_and_grad: want / views /
 * device_views / stats, the sweep forms, the checkpoint levels, the kept steps of an adaptive solve, what fn_params holds and the
 * refusals of a missing trajectory or a stale shared checkpoint.  Every sum has a fixed order and no atomics -- R, EA, EB: lane l of a
 * wave adds outputs l, l + 64, ... ascending with the pairs ascending inside, then the shuffle tree; the reduction: lane l holds lags
 * l, l + 64, ..., the maximum first, then the exponent sums; c: the A-side pairs then the B-side pairs, pairs and lags ascending -- so
 * the same history gives the same bits.
 * Return 1 (dfx_last_error says why): n_pairs < 1, a NULL pair array, a pair index or template column out of range, a template column
 * named with templates == NULL, max_lag outside [0, T - 1], an unknown normalisation or reduction, lag0 outside [-max_lag, max_lag]
 * (DFX_XCORR_AT), beta <= 0 or non-finite (DFX_XCORR_SOFTMAX), w_delay != 0 without DFX_XCORR_SOFTMAX, a non-finite template, weight or
 * delay_target, and everything the signal entries refuse. */
#define DFX_XCORR_NORM_REFERENCE 0
#define DFX_XCORR_NORM_COEFFICIENT 1
#define DFX_XCORR_NORM_NONE 2
#define DFX_XCORR_AT 0
#define DFX_XCORR_MAX 1
#define DFX_XCORR_SOFTMAX 2
int dfx_signal_xcorr(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                     const double* term_coef, int32_t n_signals, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b,
                     const double* templates, int32_t n_templates, int32_t templates_per_member, int32_t max_lag, int32_t normalisation,
                     double* values);
int dfx_signal_xcorr_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                           const int32_t* term_component, const double* term_coef, int32_t n_signals, int32_t n_pairs, const int32_t* pair_a,
                           const int32_t* pair_b, const double* templates, int32_t n_templates, int32_t templates_per_member, int32_t max_lag,
                           int32_t normalisation, int32_t reduce, int32_t lag0, double beta, double w_peak, double w_delay,
                           double delay_target, double* objective, double* peak, double* delay);
int dfx_signal_xcorr_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                    const int32_t* term_component, const double* term_coef, int32_t n_signals, int32_t n_pairs,
                                    const int32_t* pair_a, const int32_t* pair_b, const double* templates, int32_t n_templates,
                                    int32_t templates_per_member, int32_t max_lag, int32_t normalisation, int32_t reduce, int32_t lag0,
                                    double beta, double w_peak, double w_delay, double delay_target, double* objective, double* peak,
                                    double* delay, const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats);

/* Signal spectral ratios on the device-resident history (HIP library only): ratios of band powers of the projections P_msj = sum_k B_jk S_mks
 * of dfx_signal_projections (the same term arrays, components 0..20, basis and hinge opt-in) -- transmissibility (the band power that
 * arrives over the band power that went in, in dB), a band gap (the worst transmission over a band of frequencies), harmonic generation
 * (the power at 2 f over the power at f).  n_groups = G >= 1 groups of a numerator and a denominator form, per member m:
 *   N_mg = n0_g + sum_s sum_j Wn_gsj P_msj^2          D_mg = d0_g + sum_s sum_j Wd_gsj P_msj^2
 * num_weights Wn, den_weights Wd: (G, n_signals, n_rows), entries >= 0, shared by the members.  num_offset n0, den_offset d0: (G,) shared,
 * or (batch, G) when offsets_per_member != 0, entries >= 0; NULL = zeros.  d0_g > 0 with Wd_g all zero normalises by a known constant (the
 * band power of a prescribed drive).  The measure of a group and the aggregate over the groups (group_coef a_g of any sign):
 *   DFX_SPECTRUM_RATIO  l_mg = N_mg / D_mg
 *   DFX_SPECTRUM_LOG    l_mg = ln N_mg - ln D_mg                (dB = 10 / ln 10 * l)
 *   DFX_SPECTRUM_SUM    J_m = sum_g a_g l_mg
 *   DFX_SPECTRUM_KS     z_g = a_g l_mg, M = max_g z_g (lowest g on a tie), J_m = M + ln( sum_g exp(beta (z_g - M)) ) / beta,  beta > 0
 * (a = +1 with KS: the worst-case transmission of a stop band, to be minimised; a = -1: minus the weakest transmission of a pass band.)
 * The cotangent: lam_g = dJ/dl_g = a_g (SUM) or a_g softmax(beta z)_g (KS); (dl/dN, dl/dD) = (1/D, -N/D^2) (RATIO) or (1/N, -1/D) (LOG);
 *   Weff_msj = 2 sum_g lam_g (dl_g/dN Wn_gsj + dl_g/dD Wd_gsj)     g ascending
 *   c_mks    = sum_j Weff_msj P_msj B_jk                           j ascending, the cotangent of J on the signals
 * A member for which some D_mg <= 0 (DFX_SPECTRUM_LOG: or some N_mg <= 0; DFX_SPECTRUM_KS: or some l_mg is not finite) gets J = NaN, NaN in
 * the offending l_mg and an all-zero cotangent: no division by zero reaches the sweep, the other members are unaffected.
 * dfx_signal_spectrum takes `measure` alone and writes (batch, G, 3) = N | D | l (NaN in l where the rule above says so), and dfx_signal_spectrum_value J (batch,) and
 * the measures l (batch, G) into `measures` (may be NULL), after any forward pass.  dfx_signal_spectrum_value_and_grad needs the kept
 * trajectory and equals dfx_adjoint on the fields_bar of these formulas -- c takes the place of tau omega (S - Starget) in
 * dfx_signal_misfit_value_and_grad, all that follows is that entry's, as for dfx_signal_projection_value_and_grad: want / views /
 * device_views / stats, the sweep forms, the checkpoint levels, the kept steps of an adaptive solve, what fn_params holds and the refusals
 * of a missing trajectory or a stale shared checkpoint.  Every sum has a fixed order and no atomics -- N, D: lane l of a wave adds the
 * flattened (signal, row) pairs l, l + 64, ... ascending (zero weights add nothing), the shuffle tree, then the offset; the reduction: lane
 * l holds groups l, l + 64, ..., the measures first, then the maximum, then the exponent sums -- so the same history gives the same bits.
 * The arrays must hold EXACTLY the sizes stated: the library cannot check a length.
 * Return 1 (dfx_last_error says why): n_groups < 1, a NULL num_weights or den_weights, a negative or non-finite weight or offset, a group
 * whose numerator has no positive weight and a zero offset, an unknown measure or aggregate, beta <= 0 or non-finite (DFX_SPECTRUM_KS), a
 * NULL or non-finite group_coef, and everything the projection entries refuse. */
#define DFX_SPECTRUM_RATIO 0
#define DFX_SPECTRUM_LOG 1
#define DFX_SPECTRUM_SUM 0
#define DFX_SPECTRUM_KS 1
int dfx_signal_spectrum(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block, const int32_t* term_component,
                        const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows, int32_t n_groups,
                        const double* num_weights, const double* den_weights, const double* num_offset, const double* den_offset,
                        int32_t offsets_per_member, int32_t measure, double* values);
int dfx_signal_spectrum_value(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                              const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis, int32_t n_rows,
                              int32_t n_groups, const double* num_weights, const double* den_weights, const double* num_offset,
                              const double* den_offset, int32_t offsets_per_member, int32_t measure, int32_t aggregate, double beta,
                              const double* group_coef, double* objective, double* measures);
int dfx_signal_spectrum_value_and_grad(dfx_handle* h, int32_t n_terms, const int32_t* term_signal, const int32_t* term_block,
                                       const int32_t* term_component, const double* term_coef, int32_t n_signals, const double* basis,
                                       int32_t n_rows, int32_t n_groups, const double* num_weights, const double* den_weights,
                                       const double* num_offset, const double* den_offset, int32_t offsets_per_member, int32_t measure,
                                       int32_t aggregate, double beta, const double* group_coef, double* objective, double* measures,
                                       const dfx_grads* want, dfx_grads* views, int32_t device_views, dfx_stats* stats);

/* Post-processing of the last forward solve on its device-resident history (problems/quads_focusing.py:319-372 with
 * energy.py:522-534): strain energies of every ligament 1/2 k (strain |l0|)^2 for the axial, shear and bending strain of
 * the NONLINEAR kinematics, (batch, T, n_bonds) each, and the kinetic energy of every block sum_d m_d v_d^2 / 2,
 * (batch, T, n_blocks).  Any pointer may be NULL. */
int dfx_response_data(dfx_handle* h, double* strain_energy_stretch, double* strain_energy_shear, double* strain_energy_bending,
                      double* kinetic_energy);

/* Test hooks: one RHS evaluation and its vector-Jacobian product on full-DOF arrays.
 * y, dy, lam, y_bar: (batch, 2, n_blocks, 3).  Constrained DOFs of y are ignored (they follow the
 * driving functions); their dy / y_bar entries are returned as 0. */
int dfx_rhs(dfx_handle* h, const double* y, double t, double* dy);
int dfx_rhs_vjp(dfx_handle* h, const double* y, double t, const double* lam, double* y_bar, dfx_grads* grads);

/* Forward mode of one RHS evaluation, the twin of dfx_rhs_vjp: n_dirs tangents of dfx_rhs at (y, t) along (y_dots, params_dots).
 * y (batch, 2, n_blocks, 3); y_dots (batch, n_dirs, 2, n_blocks, 3) or NULL; params_dots: n_dirs entries with the shapes and the NULL
 * rules of dfx_forward_tangent_multi, or NULL.  dy (batch, 2, n_blocks, 3), may be NULL, equals dfx_rhs's result to rounding; dy_dots
 * (batch, n_dirs, 2, n_blocks, 3): velocity tangents in the position rows, acceleration tangents in the velocity rows.  The primal
 * parameters are those of the last dfx_set_params; t is not differentiated.  Constrained DOFs of y and of y_dots are ignored: they follow
 * c(t), their position tangent is dc(t)/d fn_params . fn_params_dot, and their rows of dy / dy_dots are returned as 0.  Over the free
 * DOFs it is the exact transpose of dfx_rhs_vjp:  sum(lam * dy_dots[:, k]) == sum(y_bar * y_dots[:, k]) + <grads, params_dots[k]>.
 * One evaluation of the tangent stage kernel on a step of size zero (no Runge-Kutta combine is used), in the pass forms of
 * dfx_forward_tangent_multi (DFX_TANGENT_MULTI_FORM applies); every bond model and contact model, 3 and 4 nodes per block; nodes with
 * more than one ligament, or n_dirs < 1: return 1.  Non-finite results: return 3.  The call uses buffers of its own: the checkpoint and
 * the resident history of the handle stay as they were (a later dfx_adjoint still reverses the solve that was kept). */
int dfx_rhs_jvp(dfx_handle* h, const double* y, double t, const double* y_dots, const dfx_params* params_dots, int32_t n_dirs,
                double* dy, double* dy_dots);

/* Potential energy of a full-DOF configuration, (batch, n_blocks, 3) -> (batch,)  (test hook) */
int dfx_energy(dfx_handle* h, const double* u, double* energy);

/* Test hook: polls after which a wave of the persistent stage loop gives up waiting for a neighbour's record (0: the default, seconds).
 * A tiny value makes a launch give up at once, which exercises what happens when a workgroup of such a launch is not resident (another
 * process on the device): the handle latches onto one launch per stage and the solve is run again that way, in the same process. */
int dfx_test_set_spin_limit(dfx_handle* h, int32_t polls);

int dfx_device_count(void);
const char* dfx_version(void);

/* Layout of the five public structs AS THIS LIBRARY WAS COMPILED: for dfx_special, dfx_problem, dfx_params, dfx_grads, dfx_stats in
 * that order, sizeof followed by offsetof of every field in declaration order -- 5 + 4 + 16 + 9 + 10 + 9 = 53 int32 values.  A binding
 * that mirrors the structs by hand (difflexmm_amd/_binding.py flattens the ControlParams tree of utils.py:48-163 into them) compares
 * them with its own before the first call (tests/test_abi.py).  Writes min(n, 53) values, returns 53. */
int dfx_abi_layout(int32_t* out, int32_t n);

/* ---- design -> geometry on the host, fused (the per-evaluation prologue of the design loop) -------------------------------------------
 * The lattice maps of the reference (geometry.py:607-952: QuadGeometry / KagomeGeometry -- every node of every block = a static base vector
 * + one row of the design), the polygon pass (geometry.py:71-127), compute_inertia (geometry.py:144-160) and the undeformed void angles
 * (energy.py:204-219 + geometry.py:181-253 at rest) in one loop over the blocks; dfx_design_vjp is the cotangent of all of it.  Plain host
 * code (no handle, no device): `design` (batch, n_design, 2) holds the design arrays of a lattice flattened and concatenated, `gather[b*n_npb+k]`
 * the row node k of block b takes.  Outputs / cotangents may be NULL where noted.  Equal to difflexmm_amd/geometry.py (NumPy) to 1e-13. */
typedef struct dfx_design_map {
  int32_t n_blocks, n_npb, n_bonds, n_design;
  const double* base;                     /* (n_blocks, n_npb, 2) node vectors of the zero design                  */
  const int32_t* gather;                  /* (n_blocks, n_npb)    row of `design` added to each node                */
  const double* ref_points;               /* (n_blocks, 2)        lattice points the centroids are measured from    */
  const int32_t* bonds;                   /* (n_bonds, 2) node ids, or NULL (no void angles)                        */
} dfx_design_map;
int dfx_design_forward(const dfx_design_map* map, const double* design, int32_t batch, double density,
                       double* block_centroids /* (batch, n_blocks, 2) or NULL */, double* centroid_node_vectors /* (batch, n_blocks, n_npb, 2) */,
                       double* inertia /* (batch, n_blocks, 3) or NULL */, double* void_angle0 /* (batch, n_bonds, 2) or NULL */);
int dfx_design_vjp(const dfx_design_map* map, const double* design, int32_t batch, double density,
                   const double* centroid_node_vectors_bar, const double* block_centroids_bar /* or NULL */, const double* inertia_bar /* or NULL */,
                   const double* void_angle0_bar /* or NULL */, double* design_bar /* (batch, n_design, 2) */);

/* ---- multi-GPU: one process per GPU, independent members per rank, ONE collective per evaluation -------------
 * Replaces the reference's pmap over forward inputs + host sum (problems/quads_kinetic_energy_static_tuning.py:454-478) and the
 * sequential list of forward problems of problems/quads_focusing_multi_input.py:66-86.  RCCL over xGMI inside the library;
 * all buffers are HOST arrays (payloads are 8 B per member / a few KB of shared-design gradient: latency-bound).
 * Rank 0 creates the unique id; the launcher hands it to the other ranks (file / environment). */
#define DFX_COMM_UID_BYTES 128
enum { DFX_REDUCE_SUM = 0, DFX_REDUCE_MAX = 1, DFX_REDUCE_MIN = 2 };
typedef struct dfx_comm dfx_comm;
int dfx_comm_unique_id(char* uid128);
int dfx_comm_init(int32_t rank, int32_t nranks, const char* uid128, int32_t device, dfx_comm** out);
int dfx_comm_destroy(dfx_comm* c);
/* RCCL version the process runs / the engine was compiled against (major*10000 + minor*100 + patch) */
int dfx_comm_rccl_version(int32_t* runtime, int32_t* compiled);
int dfx_comm_rank(const dfx_comm* c);
int dfx_comm_size(const dfx_comm* c);
/* all[r * n_local + i] = local[i] of rank r, on every rank (one ncclAllGather) */
int dfx_gather_objectives(dfx_comm* c, const double* local, int32_t n_local, double* all);
/* sum over ranks, in place (one ncclAllReduce): gradients w.r.t. a design every rank shares */
int dfx_reduce_grads(dfx_comm* c, double* inout, int64_t n);
int dfx_comm_allreduce(dfx_comm* c, double* inout, int64_t n, int32_t op /* DFX_REDUCE_* */);
int dfx_comm_barrier(dfx_comm* c);
const char* dfx_comm_last_error(void);

/* device helpers (free / total HBM of a device, wait for everything queued on it) */
int dfx_mem_info(int32_t device, int64_t* free_bytes, int64_t* total_bytes);
int dfx_device_synchronize(int32_t device);

#ifdef __cplusplus
}
#endif

#ifdef DFX_ABI_LAYOUT_IMPL   /* the body of dfx_abi_layout, compiled into each library that implements this header */
#include <stddef.h>
static inline int dfxabi_fill(int32_t* out, int32_t n) {
  const int32_t v[] = {
      (int32_t)sizeof(dfx_special), (int32_t)offsetof(dfx_special, block), (int32_t)offsetof(dfx_special, con_mask),
      (int32_t)offsetof(dfx_special, con_coef), (int32_t)offsetof(dfx_special, load_coef),
      (int32_t)sizeof(dfx_problem), (int32_t)offsetof(dfx_problem, n_blocks), (int32_t)offsetof(dfx_problem, n_npb),
      (int32_t)offsetof(dfx_problem, n_bonds), (int32_t)offsetof(dfx_problem, bonds), (int32_t)offsetof(dfx_problem, bond_model),
      (int32_t)offsetof(dfx_problem, contact), (int32_t)offsetof(dfx_problem, n_special), (int32_t)offsetof(dfx_problem, special),
      (int32_t)offsetof(dfx_problem, n_fns), (int32_t)offsetof(dfx_problem, fn_type), (int32_t)offsetof(dfx_problem, batch),
      (int32_t)offsetof(dfx_problem, tableau), (int32_t)offsetof(dfx_problem, device), (int32_t)offsetof(dfx_problem, fn_table_n),
      (int32_t)offsetof(dfx_problem, fn_table), (int32_t)offsetof(dfx_problem, streams),
      (int32_t)sizeof(dfx_params), (int32_t)offsetof(dfx_params, centroid_node_vectors), (int32_t)offsetof(dfx_params, reference_vector),
      (int32_t)offsetof(dfx_params, k_bond), (int32_t)offsetof(dfx_params, inertia), (int32_t)offsetof(dfx_params, damping),
      (int32_t)offsetof(dfx_params, void_angle0), (int32_t)offsetof(dfx_params, contact), (int32_t)offsetof(dfx_params, fn_params),
      (int32_t)offsetof(dfx_params, block_centroids),
      (int32_t)sizeof(dfx_grads), (int32_t)offsetof(dfx_grads, centroid_node_vectors), (int32_t)offsetof(dfx_grads, reference_vector),
      (int32_t)offsetof(dfx_grads, k_bond), (int32_t)offsetof(dfx_grads, inertia), (int32_t)offsetof(dfx_grads, damping),
      (int32_t)offsetof(dfx_grads, void_angle0), (int32_t)offsetof(dfx_grads, contact), (int32_t)offsetof(dfx_grads, fn_params),
      (int32_t)offsetof(dfx_grads, state0), (int32_t)offsetof(dfx_grads, block_centroids),
      (int32_t)sizeof(dfx_stats), (int32_t)offsetof(dfx_stats, steps), (int32_t)offsetof(dfx_stats, rhs_evals),
      (int32_t)offsetof(dfx_stats, launches), (int32_t)offsetof(dfx_stats, kernel_ms), (int32_t)offsetof(dfx_stats, stage_kernel_us),
      (int32_t)offsetof(dfx_stats, streams), (int32_t)offsetof(dfx_stats, stage_checkpoint), (int32_t)offsetof(dfx_stats, checkpoint_records),
      (int32_t)offsetof(dfx_stats, tile_kernels)};
  const int32_t total = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; i < total && i < n; ++i) out[i] = v[i];
  return total;
}
#endif
#endif /* DFX_H */
