/*
 * nmpc_solver.h -- C ABI of the MI355X batched NMPC solver (libnmpc_hip.so).
 *
 * This is the drop-in boundary for the one hot path of wljungbergh/mpc-trajectory-generator that
 * this project accelerates: the NMPC solve that the reference performs through OpEn's generated
 * solver.  Reference interface each entry point replaces (paths relative to the reference repo):
 *
 *   nmpc_new / nmpc_free      og.tcp.OptimizerTcpManager(path).start() / .kill()
 *                             src/path_generator.py:218-220,408,417 ; src/mpc/mpc_generator.py:220
 *                             (and the offline code generation of src/mpc/mpc_generator.py:173-193:
 *                             the quantities that build() bakes into the generated crate are the
 *                             fields of nmpc_problem / nmpc_opts)
 *   nmpc_ping                 mng.ping()                       src/path_generator.py:222
 *   nmpc_solve_batch_host     mng.call(parameters)             src/mpc/mpc_generator.py:206
 *   nmpc_solve_batch_device   same, operands already in HBM    (B parameter vectors per call)
 *   nmpc_status fields        solution_data.exit_status / .solve_time_ms / ...
 *                             src/mpc/mpc_generator.py:211-214
 *   nmpc_eval_batch_*         the generated cost / grad / mapping_f1 / mapping_f2 C functions that
 *                             build() emits (declared by src/mpc/mpc_generator.py:66-175)
 *
 * The shape follows OpEn's own generated C bindings (<name>_new / <name>_solve / <name>_free with a
 * status struct), widened from one instance to a batch.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 on success
 * or a negative nmpc_error, never throws; buffers are caller-allocated; a handle is not
 * thread-safe, distinct handles are.  A handle owns device scratch (work queue, launch order, the pools
 * instances wait in between outer iterations): its asynchronous calls must be ordered on ONE stream
 * at a time; two batches in flight take two handles (bench.py's `pipelined` leg).
 * Data layout (all IEEE f64, row-major):
 *   p  [B][n_p]   parameter vectors, layout of reference src/path_generator.py:378-379
 *   u  [B][n_u]   decision vectors (v_0, w_0, v_1, w_1, ...)   src/mpc/mpc_generator.py:83,157-158
 *   y  [B][n1]    ALM multipliers of F1 = [acc ; omega_acc]    src/mpc/mpc_generator.py:162
 */
#ifndef NMPC_SOLVER_H
#define NMPC_SOLVER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMPC_ABI_VERSION 3
#define NMPC_MAX_HORIZON 40     /* longest N_hor served: the reference ships N_hor = 20 and 15 (configs/default.yaml:7,
                                   configs/smooth_velocity.yaml:7); BASELINE's long-horizon case is 40.  nmpc_new returns
                                   NMPC_ERR_BAD_PROBLEM beyond it (the one-point kernel that took 40 < N <= 64 until ABI 3's
                                   first release -- another L-BFGS arithmetic, no obstacle certificate -- is gone) */

typedef enum nmpc_error {
    NMPC_OK = 0,
    NMPC_ERR_BAD_PROBLEM = -1,      /* unsupported dims; ts not finite and > 0; a bound that is NaN or infinite;
                                       vmin > vmax, amin > amax, wmax < 0 or awmax < 0 (equal bounds are accepted) */
    NMPC_ERR_BAD_OPTS = -2,
    NMPC_ERR_BAD_ARG = -3,          /* NULL pointer, B < 0, B > max_batch                     */
    NMPC_ERR_NO_DEVICE = -4,        /* no HIP device / wrong architecture                     */
    NMPC_ERR_HIP = -5,              /* a HIP runtime call failed; see nmpc_last_error()       */
    NMPC_ERR_DEAD_HANDLE = -6       /* handle was killed                                      */
} nmpc_error;

/* What the reference bakes into the generated solver at build() time
 * (configs/default.yaml:6-13,18,34-40 ; src/mpc/mpc_generator.py:70-71,151-168). */
typedef struct nmpc_problem {
    int32_t N;        /* N_hor, 2..NMPC_MAX_HORIZON                 */
    int32_t nobs;     /* Nobs    : static circle slots, 0..64       */
    int32_t ndyn;     /* Ndynobs : dynamic ellipse slots, 0..3      */
    int32_t reserved;
    double ts;
    double vmin, vmax, wmax;     /* U = ([vmin,vmax] x [-wmax,wmax])^N      (:151-153) */
    double amin, amax, awmax;    /* C = [amin,amax]^N x [-awmax,awmax]^N    (:164-168) */
} nmpc_problem;

/* OpEn solver configuration (src/mpc/mpc_generator.py:184-186; opengen defaults otherwise).
 * The reference also stops on wall-clock (max_duration 0.5 s, :9,186).  Here that stop is opt-in and
 * lives outside this struct: nmpc_set_time_limits (per instance, OpEn's max_duration, and per batch).
 * By default only the iteration caps apply, plus -- when asked for -- max_total_inner, the
 * deterministic stand-in for max_duration; a solve the clock stops returns exactly what the solve with
 * max_total_inner = its num_inner_iterations returns. */
typedef struct nmpc_opts {
    /* ALM knobs: default, then the range nmpc_new accepts (anything else, NaN included, is NMPC_ERR_BAD_OPTS).
     * The ranges are OpEn's builder assertions as recalled in SURVEY.md App. C, not checked against OpEn. */
    double tolerance;            /* 1e-4   epsilon: finite, > 0                        */
    double initial_tolerance;    /* 1e-4   epsilon_0: finite, >= tolerance             */
    double delta_tolerance;      /* 1e-4   delta: finite, > 0                          */
    double initial_penalty;      /* 1.0    c0: finite, > 0                             */
    double penalty_update;       /* 5.0    rho: finite, > 1                            */
    double tolerance_update;     /* 0.1    beta: in (0, 1)                             */
    double sufficient_decrease;  /* 0.1    theta: in (0, 1)                            */
    int32_t lbfgs_memory;        /* 10 (1..10) */
    int32_t max_inner;           /* 500  */
    int32_t max_outer;           /* 10   */
    int32_t max_total_inner;     /* 0 = off.  PANOC iterations one solve may spend in total; beyond it the
                                    solve returns the feasible half step with NMPC_NOT_CONVERGED_OUT_OF_TIME
                                    (what max_duration does in the reference, src/mpc/mpc_generator.py:9,186,
                                    configs/default.yaml:49, counted in iterations instead of microseconds) */
    /* Restatement switches: choices of the PANOC/ALM restatement that cannot be checked against OpEn
     * here.  0 = what every published figure of this project uses unless it
     * says otherwise; oracle and kernels implement all of them, bit for bit. */
    int32_t akkt_gradient;       /* "previous gradient" of the AKKT residual ||r/gamma + grad - grad_prev||:
                                    0 cached before every line-search trial, carried across inner solves
                                    1 cached at the top of step() from iteration 1 on, zero at iteration 0
                                    2 no AKKT test (PANOC stops on ||r|| < tolerance alone)                 */
    int32_t ls_failure;          /* all 11 line-search trials fail: 0 take the last one, 1 tau = 0 (FB step) */
    int32_t inner_status;        /* outer criteria hold: 0 report the last inner status, 1 report Converged */
    int32_t reserved;
} nmpc_opts;

typedef enum nmpc_exit {
    NMPC_CONVERGED = 0,
    NMPC_NOT_CONVERGED_ITERATIONS = 1,
    NMPC_NOT_CONVERGED_OUT_OF_TIME = 2,      /* opts.max_total_inner spent (deterministic max_duration), or a limit of nmpc_set_time_limits reached */
    NMPC_NOT_CONVERGED_COST = 3,
    NMPC_NOT_CONVERGED_NOT_FINITE = 4        /* Deviation from OpEn, which checks the returned u only: raised as well when
                                                the cost or the residual norm ||r|| of an inner solve is not finite
                                                while the projected half step u still is (e.g. an initial penalty that
                                                overflows psi).  Through tcp_shim this is error 2000; the reference
                                                would go on with clamped controls (tests: test_nonfinite_cost_*) */
} nmpc_exit;

/* One per instance: the fields of OpEn's solver status plus evaluation
 * counters.  72 bytes. */
typedef struct nmpc_status {
    int32_t  exit_status;            /* nmpc_exit                                   */
    uint32_t num_outer_iterations;
    uint32_t num_inner_iterations;
    uint32_t num_cost_evals;         /* forward-only evaluations of psi             */
    uint32_t num_grad_evals;         /* forward + adjoint evaluations               */
    uint32_t reserved;               /* diagnostic: evaluation passes this solve needs in the kernel's schedule --
                                        three query points per pass (nmpc_solve_hyb_kernel, N_hor <= 20; a pass whose
                                        trials were evaluated by helper waves of the team counts like one the owner
                                        ran itself, so the figure is deterministic; nmpc_solve_hyb2_kernel likewise for
                                        20 < N_hor <= 40) */
    double last_problem_norm_fpr;
    double delta_y_norm_over_c;
    double f2_norm;
    double penalty;
    double cost;
    double solve_time_ms;            /* THIS instance: first start -> finish on the device's constant 100 MHz clock
                                        (what the reference reads per solve, src/mpc/mpc_generator.py:214); the
                                        wall time of a whole host-path batch is nmpc_last_batch_ms()          */
} nmpc_status;

typedef struct nmpc_handle nmpc_handle;

void nmpc_default_opts(nmpc_opts *opts);
int nmpc_n_u(const nmpc_problem *pb);
int nmpc_n_p(const nmpc_problem *pb);
int nmpc_n1(const nmpc_problem *pb);
int nmpc_n2(const nmpc_problem *pb);

/* Creates a solver for one problem shape on HIP device `device_id`, with room for `max_batch`
 * instances.  opts == NULL selects nmpc_default_opts. */
int nmpc_new(const nmpc_problem *pb, const nmpc_opts *opts, int device_id, int max_batch,
             nmpc_handle **out);
void nmpc_free(nmpc_handle *h);
int nmpc_ping(const nmpc_handle *h);
const char *nmpc_last_error(const nmpc_handle *h);
int nmpc_abi_version(void);
/* 0 for the shipped library: it reads no environment variable and has no tuning knob beyond nmpc_opts.  1 for the experiments build
 * (-DNMPC_EXPERIMENTS, csrc/variants/libnmpc_experiments.so), which tests and measurement scripts use to force alternative kernels and
 * scheduling policies and check that they give the same bits.  (The interface being replaced has no knobs: src/path_generator.py:218-222.) */
int nmpc_experiments_build(void);
/* Diagnostic: the solve kernel this handle launches (the name a rocprofv3 kernel trace shows). */
const char *nmpc_kernel_name(const nmpc_handle *h);
/* Diagnostic: the radius in metres of the circle culling this handle's solves use, 1.1 * N * ts * max(|vmin|, |vmax|): what the
 * bounds let a robot travel in a horizon, plus a margin.  Any value gives the same results; 0 for a NULL handle. */
double nmpc_cull_radius(const nmpc_handle *h);
/* Diagnostic: how this handle would launch a solve of B instances (0 <= B <= max_batch), and two constants of the handle.  Launches
 * nothing.  With W = resident_waves -- the waves the chip holds at once, CUs x 8 for N_hor <= 20 (x 4 if two teams' LDS do not fit a
 * CU) and CUs x 4 for 20 < N_hor <= 40 -- and G = W / 4, the workgroups of four waves that fit:
 *   grid        waves that take instances, min(B, W)
 *   owners      waves per workgroup that take instances: ceil(B / G), at least 1 and at most 4; the other waves help
 *   workgroups  ceil(grid / owners), at most G
 *   ordered     1 if B > W: the instances are handed out hard-looking ones first (two more kernels ahead of the solve)
 *   pools       1 if B > W: instances may leave their wave at outer-iteration boundaries (the pools and their counters are cleared)
 *               (the experiments build's knobs can switch either off)
 *   pool_cap    slots of a pool's ring in this launch, B
 *   staging_chunk_bytes   the size of each of the host path's two pinned bounce buffers: arrays travel in chunks of it
 * NMPC_ERR_BAD_ARG for a NULL argument or a B outside the range. */
typedef struct nmpc_launch_info {        /* 40 bytes */
    int32_t grid, owners, workgroups, ordered, pools, pool_cap, resident_waves, reserved;
    int64_t staging_chunk_bytes;
} nmpc_launch_info;
int nmpc_launch_geometry(const nmpc_handle *h, int B, nmpc_launch_info *out);

/* Device path: every pointer is device memory on the handle's device; the launch is enqueued on
 * `stream` (a hipStream_t, NULL = default stream) and the call returns without synchronising.
 * Everything a launch enqueues -- the clearing of the work queue, of the pools and of their counters, the kernels that order the
 * instances, the solve -- goes to `stream`.  The handle owns those queue, order and pool buffers, one set for all of its launches:
 * launches of one handle are ordered only when they are enqueued on one stream, and two launches of one handle in flight on different
 * streams are undefined.  Two batches in flight take two handles.
 *   d_u      [B][n_u]  in: initial guess, out: solution
 *   d_y0     [B][n1]   initial multipliers, or NULL (zeros)
 *   d_c0     [B]       initial penalties, or NULL (opts.initial_penalty)
 *   d_y_out  [B][n1]   final multipliers, or NULL
 *   d_status [B]       or NULL                                                              */
int nmpc_solve_batch_device(nmpc_handle *h, int B, const double *d_p, double *d_u,
                            const double *d_y0, const double *d_c0, double *d_y_out,
                            nmpc_status *d_status, void *stream);

/* Host path: same operands in host memory; copies in, solves, copies out, synchronises. */
int nmpc_solve_batch_host(nmpc_handle *h, int B, const double *p, double *u, const double *y0,
                          const double *c0, double *y_out, nmpc_status *status);
/* Kernel time (HIP events around the launch) of the last nmpc_solve_batch_host call on this handle, in ms. */
double nmpc_last_batch_ms(const nmpc_handle *h);

/* Wall-clock limits for this handle's later solves, on the device's 100 MHz constant clock; 0 = off (the default).
 *   max_duration_ms  per instance, from its first start (what status.solve_time_ms measures): OpEn's max_duration
 *   batch_budget_ms  per launch, from the launch's start on the device: no instance starts a new PANOC iteration after it
 * Checked where opts.max_total_inner is checked, at the end of each PANOC iteration, with the same consequences.
 * The instance returns the feasible half step with NMPC_NOT_CONVERGED_OUT_OF_TIME (or what the ALM layer reports after an
 * out-of-budget inner solve, exactly as with max_total_inner).  Every instance does at least one PANOC iteration.
 * Applies to nmpc_solve_batch_device/_host and to every step of a loop built on this handle.
 * NMPC_ERR_BAD_OPTS for a negative, NaN or infinite value, and the limits in force are left unchanged. */
int nmpc_set_time_limits(nmpc_handle *h, double max_duration_ms, double batch_budget_ms);

/* psi(u; c, y, p), grad_u psi, F1, F2 for B instances (c == NULL: zeros -> plain f; y == NULL: zeros).
 * Outputs may be NULL.  psi [B], grad [B][n_u], F1 [B][n1], F2 [B][n2]. */
int nmpc_eval_batch_device(nmpc_handle *h, int B, const double *d_p, const double *d_u,
                           const double *d_c, const double *d_y, double *d_psi, double *d_grad,
                           double *d_F1, double *d_F2, void *stream);
int nmpc_eval_batch_host(nmpc_handle *h, int B, const double *p, const double *u, const double *c,
                         const double *y, double *psi, double *grad, double *F1, double *F2);

/* ---- the receding-horizon loop on device ------------------------------------------------------
 * B robots follow one route (or R routes, nmpc_loop_new_routes) in lock step; one step = assemble p
 * (the body of the reference's PathGenerator.run loop, src/path_generator.py:290-382), solve the batch warm-started from the
 * previous controls and multipliers (mng.call, src/mpc/mpc_generator.py:206), advance the states
 * over num_steps_taken controls (src/mpc/mpc_generator.py:223-235) and evaluate the terminal test
 * (src/path_generator.py:397).  Nothing crosses PCIe between steps. */
typedef struct nmpc_route {
    int32_t n_ref;             /* samples of rough_ref                       src/mpc/mpc_generator.py:17-57  */
    int32_t n_vert;            /* vertices the route bends around            src/visibility/visibility.py:126-139 */
    int32_t n_brake;           /* entries of the braking tables (>= 1)       src/path_generator.py:439-477   */
    int32_t num_steps_taken;   /* controls applied per solve                 configs/default.yaml:16         */
    const double *x_ref, *y_ref, *theta_ref;    /* [n_ref]   host memory, copied by nmpc_loop_new */
    const double *vert_xy;                      /* [n_vert][2]                                       */
    const double *brake_vel, *brake_dist;       /* [n_brake]                                         */
    double end[3];             /* goal pose                                  src/path_generator.py:327      */
    double base_speed;         /* lin_vel_max * throttle_ratio               src/path_generator.py:284      */
    double radius;             /* static circle radius                       src/path_generator.py:300-301  */
    double dyn_pad;            /* added to the ellipse radii                 src/visibility/visibility.py:208-209 */
    double weights[10];        /* p[10:20]                                   src/path_generator.py:226-227  */
} nmpc_route;

typedef struct nmpc_loop nmpc_loop;

/* starts [B][3] (x, y, theta); idx0 [B] = reference sample each robot starts at, or NULL (0, as
 * the reference).  K <= Ndynobs moving ellipses per robot, dyn [B][K][10] = (p1x, p1y, p2x, p2y,
 * freq, rx, ry, angle, sinus, direction): the reference's linear law (visibility.py:156-166), or
 * with sinus != 0 its sinusoidal law (:177-196, amplitude 1.5; direction = atan2(p2y - p1y,
 * p2x - p1x), computed by the caller); NULL with K = 0.
 * max_steps > 0 also records the trajectory on device. */
int nmpc_loop_new(nmpc_handle *h, const nmpc_route *route, int B, const double *starts,
                  const int32_t *idx0, int K, const double *dyn, int max_steps, nmpc_loop **out);
/* A fleet on R routes: robot b follows routes[route_of[b]] (route_of [B], values in [0, R); NULL only with
 * R == 1, which is nmpc_loop_new).  Every field of nmpc_route is per route (tables, end, base_speed, radius,
 * dyn_pad, weights), except num_steps_taken, which every route must share (the fleet moves in lock step).
 * idx0[b] is checked against the n_ref of b's own route.  Everything else as nmpc_loop_new; the loop it
 * returns is stepped, read and freed like one from nmpc_loop_new.  NMPC_ERR_BAD_ARG, with nothing allocated,
 * for R < 1, route_of NULL with R > 1, a route_of[b] out of range, an invalid route, routes that differ in
 * num_steps_taken, or an idx0[b] outside its route. */
int nmpc_loop_new_routes(nmpc_handle *h, const nmpc_route *routes, int R, const int32_t *route_of,
                         int B, const double *starts, const int32_t *idx0, int K, const double *dyn,
                         int max_steps, nmpc_loop **out);
/* Peers: the robots of a group see each other as moving ellipses (the rule: DESIGN.md section 5.9).  Every step, between the
 * assembly of p and the solve, each robot's poses over the horizon are predicted from its state and its previous plan (the
 * Euler step of the state advance; before the first solve everybody stands still), and for each robot the M robots of its
 * group whose predicted positions come closest to its own -- min over the stages of the squared distance, below range^2,
 * sorted by (distance, robot index) -- are written over the ellipse slots K .. K + M - 1 of its p, stage by stage, as
 * (x, y, rx, ry, theta).  A slot that finds no peer keeps what the assembly put there; the block the loop carries from step
 * to step never sees peers.
 *   group_of [B]  the group of each robot, values in [0, B); NULL = one group.  Robots of different groups never see each
 *                 other, whatever routes they follow.
 *   M             ellipse slots given to peers, M >= 1 and K + M <= Ndynobs
 *   rx, ry        the ellipse's radii as the cost reads them (no padding is added), range: all finite and > 0
 * To be called once, before the loop's first step.  NMPC_ERR_BAD_ARG with a message, and nothing changed, for M < 1,
 * K + M > Ndynobs, a group_of[b] out of range, an rx, ry or range that is not finite and positive, a call after a step, or
 * a second call.  A loop without peers enqueues what it enqueued before this function existed.  On a loop with a crowd
 * (nmpc_loop_set_crowd, Mc slots) the peers' slots are K + Mc .. K + Mc + M - 1, and K + Mc + M > Ndynobs is refused. */
int nmpc_loop_set_peers(nmpc_loop *l, const int32_t *group_of, int M, double rx, double ry, double range);
/* Peers found through a grid: the rule and the results of nmpc_loop_set_peers, bit for bit, at a cost that grows with the robots
 * near each other, not with the group (the rule, and why it misses nobody: DESIGN.md section 5.9).  Every step, on the device, each
 * robot's box over its predicted positions is filed in a uniform grid of edge `cell` (metres; the edge grows where the fleet's extent
 * would need more than 128 cells on an axis), and a robot forms its distances to the robots filed in the cells its range can reach
 * instead of to all of its group.  group_of keeps its meaning (NULL = everybody: "avoid whoever is near").  Three kernels take the
 * place of the all-pairs one.
 * This is the loop's peers call: either setter after the other, a second call or a call after a step is refused.  NMPC_ERR_BAD_ARG
 * with a message, and nothing changed, for everything nmpc_loop_set_peers refuses and for a cell that is not finite and positive. */
int nmpc_loop_set_peers_grid(nmpc_loop *l, const int32_t *group_of, int M, double rx, double ry, double range, double cell);
/* The grid of the last step, for tests and reports: the minimum of the filed robots' lower box corners, the cells' edges per axis,
 * the fleet's largest box extent per axis, the cells per axis and the robots filed (those with a stage at which both coordinates
 * are finite). */
typedef struct nmpc_peer_grid {      /* 64 bytes */
    double origin[2], h[2], W[2];
    int32_t nx, ny, filed, reserved;
} nmpc_peer_grid;
/* Synchronises, then copies out the last step's grid and, if asked for (NULL = skip), cell_of [B]: the cell each robot is filed
 * under (row-major, y * nx + x), -1 for an unfiled one.  NMPC_ERR_BAD_ARG on a loop without nmpc_loop_set_peers_grid or before its
 * first step. */
int nmpc_loop_peer_grid(nmpc_loop *l, nmpc_peer_grid *out, int32_t *cell_of);
/* Retirement: robots that reach their goal leave the loop, as the reference's `while not terminal` ends for one robot
 * (src/path_generator.py:290,397).  Off unless on != 0 is given here; a loop without it enqueues what it enqueued before this
 * function existed.  With it, every robot is active at the first step; after a step's advance an active robot whose terminal
 * test holds is retired for good, and from the next step on it is not assembled, not solved and not advanced: its state, last_u,
 * idx, p, u, y and status keep the values of its last step, its done stays 1, and its rows of a recorded trajectory repeat its
 * final pose.  Each step solves the active robots only, as one batch, in ascending robot index; the wall-clock limits apply to
 * that batch.  For peers a retired robot is a parked obstacle: its predicted pose is its state at every stage, and it stays a
 * candidate for the others while receiving no peers itself.  A step with nobody active launches no solve and still counts.
 * The host sizes a step by the number of active robots, which it learns from the step before: nmpc_loop_step then waits for
 * the previous step's count (an event on its stream, not the device: loops on other streams keep running).  Only a retiring
 * loop has this one-step coupling.
 * To be called once, before the loop's first step: NMPC_ERR_BAD_ARG with a message, and nothing changed, for a call after a
 * step or a second call. */
int nmpc_loop_set_retire(nmpc_loop *l, int on);
/* Synchronises, then gives the number of active robots and retired_at [B] (NULL = skip): the number of steps (solves) a retired
 * robot took, -1 for an active one.  A loop without retirement reports B and -1 everywhere. */
int nmpc_loop_active(nmpc_loop *l, int32_t *n_active, int32_t *retired_at);
/* Steps a retiring loop until nobody is active, max_steps steps are taken or the trajectory buffer is full; returns the number
 * of steps taken, or < 0.  Between steps it waits as nmpc_loop_step does, and does not synchronise after the last.
 * NMPC_ERR_BAD_ARG on a loop without retirement. */
int nmpc_loop_run(nmpc_loop *l, int max_steps, void *stream);
/* Missions: a robot drives a sequence of routes, leg after leg, as the reference's user calls `PathGenerator.run(graph, start, end)`
 * again from where the robot stands (src/main.py:23, src/path_generator.py:197-290).  Off unless asked for here; a loop without
 * missions enqueues what it enqueued before this function existed.  Robot b's legs are the routes leg_route[leg_off[b] ..
 * leg_off[b + 1]), indices into the R routes of the loop, the first one the route_of[b] it was created with.  With missions, one
 * more kernel per step, after the advance (and the monitor) and before the active list is rebuilt: an active robot whose terminal
 * test holds against the goal of its current route ends that leg at this step (leg_at = the loop's step count, this step included).
 * If it has another leg it is re-dispatched in the same step and stays active: leg + 1, route_of = that leg's route, idx = 0,
 * last_u = (0, 0), every entry of its u and y +0.0, done = 0; its state, carried dynamic block, p, status and clearance record are
 * not touched.  The next step therefore treats it as `run()` called anew from its pose: window search from sample 0 of the new
 * route, that route's circles, goal, weights, base speed, radius and braking tables, no previous control in p, a cold solve.  After
 * its last leg it is retired as nmpc_loop_set_retire describes, retired_at equal to that leg's leg_at.  Every leg is solved at
 * least once.  One deviation from the reference: the loop's clock and the carried dynamic block run on across legs (the scripted
 * ellipses belong to the world, not to a leg); with K == 0 a mission equals, bit for bit, its legs driven one after another.
 *   leg_off   [B + 1]         ascending from 0, every robot has at least one leg
 *   leg_route [leg_off[B]]    values in [0, R), leg_route[leg_off[b]] == route_of[b]
 * To be called once, after nmpc_loop_set_retire(l, 1) and before the loop's first step.  NMPC_ERR_BAD_ARG with a message, and
 * nothing changed, for a NULL argument, a loop that does not retire, a call after a step, a second call, leg_off[0] != 0, a robot
 * with no leg, a leg_route entry outside [0, R), or a first leg that is not the robot's route_of. */
int nmpc_loop_set_missions(nmpc_loop *l, const int32_t *leg_off, const int32_t *leg_route);
/* Synchronises, then copies what is asked for (NULL = skip): leg [B] the leg each robot is on, route_of [B] its current route,
 * leg_at [leg_off[B]] the steps at which each leg ended (-1: not yet).  A loop without missions reports leg = 0 and the route_of of
 * its creation, and writes no leg_at. */
int nmpc_loop_legs(nmpc_loop *l, int32_t *leg, int32_t *route_of, int32_t *leg_at);
/* Clearance monitor: per robot, the closest approach to the static circles, to the scripted ellipses and to the other robots of
 * its monitor group over everything driven so far, and the trajectory row of each (the rule: DESIGN.md section 5.9).  It observes
 * only: no p, u, y, state or status differs by a bit from the loop without it.  One more kernel per step, after the advance, over
 * the robots the step drove (those it retires at its end included); for the s = num_steps_taken rows r the step appends, with the
 * pose (x, y) of row r and p the robot's parameter vector of this step as the solve read it, in unfused f64:
 *   circle   sqrt(dx*dx + dy*dy) - rc over the circle slots of p with rc > 0, in metres (negative: inside)
 *   ellipse  (a*a)/(rx*rx) + (c*c)/(ry*ry), a = dx*cos A + dy*sin A, c = dx*sin A - dy*cos A, over the K scripted slots, at the
 *            slot's entry for that pose (below 1: inside the padded ellipse, the cost's own quantity); peer and unused slots are not read
 *   peer2    dx*dx + dy*dy to every other robot j of the group in the same row; a robot retired before the step stands at its state
 * Each record is the lexicographic minimum of (value, row) -- (value, row, j) for peers -- so among equal values the earlier row,
 * then the smaller robot index; a comparison that is false (a NaN value) keeps the record.  Initially +inf, row -1, peer -1, which
 * is what a robot keeps that never meets an obstacle of that kind; a retired robot keeps its record.
 *   group_of [B]  the monitor's own groups, values in [0, B); NULL = one group of all B.  Independent of nmpc_loop_set_peers.
 * To be called once, before the loop's first step, on a loop that records its trajectory (max_steps > 0: the step's rows are read
 * from that table).  NMPC_ERR_BAD_ARG with a message, and nothing changed, for a call after a step, a second call, a group_of[b]
 * out of range or a loop with max_steps == 0 (a NULL loop: NMPC_ERR_BAD_ARG).  A loop without a monitor enqueues what it enqueued
 * before this function existed. */
typedef struct nmpc_clearance {      /* 40 bytes */
    double circle, ellipse, peer2;
    int32_t circle_row, ellipse_row, peer_row, peer;
} nmpc_clearance;
int nmpc_loop_set_monitor(nmpc_loop *l, const int32_t *group_of);
/* Synchronises, then copies the records out [B]; on a loop without a monitor the initial record everywhere. */
int nmpc_loop_clearance(nmpc_loop *l, nmpc_clearance *out);
void nmpc_loop_free(nmpc_loop *l);
/* Enqueues assemble -> solve -> advance on `stream`; does not synchronise. */
int nmpc_loop_step(nmpc_loop *l, void *stream);
/* Synchronises, then copies what is asked for (NULL = skip) to host memory:
 * state [B][3], last_u [B][2], idx [B], done [B], status [B] of the last solve. */
int nmpc_loop_read(nmpc_loop *l, double *state, double *last_u, int32_t *idx, uint8_t *done,
                   nmpc_status *status);
/* The parameter vectors of the last step p [B][n_p], the controls u [B][n_u] and multipliers y [B][n1]. */
int nmpc_loop_params(nmpc_loop *l, double *p, double *u, double *y);
/* Recorded trajectory: rows [steps * num_steps_taken + 1][B][3]; returns the row count (or < 0). */
int nmpc_loop_trajectory(nmpc_loop *l, double *rows, int max_rows);

/* ---- a route per robot, planned on device ---------------------------------------------------------
 * Batched shortest paths over the visibility graph of one scene: what the reference's front-end answers for one start / goal pair
 * (src/visibility/visibility.py:49-88: inflate the obstacles and deflate the boundary, build the visibility graph, shortest path;
 * :126-139 maps the path's corners back to original vertices, which stays with the caller), for B pairs at once, so that every robot
 * of a fleet can have its own start and goal as the reference's user gives them (src/path_generator.py:197-251).  A planner is a
 * handle of its own, independent of nmpc_handle and of any problem shape; like a handle it is not thread-safe, distinct planners are.
 * The rule -- the segment test, the search and its tie rule -- is DESIGN.md section 5.11; its host statement is
 * frontend.plan_batch_mirror, whose bits the kernels give.
 *
 * The scene (visibility.py:49-67 has produced the polygons): the graph's nodes (the corners a path can bend around) and every edge
 * of the inflated obstacles and the deflated boundary.  Limits: n_node <= 254, 3 <= n_edge <= 1024. */
typedef struct nmpc_scene {
    int32_t n_node, n_edge, n_poly, reserved;
    const double *node_xy;     /* [n_node][2]                                     visibility.py:69-80   */
    const double *edge;        /* [n_edge][4] x1 y1 x2 y2, polygon by polygon: the obstacles first, the boundary last */
    const int32_t *poly_off;   /* [n_poly + 1]: polygon k owns the edges poly_off[k] .. poly_off[k + 1]; ascending from 0 to n_edge,
                                  three edges per polygon at least */
} nmpc_scene;

typedef struct nmpc_planner nmpc_planner;

/* Copies the scene to HIP device `device_id`, judges the node-node visibility there (one kernel over the n_node^2 pairs; synchronises) and
 * makes room for `max_batch` queries (1 .. 2^20).  NMPC_ERR_BAD_ARG, with nothing allocated, for a NULL argument, a scene outside the
 * limits, a malformed poly_off or a max_batch out of range; NMPC_ERR_NO_DEVICE / NMPC_ERR_HIP as nmpc_new. */
int nmpc_planner_new(const nmpc_scene *scene, int device_id, int max_batch, nmpc_planner **out);
void nmpc_planner_free(nmpc_planner *pl);
/* The node-node visibility vis [n_node][n_node] to host memory: entry (i, j) = 1 if the segment from node i to node j is free. */
int nmpc_planner_visibility(nmpc_planner *pl, uint8_t *vis);
/* B queries; the points of a query are [start, goal] + nodes, n = n_node + 2.  Two kernels: the visibility of the query's own
 * 2 n_node + 1 segments -- (start, node k), (goal, node k), (start, goal) -- then per query Dijkstra over the n points: at most n
 * rounds, each settling the unsettled point with the smallest (distance, index).  The search stops when that distance is not
 * finite or the point is the goal, and relaxes every unsettled visible point j on the strict dist[i] + |p_i - p_j| < dist[j].
 * A NaN or infinite coordinate blocks every segment it is part of: such a query ends as "no path".
 * Device path: every pointer is device memory on the planner's device; enqueued on `stream`, no synchronisation.
 *   d_start, d_goal [B][2]
 *   d_n_wp   [B]            waypoints of the path, start and goal included; 0 = no path
 *   d_wp     [B][n]         their point indices from 0 (the start) to 1 (the goal), -1 behind them
 *   d_length [B]            the path's length, +inf without a path
 *   d_vis    [B][2 n_node + 1]  the visibility of the query's own segments, or NULL (kept in the planner's scratch)
 * B == 0 is NMPC_OK and launches nothing; B < 0, B > max_batch or a NULL required pointer is NMPC_ERR_BAD_ARG.  A planner's
 * asynchronous calls must be ordered on one stream at a time. */
int nmpc_plan_batch_device(nmpc_planner *pl, int B, const double *d_start, const double *d_goal, int32_t *d_n_wp, int32_t *d_wp,
                           double *d_length, uint8_t *d_vis, void *stream);
/* Host path: same operands in host memory; copies in, plans, copies out, synchronises. */
int nmpc_plan_batch_host(nmpc_planner *pl, int B, const double *start, const double *goal, int32_t *n_wp, int32_t *wp,
                         double *length, uint8_t *vis);
/* Kernel time (HIP events around the two launches) of the last nmpc_plan_batch_host call on this planner, in ms. */
double nmpc_planner_last_ms(const nmpc_planner *pl);

/* ---- map monitor: each robot's closest approach to the map's walls, on device ----------------------
 * The clearance monitor sees what the solver sees in p; the map itself -- a wall between two corners, an obstacle the route merely
 * passes, the boundary -- is kept away by soft costs only.  The map monitor is an opt-in stage of the loop that checks every pose a
 * robot drives against the polygons of a map (the rule: DESIGN.md section 5.9).  It observes only: no p, u, y, state, status,
 * trajectory or clearance record differs by a bit from the loop without it.  One more kernel per step, after the advance (and the
 * clearance monitor), over the robots the step drove (those it retires at its end included).
 *   The map: the scene's edge [n_edge][4] and poly_off [n_poly + 1], the obstacles first and the boundary LAST; the node fields are
 *   ignored.  3 <= n_edge <= 1024, n_poly >= 1, poly_off ascending from 0 to n_edge in steps of three edges at least, every
 *   coordinate finite.
 * For each of the s = num_steps_taken rows r a step appends, with (x, y) the robot's pose of row r and (ax, ay) its pose of row
 * r - 1, in unfused f64 in the order written, / correctly rounded, no sqrt:
 *   wall distance, squared, per edge e: ex = x2 - x1, ey = y2 - y1, L2 = ex*ex + ey*ey; t = 0 unless L2 > 0, then t = ((x - x1)*ex +
 *     (y - y1)*ey)/L2, if (t < 0) t = 0, if (t > 1) t = 1; cx = x1 + t*ex, cy = y1 + t*ey, dx = x - cx, dy = y - cy, v = dx*dx + dy*dy
 *   containment of polygon k, even-odd: an edge with (y1 > y) != (y2 > y) and xi = x1 + ((y - y1)*(x2 - x1))/(y2 - y1) is a crossing
 *     if xi > x; an obstacle fails on an odd count, the boundary (k = n_poly - 1) on an even one; no on-edge tolerance
 *   crossing between the two rows: with orient(p, q, r) = (qx - px)*(ry - py) - (qy - py)*(rx - px), a = (ax, ay), b = (x, y) and the
 *     edge (c, d), o1 = orient(a, b, c), o2 = orient(a, b, d), o3 = orient(c, d, a), o4 = orient(c, d, b): the edge is crossed if
 *     o1*o2 < -1e-9 and o3*o4 < -1e-9, and the polygon that owns it fails
 * A row is a hit if any polygon fails (a NaN pose fails the boundary).  The record: (wall2, wall_row, wall_edge) = the lexicographic
 * minimum of (v, r, e) over everything seen so far (a comparison that is false keeps the record, so a NaN v is passed over), hits =
 * the rows that were hits, hit_row the first of them, hit_poly the smallest failing polygon index in that row.  Initially +inf, -1,
 * -1, 0, -1, -1, 0.  A robot retired earlier keeps its record, a step with nobody active updates nothing, records run across legs.
 * To be called once, before the loop's first step, in any order with the other setters, on a loop that records its trajectory.
 * NMPC_ERR_BAD_ARG with a message that names the function, and nothing changed or allocated, for a NULL map (a NULL loop:
 * NMPC_ERR_BAD_ARG), a call after a step, a second call, a loop with max_steps == 0, n_edge or n_poly outside the limits, a
 * malformed poly_off or a coordinate that is not finite.  A loop without the stage enqueues what it enqueued before this function
 * existed. */
typedef struct nmpc_map_clearance {      /* 32 bytes */
    double wall2;
    int32_t wall_row, wall_edge, hits, hit_row, hit_poly, reserved;
} nmpc_map_clearance;
int nmpc_loop_set_map_monitor(nmpc_loop *l, const nmpc_scene *map);
/* Synchronises, then copies the records out [B]; on a loop without the stage the initial record everywhere. */
int nmpc_loop_map_clearance(nmpc_loop *l, nmpc_map_clearance *out);

/* ---- track monitor: how closely each robot followed its route, on device --------------------------
 * The controller's cost is built around the distance to the route (cte_penalty, q, qtheta), and the reference's users judge a tuning by
 * laying the driven path over the planned one (src/eval_diff_configs.py, src/gen_res_diff_maps.py).  The track monitor is an opt-in
 * stage of the loop that keeps that comparison on the device (the rule: DESIGN.md section 5.9).  It observes only: no p, u, y, state,
 * status, trajectory or other record differs by a bit from the loop without it.  One more kernel per step, after the advance (or the
 * plant) and the clearance, map and crowd monitors and before the log and the missions' dispatch, over the robots the step drove
 * (those it retires at its end included).  With s = num_steps_taken, step n appends the trajectory rows r = n*s + 1 + i, i = 0 .. s - 1;
 * (x, y, th) is the pose of row r (with a plant the true pose) and the route is routes[route_of[b]] as the step found it, so under
 * missions a row is measured against the leg it was driven on.  Its polyline has the points Q_j = (x_ref[j], y_ref[j]), j = 0 ..
 * n_ref - 1, and n_seg = max(n_ref - 1, 1) segments, segment j from Q_j to Q_e, e = min(j + 1, n_ref - 1) (n_ref = 1: one segment of
 * zero length).  Unfused f64 in the order written, IEEE division, no sqrt; a comparison that is false (a NaN) has the literal consequence:
 *   squared distance to segment j: ex = x2 - x1, ey = y2 - y1, L2 = ex*ex + ey*ey; t = 0 unless L2 > 0, then t = ((x - x1)*ex +
 *     (y - y1)*ey)/L2; if (t < 0 && j > 0) t = 0; if (t > 1) t = 1; cx = x1 + t*ex, cy = y1 + t*ey, dx = x - cx, dy = y - cy,
 *     v = dx*dx + dy*dy.  Segment 0 is NOT clamped below: the reference's table begins one sample after the start
 *     (src/mpc/mpc_generator.py:17-57), and a robot still leaving its start, or the end of its previous leg, is on the line
 *   per row: (v*, j*) from (+inf, -1), the segments ascending, taking v on the strict v < v* (the first minimal segment stays, a NaN is
 *     passed over).  j* = -1 (a NaN pose): the row adds 1 to `rows` and nothing else.  Otherwise d = th - theta_ref[e*], e* = min(j* + 1,
 *     n_ref - 1), a = d < 0 ? -d : d.  The heading error is NOT wrapped: the cost does not wrap either (cost_fn,
 *     src/mpc/mpc_generator.py:59-63), so this is the error the controller itself sees
 *   the record, in row order: rows += 1; cte2_sum = cte2_sum + v*; dth2_sum = dth2_sum + d*d; if v* > cte2_max: cte2_max = v*,
 *     cte_row = r, cte_seg = j*; if a > dth_max: dth_max = a, dth_row = r; last_seg = j* (progress along the route: it drops when a new
 *     leg begins); if v* > tol*tol: off_rows += 1, and off_row = r if it was -1.  Both maxima are strict: the earliest row stays, and
 *     a robot exactly on its route keeps -1
 * Initially 0, 0, 0, 0, 0, -1, -1, -1, -1, 0, -1, 0.  A robot retired earlier keeps its record, a step with nobody active launches
 * nothing for this stage, records run across legs.  sizeof(nmpc_tracking) == 64.
 * To be called once, before the loop's first step, in any order with the other setters, on a loop that records its trajectory.
 * NMPC_ERR_BAD_ARG with a message that names the function, and nothing changed or allocated, for a tol that is negative or not finite
 * (a NULL loop: NMPC_ERR_BAD_ARG), a call after a step, a second call or a loop with max_steps == 0.  A loop without the stage
 * enqueues what it enqueued before this function existed. */
typedef struct nmpc_tracking {           /* 64 bytes */
    double cte2_max, cte2_sum, dth_max, dth2_sum;
    int32_t rows, cte_row, cte_seg, dth_row, last_seg, off_rows, off_row, reserved;
} nmpc_tracking;
int nmpc_loop_set_track_monitor(nmpc_loop *l, double tol);
/* Synchronises, then copies the records out [B] (before the first step: the initial records); NMPC_ERR_BAD_ARG on a loop without the
 * stage. */
int nmpc_loop_tracking(nmpc_loop *l, nmpc_tracking *out);

/* ---- drive log: each robot's applied controls and solve outcomes, on device -----------------------
 * The reference's PathGenerator.run gives back the path, the controls that were applied and how long each solve took, and reports a
 * bad exit status at the step where it occurs (src/path_generator.py:385-394,431-437).  The drive log is an opt-in stage of the loop
 * that keeps all of that on the device (the rule: DESIGN.md section 5.9).  It observes only: no p, u, y, state, status, trajectory,
 * clearance or map record differs by a bit from the loop without it.  Two more kernels per step, after the advance and the monitors
 * and before the missions' dispatch: one over the robots the step drove (those it retires at its end included), one workgroup for
 * the step's fleet totals.  With s = num_steps_taken and `step` the loop's step count, this step included (1-based, as retired_at):
 *   ctrl [max_steps * s][B][2]  row step_before * s + i = the (v, w) applied between trajectory rows step_before * s + i and the next:
 *                               the first s control pairs of the robot's u, as the advance read them.  +0.0 where a robot was not driven.
 *                               With a plant (below) these stay the COMMANDED controls; what acted is the plant's `applied`, and `length`
 *                               and the monitors see the true rows.
 *   rec  [max_steps][B]         nmpc_step_record of row step - 1: the fields of the step's nmpc_status after the solve, and the leg the
 *                               solve belonged to (before the step's dispatch; 0 without missions).  A robot the step did not drive
 *                               keeps exit_status = -1 and zeros.
 *   sum  [B]                    nmpc_drive_summary, cumulative; a retired robot keeps its summary, and it runs on across legs:
 *     steps, rows               + 1, + s
 *     exits[e]                  + 1 for e = the solve's exit_status (0 .. 4)
 *     inner_total               + num_inner_iterations; inner_max / inner_max_step: the largest count and the step it occurred at
 *     length                    length = length + sqrt(dx*dx + dy*dy) over the step's rows in order, (dx, dy) from trajectory row r - 1 to
 *                               row r, unfused f64
 *     v_abs_max, w_abs_max      fabs of the applied controls
 *     acc_*, wacc_*             a = (v_i - v_prev) / ts (IEEE division), v_prev = p[3] for the step's first control -- the very v_-1 the
 *                               solve formed F1 from; 0 after a mission's re-dispatch -- and the control before for the others; w likewise
 *                               with p[4].  *_abs_max takes fabs(a), *_sq_sum = *_sq_sum + a*a, sequential, no fma
 *     f2_max / f2_max_step      the largest f2_norm and the step it occurred at
 *     Every maximum is updated by `if (x > m) m = x` from +0.0: a comparison that is false (a NaN) keeps the record, and among equal
 *     values the earliest step stays.  The two *_step fields start at -1.
 *   tot  [max_steps]            nmpc_step_totals of row step - 1, over the robots the step drove: their number, their solves per exit
 *                               status, the sum of their num_inner_iterations, the largest one and the smallest robot index that has it,
 *                               and the largest solve_time_ms.  A step with nobody active writes zeros.
 * To be called once, before the loop's first step, in any order with the other setters, on a loop that records its trajectory
 * (max_steps > 0: that is the log's length, and `length` reads the trajectory's rows).  NMPC_ERR_BAD_ARG with a message that names the
 * function, and nothing changed or allocated, for a call after a step, a second call or a loop with max_steps == 0 (a NULL loop:
 * NMPC_ERR_BAD_ARG).  A loop without the stage enqueues what it enqueued before this function existed. */
typedef struct nmpc_step_record {        /* 40 bytes */
    int32_t  exit_status;            /* nmpc_exit; -1: the robot was not solved in this step */
    int32_t  leg;                    /* the leg this solve belonged to (before the step's dispatch); 0 without missions */
    uint32_t num_inner_iterations, num_outer_iterations;
    double   cost, f2_norm, solve_time_ms;
} nmpc_step_record;
typedef struct nmpc_drive_summary {      /* 112 bytes */
    int32_t  steps, rows;            /* solves taken, controls applied */
    uint32_t exits[5];               /* solves per nmpc_exit value */
    uint32_t inner_max;
    uint64_t inner_total;
    int32_t  inner_max_step, f2_max_step;
    double   length;
    double   v_abs_max, w_abs_max;
    double   acc_abs_max, wacc_abs_max, acc_sq_sum, wacc_sq_sum;
    double   f2_max;
} nmpc_drive_summary;
typedef struct nmpc_step_totals {        /* 48 bytes */
    int32_t  solved;                 /* the step's active count */
    uint32_t exits[5];
    uint32_t inner_max;
    int32_t  inner_max_robot;        /* among the robots with the largest count, the smallest index */
    uint64_t inner_total;
    double   solve_ms_max;
} nmpc_step_totals;
#ifdef __cplusplus
static_assert(sizeof(nmpc_step_record) == 40 && sizeof(nmpc_drive_summary) == 112 && sizeof(nmpc_step_totals) == 48, "drive log layouts");
#else
_Static_assert(sizeof(nmpc_step_record) == 40 && sizeof(nmpc_drive_summary) == 112 && sizeof(nmpc_step_totals) == 48, "drive log layouts");
#endif
int nmpc_loop_set_log(nmpc_loop *l);
/* Synchronises, then copies what is asked for (NULL = skip) of the steps taken so far: ctrl [steps * s][B][2] and rec [steps][B].
 * Returns the step count (or < 0); NMPC_ERR_BAD_ARG if max_steps, the steps the caller's buffers hold, is smaller.  A loop without a
 * log reports 0 steps and writes nothing. */
int nmpc_loop_log(nmpc_loop *l, double *ctrl, nmpc_step_record *rec, int max_steps);
/* Synchronises, then copies the summaries out [B]; on a loop without a log the initial summary everywhere. */
int nmpc_loop_drive_summary(nmpc_loop *l, nmpc_drive_summary *out);
/* Synchronises, then copies the totals of the steps taken so far out [steps] and returns the step count (or < 0), as nmpc_loop_log. */
int nmpc_loop_step_totals(nmpc_loop *l, nmpc_step_totals *out, int max_steps);
/* Crowd: D moving obstacles that belong to the world and are shared by the whole fleet (the rule: DESIGN.md section 5.9), where
 * nmpc_loop_new* gives every robot a private copy of at most Ndynobs.  One table [D][N][5] of every obstacle's ellipses over the horizon is
 * advanced on the device once per step -- every step, whoever is active, across mission legs: all stages fresh at the first step, later a
 * shift by the s stages taken inside each obstacle's row and the last s stages fresh -- by the arithmetic of the scripted ellipses, so that
 * row d equals, bit for bit, the block a loop carries for a scripted obstacle with the same ten parameters.  Every step, between the assembly
 * of p and the solve, each active robot's predicted poses (those of nmpc_loop_set_peers) are compared with this step's table: C(b, d) = min
 * over the stages k of |pred[b][k] - table[d][k]|^2 (unfused f64; a comparison that is false because of a NaN neither lowers the minimum nor
 * makes a candidate), and the first M obstacles with C < range^2 in (C, d) order are copied, row by row, over the ellipse slots K .. K + M - 1
 * of its p.  A slot that finds no obstacle keeps what the assembly put there; the block the loop carries never sees the crowd; a retired
 * robot keeps its p and its seen.  With a crowd the peers' slots follow the crowd's: scripted [0, K), crowd [K, K + M), peers from K + M on.
 *   obst [D][10]  (p1x, p1y, p2x, p2y, freq, rx, ry, angle, sinus, direction) per obstacle, as dyn of nmpc_loop_new.  The values are not
 *                 checked: an obstacle with a NaN is never a candidate, and no loop's bounds depend on them.
 *   pad           added to both radii (nmpc_route.dyn_pad of the scripted ellipses), finite
 *   M             ellipse slots given to the crowd, M >= 1 and K + M (+ the peers' M) <= Ndynobs
 *   range         finite and > 0
 * To be called once, before the loop's first step, in any order with the other setters; whichever of this and the peers setters comes second
 * checks that all three kinds fit.  NMPC_ERR_BAD_ARG with a message, nothing changed and nothing allocated, for D < 1 or D > 16384, obst NULL,
 * M < 1, K + M (+ the peers' M) > Ndynobs, a pad that is not finite, a range that is not finite and positive, a call after a step, or a
 * second call.  A loop without a crowd enqueues what it enqueued before this function existed. */
int nmpc_loop_set_crowd(nmpc_loop *l, int D, const double *obst, double pad, int M, double range);
/* Synchronises, then copies what is asked for (NULL = skip): table [D][N][5] as the last step wrote it, and seen [B][M], the obstacle in
 * slot K + m of each robot's p at its last step, -1 for none.  NMPC_ERR_BAD_ARG on a loop without a crowd or before its first step. */
int nmpc_loop_crowd(nmpc_loop *l, double *table, int32_t *seen);
/* The crowd through a grid in space and stage: nmpc_loop_set_crowd with the same rule, table, slots, seen and observer, bit for bit, for
 * up to 131072 obstacles, at a cost that grows with what is near a robot and not with the world (the rule, and why it misses nobody and
 * keeps nobody twice: DESIGN.md section 5.9).  The setter fixes the geometry on the host: origin = the minimum per axis over the end
 * points p1, p2 of obst whose two coordinates are finite, per axis floor(extent / cell) + 1 cells of edge `cell`, or 128 cells of edge
 * extent / 128 where that would be more (one cell at (0, 0) without a finite end point), and N layers, one per stage.  Every step with an
 * active robot, behind the table's advance, entry (d, k) of the table is filed under the cell of its position in layer k (unfiled if a
 * coordinate is not finite; a position outside the extent goes to the edge cell), by a counting sort of five kernels; a robot then
 * looks, per stage k at which its predicted position is finite, at the entries filed in the cells from that of (x - range) to that of
 * (x + range) per axis in layer k, and entry (d, k) makes d a candidate, with the C(b, d) of nmpc_loop_set_crowd, if its d_k < range^2
 * and no stage j < k has d_j < range^2.  One kernel takes the place of the all-obstacles selection.  The observer
 * (nmpc_loop_set_crowd_monitor) stays all obstacles: its level has no cut-off a grid could use.
 * This is the loop's crowd call: either setter after the other, a second call or a call after a step is refused.  NMPC_ERR_BAD_ARG with
 * a message, nothing changed and nothing allocated, for everything nmpc_loop_set_crowd refuses (but D up to 131072 is taken) and for a
 * cell that is not finite and positive.  nmpc_loop_crowd, nmpc_loop_set_crowd_monitor and nmpc_loop_crowd_clearance work on either kind. */
int nmpc_loop_set_crowd_grid(nmpc_loop *l, int D, const double *obst, double pad, int M, double range, double cell);
/* The crowd's grid, for tests and reports: the origin, the cells' edges and the cells per axis, the layers (N), and the entries filed at
 * the last build (0 before any build). */
typedef struct nmpc_crowd_grid {     /* 48 bytes */
    double  origin[2], h[2];
    int32_t nx, ny, layers, filed;
} nmpc_crowd_grid;
#ifdef __cplusplus
static_assert(sizeof(nmpc_crowd_grid) == 48, "nmpc_crowd_grid layout");
#else
_Static_assert(sizeof(nmpc_crowd_grid) == 48, "nmpc_crowd_grid layout");
#endif
/* Synchronises, then copies what is asked for (NULL = skip): the header (available right after the setter), cell_of [D][N], the cell
 * (layer * nx * ny + y * nx + x) each entry of the last step's table was filed under, -1 for an unfiled one, and looked [B], the filed
 * entries in each robot's windows at its last step (a retired robot keeps its last; the all-obstacles selection looks at D * N).
 * NMPC_ERR_BAD_ARG on a loop without nmpc_loop_set_crowd_grid, and for cell_of or looked before the loop's first step. */
int nmpc_loop_crowd_grid(nmpc_loop *l, nmpc_crowd_grid *out, int32_t *cell_of, int32_t *looked);
/* Crowd observer: each robot's closest approach to ANY obstacle of the crowd, in a slot of its p or not.  One more kernel per step, after the
 * advance, over the robots the step drove: for each of the step's s trajectory rows r = first + i and every d < D, the cost's level
 * (a*a)/(rx*rx) + (c*c)/(ry*ry) of the pose of row r against entry i of obstacle d's row of this step's table ((a, c) as nmpc_clearance's
 * ellipse).  The record is the lexicographic minimum of (level, row, obstacle) from (+inf, -1, -1); a comparison that is false keeps it, and a
 * retired robot keeps its record.  It observes only.  To be called once, before the first step and after nmpc_loop_set_crowd, on a loop that
 * records its trajectory.  NMPC_ERR_BAD_ARG with a message, nothing changed and nothing allocated, for a loop without a crowd, a loop with
 * max_steps == 0, a call after a step, or a second call. */
typedef struct nmpc_crowd_clearance {    /* 16 bytes */
    double  level;
    int32_t row, obstacle;
} nmpc_crowd_clearance;
#ifdef __cplusplus
static_assert(sizeof(nmpc_crowd_clearance) == 16, "nmpc_crowd_clearance layout");
#else
_Static_assert(sizeof(nmpc_crowd_clearance) == 16, "nmpc_crowd_clearance layout");
#endif
int nmpc_loop_set_crowd_monitor(nmpc_loop *l);
/* Synchronises, then copies the records out [B]; on a loop without the observer the initial record everywhere. */
int nmpc_loop_crowd_clearance(nmpc_loop *l, nmpc_crowd_clearance *out);

/* ---- plant: seeded actuation, process and measurement noise, drawn on the device ------------------
 * A loop closes on its own model: the advance applies exactly the controls the solve returned, by exactly the Euler step the solver
 * predicts with.  The plant is an opt-in stage that stands where the advance stands and disturbs what the robot does, where that takes
 * it and what the controller is told (the rule: DESIGN.md section 5.9).  Disturbances are xi(id, r, c): Philox4x32-10 on the counter
 * (id, r, c, 0) under the key (seed & 0xffffffff, seed >> 32), the four output words summed to S, xi = double(S + 2 - 2^33) * C with
 * C = 0x1.bb67ae8584caap-32, the double nearest sqrt(3) * 2^-32: symmetric, mean 0, variance 1, |xi| <= 2 sqrt(3), and the same double
 * on every machine.  id = ids[b] (NULL: b), r = a trajectory row, c = a channel: a robot's disturbances do not depend on who else is
 * active, on how a fleet is split over loops, or on any launch order.  Unfused f64, the statements in the order written:
 *   measurement, at the start of a step, for every active robot, m = the row of its pose (step_before * s; row 0 is the start):
 *       meas_x = x + meas[0]*xi(id, m, 5), y and theta likewise with channels 6 and 7; a channel whose sigma is 0 copies the value.
 *       The assembly of p and the predicted poses (peers, crowd) start from the measured pose; nothing else reads it.
 *   plant, in the place of the advance, for control i of the step, r = step_before * s + 1 + i, (v, w) the pair the solve returned:
 *       t = act_gain[0]*v;  t = t + act_add[0];  va = v + t*xi(id, r, 0)      (skipped, va = v, if act_gain[0] == 0 and act_add[0] == 0)
 *       wa likewise with index 1 and channel 1
 *       x  = x + ts*(va*cos th);  x  = x  + proc[0]*xi(id, r, 2)              (the second statement skipped if proc[0] == 0)
 *       y  = y + ts*(va*sin th);  y  = y  + proc[1]*xi(id, r, 3)
 *       th = th + ts*wa;          th = th + proc[2]*xi(id, r, 4)
 * The trajectory, the state, the monitors, the drive log's path length, retirement and the missions see the true pose; last_u, p[3],
 * p[4] and the drive log's controls are the COMMANDED controls, what the controller knows it sent, and the terminal test reads the true
 * pose and the commanded v.  A plant whose sigmas are all 0 executes the advance's operations and no others: the loop's bits are those
 * of the loop without it.  With keep_applied the pairs (va, wa) are kept, applied [max_steps * s][B][2], +0.0 where a robot was not driven.
 * To be called once, before the loop's first step, in any order with the other setters.  NMPC_ERR_BAD_ARG with a message that names the
 * function, and nothing changed or allocated, for plant NULL, a sigma that is negative, infinite or a NaN, keep_applied on a loop with
 * max_steps == 0, a call after a step, or a second call (a NULL loop: NMPC_ERR_BAD_ARG).  A loop without a plant enqueues what it
 * enqueued before this function existed. */
typedef struct nmpc_plant {              /* 96 bytes */
    uint64_t seed;
    double   act_gain[2], act_add[2];    /* v, w: sigma of the actuation noise = act_gain * control + act_add */
    double   proc[3];                    /* x, y, theta: sigma per applied control */
    double   meas[3];                    /* x, y, theta */
    int32_t  keep_applied, reserved;
} nmpc_plant;
#ifdef __cplusplus
static_assert(sizeof(nmpc_plant) == 96, "nmpc_plant layout");
#else
_Static_assert(sizeof(nmpc_plant) == 96, "nmpc_plant layout");
#endif
int nmpc_loop_set_plant(nmpc_loop *l, const nmpc_plant *plant, const uint32_t *ids);
/* Synchronises, then copies the controls that acted so far out [steps * s][B][2] and returns their number of rows (or < 0);
 * NMPC_ERR_BAD_ARG if `rows`, the rows the caller's buffer holds, is smaller.  A loop that keeps none reports 0 rows and writes nothing. */
int nmpc_loop_plant_applied(nmpc_loop *l, double *out, int rows);
/* Synchronises, then copies out [B][3] what the last step's solves were given as poses: the measured poses on a loop whose plant has a
 * meas > 0 (a retired robot's: of its last step), else p[0 .. 3) of every robot; before the first step the start states. */
int nmpc_loop_plant_measured(nmpc_loop *l, double *out);

/* ---- ensemble: per-group pose statistics after every step, on device -----------------------------
 * B copies of one robot under a plant are a Monte-Carlo study of one controller, G routes or tunings x M seeded copies a comparison of
 * G controllers; what such a run is asked for is where the copies are on average, how far they have spread and how many have arrived,
 * step by step.  The ensemble is an opt-in stage of the loop that keeps one nmpc_ensemble_stat per group and step on the device,
 * ens [max_steps][G] (the rule: DESIGN.md section 5.9).  It observes only: no p, u, y, state, status, trajectory or other record
 * differs by a bit from the loop without it.  One more kernel per step, one workgroup per group, the step's LAST: behind the drive
 * log, the missions' dispatch and, on a retiring loop, the compaction.  Unfused f64 in the order written:
 *   members   of group g: the robots b with group_of[b] == g in ascending b, m_0 < ... < m_{n-1} (group_of NULL: one group of
 *             everybody).  Every member counts, active, retired or re-dispatched; the pose read is the true `state` (under a plant
 *             never the measured one), a retired robot's the pose it was parked at.  A group may be empty.
 *   when      at the end of step k (1-based, the step retired_at takes), row k - 1; also in a step in which nobody is active any more.
 *   n         the member count.
 *   arrived   on a retiring loop the members with retired_at[b] >= 0, this step's retirements included (a mission robot between legs
 *             is not counted); otherwise the members with done[b] != 0: this row's terminal test, not a latch.
 *   SUM(v)    of one value per member, a fixed tree: slot t of 256 starts at +0.0 and takes acc = acc + v[m_i] for i = t, t + 256, ...
 *             in ascending i; within each block of 64 slots, for off = 32, 16, 8, 4, 2, 1: a[l] = a[l] + a[l + off] for l < off (what an
 *             xor butterfly leaves in every lane, IEEE addition being commutative); the four block sums w0 .. w3 give
 *             ((w0 + w1) + w2) + w3.
 *   mean      S = (SUM x, SUM y, SUM theta); mean = S / double(n), one IEEE division each.
 *   cov       against the mean just formed, dx = x - mean_x, dy and dth likewise:
 *             (SUM dx*dx, SUM dx*dy, SUM dy*dy, SUM dth*dth) / double(n).  Each product is rounded before it enters the tree; a
 *             population covariance; theta as the loop keeps it, not wrapped.
 *   far2, far_robot   the largest r2 = dx*dx + dy*dy over the members and the smallest robot index that has it: the lexicographic
 *             extreme of (r2, b) by `r2 > far2 || (r2 == far2 && b < far_robot)` from (-1.0, -1).  A comparison that is false because
 *             of a NaN keeps the record.
 *   an empty group: n = 0, arrived = 0, every double +0.0, far2 = -1.0, far_robot = -1.
 * To be called once, before the loop's first step, in any order with the other setters, on a loop with max_steps > 0 (the table's
 * length).  NMPC_ERR_BAD_ARG with a message that names the function, and nothing changed or allocated, for max_steps == 0, a call
 * after a step, a second call, G < 1 or G > 65536, group_of NULL with G != 1 or a group_of[b] outside [0, G) (a NULL loop:
 * NMPC_ERR_BAD_ARG).  A loop without the stage enqueues what it enqueued before this function existed. */
typedef struct nmpc_ensemble_stat {      /* 80 bytes */
    int32_t n, arrived, far_robot, reserved;     /* reserved: 0 */
    double  mean[3];                     /* x, y, theta */
    double  cov[4];                      /* xx, xy, yy, theta-theta */
    double  far2;
} nmpc_ensemble_stat;
#ifdef __cplusplus
static_assert(sizeof(nmpc_ensemble_stat) == 80, "nmpc_ensemble_stat layout");
#else
_Static_assert(sizeof(nmpc_ensemble_stat) == 80, "nmpc_ensemble_stat layout");
#endif
int nmpc_loop_set_ensemble(nmpc_loop *l, const int32_t *group_of, int G);
/* Synchronises, then copies the records of the steps taken so far out [steps][G] and returns the step count (or < 0);
 * NMPC_ERR_BAD_ARG if max_steps, the steps the caller's buffer holds, is smaller.  A loop without the stage reports 0 steps and writes
 * nothing. */
int nmpc_loop_ensemble(nmpc_loop *l, nmpc_ensemble_stat *out, int max_steps);
/* G, or 0 on a loop without the stage. */
int nmpc_loop_ensemble_groups(nmpc_loop *l);

/* ---- walls: the nearest points of the map's wall segments, as circles, on device --------------------
 * The only static obstacles the assembly puts into p are circles on the vertices a route bends around; a wall between two corners, an
 * obstacle the route merely passes and the boundary are not in p, and the map monitor can count wall hits but nothing prevents them.
 * The walls are an opt-in stage of the loop (the rule: DESIGN.md section 5.9): every step, between the assembly of p and the solve --
 * behind the crowd's and the peers' overlays, in front of the gather of a retiring loop -- each active robot's closest points on the E wall
 * segments, measured against its predicted poses (X_k, Y_k), k = 0 .. N - 1 (those of the peers setters and of the crowd: with a plant
 * that measures they start from the measured pose), become circles in the LAST M static-circle slots of its p.  Unfused f64 in the order
 * written, `/` IEEE, no sqrt:
 *   per edge e and stage k   the map monitor's wall distance: ex = x2 - x1, ey = y2 - y1, L2 = ex*ex + ey*ey; t = 0 unless L2 > 0, then
 *                            t = ((X - x1)*ex + (Y - y1)*ey)/L2, `if (t < 0) t = 0; if (t > 1) t = 1`; cx = x1 + t*ex, cy = y1 + t*ey,
 *                            dx = X - cx, dy = Y - cy, v = dx*dx + dy*dy
 *   per edge                 D(e) from +inf takes v on the strict v < D, stages ascending (a NaN never lowers it, the first of equal stages
 *                            stays); k*(e) is that stage and (cx, cy) of that stage the edge's centre; a candidate if D(e) < range*range
 *   selection                the candidates in ascending (D, e) order; one is skipped if ddx*ddx + ddy*ddy < spacing*spacing against the
 *                            centre of any candidate already taken (spacing = 0 skips nothing), otherwise taken; M taken at the most
 *   placement                the m-th taken (m = 0, 1, ...) over circle slot Nobs - M + m of p as (cx, cy, radius); a slot that finds no
 *                            candidate keeps what the assembly put there, zeros
 *   record                   wall_edge [B][M] = the edge in that slot, wall_stage [B][M] = its k*, -1 for none
 * The last M slots are free because the setter refuses a loop on which any of its R routes has n_vert + M > Nobs (under missions every
 * route is a candidate for every robot): the assembly fills at most n_vert slots from the front and zeroes the rest every step.  A retired
 * robot keeps its p and its record, a step with nobody active launches nothing for the stage.  The solver does not change: a circle is
 * culled by its own radius.  The clearance monitor reads the circle slots of p as the solve read them, radius > 0, so its `circle`
 * record sees the wall circles too: that is intended.
 *   edge [n_edge][4]  x1 y1 x2 y2 per wall segment, every coordinate finite, 1 <= n_edge <= 1024; no polygon structure is needed
 *   M                 circle slots given to the walls, 1 <= M <= Nobs and n_vert + M <= Nobs on every route
 *   radius, range     finite and > 0;  spacing  finite and >= 0
 * To be called once, before the loop's first step, in any order with the other setters; it makes the predicted poses exist as a crowd
 * alone does.  NMPC_ERR_BAD_ARG with a message that names the function, and nothing changed or allocated, for a NULL edge (a NULL loop:
 * NMPC_ERR_BAD_ARG), n_edge outside 1 .. 1024, a coordinate that is not finite, M < 1, M > Nobs, a route with n_vert + M > Nobs (the
 * message names it), a radius or a range that is not finite and positive, a spacing that is negative or not finite, a call after a step,
 * or a second call.  A loop without the stage enqueues what it enqueued before this function existed. */
int nmpc_loop_set_walls(nmpc_loop *l, int n_edge, const double *edge, int M, double radius, double range, double spacing);
/* Synchronises, then copies what is asked for (NULL = skip): wall_edge [B][M] and wall_stage [B][M] of each robot's last step, -1 for
 * none.  NMPC_ERR_BAD_ARG on a loop without walls or before its first step. */
int nmpc_loop_walls(nmpc_loop *l, int32_t *wall_edge, int32_t *wall_stage);

/* ---- walls of large maps: the edges a robot measures are found through a grid ---------------------
 * nmpc_loop_set_walls measures every edge against every robot and takes 1024 edges at the most.  nmpc_loop_set_walls_grid is the same
 * stage with the same rule -- its result IS nmpc_loop_set_walls' rule over all n_edge edges, for any n_edge it accepts: D(e), k*(e), the
 * (D, e) selection with spacing, the placement and the record are the ones above -- but a robot forms D(e) only for the edges filed near
 * it in a uniform grid.  The edges never move: the setter builds the grid once, on the host, and uploads it (DESIGN.md section 5.9 has
 * the rule and the argument that no edge with D(e) < range*range is ever hidden).
 *   grid      origin = the minimum over all edge end points, per axis; per axis n = floor(extent/cell) + 1 cells of edge h = cell, or, where
 *             that would be more than 512 (the cap), n = 512 cells of edge h = extent/512; nx, ny >= 1
 *   cellof    cellof(v) = clamp(floor((v - origin)/h), 0, n - 1) per axis, clamped in double before the conversion: monotone in v
 *   filing    edge e in every cell of cellof(min(x1, x2)) .. cellof(max(x1, x2)) x cellof(min(y1, y2)) .. cellof(max(y1, y2))
 *   storage   CSR, cells row-major (y*nx + x): cell c holds cell_edge[cell_off[c] .. cell_off[c + 1]), edge indices ascending
 *   window    lo, hi = the minimum and maximum of the robot's predicted positions over the stages at which both coordinates are finite (a
 *             robot without such a stage looks at nothing and gets no wall); per axis the cells cellof((lo - range) - m(lo)) ..
 *             cellof((hi + range) + m(hi)) with the margin m(v) = slack + 2^-40*|v|, slack = 2^-40*(range + A) + 2^-500, A the largest
 *             |coordinate| of an edge
 *   looked    [B]: the distinct edges of the window's cells, each measured once however many cells it is filed in
 * One kernel per step, one wave per active robot, in nmpc_loop_walls_kernel's place.  Candidates go to a list of 256 in LDS; a robot with
 * more takes exact rounds that measure the window again for "the smallest (D, e) behind the last one considered": no bound on candidates.
 *   n_edge            1 .. 1048576
 *   cell              finite and > 0, metres
 *   filings           8388608 (2^23) at the most over all edges
 * Everything else as nmpc_loop_set_walls, refusals included; in addition NMPC_ERR_BAD_ARG, with a message that names the function and
 * nothing changed or allocated on the device, for a cell that is not finite and positive and for a map with more filings than the limit
 * (the message says to use a larger cell or shorter edges).  It is the loop's walls call: a second call, a call after a step and a call
 * after nmpc_loop_set_walls are refused, and nmpc_loop_set_walls after it.  nmpc_loop_walls reads the record of either setter. */
int nmpc_loop_set_walls_grid(nmpc_loop *l, int n_edge, const double *edge, int M, double radius, double range, double spacing, double cell);
typedef struct nmpc_wall_grid {
    double origin[2], h[2];
    int32_t nx, ny, entries, reserved;
} nmpc_wall_grid;
/* Synchronises, then copies what is asked for (NULL = skip): the grid's header, cell_off [nx*ny + 1], cell_edge [entries] (read the
 * header first for the sizes) and looked [B] of the last step (a retired robot keeps its last).  NMPC_ERR_BAD_ARG on a loop without
 * nmpc_loop_set_walls_grid, and when looked is asked for before the loop's first step. */
int nmpc_loop_wall_grid(nmpc_loop *l, nmpc_wall_grid *out, int32_t *cell_off, int32_t *cell_edge, int32_t *looked);

/* ---- map monitor of large maps: the edges a row is judged against are found through the walls grid --
 * nmpc_loop_set_map_monitor measures every pose against every edge and takes 1024 edges at the most.  nmpc_loop_set_map_monitor_grid is
 * the same stage with the same record over a map of up to 1048576 edges: a row is judged against the edges filed near it in THE WALLS
 * GRID above (origin, the cap of 512 cells per axis, cellof, the filing of an edge in the rectangle of its end points' cells, CSR with
 * ascending edge indices, 2^23 filings at the most, m(v) = slack + 2^-40*|v| with slack = 2^-40*(range + A) + 2^-500 and A the largest
 * |coordinate| of an edge), built once by the setter over the map's edges.  Everything is unfused f64 in the order written, as the
 * all-edges rule above, whose v, containment predicate and crossing test are used word for word.  For the pose P = (x, y) of row r and
 * A = (ax, ay) of row r - 1:
 *   window W(r)   per axis the cells cellof((lo - range) - m(lo)) .. cellof((hi + range) + m(hi)), lo and hi the smaller and larger of the
 *                 two rows' coordinates on that axis; every distinct edge filed in W(r) is taken once, however many cells hold it
 *   wall distance for those edges, v against P; only v < range*range is a candidate; the record keeps the lexicographic minimum of
 *                 (v, r, e) as above
 *   crossing      for those edges, o1*o2 < -1e-9 && o3*o4 < -1e-9; the polygon that owns a crossed edge fails
 *   containment   the cells of grid row cellof_y(y) from column cellof_x(x - m(x)) to the last; every distinct edge filed there is taken
 *                 once: (y1 > y) != (y2 > y) and x1 + ((y - y1)*(x2 - x1))/(y2 - y1) > x is a crossing of the edge's polygon; parity per
 *                 polygon, an obstacle fails on an odd count, the boundary on an even one
 *   non-finite    if x, y, ax or ay is not finite the row takes the whole grid for all three tests, every edge once: the all-edges rule
 *   verdict       as above: the smallest failing polygon index, hits, hit_row, hit_poly; the record, its initial values, retired robots
 *                 and legs as above
 * Wall distance (restricted to v < range*range) and containment are the all-edges rule's for every input, and an edge the all-edges
 * rule finds crossed lies in W(r) under the bound of DESIGN.md section 5.9, which has the arguments.  Nothing bounds the candidates or
 * the ray's hits: a pose whose ray meets more obstacle edges than the kernel's list holds (512) is judged in exact rounds.
 *   n_edge            3 .. 1048576, n_poly >= 1
 *   range, cell       finite and > 0, metres
 *   filings           8388608 (2^23) at the most over all edges
 * Everything nmpc_loop_set_map_monitor refuses is refused here, and a range or a cell that is not finite and positive and a map with
 * more filings than the limit: NMPC_ERR_BAD_ARG with a message that names the function, nothing changed or allocated on the device.  It
 * is the loop's map-monitor call: a second call, a call after a step and a call after nmpc_loop_set_map_monitor are refused, and
 * nmpc_loop_set_map_monitor after it.  nmpc_loop_map_clearance reads the record of either setter. */
int nmpc_loop_set_map_monitor_grid(nmpc_loop *l, const nmpc_scene *map, double range, double cell);
/* Synchronises, then copies what is asked for (NULL = skip): the grid's header, cell_off [nx*ny + 1], cell_edge [entries] (read the
 * header first for the sizes) and looked [B]: the distinct edges of W(r) summed over the rows of each robot's last step (a retired
 * robot keeps its last).  NMPC_ERR_BAD_ARG on a loop without nmpc_loop_set_map_monitor_grid, and when looked is asked for before the
 * loop's first step. */
int nmpc_loop_map_grid(nmpc_loop *l, nmpc_wall_grid *out, int32_t *cell_off, int32_t *cell_edge, int32_t *looked);

/* Arithmetic primitives of the kernels, exported for bit-level checks: out_s/out_c [n]. */
int nmpc_test_sincos_host(nmpc_handle *h, int n, const double *x, double *out_s, double *out_c);
/* a/b and sqrt(a) as the device computes them: out_div/out_sqrt [n]. */
int nmpc_test_divsqrt_host(nmpc_handle *h, int n, const double *a, const double *b,
                           double *out_div, double *out_sqrt);

#ifdef __cplusplus
}
#endif
#endif
