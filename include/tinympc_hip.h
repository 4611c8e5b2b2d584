/* libtinympc_hip.so — C-ABI of the MI355X batched TinyMPC ADMM engine.
 *
 * Drop-in boundary: the reference's Julia module reaches its solver through
 * `ccall((:sym, libtinympc_jl), Int32, ...)` into src/bindings.cpp
 * (reference: src/TinyMPC.jl:12-14, src/bindings.cpp:15-490).  This header
 * declares
 *   (1) the same symbol names with the SAME argument lists and return
 *       conventions as bindings.cpp, operating on one process-global solver, so
 *       the unmodified TinyMPC.jl can ccall this library instead; the batch
 *       dimension rides on the (rows, cols) arguments the reference already
 *       passes (x0 as nx x B, x_ref as nx x N*B, ...), and
 *   (2) a handle-based extension (`tinympc_*`) adding what a batched, device-
 *       resident engine needs: batch size, per-instance status, cold reset,
 *       device-pointer I/O and stream-ordered solves.
 *
 * Conventions (as bindings.cpp): every matrix is column-major fp64 passed as
 * pointer + (rows, cols); inputs are borrowed for the call only; outputs are
 * written into caller-allocated buffers; return 0 = OK, -1 = error (message on
 * stderr); solve_mpc passes the solver status through (0 all converged, 1 some
 * instance hit max_iter).  Plain C, no torch / HIP types except the opaque
 * stream handle (void*).  The library has no CPU fallback: every entry point
 * that computes fails with -1 when no HIP device is usable.
 */
#ifndef TINYMPC_HIP_H
#define TINYMPC_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* (1) process-global solver: the reference's own entry points               */
/* ------------------------------------------------------------------------- */

/* replaces bindings.cpp:21-73 setup_solver.  A non-zero fdyn (affine dynamics x+ = A x + B u + f)
 * is honoured, but its arithmetic lives only in the un-vendored TinyMPC submodule (SURVEY.md §0
 * fact 2): parity for it is UNPINNED, and such problems run on the stream (or generic) kernel.
 * Batch starts at 1; see set_batch_size. */
int setup_solver(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols,
                 double *fdyn_data, int fdyn_rows, int fdyn_cols, double *Q_data, int Q_rows,
                 int Q_cols, double *R_data, int R_rows, int R_cols, double rho, int nx, int nu,
                 int N, int verbose);

/* replaces bindings.cpp:75-96.  x0 is nx x 1 (broadcast to every instance) or nx x batch. */
int set_x0(double *x0_data, int x0_rows, int x0_cols, int verbose);
/* replaces bindings.cpp:98-119.  nx x N (shared by the batch) or nx x (N*batch). */
int set_x_ref(double *x_ref_data, int x_ref_rows, int x_ref_cols, int verbose);
/* replaces bindings.cpp:121-142.  nu x (N-1) (shared) or nu x ((N-1)*batch). */
int set_u_ref(double *u_ref_data, int u_ref_rows, int u_ref_cols, int verbose);
/* replaces bindings.cpp:144-159.  0: every instance converged, 1: some hit max_iter, -1: error. */
int solve_mpc(int verbose);
/* replace bindings.cpp:161-203.  Buffers hold nx*N*batch / nu*(N-1)*batch doubles;
 * rows = nx / nu, cols = N*batch / (N-1)*batch (Julia: reshape to (nx, N, batch)). */
int get_states(double *states_buffer, int *rows, int *cols);
int get_controls(double *controls_buffer, int *rows, int *cols);
/* replaces bindings.cpp:205-208 */
void cleanup_solver(void);
/* Additions next to bindings.cpp:75,161,183 for hosts that keep Float32 arrays: the same three per-solve transfers without
 * the fp64 narrowing / widening pass on the host (the device buffers are fp32; a 65 536-instance cartpole round trip is
 * 1.3 ms through the fp64 forms, most of it that pass).  Shapes and conventions as set_x0 / get_states / get_controls. */
int set_x0_f32(float *x0_data, int x0_rows, int x0_cols, int verbose);
int get_states_f32(float *states_buffer, int *rows, int *cols);
int get_controls_f32(float *controls_buffer, int *rows, int *cols);
/* Page-lock / release a caller-owned host array that is reused with the fp32 forms above (direct DMA instead of a bounce
 * through pageable memory).  The library never registers caller memory on its own; unpin before the array is freed. */
int set_precision(int precision);   /* tinympc_set_precision on the process-global solver: 0 default, 1 all fp32, 2 all fp64 */
int pin_host_buffer(void *ptr, size_t bytes);
int unpin_host_buffer(void *ptr);
/* replaces bindings.cpp:336-376.  en_*_soc / en_*_linear switch the sets given to set_cone_constraints /
 * set_linear_constraints on and off (parity unpinned).  adaptive_rho != 0 turns on the per-instance rho adaptation of
 * admm.cpp:147-174 (see tinympc_set_adaptive_rho; runs on the generic kernel).  check_termination <= 0 means "never check"
 * (the reference divides by it, admm.cpp:91). */
int update_settings(double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                    int en_state_bound, int en_input_bound, int en_state_soc, int en_input_soc,
                    int en_state_linear, int en_input_linear, int adaptive_rho,
                    double adaptive_rho_min, double adaptive_rho_max,
                    int adaptive_rho_enable_clipping, int verbose);
/* replaces bindings.cpp:378-411.  Bounds are per knot (nx x N, nu x (N-1)), shared by the batch;
 * enables en_state_bound and en_input_bound on success.  With batch > 1 the batch dimension may ride on the column counts, as
 * it does for set_x_ref: x_min / x_max nx x (N*batch) together with u_min / u_max nu x ((N-1)*batch) give every instance its own
 * bounds at every knot (tinympc_set_instance_bounds with per_knot = 1; a set_gpus solver scatters them to its shards).  All
 * four arrays must then have the per-instance width: mixed widths are an error. */
int set_bound_constraints(double *x_min_data, int x_min_rows, int x_min_cols, double *x_max_data,
                          int x_max_rows, int x_max_cols, double *u_min_data, int u_min_rows,
                          int u_min_cols, double *u_max_data, int u_max_rows, int u_max_cols,
                          int verbose);
/* replaces bindings.cpp:262-293 */
int set_cache_terms(double *Kinf_data, int Kinf_rows, int Kinf_cols, double *Pinf_data,
                    int Pinf_rows, int Pinf_cols, double *Quu_inv_data, int Quu_inv_rows,
                    int Quu_inv_cols, double *AmBKt_data, int AmBKt_rows, int AmBKt_cols,
                    int verbose);
/* The sensitivities the reference takes through codegen_with_sensitivity (bindings.cpp:298-334; TinyMPC.jl:374-394) for
 * its generated solver, here for the live one: dK (nu x nx), dP (nx x nx); dC1 / dC2 may be NULL (see
 * tinympc_set_sensitivity).  Optional: update_settings(adaptive_rho = 1) without it computes them on first use. */
int set_sensitivity(double *dK_data, int dK_rows, int dK_cols, double *dP_data, int dP_rows, int dP_cols,
                    double *dC1_data, int dC1_rows, int dC1_cols, double *dC2_data, int dC2_rows, int dC2_cols,
                    int verbose);
/* rho of every instance after adaptation (the reference's solver->cache->rho, one per instance); *count = batch */
int get_adaptive_rho(double *rho_buffer, int *count);
/* replaces bindings.cpp:228-259 */
int print_problem_data(int verbose);
/* replace bindings.cpp:413-490.  set_linear_constraints: Alin_x x <= blin_x and Alin_u u <= blin_u at every knot
 * (README.md:115-116), column-major (rows x nx) / (rows x nu), at most 8 rows per side (an equality is two rows,
 * TinyMPC.jl:258-267); enables the non-empty halves.  set_cone_constraints: per-knot second-order cones, inputs first; cone i covers rows
 * [Ac[i], Ac[i]+qc[i]) of each knot, the LAST row is the axis: ||head|| <= c[i] * axis
 * (rocket_landing_constraints.jl:51-57,132); at most 8 cones per side; enables the non-empty halves.
 * Cone, linear-inequality and fdyn arithmetic lives only in the absent submodule — parity UNPINNED.
 * With batch > 1 the batch dimension may ride on the widths, as it does for set_bound_constraints: Alin_x rows_x x (nx*batch)
 * with blin_x_len = rows_x*batch, Alin_u rows_u x (nu*batch) with blin_u_len = rows_u*batch give every instance its own rows
 * (tinympc_set_instance_linear: [batch] blocks of rows x n, column-major, and [batch][rows]; a set_gpus solver scatters the
 * slices to its shards).  Every non-empty side must then have the per-instance width: mixed widths are an error.
 * set_cone_constraints takes the batch on its widths likewise: cu_len == Acu_len*batch and cx_len == Acx_len*batch, laid out
 * [batch][cone], give every instance its own coefficients over the one layout (tinympc_set_instance_cones; +inf: a cone the
 * instance does not have); mixed widths are an error. */
int set_linear_constraints(double *Alin_x_data, int Alin_x_rows, int Alin_x_cols,
                           double *blin_x_data, int blin_x_len, double *Alin_u_data,
                           int Alin_u_rows, int Alin_u_cols, double *blin_u_data, int blin_u_len,
                           int verbose);
int set_cone_constraints(int *Acu_data, int Acu_len, int *qcu_data, int qcu_len, double *cu_data,
                         int cu_len, int *Acx_data, int Acx_len, int *qcx_data, int qcx_len,
                         double *cx_data, int cx_len, int verbose);

/* --- batch extensions on the global solver (no counterpart in bindings.cpp) --- */
/* Re-shapes the global solver to `batch` instances; per-instance inputs/state are reset. */
int set_batch_size(int batch);
int get_batch_size(void);
/* Per-instance iteration count, solved flag and the 4 residuals
 * (pri_state, dua_state, pri_input, dua_input) — the batched form of
 * solution->iter / solution->solved / work->*_residual_* (types.hpp:32-37,128-131).
 * Any pointer may be NULL. */
int get_status(int *iter, int *solved, double *residuals4);
/* Cold start: zero d, y, g, v, z of every instance (what tiny_setup leaves, tiny_api.cpp:73-88). */
int reset_workspace(void);
/* The fused closed loop on the process-global solver (tinympc_mpc_rollout / tinympc_set_ref_sequence below): `steps`
 * repetitions of  set_x0 -> [set_x_ref / set_u_ref of the step] -> solve -> x0 = A x0 + B u0 + f  in one launch — the loop of
 * examples/cartpole_example_mpc.jl:35-51 and examples/rocket_landing_constraints.jl:97-134.  Returns the status of the last
 * step's solve (0 / 1) or -1; logs (any may be NULL) as tinympc_get_mpc_log. */
int set_ref_sequence(double *x_ref_seq, int x_rows, int x_cols, double *u_ref_seq, int u_rows, int u_cols, int steps);
int mpc_rollout(int steps, double *x_log, double *u_log, int *iter_log);
/* ... against a plant of its own and under an additive disturbance (tinympc_set_plant / tinympc_set_disturbance below, which
 * describe them).  Shapes are checked: A nx x nx, B nx x nu, f_len nx (f NULL: zero), or with per_instance = 1 A nx x (nx batch),
 * B nx x (nu batch), f_len nx batch; w nx x steps or nx x (steps batch), the step count taken from w_cols.  A = B = NULL and
 * w = NULL drop them.  Not on a set_gpus solver, which has no mpc_rollout. */
int set_plant(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols, double *f_data, int f_len, int per_instance);
int set_disturbance(double *w_data, int w_rows, int w_cols, int per_instance);
int plant_mode(void);
/* ... and along a reference trajectory, windowed on the device (tinympc_set_ref_trajectory below, which describes it): x_data
 * nx x Lx and u_data nu x Lu column-major (u_data NULL: zero input references), or with per_instance = 1 nx x (Lx batch) and
 * nu x (Lu batch), instance after instance — the batch rides on the column count.  Row counts and widths are checked.
 * x_data = NULL drops it.  set_ref_cursor (refused when negative) / ref_cursor move and read the cursor.  Not on a set_gpus
 * solver, which has no mpc_rollout. */
int set_ref_trajectory(double *x_data, int x_rows, int x_cols, double *u_data, int u_rows, int u_cols, int per_instance, int verbose);
int set_ref_cursor(int cursor);
int ref_cursor(void);
/* ... and under seeded process / measurement noise drawn on the device (tinympc_set_process_noise below, which describes it):
 * G_data nx x nx column-major, or with per_instance = 1 nx x (nx batch), instance after instance; row and column counts are
 * checked.  G_data = NULL drops that kind.  set_noise_cursor (refused when negative) / noise_cursor move and read the one cursor
 * both kinds share; noise_mode, get_noise and get_mpc_measured are the handle calls' forms.  Not on a set_gpus solver. */
int set_process_noise(double *G_data, int G_rows, int G_cols, int per_instance, unsigned long long seed);
int set_measurement_noise(double *G_data, int G_rows, int G_cols, int per_instance, unsigned long long seed);
int set_noise_cursor(int t);
int noise_cursor(void);
int noise_mode(void);
int get_noise(int which, int t0, int steps, double *buf);
int get_mpc_measured(double *y);
/* ... and through a state estimator stepped on the device (tinympc_set_estimator below, which describes it): C_data ny x nx and
 * L_data nx x ny column-major, or with per_instance = 1 ny x (nx batch) and nx x (ny batch), instance after instance; ny is
 * C_rows; the counts are checked.  Both NULL drop it.  set_estimator_state: xhat nx x 1 (shared) or nx x batch, NULL re-arms the
 * estimate at x0.  The others are the handle calls' forms.  Not on a set_gpus solver. */
int set_estimator(double *C_data, int C_rows, int C_cols, double *L_data, int L_rows, int L_cols, int per_instance);
int set_estimator_state(double *xhat_data, int xhat_rows, int xhat_cols);
int estimator_mode(void);
int estimator_outputs(void);
int get_estimator_state(double *xhat);
int get_mpc_estimate(double *xhat);
int get_mpc_outputs(double *y);
/* ... scored on the device (tinympc_set_rollout_metrics below, which describes the eleven slots): qw_data / rw_data with their
 * lengths (checked: nx / nu; NULL with length 0: the diagonal of Q / R), the four limit arrays of nx / nu doubles or NULL.
 * get_rollout_metrics fills [batch][11], get_rollout_summary [11][4].  Not on a set_gpus solver. */
int set_rollout_metrics(int enable, double *qw_data, int qw_len, double *rw_data, int rw_len, double *x_lo, double *x_hi,
                        double *u_lo, double *u_hi);
int reset_rollout_metrics(void);
int get_rollout_metrics(double *per_instance);
int get_rollout_summary(double *summary);
/* One problem family PER INSTANCE on the process-global solver (tinympc_create_families / _create_families_device,
 * tinympc_set_families, tinympc_get_family_cache, tinympc_families_setup_mode below, which describe them).  setup_families
 * replaces the global solver as setup_solver does: A_data nx x (nx batch), B_data nx x (nu batch), Q_data nx x (nx batch),
 * R_data nu x (nu batch) — the instances' column-major blocks side by side, the counts are checked — rho_data of batch
 * entries; on_device: the Riccati caches by a kernel instead of the host.  set_families: the handle call's arrays, NULL
 * keeps.  Not on a set_gpus solver. */
int setup_families(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols, double *Q_data, int Q_rows,
                   int Q_cols, double *R_data, int R_rows, int R_cols, double *rho_data, int rho_len, int nx, int nu, int N,
                   int batch, int on_device, int verbose);
int set_families(double *A_data, double *B_data, double *Q_data, double *R_data, double *rho_data);
int get_family_cache(int first, int count, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps);
int families_setup_mode(void);

/* ------------------------------------------------------------------------- */
/* (2) handle API                                                           */
/* ------------------------------------------------------------------------- */
typedef struct tinympc_solver tinympc_solver;

/* device < 0: current HIP device. */
int tinympc_create(tinympc_solver **out, const double *A, const double *B, const double *Q,
                   const double *R, double rho, int nx, int nu, int N, int batch, int device,
                   int verbose);
/* One problem family PER INSTANCE (no counterpart in the reference, whose solver holds one
 * family): A [batch][nx*nx], B [batch][nx*nu], Q [batch][nx*nx], R [batch][nu*nu] (each block column-major),
 * rho [batch].  Every instance gets its own host-side fp64 Riccati cache; bounds, settings and references
 * behave as in the single-family solver.  Needs (nx, nu) in the stream-kernel grid
 * (nx in {2,3,4,6,8,10,12}, nu <= 4); the batch size is fixed. */
int tinympc_create_families(tinympc_solver **out, const double *A, const double *B, const double *Q,
                            const double *R, const double *rho, int nx, int nu, int N, int batch,
                            int device, int verbose);
/* Families set up ON THE DEVICE.  tinympc_create_families_device takes what tinympc_create_families takes and
 * makes the same solver, but every instance's Riccati cache is computed by a kernel (the rule: csrc/riccati.h — the host
 * recursion of tinympc_host_precompute: at most 1000 sweeps, exit at max|K - K_prev| < 1e-5, LU with partial pivoting) and
 * the stream kernel's coefficient pack is written on the device from that cache; the host keeps A, B, the diagonals of Q and
 * R and rho, not the caches.  Fails, naming the first singular instance and their count, when R + B'PB is singular for one.
 *
 * tinympc_set_families replaces EVERY instance's family on an existing family solver of either setup mode: re-linearisation
 * along a trajectory, gain scheduling, a sweep over rho.  Arrays as tinympc_create_families takes them; A and B come
 * together, so do Q and R, and a NULL pair / a NULL rho keeps what the solver holds.  The caches are recomputed on the device
 * and the solver is in device mode from then on.  Kept: settings, bounds (shared and per instance), linear rows, cones, the
 * affine term, references and a reference trajectory, an installed plant, disturbance, noise, estimator and metrics, the
 * precision, and the warm-start workspace (tinympc_reset clears it as always); the model plant and the estimator's predict
 * follow the new A, B.  Waits for a launch in flight.  The new caches are computed into staging buffers and committed only if
 * no instance is singular: otherwise -1, tinympc_last_error names the first singular instance and how many there are, and
 * the solver is exactly as it was.  Refused on a solver that is not a family solver.
 *
 * tinympc_get_family_cache copies the caches of instances [first, first + count) in either mode: Kinf [count][nu*nx], Pinf
 * [count][nx*nx], Quu_inv [count][nu*nu], AmBKt [count][nx*nx], each block column-major, and sweeps [count], the Riccati sweeps
 * the instance ran (1000: it stopped at the cap); any output may be NULL.  tinympc_families_setup_mode: 0 not a family
 * solver, 1 set up on the host, 2 on the device.  tinympc_families_setup_ms: the kernel times in ms of the last device setup
 * (ms[0], riccati_families_kernel) and of the last pack fill (ms[1], fill_family_pack_kernel), -1 where none has run.
 * Not built: a sharded handle for families, adaptive rho and precision 2 on families, a per-instance affine term. */
int tinympc_create_families_device(tinympc_solver **out, const double *A, const double *B, const double *Q,
                                   const double *R, const double *rho, int nx, int nu, int N, int batch,
                                   int device, int verbose);
int tinympc_set_families(tinympc_solver *s, const double *A, const double *B, const double *Q, const double *R,
                         const double *rho);
int tinympc_get_family_cache(tinympc_solver *s, int first, int count, double *Kinf, double *Pinf, double *Quu_inv,
                             double *AmBKt, int *sweeps);
int tinympc_families_setup_mode(tinympc_solver *s);
int tinympc_families_setup_ms(tinympc_solver *s, double *ms);
void tinympc_destroy(tinympc_solver *s);
int tinympc_update_settings(tinympc_solver *s, double abs_pri_tol, double abs_dua_tol,
                            int max_iter, int check_termination, int en_state_bound,
                            int en_input_bound);
int tinympc_set_bound_constraints(tinympc_solver *s, const double *x_min, const double *x_max,
                                  const double *u_min, const double *u_max);
/* Box bounds PER INSTANCE (no counterpart in the reference, whose solver holds one constraint set: a fleet with different
 * actuator limits, a sweep over limits, corridor bounds that differ per instance).
 *   per_knot = 0: x_min / x_max nx x batch, u_min / u_max nu x batch, column-major; column b is instance b's bound at every knot;
 *   per_knot = 1: x_min / x_max [batch][N][nx] (nx x (N*batch), the layout of per-instance x_ref), u_min / u_max [batch][N-1][nu].
 * +-1e17 or beyond, +-inf included, mean "no bound".  Enables en_state_bound and en_input_bound on success, as
 * tinympc_set_bound_constraints does; tinympc_update_settings switches either side off and on again without a new upload.
 * The solver keeps host copies (a later tinympc_set_precision keeps the bounds); re-batching a solver (set_batch_size, set_gpus)
 * drops them and returns to the shared bounds, as it resets every per-instance input.  tinympc_set_bound_constraints
 * afterwards drops them too: back to the shared set and to the kernels that serve it.
 * Such a solver runs on the `ib` forms of the run-time-shape kernels, whatever on-chip kernel its shape has (their packs hold
 * one bound image): the stream kernel's for (nx, nu) in {(4,1), (6,3), (12,4)} at precision 0 — any horizon, one family or one
 * per instance, the affine term, cones, linear rows, chunked solves — and the generic kernel's for every other shape and for
 * precision 1 and 2; tinympc_kernel_name reports "stream4<NX,NU;ib>", "generic<ib>" or "generic<f64;ib>".  A per-instance-family
 * solver needs the stream form.  Refused, tinympc_last_error naming the condition: adaptive rho beside per-instance bounds (in
 * either order); tinympc_mpc_rollout, unless TINYMPC_HIP_STREAM_MPC=1 gives the solver the chain of launches (there is no
 * in-kernel loop with per-instance bounds).  Linear rows per instance: tinympc_set_instance_linear; cone coefficients per instance:
 * tinympc_set_instance_cones. */
int tinympc_set_instance_bounds(tinympc_solver *s, const double *x_min, const double *x_max, const double *u_min,
                                const double *u_max, int per_knot);
/* 0: shared bounds, 1: per instance and constant over the horizon, 2: per instance and per knot */
int tinympc_bounds_mode(tinympc_solver *s);
int tinympc_set_cache_terms(tinympc_solver *s, const double *Kinf, const double *Pinf,
                            const double *Quu_inv, const double *AmBKt);
/* Unpinned extensions (see setup_solver / set_cone_constraints above). */
int tinympc_set_fdyn(tinympc_solver *s, const double *fdyn /* nx, NULL = zero */);
int tinympc_set_cone_constraints(tinympc_solver *s, const int *Acu, const int *qcu, const double *cu,
                                 int n_input_cones, const int *Acx, const int *qcx, const double *cx,
                                 int n_state_cones);
int tinympc_enable_cones(tinympc_solver *s, int en_state_soc, int en_input_soc);
int tinympc_set_linear_constraints(tinympc_solver *s, const double *Alin_x, int rows_x, const double *blin_x,
                                   const double *Alin_u, int rows_u, const double *blin_u);
int tinympc_enable_linear(tinympc_solver *s, int en_state_linear, int en_input_linear);
/* Linear rows PER INSTANCE (no counterpart in the reference, whose solver holds one constraint set: every vehicle of a fleet
 * its own obstacle plane, a sweep over constraint placements, corridor walls that are not axis aligned).  The rule is the
 * shared set's, applied per instance: instance b's rows of a side are projected one after the other, in order, at every knot.
 *   Alin_x: [batch] blocks of rows_x x nx, column-major; blin_x: [batch][rows_x]; Alin_u / blin_u alike with nu.
 * The row counts are one pair for the whole batch, each at most 8; a side with 0 rows is empty (its pointers may be null).  An
 * all-zero row of an instance means "this instance has no row k" (stored as a = 0, b = FLT_MAX, |a|^2 = 1: never violated) —
 * that is how instances carry different numbers of rows.  A side that is enabled carries its slack and dual for every
 * instance, an instance whose rows on that side are all absent included — as a shared set whose rows never act does: such
 * an instance's iterates are those of a solver with rows that never bind, not bit for bit those of a solver without rows.
 * Rows are constant over the horizon.  Values are rounded to fp32 as the shared set's are, so per-instance rows that all equal
 * a shared set reproduce the shared-rows stream kernel bit for bit.  Non-empty sides are enabled on success, as
 * tinympc_set_linear_constraints does; tinympc_enable_linear / tinympc_update_settings switch a side off and on again
 * without a new upload.  The solver keeps host copies (a later tinympc_set_precision keeps the rows); re-batching a solver
 * (set_batch_size, set_gpus) drops them, as it resets every per-instance input; tinympc_set_linear_constraints afterwards
 * drops them too: back to the shared set and to the kernels that serve it.  Both sides empty: no rows at all, shared mode.
 * Such a solver runs on the `il` forms of the run-time-shape kernels, whatever on-chip kernel its shape has: the stream
 * kernel's for (nx, nu) in {(4,1), (6,3), (12,4)} at precision 0 — any horizon the LDS image holds, one family or one per
 * instance, the affine term, cones, chunked solves — and the generic kernel's for every other shape and for precision 1 and
 * 2; tinympc_kernel_name reports "stream4<NX,NU;il>", "generic<il>" or "generic<f64;il>".  The `il` forms read their box bounds
 * per instance, so per-instance bounds (tinympc_set_instance_bounds) combine with the rows at no extra cost and under the
 * same names; tinympc_bounds_mode keeps reporting what the caller set.  A per-instance-family solver needs the stream form.
 * Refused, tinympc_last_error naming the condition: more than 8 rows on a side; a null side with rows > 0; adaptive rho beside
 * per-instance rows (in either order); tinympc_mpc_rollout unless the solver has a plant of its own / a disturbance / a
 * reference trajectory (whose loop is a chain of launches) or TINYMPC_HIP_STREAM_MPC=1 gives it that chain — there is no
 * in-kernel loop with per-instance rows.  Cone coefficients per instance: tinympc_set_instance_cones.  Follow-ups, not built: rows per knot, the on-chip families, the
 * fp64-state and adaptive stream forms, loop forms, units specialised at setup, per-instance equality helpers. */
int tinympc_set_instance_linear(tinympc_solver *s, const double *Alin_x, int rows_x, const double *blin_x,
                                const double *Alin_u, int rows_u, const double *blin_u);
/* 0: no rows or rows shared by the batch, 1: per instance */
int tinympc_lin_mode(tinympc_solver *s);
/* Second-order cones with a coefficient PER INSTANCE (no counterpart in the reference, whose solver holds one constraint set:
 * a sweep over glide-slope angles or friction coefficients, a fleet whose vehicles have different thrust-vector limits, a
 * policy trained under a randomised cone).  The LAYOUT stays one for the batch — first row Acu[i] / Acx[i] and dimension
 * qcu[i] / qcx[i] of each cone, inputs first, at most 8 a side, the last row of a block the axis, as for
 * tinympc_set_cone_constraints — and the coefficient becomes per instance:
 *   cu: [batch][n_input_cones], cx: [batch][n_state_cones]
 * Instance b projects cone i with its own mu[b][i], by exactly the rule of the shared set.  mu = +inf means "instance b has no
 * cone i": its rows are then left as they are, as rows outside every cone are — that is how instances carry different cones.
 * A side that is enabled carries its slack and dual for every instance, an instance whose cones on that side are all absent
 * included — as a shared set whose cones never act does: such an instance's iterates are those of a solver with cones that
 * never bind, not bit for bit those of a solver without cones.  Values are rounded to fp32 as the shared set's are, so
 * coefficients that all equal a shared set reproduce the shared-cones stream kernel bit for bit.  Non-empty sides are enabled
 * on success, as tinympc_set_cone_constraints does; tinympc_enable_cones / tinympc_update_settings switch a side off and on
 * again without a new upload.  The solver keeps host copies (a later tinympc_set_precision keeps the coefficients);
 * re-batching a solver (set_batch_size, set_gpus) drops them, as it resets every per-instance input;
 * tinympc_set_cone_constraints afterwards drops them too: back to the shared set and to the kernels that serve it.  Both
 * sides empty: no cones at all, shared mode.
 * Such a solver runs on the `ic` forms of the run-time-shape kernels, whatever on-chip kernel its shape has (the matrix-core
 * kernels and the units specialised for a cone list hold one coefficient set): the stream kernel's for (nx, nu) in {(4,1),
 * (6,3), (12,4)} at precision 0 — any horizon the LDS image holds, one family or one per instance, the affine term,
 * references, chunked solves — and the generic kernel's for every other shape and for precision 1 and 2;
 * tinympc_kernel_name reports "stream4<NX,NU;ic>", "generic<ic>" or "generic<f64;ic>".  The `ic` forms are `il` forms: they read
 * box bounds and linear rows per instance, so per-instance bounds and rows (tinympc_set_instance_bounds,
 * tinympc_set_instance_linear) combine with the cones under the same names, and shared ones are uploaded replicated;
 * tinympc_bounds_mode and tinympc_lin_mode keep reporting what the caller set.  A per-instance-family solver needs the stream
 * form.  Refused, tinympc_last_error naming the condition: more than 8 cones on a side; a null side with cones > 0; a cone
 * outside the rows; mu <= 0 or non-finite other than +inf; adaptive rho beside per-instance cones (in either order);
 * precision 2 or adaptive rho on per-instance families, as without them; tinympc_mpc_rollout unless the solver has a plant
 * of its own / a disturbance / a reference trajectory (whose loop is a chain of launches) or TINYMPC_HIP_STREAM_MPC=1 gives
 * it that chain — there is no in-kernel loop with per-instance cones.  Follow-ups, not built: a per-instance cone layout
 * (Ac, qc), cones per knot, the on-chip families and units specialised at setup, the fp64-state and adaptive stream forms,
 * loop forms. */
int tinympc_set_instance_cones(tinympc_solver *s, const int *Acu, const int *qcu, const double *cu /* [batch][n_input_cones] */,
                               int n_input_cones, const int *Acx, const int *qcx, const double *cx /* [batch][n_state_cones] */,
                               int n_state_cones);
/* 0: no cones or cones shared by the batch, 1: a coefficient per instance */
int tinympc_cone_mode(tinympc_solver *s);
int tinympc_get_cache_terms(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv,
                            double *AmBKt);
/* Adaptive rho — admm.cpp:147-174 + rho_benchmark.cpp, per instance: every 5th ADMM iteration each instance predicts
 * a new rho from its normalised residuals (clipped to [rho_min, rho_max] if enable_clipping) and moves ITS Kinf, Pinf
 * by delta_rho * sensitivity.  The adapted (rho, Kinf, Pinf) are solver state and persist between solves, as the
 * reference's mutated cache does; tinympc_reset / set_cache_terms / toggling the switch return them to the family's
 * cache.  Settings: bindings.cpp:360-364.  Not available on per-instance-family solvers or in mpc_rollout. */
int tinympc_set_adaptive_rho(tinympc_solver *s, int enable, double rho_min, double rho_max, int enable_clipping);
/* dKinf/drho (nu x nx) and dPinf/drho (nx x nx), column-major — what codegen_with_sensitivity receives
 * (bindings.cpp:298-334) and tiny_setup hard-codes for the 12x4 quadrotor (tiny_api.cpp:269-329).  dC1 / dC2 may be
 * NULL: the reference applies them to copies the iteration never reads.  If never set, the first adaptive solve
 * computes them as TinyMPC.jl:301-352 does (tinympc_compute_sensitivity). */
int tinympc_set_sensitivity(tinympc_solver *s, const double *dKinf, const double *dPinf, const double *dC1,
                            const double *dC2);
/* Host-side finite differences (h = 1e-6) of the rho-regularised LQR — TinyMPC.jl:301-352
 * (compute_sensitivity_autograd / solve_lqr).  Any output may be NULL. */
int tinympc_compute_sensitivity(tinympc_solver *s, double *dKinf, double *dPinf, double *dC1, double *dC2);
/* Per-instance adapted values: rho [batch], Kinf [batch][nu*nx], Pinf [batch][nx*nx] (column-major each); any may be
 * NULL.  Before any adaptive solve: the family's values. */
int tinympc_get_adaptive_state(tinympc_solver *s, double *rho, double *Kinf, double *Pinf);
int tinympc_set_x0(tinympc_solver *s, const double *x0, int cols);       /* cols: 1 | batch */
int tinympc_set_x_ref(tinympc_solver *s, const double *x_ref, int cols); /* cols: N | N*batch */
int tinympc_set_u_ref(tinympc_solver *s, const double *u_ref, int cols); /* N-1 | (N-1)*batch */
int tinympc_reset(tinympc_solver *s);
/* warm_start: 0 = every solve starts from the zero workspace and keeps no state (benchmark
 * configs); 1 = the workspace (d, y, g, v, z) persists between solves like the reference's
 * (SURVEY.md 3.5).  Default 1. */
int tinympc_set_warm_start(tinympc_solver *s, int warm_start);
int tinympc_solve(tinympc_solver *s);
int tinympc_get_states(tinympc_solver *s, double *buf);
int tinympc_get_controls(tinympc_solver *s, double *buf);
int tinympc_get_status(tinympc_solver *s, int *iter, int *solved, double *residuals4);
/* Warm-start state of every instance, instance-major: d,y,z [batch][N-1][nu]; g,v [batch][N][nx]. */
int tinympc_get_workspace(tinympc_solver *s, double *d, double *y, double *g, double *v, double *z);
int tinympc_set_workspace(tinympc_solver *s, const double *d, const double *y, const double *g,
                          const double *v, const double *z);

/* --- device-resident I/O (fp32, instance-major), for callers that keep data in HBM --- */
/* Device pointers owned by the solver; valid until destroy / re-batch.
 *   x0 [batch][nx]; x_ref [batch][N][nx] (or [N][nx] when shared); u_ref likewise;
 *   states [batch][N][nx]; controls [batch][N-1][nu]; iter/solved [batch] int32;
 *   residuals [batch][4]; gstat: 8 x uint32 (max residual bits [0..3], unsolved count [4]). */
int tinympc_device_buffers(tinympc_solver *s, void **x0, void **x_ref, void **u_ref,
                           void **states, void **controls, void **iter, void **solved,
                           void **residuals, void **gstat);
/* Declare how the device-side reference buffers are to be read: 0 zero, 1 shared, 2 per instance. */
int tinympc_set_ref_mode(tinympc_solver *s, int ref_mode);
/* Enqueue one batched solve on `hip_stream` (NULL = default stream) without synchronising;
 * results are in the device buffers when the stream reaches this point. */
int tinympc_solve_async(tinympc_solver *s, void *hip_stream);
/* After the stream has been synchronised: 0 all converged / 1 otherwise (reads gstat). */
int tinympc_solve_status(tinympc_solver *s);
/* fp32 host buffers (plain copies to / from the fp32 device buffers, no conversion pass): x0 nx x 1 or nx x batch;
 * states nx*N*batch, controls nu*(N-1)*batch floats, instance-major as the fp64 forms.  The library never page-locks
 * memory it does not own: a caller that reuses its buffers and wants direct DMA into them registers them itself with
 * tinympc_pin_host and removes the registration with tinympc_unpin_host BEFORE freeing the memory (whatever is still
 * registered at tinympc_destroy is unregistered there). */
int tinympc_set_x0_f32(tinympc_solver *s, const float *x0, int cols);
int tinympc_get_states_f32(tinympc_solver *s, float *buf);
int tinympc_get_controls_f32(tinympc_solver *s, float *buf);
int tinympc_pin_host(tinympc_solver *s, void *ptr, size_t bytes);
int tinympc_unpin_host(tinympc_solver *s, void *ptr);
/* Fused closed loop (the caller pattern of examples/cartpole_example_mpc.jl:35-51):
 * `steps` repetitions of  solve -> u0 = controls[:,0] -> x0 = A x0 + B u0 -> set_x0  in ONE launch,
 * the warm-start workspace staying on chip between steps.  Needs warm-start mode and a specialised
 * kernel for the shape.  Synchronous; returns the solve status of the LAST step (0/1) or -1.
 * Afterwards x0 holds the plant state after the last step and get_states/get_controls/get_status
 * describe the last solve.  Logs, instance-major: x [batch][steps][nx] (plant state after each
 * step), u [batch][steps][nu] (control applied), iter [batch][steps] (ADMM iterations of the step,
 * negated when the step hit max_iter).  Any log pointer may be NULL.
 * Environment switches, read when the solver is created (both off by default): TINYMPC_HIP_LEAN_WS=1 runs the loop of a
 * cartpole-class shape with at least 20 480 instances on the headline (lean) kernel, as a stream-ordered chain of `steps`
 * workspace-carrying launches and plant updates; TINYMPC_HIP_LEAN_LOOP=1 beside it (no effect alone) as ONE launch of that
 * kernel's in-kernel loop, every instance's workspace kept on chip between the steps — except with a reference sequence
 * (below), which keeps the chain.  Results, logs and workspace are those of the chain.
 * Shapes and option sets that run on the stream or the generic kernel — a horizon without a built-in entry, linear rows,
 * cone / affine-term layouts outside the transposed-sets kernel, per-instance families, any (nx, nu) outside the stream
 * grid, every solver at precision 2 — have no closed loop by default: the call fails, naming the condition.
 * TINYMPC_HIP_STREAM_MPC=1 (off by default, read when the solver is created) gives them one as the same kind of chain —
 * `steps` workspace-carrying launches, the plant x0 = f + A x0 + B u0 (per-instance A, B on a family solver) in fp64
 * between them, each solve started from the fp32 rounding of the plant state — at precision 0, 1 and 2, with a reference
 * sequence too; TINYMPC_HIP_STREAM_LOOP=1 beside it (no effect alone) runs ONE launch of the stream kernel's in-kernel loop
 * where one is built ((4,1), (6,3) at precision 0 and 2, (12,4) at precision 2; bit-identical to the chain) and the chain
 * elsewhere.  Still refused there: adaptive rho, families at precision 2, a solver without the persistent workspace.
 * Two such loops in a row continue the fp64 plant state of the first unless x0 was set in between. */
int tinympc_mpc_rollout(tinympc_solver *s, int steps, void *hip_stream);
int tinympc_get_mpc_log(tinympc_solver *s, double *x, double *u, int *iter);
/* Shared references of EVERY step of the next closed loops — the caller pattern of
 * examples/rocket_landing_constraints.jl:97-134, which shifts x_ref by one knot per step (:107-115) before each solve:
 * x_ref_seq is nx x (N*steps), u_ref_seq nu x ((N-1)*steps), column-major, step after step (what `steps` calls of
 * set_x_ref / set_u_ref would have passed).  The plant step of such a loop includes the affine term,
 * x0 = A x0 + B u0 + f (:123).  Step 0's references become the solver's own shared references and stay installed when
 * the sequence is dropped (by a later shared set_x_ref / set_u_ref, which replaces them, or by steps = 0, which does not).
 * Supported wherever mpc_rollout is: inside the launch on the transposed-sets kernel (mfmat) and on the lanes-per-instance
 * kernels at horizons up to 20 (quad: the step's references are re-staged in LDS before the step's first iteration), and
 * launch by launch on the chained loops (mfma, and the lean kernel's behind TINYMPC_HIP_LEAN_WS), whose launches read their
 * step's slice of the sequence in place.  tinympc_mpc_rollout fails, naming the condition, with fewer sequence steps than
 * loop steps, with per-instance references (set after the sequence, or through tinympc_set_ref_mode(2)), with adaptive rho,
 * at precision 2, on a quad entry with a horizon above 20, and on shapes that have no closed loop at all (stream / generic
 * kernels) — the last two unless TINYMPC_HIP_STREAM_MPC=1 gives those solvers their chained loop (above), whose launches
 * read their step's slice like the other chains'; a sharded solver takes no sequence. */
int tinympc_set_ref_sequence(tinympc_solver *s, const double *x_ref_seq, int x_rows, int x_cols, const double *u_ref_seq,
                             int u_rows, int u_cols, int steps);
/* The plant mpc_rollout steps, when it is not the model: x+ = f_p + A_p x + B_p u0 (+ w).  per_instance = 0: A nx x nx, B nx x nu
 * (column-major), f nx (NULL = zero).  per_instance = 1: A [batch][nx*nx], B [batch][nx*nu], f [batch][nx] (NULL = zero), the
 * layout of tinympc_create_families.  A = B = NULL drops it: back to the model and to the routes that serve it.
 * For Monte-Carlo over disturbances, a fleet whose true parameters differ from the controller's model, robustness sweeps: the
 * controller (model, caches, kernels) is untouched.  The plant is fp64 on the host and on the device; tinympc_set_precision keeps
 * it, re-batching (set_batch_size) drops it as it drops every per-instance input.  A solver with a plant or a disturbance
 * installed takes tinympc_mpc_rollout as a chain — per step its ordinary kept-workspace launch from the fp32 rounding of the
 * state, then the plant step — on whatever kernel such a solve runs on: every kernel family, every precision, no environment
 * switch, shapes without a fused closed loop included; a reference sequence is read launch by launch (precision 2 too); two
 * loops in a row continue the fp64 state unless x0 was set in between.  The step, row r, with u0 the fp32 control of knot 0
 * widened to fp64: acc = f_p[r]; A_p's row by ascending column, then B_p's, one fma each; with a disturbance one fp64 add
 * acc + w[r] last; the fp64 state is acc, x0 and the log its fp32 rounding.  Refused by tinympc_mpc_rollout, the error naming
 * the condition: a disturbance with fewer rows than steps, adaptive rho, no persistent workspace (set_warm_start(0)),
 * per-instance bounds without TINYMPC_HIP_STREAM_MPC, and the reference sequence's own conditions on length and per-instance
 * references. */
int tinympc_set_plant(tinympc_solver *s, const double *A, const double *B, const double *f, int per_instance);
/* Additive disturbance of every step of the next closed loops: per_instance = 0: w nx x steps, shared; 1: w [batch][steps][nx]
 * (the layout of the x log).  Every mpc_rollout reads it from row 0 (as a reference sequence is read).  w = NULL or steps = 0 drops it.
 * Without tinympc_set_plant it disturbs the model plant (A, B and the affine term; on a per-instance-family solver every
 * instance's own A_b, B_b). */
int tinympc_set_disturbance(tinympc_solver *s, const double *w, int steps, int per_instance);
/* 0 model, 1 shared plant, 2 per-instance plant;  | 4 shared disturbance, | 8 per-instance disturbance */
int tinympc_plant_mode(tinympc_solver *s);
/* A reference trajectory, windowed on the device: every instance tracks a moving target of its own through a closed loop.
 * x_traj is Lx rows of nx, u_traj (NULL = zero input references) Lu rows of nu, row after row (an nx x Lx / nu x Lu
 * column-major matrix).  per_instance = 0: one trajectory shared by the batch; 1: x_traj [batch][Lx][nx], u_traj
 * [batch][Lu][nu], the layout of tinympc_get_mpc_log's x / u, so one run's log can be another run's trajectory.  The rule: with
 * the cursor c, the references of a solve are the window  x_ref[k] = x_traj[min(c + k, Lx - 1)], k = 0 .. N-1,
 * u_ref[k] = u_traj[min(c + k, Lu - 1)], k = 0 .. N-2  — the last row is held beyond the end, so any Lx, Lu >= 1 serve any
 * number of steps.  Values are rounded to fp32 once, here, as set_x_ref rounds; a window is a copy of those floats.
 * A newly installed trajectory starts at cursor 0.  tinympc_solve uses the window at c and leaves c; tinympc_mpc_rollout(steps)
 * uses the windows at c .. c + steps - 1 and leaves c + steps, so two loops in a row continue the trajectory as they continue
 * the fp64 plant state; tinympc_set_ref_cursor moves it (a negative cursor is refused), tinympc_ref_cursor reads it.
 * Routes: while a trajectory is installed the reference arrays are device-owned in its mode (shared or per instance, as after
 * tinympc_set_ref_mode) and one small kernel cuts the window out of the device-resident trajectory whenever the window there
 * is not the one the next launch needs — before a plain solve, and per step in the loop: nothing is uploaded per step.  Such a
 * solver takes tinympc_mpc_rollout as the chain of tinympc_set_plant (above) — per step its ordinary kept-workspace launch,
 * then the plant step — against the model (A, B, the affine term; a family solver's own A_b, B_b), or against the installed
 * plant and disturbance: every kernel family, every precision, no environment switch; TINYMPC_HIP_LEAN_WS / _LEAN_LOOP /
 * _STREAM_MPC / _STREAM_LOOP leave it on that chain (`steps` launches, tmpc_last_rollout_launches).
 * x_traj = NULL drops the trajectory: the window at the cursor stays installed as the solver's ordinary references, shared or
 * per instance, and the solver returns to the routes that serve those.  tinympc_set_x_ref / _set_u_ref do the same and then
 * replace their side; tinympc_set_ref_sequence with steps > 0 and tinympc_set_ref_mode replace the trajectory outright;
 * tinympc_set_ref_trajectory drops a sequence: the later call wins.  tinympc_set_precision keeps the trajectory, re-batching
 * (set_batch_size) drops it as it drops every per-instance input.
 * Refused here: Lx < 1, Lu < 1 with a u_traj, per_instance other than 0 / 1 (one flag: x_traj and u_traj are both shared or
 * both per instance; the global form below also checks row counts and that per-instance widths are L * batch).  Refused by
 * tinympc_mpc_rollout, the error naming the condition: adaptive rho, no persistent workspace (set_warm_start(0)), per-instance
 * bounds without TINYMPC_HIP_STREAM_MPC, a disturbance with fewer rows than steps (it is read from row 0 whatever the cursor).
 * A sharded solver (set_gpus / tinympc_sharded_*) has no mpc_rollout and takes no trajectory. */
int tinympc_set_ref_trajectory(tinympc_solver *s, const double *x_traj, int Lx, const double *u_traj, int Lu, int per_instance);
int tinympc_set_ref_cursor(tinympc_solver *s, int cursor);
int tinympc_ref_cursor(tinympc_solver *s);
/* 0 none, 1 shared, 2 per instance */
int tinympc_ref_trajectory_mode(tinympc_solver *s);
/* Seeded process and measurement noise, drawn on the device: Monte-Carlo sweeps of a closed loop with nothing drawn on the host,
 * uploaded or stored.  A draw is a pure function of (seed, kind, instance b, step t):
 *   standard normals xi[which][b][t][i], which 0 process / 1 measurement, i < nx: Philox4x32-10 (multipliers 0xD2511F53 and
 *   0xCD9E8D57, Weyl increments 0x9E3779B9 and 0xBB67AE85), key (seed low 32, seed high 32), counter (b low 32, b high 32, t,
 *   (which << 16) | j) with j = i / 2; from its words w0..w3  u1 = (((w1:w0) >> 11) + 1) 2^-53 in (0, 1],
 *   u2 = ((w3:w2) >> 11) 2^-53 in [0, 1), r = sqrt(-2 ln u1), xi[2j] = r cos(2 pi u2), xi[2j+1] = r sin(2 pi u2), all fp64 (an odd
 *   nx drops the last sine);
 *   the noise vector n = G xi, G nx x nx column-major fp64 — any matrix, the covariance is G G' — row r: acc = 0, then
 *   acc = fma(G[r + i nx], xi[i], acc) for i ascending.
 * G is shared (per_instance = 0) or [batch][nx*nx] (1); G = NULL drops that kind.  The loop: a solver with either noise is an
 * own-plant solver (tinympc_set_plant above): tinympc_mpc_rollout is the chain of `steps` kept-workspace launches on every
 * kernel family and precision, no environment switch, against the model or the installed plant.  With the noise cursor c and loop
 * step s, t = c + s:
 *   measurement noise: the solve of step s starts from (float)(x_t + G_v xi_v[b][t]), x_t the fp64 plant state, which the
 *     measurement never contaminates;
 *   process noise: the plant step is x+ = f_p + A_p x + B_p u0, then the uploaded disturbance if any, then one fp64 add of the
 *     draw, last: acc = (acc + w[r]) + (G_w xi_w[b][t])[r];
 *   the x log, the fp64 state and x0 hold the true state and its fp32 rounding: between loops x0 is the rounding of the true
 *     state, so two loops in a row continue the state as before;
 *   after the loop the cursor is c + steps: two loops in a row continue the noise streams.  One cursor serves both kinds; a newly
 *     installed noise leaves it alone; a new solver has cursor 0; tinympc_set_noise_cursor moves it (t < 0 is refused).
 *   What each step's solve started from is logged, [batch][steps][nx], while measurement noise is installed:
 *     tinympc_get_mpc_measured (after a loop with it).
 * tinympc_noise_mode: 1 shared / 2 per-instance process factor;  | 4 shared / | 8 per-instance measurement factor.
 * tinympc_plant_mode is unchanged by noise.  tinympc_set_precision keeps the noise, re-batching (set_batch_size) drops it as it
 * drops every per-instance input.  A solver without noise launches exactly what it launched before.
 * tinympc_get_noise: the realised G xi of the steps t0 .. t0 + steps - 1 of an installed kind, [batch][steps][nx] fp64, computed
 * on the device by the loop's own device function — as a disturbance (tinympc_set_disturbance) it reproduces the process noise
 * bit for bit.  tinympc_host_noise: the same rule on the host, no device needed (G NULL = identity, out nx doubles);
 * tmpc_philox4x32_10: the block function alone, on the host, for known-answer tests.
 * Refused here: per_instance other than 0 / 1, a negative cursor.  Refused by tinympc_mpc_rollout, the error naming the
 * condition: adaptive rho, no persistent workspace (set_warm_start(0)), per-instance bounds without TINYMPC_HIP_STREAM_MPC, a
 * cursor that would pass INT_MAX.  The uploaded disturbance is still read from row 0 whatever the cursor.
 * A sharded solver (set_gpus / tinympc_sharded_*) has no mpc_rollout and takes none of it. */
int tinympc_set_process_noise(tinympc_solver *s, const double *G, int per_instance, unsigned long long seed);
int tinympc_set_measurement_noise(tinympc_solver *s, const double *G, int per_instance, unsigned long long seed);
int tinympc_set_noise_cursor(tinympc_solver *s, int t);
int tinympc_noise_cursor(tinympc_solver *s);
int tinympc_noise_mode(tinympc_solver *s);
int tinympc_get_noise(tinympc_solver *s, int which, int t0, int steps, double *buf);
int tinympc_get_mpc_measured(tinympc_solver *s, double *y);
int tinympc_host_noise(unsigned long long seed, int which, long long b, int t, int nx, const double *G, double *out);
int tmpc_philox4x32_10(const unsigned *ctr4, const unsigned *key2, unsigned *out4);
/* Output feedback: measured outputs y = C x + v, ny <= nx of them, and a fixed-gain state estimator (Luenberger / steady-state
 * Kalman, current-estimator form) stepped in fp64 on the device, so that a closed loop under sensor noise that does not see its
 * whole state still never leaves the device.
 * THE RULE (csrc/estimator.h, the text the device kernel and tinympc_host_estimator_step compile), everything fp64, C ny x nx and
 * L nx x ny column-major; per instance b and loop step s, t = noise cursor + s:
 *   output   y_t[i] = (sum_j C[i + j ny] x_t[j]) + v_t[i]: acc = 0, one fma per j ascending, then one add; x_t is the true plant
 *            state, v_t[i] row i < ny of the measurement noise G_v xi_v[b][t] (tinympc_get_noise(1, ..)[.., :ny]); without
 *            measurement noise v = 0 and there is no add;
 *   correct  e[i] = y_t[i] - (C xhat-_t)[i] (the same fma order); xhat_t[r] = xhat-_t[r], then fma(L[r + i nx], e[i], .), i ascending;
 *   solve    from x0 = (float)xhat_t; u_t is its first control; the plant step is unchanged (and steps the true state);
 *   predict  xhat-_{t+1}[r] = f[r], then fma(A[r + j nx], xhat_t[j], .), j ascending, then fma(B[r + a nx], u_t[a], .): the MODEL's A,
 *            B and set_fdyn term (a per-instance-family solver: each instance's own A_b, B_b), never an installed plant.
 * C and L are shared (per_instance = 0) or [batch] of each (1); C = L = NULL drops the estimator.  A solver with one is an
 * own-plant solver: tinympc_mpc_rollout is the chain of `steps` launches on whatever kernel a kept-workspace solve takes, every
 * kernel family and precision, no environment switch.  Between rollouts the solver holds xhat- of the next step in fp64, so
 * mpc_rollout(a) then mpc_rollout(b) is mpc_rollout(a + b) bit for bit; a rollout leaves x0 = (float)(true state).  xhat-_0 is the
 * caller's x0 (as the device holds it, fp32) at the first rollout after the estimator is installed, replaced or re-armed
 * (tinympc_set_estimator_state with NULL), else what tinympc_set_estimator_state installed (xhat nx, shared, or [batch][nx]).
 * tinympc_set_x0 moves the plant, not the estimate.
 * Logs of the last rollout: tinympc_get_mpc_estimate [batch][steps][nx], what each solve started from; tinympc_get_mpc_outputs
 * [batch][steps][ny], (float)y_t; tinympc_get_mpc_measured is refused while an estimator is installed.  tinympc_get_mpc_log and the
 * rollout metrics keep the true state.  tinympc_get_estimator_state: the current xhat- [batch][nx] fp64.
 * tinympc_estimator_mode: 0 none / 1 shared / 2 per instance; tinympc_estimator_outputs: ny (0: none).
 * tinympc_set_precision keeps the estimator, re-batching drops it.  A solver without one launches exactly what it launched before.
 * Refused here: ny < 1, ny > nx, only one of C and L, per_instance other than 0 / 1; by tinympc_mpc_rollout: adaptive rho, no
 * persistent workspace.  TINYMPC_HIP_ESTIMATOR_SPLIT=1 launches predict and correct separately (same bits; a timing aid).
 * tinympc_host_estimator_step: one predict and / or correct of the rule for one instance on the host, no device needed: xhat nx in
 * and out; the predict reads A, B, f (NULL: zero) and u (nu); the correct reads C, L, the true state x, v (ny, NULL: none) and
 * writes y (ny).  Both: predict first, as the fused kernel.
 * tinympc_host_kalman_gain: the steady-state gain, host only: the filter Riccati recursion
 * P <- A (P - P C' (C P C' + V)^-1 C P) A' + W from P = W until the update is <= 1e-13 |P|_inf (the ny x ny solve by Cholesky), then
 * L = P C' (C P C' + V)^-1 (nx x ny) and, where P is not NULL, the prediction covariance.  -1 with a message after 100 000
 * iterations, on a non-positive pivot or a covariance beyond 1e300 (an undetectable pair).  The setter always takes L. */
int tinympc_set_estimator(tinympc_solver *s, const double *C, int ny, const double *L, int per_instance);
int tinympc_set_estimator_state(tinympc_solver *s, const double *xhat, int per_instance);
int tinympc_estimator_mode(tinympc_solver *s);
int tinympc_estimator_outputs(tinympc_solver *s);
int tinympc_get_estimator_state(tinympc_solver *s, double *xhat);
int tinympc_get_mpc_estimate(tinympc_solver *s, double *xhat);
int tinympc_get_mpc_outputs(tinympc_solver *s, double *y);
int tinympc_host_estimator_step(int nx, int nu, int ny, int predict, int correct, const double *A, const double *B, const double *f,
                                const double *C, const double *L, const double *u, const double *x, const double *v, double *xhat, double *y);
int tinympc_host_kalman_gain(const double *A, const double *C, const double *W, const double *V, int nx, int ny, double *L, double *P);
/* Per-instance metrics of the closed loop, folded on the device: what a Monte-Carlo sweep wants of its rollouts without the log
 * leaving the device.  While enabled, every tinympc_mpc_rollout — whatever its route — is followed on its stream by one kernel
 * that reads the log the rollout wrote and updates [batch][TMPC_METRIC_COUNT] fp64 accumulators, so the metrics accumulate over
 * every step folded since the last reset: a long run is a sequence of short rollouts on a fixed-size log.
 * THE RULE (csrc/metrics.h, the text the device kernel and tinympc_host_rollout_metrics compile), everything fp64:
 *   for instance b and loop step s of a rollout, x_s = the logged state after the step (an fp32 widened to fp64), u_s the logged
 *   control, it_s the logged signed iteration count (negative: the solve hit max_iter).  The target of the step is taken from the
 *   references that step's solve used, xr_s = knot 1 of its x_ref and ur_s = knot 0 of its u_ref, fp32 device values widened:
 *     a reference trajectory at cursor c (the one the rollout started from): xr_s = row min(c + s + 1, Lx - 1), ur_s = row
 *       min(c + s, Lu - 1), zero without a u_traj;  a reference sequence: step s's slice;  constant references, shared or per
 *       instance: the installed arrays;  no references: zero.
 *   e = x_s - xr_s, v = u_s - ur_s, and the slots are
 *     0 steps          number of steps folded
 *     1 cost_x         sum_s sum_r qw[r] e[r]^2
 *     2 cost_u         sum_s sum_a rw[a] v[a]^2
 *     3 peak_err       max_s max_r |e[r]|
 *     4 final_err      max_r |e[r]| of the last step folded
 *     5 x_viol_max     max_s max_r max(x_s[r] - x_hi[r], x_lo[r] - x_s[r], 0)
 *     6 x_viol_steps   number of steps with any row strictly outside [x_lo, x_hi]
 *     7 first_viol     1 + (index, counted since the reset, of the first such step); 0 if never
 *     8 u_sat_steps    number of steps with any u_s[a] >= u_hi[a] or <= u_lo[a]
 *     9 iters          sum_s |it_s|
 *    10 maxiter_steps  number of steps with it_s < 0
 *   Counts are doubles holding integers.  Within a rollout the sums are taken in a fixed order that is not the host's step after
 *   step; they agree with it to rounding, every other slot exactly.
 * qw (nx) and rw (nu): non-negative weights shared by the batch; NULL: the diagonal of the solver's Q / R — refused on a
 * per-instance-family solver, which has no one Q and R: give the weights.  x_lo, x_hi (nx), u_lo, u_hi (nu): shared limits, the
 * metric's OWN safe set and deliberately not the solver's bounds (a soft corridor can be scored against a hard one); NULL: none,
 * that side never counts.  Refused: a negative weight, lo > hi in any row.
 * tinympc_set_rollout_metrics: enable = 1 installs or replaces the configuration and zeroes the accumulators; enable = 0 drops
 * the configuration and frees the buffers (the getters and the reset are then refused).  tinympc_reset_rollout_metrics: the
 * accumulators to zero, the configuration kept.  tinympc_rollout_metrics_mode: 0 off, 1 on.
 * tinympc_get_rollout_metrics: the accumulators, [batch][TMPC_METRIC_COUNT].  tinympc_get_rollout_summary: over the instances,
 * [TMPC_METRIC_COUNT][4] = per slot the sum, the minimum, the maximum and the number of instances whose value is > 0, folded on
 * the device in a fixed order without atomics — the same bits from run to run.  Both wait for the last launch; before any
 * rollout they return zeros.
 * The fold is inside what tinympc_mpc_rollout(…, stream) orders and the getters wait for.  A solver without metrics launches
 * exactly what it launched before.  tinympc_set_precision keeps configuration and accumulators, re-batching (set_batch_size)
 * drops both as it drops every per-instance state.  A sharded solver has no mpc_rollout and takes none of it.
 * tinympc_host_rollout_metrics: the same rule on the host, no device needed — one instance's log of `steps` steps (x_log
 * [steps][nx], u_log [steps][nu], iter_log [steps]; xr [steps][nx] / ur [steps][nu] the targets step by step, NULL: zero) folded
 * step after step into acc11, which is read and written: zeros to start, or what an earlier call left, to continue.  qw and rw
 * are required here; the limits may be NULL. */
#define TMPC_METRIC_COUNT 11
int tinympc_set_rollout_metrics(tinympc_solver *s, int enable, const double *qw, const double *rw, const double *x_lo,
                                const double *x_hi, const double *u_lo, const double *u_hi);
int tinympc_reset_rollout_metrics(tinympc_solver *s);
int tinympc_rollout_metrics_mode(tinympc_solver *s);
int tinympc_get_rollout_metrics(tinympc_solver *s, double *per_instance /* [batch][11] */);
int tinympc_get_rollout_summary(tinympc_solver *s, double *summary /* [11][4] */);
int tinympc_host_rollout_metrics(int nx, int nu, int steps, const float *x_log, const float *u_log, const int *iter_log,
                                 const float *xr, const float *ur, const double *qw, const double *rw, const double *x_lo,
                                 const double *x_hi, const double *u_lo, const double *u_hi, double *acc11);
/* Tolerance-terminated solves of big batches: with chunk_iters > 0 (rounded up to a multiple of check_termination)
 * a solve runs in chunks of that many iterations and, between chunks, gathers the instances still iterating into
 * a dense list, so that wavefronts do not idle behind their slowest instance.  Iterates, iteration counts and
 * residuals are those of the single-launch solve.  The solve then synchronises its stream.  Ignored for
 * fixed-iteration settings (a tolerance <= 0), per-instance families, closed-loop rollouts.  0 = off (default). */
int tinympc_set_compaction(tinympc_solver *s, int chunk_iters);
/* Kernel timing: when enabled, every solve records HIP events immediately around the ADMM kernel
 * launch on the launch stream; tinympc_kernel_elapsed_ms returns the last kernel's duration,
 * tinympc_kernel_elapsed_mean_ms the mean over the last `last_n` launches (at most 256)
 * (call after the stream has been synchronised; < 0 if unavailable). */
int tinympc_set_profiling(tinympc_solver *s, int enable);
double tinympc_kernel_elapsed_ms(tinympc_solver *s);
double tinympc_kernel_elapsed_mean_ms(tinympc_solver *s, int last_n);
/* Arithmetic of the two serial recurrences (rollout, Riccati gradient): 0 = fp64 accumulation
 * with fp64 coefficients (default; ADMM state and elementwise steps stay fp32), 1 = all fp32,
 * 2 = all fp64 — the reference's own arithmetic end to end (types.hpp:15): recurrences, slacks, duals, residual
 * comparisons and the workspace kept between solves in fp64, on the generic kernel (any shape and option set of the
 * single-family solvers; no closed loop unless TINYMPC_HIP_STREAM_MPC=1, see tinympc_mpc_rollout); x0 / references / bounds go in and the solution comes out as the fp32
 * device arrays.  It is the mode for callers who need the reference's digits rather than the 1e-5 of the fp32-state
 * kernels (families whose duals lose digits to fp32 rounding miss 1e-5 there); it is the slowest path of the library —
 * except cold one-shot solves of cartpole-class shapes ((4,1) to N = 30, (3,2), (2,x)), which are launched on the headline
 * kernel's fp64-state variant, compiled on request (csrc/jit.cpp; tinympc_last_launch_name: "lean<...;f64>"): the same
 * digits at that kernel's speed.  With TINYMPC_HIP_STREAM_F64=1 in the environment when the solver is created (off by
 * default), every other precision-2 solve of a shape that has the stream kernel's fp64-state form — (4,1), (6,3), (12,4);
 * any horizon, the affine term, cones, linear rows, cold or kept workspace; not adaptive rho, not chunked solves — runs
 * on that form ("stream4<NX,NU;f64>"): the same digits and iteration counts, 9 to 24 times faster than the generic kernel
 * on the benchmark shapes (profiles/r09_stream_f64_time.txt).
 * Switching to or from precision 2 restarts the workspace cold.
 * precision = 1 is a request to save time and does NOT meet the 1e-5 parity target on every instance (3 of the 65 536
 * benchmark cartpole instances miss it, worst 1.6e-5).  Where a shape has a matrix-core kernel that kernel is faster than the
 * fp32 one, so such solves run there — with fp64 recurrences — unless tinympc_set_strict_precision(s, 1) insists on fp32.
 * tinympc_effective_precision returns the recurrence precision (0 / 1) the solver's current options run with. */
int tinympc_set_precision(tinympc_solver *s, int precision);
int tinympc_set_strict_precision(tinympc_solver *s, int strict);
/* Tuning / test aid.  The TINYMPC_HIP_* environment switches are read ONCE, when a solver is created —
 * nothing on the solve path calls getenv; this re-reads them for a live solver. */
int tinympc_reload_switches(tinympc_solver *s);
int tinympc_effective_precision(tinympc_solver *s);
/* Name of the kernel family the solver's shape / options select: "quad<nx,nu,N,gG>", "mfma<...>", "mfmat<...>",
 * "stream4<nx,nu>", "generic", ...; with per-instance bounds "stream4<nx,nu;ib>", "generic<ib>", "generic<f64;ib>"; with
 * per-instance linear rows (beside per-instance bounds or not) "stream4<nx,nu;il>", "generic<il>", "generic<f64;il>"; with
 * per-instance cone coefficients (beside either or not) "stream4<nx,nu;ic>", "generic<ic>", "generic<f64;ic>" */
const char *tinympc_kernel_name(tinympc_solver *s);
/* Name of the kernel the most recent launch actually ran: the family above, or the variant a launch of that family took
 * for its calling pattern — "lean<nx,nu,N>" for one-shot solves (cold start, workspace not kept) of a one-lane-per-instance
 * quad entry without an active state bound, zero references, fp64 recurrences (admm_lean.hip.h). */
const char *tinympc_last_launch_name(tinympc_solver *s);
/* Algorithmic HBM bytes and FLOPs of one solve of the whole batch (SURVEY.md 8d formulas);
 * flops assume `iters` ADMM iterations per instance.  Per-instance bounds count too: given per knot, 2 (nx N + nu (N-1)) floats
 * per instance and iteration (max_iter of them); constant over the horizon, 2 (nx + nu) floats per instance, once.  Per-instance
 * linear rows: rows_x (nx + 2) + rows_u (nu + 2) floats per instance, once.  Per-instance cone coefficients: one float per cone
 * and instance, once. */
double tinympc_algorithmic_bytes(tinympc_solver *s);
double tinympc_algorithmic_flops(tinympc_solver *s, int iters);
const char *tinympc_last_error(void);
/* Specialisation at setup.  The reference takes any (nx, nu, N) at run time (tiny_api.cpp:21-71); the on-chip kernels here are
 * compiled per shape.  For a shape the library was not built with, tinympc_create / setup_solver compile the one instantiation
 * that suits it (hipcc as a child process, from the library's own csrc/ headers), cache it under $TINYMPC_HIP_CACHE or
 * ~/.cache/tinympc_hip/<source hash>/ and load it; the time of the one-off compile is printed on stderr.  Without a
 * compiler or the sources, when the shape's state does not fit the chip, or with TINYMPC_HIP_NO_JIT=1, such a solver runs
 * on the run-time-shape kernels (stream / generic) as before.  This entry point does the same ahead of time (no GPU needed):
 * returns 1 if an on-chip kernel exists for the shape afterwards, 0 if not. */
int tinympc_specialise(int nx, int nu, int N, int verbose);
/* Host-only fp64 part of setup() — the infinite-horizon Riccati precompute of
 * tiny_precompute_and_set_cache (tiny_api.cpp:124-190, incl. the rho-twice quirk of
 * tiny_setup :90-91,113).  Needs no GPU.  Outputs column-major: Kinf nu x nx, Pinf nx x nx,
 * Quu_inv nu x nu, AmBKt nx x nx.  Returns 0, or -1 if R + B'PB is singular. */
int tinympc_host_precompute(const double *A, const double *B, const double *Q, const double *R,
                            double rho, int nx, int nu, double *Kinf, double *Pinf,
                            double *Quu_inv, double *AmBKt);
/* Host-only (no GPU): the Riccati sweeps tinympc_host_precompute runs for that family (1000: it stopped at the cap), -1 if
 * R + B'PB is singular. */
int tinympc_host_precompute_sweeps(const double *A, const double *B, const double *Q, const double *R, double rho, int nx,
                                   int nu);
/* Host-only (no GPU): the same precompute by the rule the device setup of per-instance families runs (csrc/riccati.h), for the
 * shapes that setup is built for (nx in {2,3,4,6,8,10,12}, nu <= 4).  Q, R full matrices (their diagonals are what enters);
 * *sweeps (may be NULL): the sweeps run, 1000 at the cap.  Returns 0, or -1: R + B'PB singular (*sweeps = -1) or the shape is
 * outside the grid.  On finite values it agrees with tinympc_host_precompute to the last bit. */
int tinympc_host_family_cache(const double *A, const double *B, const double *Q, const double *R, double rho, int nx, int nu,
                              double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps);
/* Host-only (no GPU): the sensitivities tinympc_compute_sensitivity returns, for a family given directly. */
int tinympc_host_sensitivity(const double *A, const double *B, const double *Q, const double *R, double rho, int nx,
                             int nu, double *dKinf, double *dPinf, double *dC1, double *dC2);

/* ------------------------------------------------------------------------- */
/* (3) multi-GPU: one handle, n_gpus devices of one node, one host process   */
/* ------------------------------------------------------------------------- */
/* SURVEY.md 8(b) "what the replacement exports": setup_solver(..., batch, n_gpus); 8(e).  The reference has one
 * process-global CPU solver (bindings.cpp:15-18) and nothing to distribute; this is the surface a `ccall` host uses to
 * drive all GPUs of a node without a process launcher.  The batch is cut into contiguous shards (shard i = instances
 * [lo_i, hi_i), sizes differing by at most one), shard i on devices[i] with its own stream; inputs are scattered and
 * outputs gathered by offset on the caller's instance-major buffers; no data moves between GPUs.  The one exchange is
 * the solve status: each solve ends with ONE all-reduce(MAX) over RCCL (ncclCommInitAll at creation, a grouped
 * ncclAllReduce of 8 uint32 per solve) of the devices' status blocks, enqueued on the shards' streams behind the
 * kernels.  librccl.so is loaded at run time by the first call of tinympc_create_sharded. */
typedef struct tinympc_sharded tinympc_sharded;
/* devices: n_gpus device ordinals, NULL = 0 .. n_gpus-1.  Needs 1 <= n_gpus <= batch.  A list that repeats a device
 * cannot form an RCCL communicator: such a handle folds the status on the host (one-GPU rehearsal of the multi-shard
 * path; see tinympc_sharded_fold_backend). */
int tinympc_create_sharded(tinympc_sharded **out, const double *A, const double *B, const double *Q, const double *R,
                           double rho, int nx, int nu, int N, int batch, int n_gpus, const int *devices, int verbose);
void tinympc_sharded_destroy(tinympc_sharded *s);
int tinympc_sharded_n_shards(tinympc_sharded *s);
/* "rccl" or "host" */
const char *tinympc_sharded_fold_backend(tinympc_sharded *s);
/* shard i: its device, its instance range [lo, hi) and its single-device handle (for the setters not mirrored below:
 * cones, linear rows, cache terms, adaptive rho ... — family-level calls, to be made on every shard).  Any out may be NULL. */
int tinympc_sharded_shard(tinympc_sharded *s, int i, int *device, int *lo, int *hi, tinympc_solver **local);
/* the partition rule itself (pure arithmetic, no GPU): shard `shard` of `n_shards` over `batch` instances */
void tinympc_shard_range(int batch, int n_shards, int shard, int *lo, int *hi);
/* family-level: applied to every shard (arguments as the tinympc_* function of the same name) */
int tinympc_sharded_update_settings(tinympc_sharded *s, double abs_pri_tol, double abs_dua_tol, int max_iter,
                                    int check_termination, int en_state_bound, int en_input_bound);
int tinympc_sharded_set_bound_constraints(tinympc_sharded *s, const double *x_min, const double *x_max,
                                          const double *u_min, const double *u_max);
int tinympc_sharded_set_warm_start(tinympc_sharded *s, int warm_start);
int tinympc_sharded_reset(tinympc_sharded *s);
int tinympc_sharded_set_precision(tinympc_sharded *s, int precision);
int tinympc_sharded_set_compaction(tinympc_sharded *s, int chunk_iters);
/* per-instance bounds over the WHOLE batch (arguments as tinympc_set_instance_bounds): both layouts are contiguous per
 * instance, shard i gets the slice [lo_i, hi_i) */
int tinympc_sharded_set_instance_bounds(tinympc_sharded *s, const double *x_min, const double *x_max, const double *u_min,
                                        const double *u_max, int per_knot);
/* per-instance linear rows over the WHOLE batch (arguments as tinympc_set_instance_linear): contiguous per instance, shard i
 * gets the slice [lo_i, hi_i) */
int tinympc_sharded_set_instance_linear(tinympc_sharded *s, const double *Alin_x, int rows_x, const double *blin_x,
                                        const double *Alin_u, int rows_u, const double *blin_u);
/* per-instance cone coefficients over the WHOLE batch (arguments as tinympc_set_instance_cones): the layout goes to every
 * shard, the coefficients are contiguous per instance, shard i gets the slice [lo_i, hi_i) */
int tinympc_sharded_set_instance_cones(tinympc_sharded *s, const int *Acu, const int *qcu, const double *cu, int n_input_cones,
                                       const int *Acx, const int *qcx, const double *cx, int n_state_cones);
/* per-instance inputs over the WHOLE batch (cols as tinympc_set_x0 / _x_ref / _u_ref), scattered to the shards */
int tinympc_sharded_set_x0(tinympc_sharded *s, const double *x0, int cols);
int tinympc_sharded_set_x_ref(tinympc_sharded *s, const double *x_ref, int cols);
int tinympc_sharded_set_u_ref(tinympc_sharded *s, const double *u_ref, int cols);
/* One batched solve on every device + the status all-reduce.  _solve = _solve_async + _wait.  Returns the GLOBAL status:
 * 0 iff every instance on every device converged, 1 otherwise, -1 on error (solve_mpc's convention, bindings.cpp:144-159). */
int tinympc_sharded_solve(tinympc_sharded *s);
int tinympc_sharded_solve_async(tinympc_sharded *s);
int tinympc_sharded_wait(tinympc_sharded *s);
/* the folded status block of the last solve: global residual maxima (pri_x, dua_x, pri_u, dua_u) and the largest
 * per-device count of unsolved instances (> 0 iff the status is 1).  Any out may be NULL. */
int tinympc_sharded_global_status(tinympc_sharded *s, double *residual_maxima4, int *max_unsolved_per_device);
/* outputs over the WHOLE batch, gathered from the shards into caller-allocated buffers (sizes as tinympc_get_*) */
int tinympc_sharded_get_states(tinympc_sharded *s, double *buf);
int tinympc_sharded_get_controls(tinympc_sharded *s, double *buf);
int tinympc_sharded_get_status(tinympc_sharded *s, int *iter, int *solved, double *residuals4);
int tinympc_sharded_get_workspace(tinympc_sharded *s, double *d, double *y, double *g, double *v, double *z);

/* The same on the process-global solver (the bare entry points of section (1)): after setup_solver / set_batch_size,
 * set_gpus(n) spreads the global solver's batch over devices 0 .. n-1 (n = 1: back to one device).  Every entry point
 * of section (1) then acts on the whole sharded batch — per-instance buffers are scattered / gathered, family-level
 * setters reach every shard, solve_mpc returns the all-reduced status — so src/TinyMPC.jl needs one extra ccall in
 * setup() and nothing else.  Inputs and the workspace are reset, as by set_batch_size. */
int set_gpus(int n_gpus);
int get_gpus(void);
/* warm_start = 0: every solve_mpc of the global solver starts from the zero workspace and keeps none (one-shot solves:
 * the regime of the benchmark configs, served by the on-chip kernels); 1 (default) = the reference's semantics, the
 * workspace persists between solves (admm.cpp:112-115).  The kernel the last solve ran on, for logs. */
int set_warm_start(int warm_start);
const char *get_kernel_name(void);
/* tinympc_cone_mode of the process-global solver (a set_gpus solver: of its first shard); -1 without a solver */
int get_cone_mode(void);

#ifdef __cplusplus
}
#endif
#endif /* TINYMPC_HIP_H */
