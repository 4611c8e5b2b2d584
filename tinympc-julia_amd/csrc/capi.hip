// extern "C" surface of libtinympc_hip.so (declared in include/tinympc_hip.h).
// The process-global entry points keep the names, argument lists and return
// conventions of the reference shim (reference: src/bindings.cpp:15-490) so that
// src/TinyMPC.jl's ccalls bind unchanged; the tinympc_* handle API adds the batch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <exception>
#include <memory>

#include "../../include/tinympc_hip.h"
#include "solver.h"
#include "noise.h"
#include "metrics.h"
#include "estimator.h"

using tmpc::set_error;

namespace {

std::unique_ptr<tinympc_solver> g_solver;  // bindings.cpp:15
// set_gpus(n > 1): the global solver's batch lives on n devices; g_solver then keeps the family-level state only
// (batch 1) so that a later set_gpus / set_batch_size can rebuild the shards from it
struct ShardedDeleter {
    void operator()(tinympc_sharded *p) const { tinympc_sharded_destroy(p); }
};
std::unique_ptr<tinympc_sharded, ShardedDeleter> g_sharded;
int g_sharded_batch = 0, g_verbose = 0;

tinympc_solver *global_shard(int i) {
    tinympc_solver *h = nullptr;
    tinympc_sharded_shard(g_sharded.get(), i, nullptr, nullptr, nullptr, &h);
    return h;
}
// a family-level call on the global solver: on the master and, when sharded, on every shard
template <class F>
int each_global(F &&f) {
    if (int rc = f(g_solver.get())) return rc;
    if (g_sharded)
        for (int i = 0; i < tinympc_sharded_n_shards(g_sharded.get()); ++i)
            if (int rc = f(global_shard(i))) return rc;
    return 0;
}
int global_batch() { return g_sharded ? g_sharded_batch : (g_solver ? g_solver->s.batch : 0); }

// (re)build the shards of the global solver for `batch` instances on `n_gpus` devices from the master's family state
int reshard_global(int batch, int n_gpus) {
    tmpc::Solver &m = g_solver->s;
    if (n_gpus <= 1) {
        g_sharded.reset();
        return m.alloc_batch(batch);
    }
    // TINYMPC_HIP_SHARD_DEVICES="0,0,...": explicit device list (test aid: several shards on one GPU, host status fold)
    std::vector<int> devs;
    if (const char *e = std::getenv("TINYMPC_HIP_SHARD_DEVICES")) {
        for (const char *p = e; *p;) {
            devs.push_back(std::atoi(p));
            while (*p && *p != ',') ++p;
            if (*p == ',') ++p;
        }
        if ((int)devs.size() != n_gpus) {
            set_error("set_gpus: TINYMPC_HIP_SHARD_DEVICES does not list n_gpus devices");
            return -1;
        }
    }
    tinympc_sharded *sh = nullptr;
    if (tinympc_create_sharded(&sh, m.A.a.data(), m.B.a.data(), m.Q.a.data(), m.R.a.data(), m.cache.rho, m.nx, m.nu, m.N,
                               batch, n_gpus, devs.empty() ? nullptr : devs.data(), g_verbose))
        return -1;
    // (a failure above leaves the previous arrangement untouched)
    g_sharded.reset(sh);
    g_sharded_batch = batch;
    for (int i = 0; i < n_gpus; ++i)
        if (global_shard(i)->s.copy_family_state(m)) {
            g_sharded.reset();
            (void)m.alloc_batch(batch);
            return -1;
        }
    return m.batch == 1 ? 0 : m.alloc_batch(1);
}

template <class F>
int guarded(const char *what, F &&f) {
    try {
        return f();
    } catch (const std::exception &e) {
        set_error(std::string(what) + " failed: " + e.what());
        return -1;
    } catch (...) {
        set_error(std::string(what) + " failed: unknown exception");
        return -1;
    }
}

int need_global(const char *what) {
    if (!g_solver) {
        set_error(std::string(what) + " failed: Solver not initialized");  // bindings.cpp:77-79
        return -1;
    }
    return 0;
}

bool dims_ok(const char *name, int r, int c, int er, int ec) {
    if (r == er && c == ec) return true;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s has %d x %d, expected %d x %d", name, r, c, er, ec);
    set_error(buf);
    return false;
}

int sync_status(tinympc_solver *s, hipStream_t stream) {
    if (!tmpc::hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize")) return -1;
    return s->s.solve_status();
}

}  // namespace

extern "C" {

/* ------------------------------ handle API ------------------------------ */

int tinympc_create(tinympc_solver **out, const double *A, const double *B, const double *Q,
                   const double *R, double rho, int nx, int nu, int N, int batch, int device,
                   int verbose) {
    return guarded("tinympc_create", [&]() -> int {
        if (!out || !A || !B || !Q || !R) {
            set_error("tinympc_create: null argument");
            return -1;
        }
        std::unique_ptr<tinympc_solver> s(new tinympc_solver());
        if (s->s.init(A, B, Q, R, rho, nx, nu, N, batch, device, verbose)) return -1;
        *out = s.release();
        return 0;
    });
}

int tinympc_create_families(tinympc_solver **out, const double *A, const double *B, const double *Q,
                            const double *R, const double *rho, int nx, int nu, int N, int batch, int device,
                            int verbose) {
    return guarded("tinympc_create_families", [&]() -> int {
        if (!out || !A || !B || !Q || !R || !rho) {
            set_error("tinympc_create_families: null argument");
            return -1;
        }
        std::unique_ptr<tinympc_solver> s(new tinympc_solver());
        if (s->s.init_families(A, B, Q, R, rho, nx, nu, N, batch, device, verbose)) return -1;
        *out = s.release();
        return 0;
    });
}

int tinympc_create_families_device(tinympc_solver **out, const double *A, const double *B, const double *Q,
                                   const double *R, const double *rho, int nx, int nu, int N, int batch, int device,
                                   int verbose) {
    return guarded("tinympc_create_families_device", [&]() -> int {
        if (!out || !A || !B || !Q || !R || !rho) {
            set_error("tinympc_create_families_device: null argument");
            return -1;
        }
        std::unique_ptr<tinympc_solver> s(new tinympc_solver());
        if (s->s.init_families(A, B, Q, R, rho, nx, nu, N, batch, device, verbose, true)) return -1;
        *out = s.release();
        return 0;
    });
}

int tinympc_set_families(tinympc_solver *s, const double *A, const double *B, const double *Q, const double *R,
                         const double *rho) {
    if (!s) return -1;
    return guarded("set_families", [&] { return s->s.set_families(A, B, Q, R, rho); });
}

int tinympc_get_family_cache(tinympc_solver *s, int first, int count, double *Kinf, double *Pinf, double *Quu_inv,
                             double *AmBKt, int *sweeps) {
    if (!s) return -1;
    return guarded("get_family_cache", [&] { return s->s.get_family_cache(first, count, Kinf, Pinf, Quu_inv, AmBKt, sweeps); });
}

int tinympc_families_setup_mode(tinympc_solver *s) { return s ? s->s.fam_mode : 0; }

int tinympc_families_setup_ms(tinympc_solver *s, double *ms) {
    if (!s || !ms) return -1;
    ms[0] = s->s.fam_ms[0], ms[1] = s->s.fam_ms[1];
    return 0;
}

void tinympc_destroy(tinympc_solver *s) { delete s; }

int tinympc_update_settings(tinympc_solver *s, double abs_pri_tol, double abs_dua_tol, int max_iter,
                            int check_termination, int en_state_bound, int en_input_bound) {
    if (!s) return -1;
    if (max_iter < 0) {
        set_error("update_settings: max_iter < 0");
        return -1;
    }
    tmpc::Settings &st = s->s.st;
    const bool flags_changed = st.en_state_bound != en_state_bound || st.en_input_bound != en_input_bound;
    st.abs_pri_tol = abs_pri_tol;
    st.abs_dua_tol = abs_dua_tol;
    st.max_iter = max_iter;
    st.check_termination = check_termination;
    st.en_state_bound = en_state_bound ? 1 : 0;
    st.en_input_bound = en_input_bound ? 1 : 0;
    if (flags_changed) s->s.packs_dirty = true, s->s.route_gen += 1;
    return 0;
}

int tinympc_enable_cones(tinympc_solver *s, int en_state_soc, int en_input_soc) {
    if (!s) return -1;
    s->s.st.en_state_soc = en_state_soc ? 1 : 0;
    s->s.st.en_input_soc = en_input_soc ? 1 : 0;
    s->s.route_gen += 1;
    s->s.packs_dirty = true;   // (upload_packs decides from extensions_active() whether the lean kernel takes one-shot solves)
    return 0;
}

int tinympc_set_bound_constraints(tinympc_solver *s, const double *x_min, const double *x_max,
                                  const double *u_min, const double *u_max) {
    if (!s || !x_min || !x_max || !u_min || !u_max) return -1;
    return guarded("set_bound_constraints", [&] { return s->s.set_bounds(x_min, x_max, u_min, u_max); });
}

int tinympc_set_instance_bounds(tinympc_solver *s, const double *x_min, const double *x_max, const double *u_min,
                                const double *u_max, int per_knot) {
    if (!s) return -1;
    if (!x_min || !x_max || !u_min || !u_max) {
        set_error("set_instance_bounds: null bound array");
        return -1;
    }
    return guarded("set_instance_bounds", [&] { return s->s.set_instance_bounds(x_min, x_max, u_min, u_max, per_knot != 0); });
}

int tinympc_bounds_mode(tinympc_solver *s) { return s ? s->s.bounds_mode : -1; }

int tinympc_set_fdyn(tinympc_solver *s, const double *fdyn) {
    if (!s) return -1;
    return guarded("set_fdyn", [&] { return s->s.set_fdyn(fdyn); });
}

int tinympc_enable_linear(tinympc_solver *s, int en_state_linear, int en_input_linear) {
    if (!s) return -1;
    s->s.st.en_state_linear = en_state_linear ? 1 : 0;
    s->s.st.en_input_linear = en_input_linear ? 1 : 0;
    s->s.lin_dirty = true;   // the device pack holds the enabled sides only
    s->s.route_gen += 1;
    s->s.packs_dirty = true;   // (upload_packs decides from extensions_active() whether the lean kernel takes one-shot solves)
    return 0;
}

int tinympc_set_linear_constraints(tinympc_solver *s, const double *Alin_x, int rows_x, const double *blin_x,
                                   const double *Alin_u, int rows_u, const double *blin_u) {
    if (!s) return -1;
    return guarded("set_linear_constraints",
                   [&] { return s->s.set_linear(Alin_x, rows_x, blin_x, Alin_u, rows_u, blin_u); });
}

int tinympc_set_instance_linear(tinympc_solver *s, const double *Alin_x, int rows_x, const double *blin_x,
                                const double *Alin_u, int rows_u, const double *blin_u) {
    if (!s) return -1;
    return guarded("set_instance_linear",
                   [&] { return s->s.set_instance_linear(Alin_x, rows_x, blin_x, Alin_u, rows_u, blin_u); });
}

int tinympc_lin_mode(tinympc_solver *s) { return s ? s->s.lin_mode : -1; }

int tinympc_set_cone_constraints(tinympc_solver *s, const int *Acu, const int *qcu, const double *cu,
                                 int n_input_cones, const int *Acx, const int *qcx, const double *cx,
                                 int n_state_cones) {
    if (!s || n_input_cones < 0 || n_state_cones < 0) return -1;
    return guarded("set_cone_constraints",
                   [&] { return s->s.set_cones(Acu, qcu, cu, n_input_cones, Acx, qcx, cx, n_state_cones); });
}

int tinympc_set_instance_cones(tinympc_solver *s, const int *Acu, const int *qcu, const double *cu, int n_input_cones,
                               const int *Acx, const int *qcx, const double *cx, int n_state_cones) {
    if (!s) return -1;
    return guarded("set_instance_cones",
                   [&] { return s->s.set_instance_cones(Acu, qcu, cu, n_input_cones, Acx, qcx, cx, n_state_cones); });
}

int tinympc_cone_mode(tinympc_solver *s) { return s ? s->s.cone_mode : -1; }

int tinympc_set_cache_terms(tinympc_solver *s, const double *Kinf, const double *Pinf,
                            const double *Quu_inv, const double *AmBKt) {
    if (!s || !Kinf || !Pinf || !Quu_inv || !AmBKt) return -1;
    tmpc::Solver &v = s->s;
    if (v.hetero) {
        set_error("set_cache_terms: not available on a per-instance-family solver");
        return -1;
    }
    v.cache.Kinf = tmpc::Mat(v.nu, v.nx, Kinf);
    v.cache.Pinf = tmpc::Mat(v.nx, v.nx, Pinf);
    v.cache.Quu_inv = tmpc::Mat(v.nu, v.nu, Quu_inv);
    v.cache.AmBKt = tmpc::Mat(v.nx, v.nx, AmBKt);
    v.packs_dirty = true;
    v.adapt_dirty = true;  // adaptive rho restarts from the new cache
    v.cache_overridden = true;  // AmBKt may no longer equal (A - B Kinf)': the quad kernel's adaptive variant relies on that identity
    return v.select_kernel();
}

int tinympc_set_adaptive_rho(tinympc_solver *s, int enable, double rho_min, double rho_max, int enable_clipping) {
    if (!s) return -1;
    tmpc::Solver &v = s->s;
    if (enable && v.hetero) {
        set_error("adaptive_rho is not available on a per-instance-family solver");
        return -1;
    }
    if (enable && v.bounds_mode) {
        set_error("adaptive_rho is not available with per-instance bounds (set_instance_bounds)");
        return -1;
    }
    if (enable && v.lin_mode) {
        set_error("adaptive_rho is not available with per-instance linear rows (set_instance_linear)");
        return -1;
    }
    if (enable && v.cone_mode) {
        set_error("adaptive_rho is not available with per-instance cones (set_instance_cones)");
        return -1;
    }
    if (enable && !(rho_min > 0.0 && rho_max >= rho_min)) {
        set_error("adaptive_rho: need 0 < rho_min <= rho_max");
        return -1;
    }
    if ((enable != 0) != (v.st.adaptive_rho != 0)) v.adapt_dirty = true;
    v.st.adaptive_rho = enable ? 1 : 0;
    v.st.adaptive_rho_min = rho_min;
    v.st.adaptive_rho_max = rho_max;
    v.st.adaptive_rho_clip = enable_clipping ? 1 : 0;
    return 0;
}

int tinympc_set_sensitivity(tinympc_solver *s, const double *dKinf, const double *dPinf, const double *dC1,
                            const double *dC2) {
    (void)dC1;  // accepted for the reference's call shape; they only ever reach dead copies there
    (void)dC2;
    if (!s || !dKinf || !dPinf) return -1;
    return guarded("set_sensitivity", [&] { return s->s.set_sensitivity(dKinf, dPinf); });
}

int tinympc_compute_sensitivity(tinympc_solver *s, double *dKinf, double *dPinf, double *dC1, double *dC2) {
    if (!s) return -1;
    return guarded("compute_sensitivity", [&] {
        tmpc::Solver &v = s->s;
        tmpc::Mat dK, dP, d1, d2;
        if (tmpc::compute_sensitivity(v.A, v.B, v.Q, v.R, v.cache.rho, dK, dP, d1, d2)) {
            set_error("compute_sensitivity: singular R + rho I + B'PB");
            return -1;
        }
        if (dKinf) std::copy(dK.a.begin(), dK.a.end(), dKinf);
        if (dPinf) std::copy(dP.a.begin(), dP.a.end(), dPinf);
        if (dC1) std::copy(d1.a.begin(), d1.a.end(), dC1);
        if (dC2) std::copy(d2.a.begin(), d2.a.end(), dC2);
        return 0;
    });
}

int tinympc_get_adaptive_state(tinympc_solver *s, double *rho, double *Kinf, double *Pinf) {
    if (!s) return -1;
    return guarded("get_adaptive_state", [&] { return s->s.get_adaptive_state(rho, Kinf, Pinf); });
}

int tinympc_get_cache_terms(tinympc_solver *s, double *Kinf, double *Pinf, double *Quu_inv,
                            double *AmBKt) {
    if (!s) return -1;
    const tmpc::Cache &c = s->s.cache;
    if (Kinf) std::copy(c.Kinf.a.begin(), c.Kinf.a.end(), Kinf);
    if (Pinf) std::copy(c.Pinf.a.begin(), c.Pinf.a.end(), Pinf);
    if (Quu_inv) std::copy(c.Quu_inv.a.begin(), c.Quu_inv.a.end(), Quu_inv);
    if (AmBKt) std::copy(c.AmBKt.a.begin(), c.AmBKt.a.end(), AmBKt);
    return 0;
}

int tinympc_set_x0(tinympc_solver *s, const double *x0, int cols) {
    if (!s || !x0) return -1;
    return guarded("set_x0", [&] { return s->s.set_x0(x0, cols); });
}
int tinympc_set_x_ref(tinympc_solver *s, const double *x_ref, int cols) {
    if (!s || !x_ref) return -1;
    return guarded("set_x_ref", [&] { return s->s.set_ref(true, x_ref, cols); });
}
int tinympc_set_u_ref(tinympc_solver *s, const double *u_ref, int cols) {
    if (!s || !u_ref) return -1;
    return guarded("set_u_ref", [&] { return s->s.set_ref(false, u_ref, cols); });
}
int tinympc_reset(tinympc_solver *s) { return s ? s->s.reset() : -1; }
int tinympc_set_warm_start(tinympc_solver *s, int warm_start) {
    if (!s) return -1;
    s->s.warm_start = warm_start != 0;
    return 0;
}

int tinympc_solve(tinympc_solver *s) {
    if (!s) return -1;
    return guarded("solve", [&]() -> int {
        if (s->s.solve_async(nullptr)) return -1;
        return sync_status(s, nullptr);
    });
}
int tinympc_solve_async(tinympc_solver *s, void *hip_stream) {
    if (!s) return -1;
    return guarded("solve_async", [&] { return s->s.solve_async((hipStream_t)hip_stream); });
}
int tinympc_solve_status(tinympc_solver *s) { return s ? s->s.solve_status() : -1; }

int tinympc_mpc_rollout(tinympc_solver *s, int steps, void *hip_stream) {
    if (!s || steps < 1) return -1;
    return guarded("mpc_rollout", [&]() -> int {
        if (s->s.solve_async((hipStream_t)hip_stream, steps)) return -1;
        return sync_status(s, (hipStream_t)hip_stream);
    });
}
int tinympc_set_ref_sequence(tinympc_solver *s, const double *x_ref_seq, int x_rows, int x_cols, const double *u_ref_seq,
                             int u_rows, int u_cols, int steps) {
    if (!s) return -1;
    return guarded("set_ref_sequence", [&]() -> int {
        if (steps > 0 && (x_rows != s->s.nx || u_rows != s->s.nu || (long)x_cols != (long)s->s.N * steps ||
                          (long)u_cols != (long)(s->s.N - 1) * steps)) {
            tmpc::set_error("set_ref_sequence: expected nx x (N steps) and nu x ((N-1) steps)");
            return -1;
        }
        return s->s.set_ref_sequence(x_ref_seq, u_ref_seq, steps);
    });
}
int tinympc_set_plant(tinympc_solver *s, const double *A, const double *B, const double *f, int per_instance) {
    if (!s) return -1;
    if (per_instance != 0 && per_instance != 1) {
        set_error("set_plant: per_instance is 0 (A nx x nx, B nx x nu, f nx) or 1 (A [batch][nx*nx], B [batch][nx*nu], f [batch][nx])");
        return -1;
    }
    return guarded("set_plant", [&] { return s->s.set_plant(A, B, f, per_instance); });
}
int tinympc_set_disturbance(tinympc_solver *s, const double *w, int steps, int per_instance) {
    if (!s) return -1;
    if (steps < 0 || (per_instance != 0 && per_instance != 1)) {
        set_error("set_disturbance: expected steps >= 0 and per_instance 0 (w nx x steps) or 1 (w [batch][steps][nx])");
        return -1;
    }
    return guarded("set_disturbance", [&] { return s->s.set_disturbance(w, steps, per_instance); });
}
int tinympc_plant_mode(tinympc_solver *s) { return s ? s->s.plant_mode() : -1; }
int tinympc_set_ref_trajectory(tinympc_solver *s, const double *x_traj, int Lx, const double *u_traj, int Lu, int per_instance) {
    if (!s) return -1;
    if (x_traj && (Lx < 1 || (u_traj && Lu < 1) || (per_instance != 0 && per_instance != 1))) {
        set_error("set_ref_trajectory: expected Lx >= 1 rows of x_traj, Lu >= 1 rows of u_traj where one is given, and per_instance 0 "
                  "(x_traj [Lx][nx], u_traj [Lu][nu]) or 1 (x_traj [batch][Lx][nx], u_traj [batch][Lu][nu])");
        return -1;
    }
    return guarded("set_ref_trajectory", [&] { return s->s.set_ref_trajectory(x_traj, Lx, u_traj, Lu, per_instance); });
}
int tinympc_set_ref_cursor(tinympc_solver *s, int cursor) {
    if (!s) return -1;
    if (cursor < 0) {
        set_error("set_ref_cursor: the cursor is a row of the reference trajectory, 0 or more (rows past the end read the last one)");
        return -1;
    }
    s->s.ref_cursor = cursor;
    return 0;
}
int tinympc_ref_cursor(tinympc_solver *s) { return s ? s->s.ref_cursor : -1; }
int tinympc_ref_trajectory_mode(tinympc_solver *s) { return s ? s->s.traj_kind : -1; }
static int set_noise_checked(tinympc_solver *s, const char *name, int which, const double *G, int per_instance, unsigned long long seed) {
    if (!s) return -1;
    if (G && per_instance != 0 && per_instance != 1) {
        set_error(std::string(name) + ": per_instance is 0 (G nx x nx column-major, shared) or 1 (G [batch][nx*nx])");
        return -1;
    }
    return guarded(name, [&] { return s->s.set_noise(which, G, per_instance, seed); });
}
int tinympc_set_process_noise(tinympc_solver *s, const double *G, int per_instance, unsigned long long seed) {
    return set_noise_checked(s, "set_process_noise", tmpc::NOISE_PROCESS, G, per_instance, seed);
}
int tinympc_set_measurement_noise(tinympc_solver *s, const double *G, int per_instance, unsigned long long seed) {
    return set_noise_checked(s, "set_measurement_noise", tmpc::NOISE_MEASUREMENT, G, per_instance, seed);
}
int tinympc_set_noise_cursor(tinympc_solver *s, int t) {
    if (!s) return -1;
    if (t < 0) {
        set_error("set_noise_cursor: the cursor is the step index of the next loop's first draw, 0 or more; a negative one is refused");
        return -1;
    }
    s->s.noise_cursor = t;
    return 0;
}
int tinympc_noise_cursor(tinympc_solver *s) { return s ? s->s.noise_cursor : -1; }
int tinympc_noise_mode(tinympc_solver *s) { return s ? s->s.noise_mode() : -1; }
int tinympc_get_noise(tinympc_solver *s, int which, int t0, int steps, double *buf) {
    if (!s) return -1;
    return guarded("get_noise", [&] { return s->s.get_noise(which, t0, steps, buf); });
}
int tinympc_get_mpc_measured(tinympc_solver *s, double *y) {
    if (!s) return -1;
    return guarded("get_mpc_measured", [&] { return s->s.get_mpc_measured(y); });
}
// the draw rule on the host: csrc/noise.h, the text the device kernels compile; touches no device
int tinympc_host_noise(unsigned long long seed, int which, long long b, int t, int nx, const double *G, double *out) {
    if (which < 0 || which > 1 || b < 0 || t < 0 || nx < 1 || !out) {
        set_error("host_noise: expected which 0 (process) or 1 (measurement), b >= 0, t >= 0, nx >= 1 and nx doubles of output");
        return -1;
    }
    std::vector<double> xi((size_t)nx + 1);
    for (int j = 0; 2 * j < nx; ++j) tmpc::noise_pair(seed, which, (uint64_t)b, (uint32_t)t, (uint32_t)j, xi[2 * j], xi[2 * j + 1]);
    for (int r = 0; r < nx; ++r) out[r] = G ? tmpc::noise_row(G, nx, r, xi.data()) : xi[r];
    return 0;
}
int tmpc_philox4x32_10(const unsigned *ctr4, const unsigned *key2, unsigned *out4) {
    if (!ctr4 || !key2 || !out4) return -1;
    tmpc::philox4x32_10(ctr4, key2, out4);
    return 0;
}
// ---- output feedback through a state estimator stepped on the device (the rule: csrc/estimator.h; the kernel: estimator.hip) ----
int tinympc_set_estimator(tinympc_solver *s, const double *C, int ny, const double *L, int per_instance) {
    if (!s) return -1;
    if ((C == nullptr) != (L == nullptr)) {
        set_error("set_estimator: expected both C (ny x nx) and L (nx x ny), or neither to drop the estimator");
        return -1;
    }
    if (C && (ny < 1 || ny > s->s.nx)) {
        set_error("set_estimator: ny = " + std::to_string(ny) + " outputs; expected 1 <= ny <= nx = " + std::to_string(s->s.nx));
        return -1;
    }
    if (C && per_instance != 0 && per_instance != 1) {
        set_error("set_estimator: per_instance is 0 (C ny x nx and L nx x ny column-major, shared) or 1 ([batch] of each)");
        return -1;
    }
    return guarded("set_estimator", [&] { return s->s.set_estimator(C, ny, L, per_instance); });
}
int tinympc_set_estimator_state(tinympc_solver *s, const double *xhat, int per_instance) {
    if (!s) return -1;
    if (xhat && per_instance != 0 && per_instance != 1) {
        set_error("set_estimator_state: per_instance is 0 (xhat nx, shared) or 1 (xhat [batch][nx])");
        return -1;
    }
    return guarded("set_estimator_state", [&] { return s->s.set_estimator_state(xhat, per_instance); });
}
int tinympc_estimator_mode(tinympc_solver *s) { return s ? s->s.est_kind : -1; }
int tinympc_estimator_outputs(tinympc_solver *s) { return s ? s->s.est_ny : -1; }
int tinympc_get_estimator_state(tinympc_solver *s, double *xhat) {
    if (!s) return -1;
    return guarded("get_estimator_state", [&] { return s->s.get_estimator_state(xhat); });
}
int tinympc_get_mpc_estimate(tinympc_solver *s, double *xhat) {
    if (!s) return -1;
    return guarded("get_mpc_estimate", [&] { return s->s.get_mpc_estimate(xhat); });
}
int tinympc_get_mpc_outputs(tinympc_solver *s, double *y) {
    if (!s) return -1;
    return guarded("get_mpc_outputs", [&] { return s->s.get_mpc_outputs(y); });
}
// the rule on the host: csrc/estimator.h, the text the device kernel compiles, one instance and one step; touches no device
int tinympc_host_estimator_step(int nx, int nu, int ny, int predict, int correct, const double *A, const double *B, const double *f, const double *C,
                                const double *L, const double *u, const double *x, const double *v, double *xhat, double *y) {
    if (nx < 1 || nu < 1 || ny < 1 || ny > nx || (!predict && !correct) || !xhat) {
        set_error("host_estimator_step: expected nx >= 1, nu >= 1, 1 <= ny <= nx, predict and / or correct, and xhat (nx doubles, in and out)");
        return -1;
    }
    if (predict && (!A || !B || !u)) {
        set_error("host_estimator_step: the predict needs the model A (nx x nx), B (nx x nu) (f nx or null: zero) and the control u (nu)");
        return -1;
    }
    if (correct && (!C || !L || !x || !y)) {
        set_error("host_estimator_step: the correct needs C (ny x nx), L (nx x ny), the true state x (nx) and y (ny doubles of output); v (ny) or null: no noise");
        return -1;
    }
    std::vector<double> model;
    if (predict) {
        model.assign(A, A + (size_t)nx * nx);
        model.insert(model.end(), B, B + (size_t)nx * nu);
        for (int r = 0; r < nx; ++r) model.push_back(f ? f[r] : 0.0);
    }
    tmpc::estimator_step_host(nx, nu, ny, predict != 0, correct != 0, model.data(), C, L, u, x, v, xhat, y);
    return 0;
}
int tinympc_host_kalman_gain(const double *A, const double *C, const double *W, const double *V, int nx, int ny, double *L, double *P) {
    if (!A || !C || !W || !V || !L || nx < 1 || ny < 1 || ny > nx) {
        set_error("host_kalman_gain: expected A (nx x nx), C (ny x nx), W (nx x nx), V (ny x ny), 1 <= ny <= nx, and L (nx x ny doubles of output; P nx x nx or null)");
        return -1;
    }
    std::string why;
    if (!tmpc::kalman_gain_host(A, C, W, V, nx, ny, L, P, why)) {
        set_error("host_kalman_gain: " + why);
        return -1;
    }
    return 0;
}
// ---- per-instance closed-loop metrics folded on the device (the rule: csrc/metrics.h; the kernels: metrics.hip) ----
int tinympc_set_rollout_metrics(tinympc_solver *s, int enable, const double *qw, const double *rw, const double *x_lo, const double *x_hi,
                                const double *u_lo, const double *u_hi) {
    if (!s) return -1;
    if (enable != 0 && enable != 1) {
        set_error("set_rollout_metrics: enable is 1 (install the configuration, zero the accumulators) or 0 (drop both)");
        return -1;
    }
    return guarded("set_rollout_metrics", [&] { return s->s.set_rollout_metrics(enable, qw, rw, x_lo, x_hi, u_lo, u_hi); });
}
int tinympc_reset_rollout_metrics(tinympc_solver *s) {
    if (!s) return -1;
    return guarded("reset_rollout_metrics", [&] { return s->s.reset_rollout_metrics(); });
}
int tinympc_rollout_metrics_mode(tinympc_solver *s) { return s ? (s->s.metrics_on ? 1 : 0) : -1; }
int tinympc_get_rollout_metrics(tinympc_solver *s, double *per_instance) {
    if (!s) return -1;
    return guarded("get_rollout_metrics", [&] { return s->s.get_rollout_metrics(per_instance); });
}
int tinympc_get_rollout_summary(tinympc_solver *s, double *summary) {
    if (!s) return -1;
    return guarded("get_rollout_summary", [&] { return s->s.get_rollout_summary(summary); });
}
// the rule on the host: csrc/metrics.h, the text the device kernel compiles, step after step; touches no device
int tinympc_host_rollout_metrics(int nx, int nu, int steps, const float *x_log, const float *u_log, const int *iter_log, const float *xr,
                                 const float *ur, const double *qw, const double *rw, const double *x_lo, const double *x_hi, const double *u_lo,
                                 const double *u_hi, double *acc11) {
    if (nx < 1 || nu < 1 || steps < 0 || !x_log || !u_log || !iter_log || !qw || !rw || !acc11) {
        set_error("host_rollout_metrics: expected nx >= 1, nu >= 1, steps >= 0, the three logs, the weights qw (nx) and rw (nu), and 11 doubles of accumulators");
        return -1;
    }
    for (int r = 0; r < nx; ++r)
        if (qw[r] < 0.0 || (x_lo && x_hi && x_lo[r] > x_hi[r])) {
            set_error("host_rollout_metrics: a negative weight, or x_lo > x_hi, in row " + std::to_string(r));
            return -1;
        }
    for (int a = 0; a < nu; ++a)
        if (rw[a] < 0.0 || (u_lo && u_hi && u_lo[a] > u_hi[a])) {
            set_error("host_rollout_metrics: a negative weight, or u_lo > u_hi, in row " + std::to_string(a));
            return -1;
        }
    const tmpc::MetricConfig cfg{qw, rw, x_lo, x_hi, u_lo, u_hi};
    for (int s = 0; s < steps; ++s) {
        const tmpc::MetricStep m = tmpc::metric_step(nx, nu, x_log + (size_t)s * nx, u_log + (size_t)s * nu, xr ? xr + (size_t)s * nx : nullptr,
                                                     ur ? ur + (size_t)s * nu : nullptr, cfg);
        double one[tmpc::METRIC_COUNT];
        tmpc::metric_step_slots(m, iter_log[s], one);
        const double had = acc11[tmpc::METRIC_STEPS];
        for (int k = 0; k < tmpc::METRIC_COUNT; ++k) acc11[k] = tmpc::metric_combine(k, acc11[k], one[k], had, 1.0);
    }
    return 0;
}
int tinympc_get_mpc_log(tinympc_solver *s, double *x, double *u, int *iter) {
    if (!s) return -1;
    return guarded("get_mpc_log", [&] { return s->s.get_mpc_log(x, u, iter); });
}

int tinympc_get_states(tinympc_solver *s, double *buf) {
    if (!s || !buf) return -1;
    return guarded("get_states", [&] { return s->s.get_traj(true, buf); });
}
int tinympc_get_controls(tinympc_solver *s, double *buf) {
    if (!s || !buf) return -1;
    return guarded("get_controls", [&] { return s->s.get_traj(false, buf); });
}
// fp32 host arrays: the device buffers are fp32, so these are plain copies — no narrowing / widening pass on the host
// (the fp64 forms spend most of a round trip on it: DESIGN.md, PCIe-inclusive rate)
int tinympc_set_x0_f32(tinympc_solver *s, const float *x0, int cols) {
    if (!s || !x0) return -1;
    return guarded("set_x0_f32", [&]() -> int {
        tmpc::Solver &v = s->s;
        if (cols != 1 && cols != v.batch) {
            tmpc::set_error("set_x0_f32: expected nx x 1 or nx x batch");
            return -1;
        }
        if (!tmpc::hip_ok(hipSetDevice(v.device), "hipSetDevice") || v.wait_last_launch()) return -1;
        if (cols == v.batch) {
            return tmpc::hip_ok(hipMemcpy(v.d_x0, x0, (size_t)v.batch * v.nx * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy") ? 0 : -1;
        }
        std::vector<float> h((size_t)v.batch * v.nx);
        for (int b = 0; b < v.batch; ++b) std::copy(x0, x0 + v.nx, h.begin() + (size_t)b * v.nx);
        return tmpc::hip_ok(hipMemcpy(v.d_x0, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy") ? 0 : -1;
    });
}
static int get_traj_f32(tinympc_solver *s, bool states, float *buf) {
    tmpc::Solver &v = s->s;
    if (!tmpc::hip_ok(hipSetDevice(v.device), "hipSetDevice") || v.wait_last_launch()) return -1;
    const size_t n = (size_t)v.batch * (states ? v.ex() : v.eu());
    return tmpc::hip_ok(hipMemcpy(buf, states ? v.d_xout : v.d_uout, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy") ? 0 : -1;
}
int tinympc_get_states_f32(tinympc_solver *s, float *buf) {
    if (!s || !buf) return -1;
    return guarded("get_states_f32", [&] { return get_traj_f32(s, true, buf); });
}
int tinympc_get_controls_f32(tinympc_solver *s, float *buf) {
    if (!s || !buf) return -1;
    return guarded("get_controls_f32", [&] { return get_traj_f32(s, false, buf); });
}
int tinympc_pin_host(tinympc_solver *s, void *ptr, size_t bytes) {
    if (!s) return -1;
    return guarded("pin_host", [&] { return s->s.pin_host_range(ptr, bytes); });
}
int tinympc_unpin_host(tinympc_solver *s, void *ptr) {
    if (!s) return -1;
    return guarded("unpin_host", [&] { return s->s.unpin_host_range(ptr); });
}
int tinympc_get_status(tinympc_solver *s, int *iter, int *solved, double *residuals4) {
    if (!s) return -1;
    return guarded("get_status", [&] { return s->s.get_status(iter, solved, residuals4); });
}
int tinympc_get_workspace(tinympc_solver *s, double *d, double *y, double *g, double *v, double *z) {
    if (!s) return -1;
    return guarded("get_workspace", [&] { return s->s.get_workspace(d, y, g, v, z); });
}
int tinympc_set_workspace(tinympc_solver *s, const double *d, const double *y, const double *g,
                          const double *v, const double *z) {
    if (!s) return -1;
    return guarded("set_workspace", [&] { return s->s.set_workspace(d, y, g, v, z); });
}

int tinympc_device_buffers(tinympc_solver *s, void **x0, void **x_ref, void **u_ref, void **states,
                           void **controls, void **iter, void **solved, void **residuals,
                           void **gstat) {
    if (!s) return -1;
    tmpc::Solver &v = s->s;
    if (x0) *x0 = v.d_x0;
    if (x_ref) *x_ref = v.d_xref;
    if (u_ref) *u_ref = v.d_uref;
    if (states) *states = v.d_xout;
    if (controls) *controls = v.d_uout;
    if (iter) *iter = v.d_iter;
    if (solved) *solved = v.d_solved;
    if (residuals) *residuals = v.d_res;
    if (gstat) *gstat = v.d_gstat;
    return 0;
}

int tinympc_set_ref_mode(tinympc_solver *s, int ref_mode) {
    if (!s || ref_mode < 0 || ref_mode > 2) return -1;
    return guarded("set_ref_mode", [&]() -> int {
        tmpc::Solver &v = s->s;
        if (v.traj_kind && v.drop_ref_trajectory(false)) return -1;   // (a reference trajectory goes: the caller writes the arrays now)
        // make the device buffers large enough for the mode, then hand them to the caller
        v.xref_kind = v.uref_kind = ref_mode;
        v.h_xref.assign(ref_mode == 2 ? (size_t)v.batch * v.ex() : (ref_mode == 1 ? v.ex() : 0), 0.f);
        v.h_uref.assign(ref_mode == 2 ? (size_t)v.batch * v.eu() : (ref_mode == 1 ? v.eu() : 0), 0.f);
        v.refs_dirty = true;
        v.refs_device_owned = false;
        if (v.upload_refs()) return -1;
        v.h_xref.clear();
        v.h_uref.clear();
        v.refs_device_owned = true;
        return 0;
    });
}

int tinympc_set_compaction(tinympc_solver *s, int chunk_iters) {
    if (!s || chunk_iters < 0) return -1;
    s->s.chunk_iters = chunk_iters;
    return 0;
}
int tinympc_set_profiling(tinympc_solver *s, int enable) {
    if (!s) return -1;
    s->s.profiling = enable != 0;
    return 0;
}
double tinympc_kernel_elapsed_ms(tinympc_solver *s) { return s ? s->s.kernel_elapsed_ms() : -1.0; }
double tinympc_kernel_elapsed_mean_ms(tinympc_solver *s, int last_n) {
    return s ? s->s.kernel_elapsed_mean_ms(last_n) : -1.0;
}
int tinympc_set_precision(tinympc_solver *s, int precision) {
    if (!s || precision < 0 || precision > 2) return -1;
    if (precision == 2 && s->s.hetero) {
        set_error("set_precision: precision 2 is not available on a per-instance-family solver");
        return -1;
    }
    if (s->s.precision != precision) {
        s->s.packs_dirty = true;
        // the workspace kept between solves does not carry over between the fp32 arrays and the fp64 block: cold restart
        if ((s->s.precision == 2) != (precision == 2) && s->s.solved_once && s->s.reset()) return -1;
    }
    s->s.precision = precision;
    return 0;
}

// tuning / test aid: the environment switches are read when a solver is created; this re-reads them for a live solver
int tinympc_reload_switches(tinympc_solver *s) {
    if (!s) return -1;
    s->s.sw = tmpc::read_switches();
    s->s.lean_enabled = !s->s.sw.no_lean;
    s->s.route_gen += 1;
    s->s.packs_dirty = true;
    return 0;
}
int tinympc_set_strict_precision(tinympc_solver *s, int strict) {
    if (!s) return -1;
    s->s.strict_precision = strict != 0;
    return 0;
}
int tinympc_effective_precision(tinympc_solver *s) {
    if (!s) return -1;
    tmpc::Solver &v = s->s;
    if (v.select_kernel()) return -1;
    // the matrix-core kernels and the lean kernel only exist with fp64 recurrences; every other family follows `precision`
    const bool matrix = (v.ke && v.ke->G == 16) || v.ce != nullptr;
    return v.precision == 2 ? 2 : (matrix ? 0 : v.precision);
}
const char *tinympc_kernel_name(tinympc_solver *s) { return s ? s->s.kernel_name.c_str() : ""; }
const char *tinympc_last_launch_name(tinympc_solver *s) {
    if (!s) return "";
    return s->s.last_launch_name.empty() ? s->s.kernel_name.c_str() : s->s.last_launch_name.c_str();
}

/* compulsory fp32 device I/O per solve, state on chip. */
double tinympc_algorithmic_bytes(tinympc_solver *s) {
    if (!s) return 0;
    const tmpc::Solver &v = s->s;
    const double EX = v.ex(), EU = v.eu();
    double per = 4.0 * v.nx + 4.0 * (EX + EU) + 24.0;             // x0 in, x/u out, iter/solved/4 res
    if (v.ref_mode == tmpc::REF_PER_INSTANCE) per += 4.0 * (EX + EU);
    if (v.warm_start) per += 2.0 * 4.0 * (3.0 * EU + 2.0 * EX);   // d,y,z,g,v in and out
    // per-instance bounds: min and max of every state and input row — per knot and iteration where they are given per knot
    // (the kernels stream them with the knot's other arrays), once where they are constant over the horizon
    if (v.bounds_mode == 2) per += 4.0 * 2.0 * (EX + EU) * v.st.max_iter;
    if (v.bounds_mode == 1) per += 4.0 * 2.0 * (v.nx + v.nu);
    // per-instance linear rows: coefficients, right-hand side and |a|^2 of every row, read once (they are constant over the horizon)
    if (v.lin_mode) per += 4.0 * (v.mlx * (v.nx + 2.0) + v.mlu * (v.nu + 2.0));
    // per-instance cone coefficients: one float per cone, read once
    if (v.cone_mode) per += 4.0 * (v.ncx + v.ncu);
    return per * v.batch;
}

/* 2(N-1)(2nx^2+4nx nu+nu^2) + (N-1)(nu+2nx) + 15(Ex+Eu) + 2nx^2 + 3nx per iteration. */
double tinympc_algorithmic_flops(tinympc_solver *s, int iters) {
    if (!s) return 0;
    const tmpc::Solver &v = s->s;
    const double nx = v.nx, nu = v.nu, N = v.N, EX = v.ex(), EU = v.eu();
    const double per_it = 2.0 * (N - 1) * (2 * nx * nx + 4 * nx * nu + nu * nu) + (N - 1) * (nu + 2 * nx) +
                          15.0 * (EX + EU) + 2 * nx * nx + 3 * nx;
    return per_it * iters * v.batch;
}

const char *tinympc_last_error(void) { return tmpc::last_error(); }

// Specialise the on-chip kernel of a shape now (what tinympc_create does by itself for a shape the library was not built with):
// 1 = an on-chip kernel exists for the shape afterwards (built in, cached, or just compiled), 0 = none (run-time-shape kernels)
int tinympc_specialise(int nx, int nu, int N, int verbose) {
    if (tmpc::find_quad_kernel(nx, nu, N, -1) || tmpc::find_mfma_kernel(nx, nu, N) || tmpc::find_trans_kernel(nx, nu, N)) return 1;
    return tmpc::jit_kernel_for(nx, nu, N, verbose) != nullptr ? 1 : 0;
}

int tinympc_host_precompute(const double *A, const double *B, const double *Q, const double *R,
                            double rho, int nx, int nu, double *Kinf, double *Pinf,
                            double *Quu_inv, double *AmBKt) {
    return guarded("host_precompute", [&]() -> int {
        if (!A || !B || !Q || !R || nx < 1 || nu < 1) return -1;
        tmpc::Cache c;
        if (tmpc::precompute_cache(tmpc::Mat(nx, nx, A), tmpc::Mat(nx, nu, B), tmpc::Mat(nx, nx, Q),
                                   tmpc::Mat(nu, nu, R), rho, c)) {
            set_error("Riccati precompute failed: R + B'PB is singular");
            return -1;
        }
        if (Kinf) std::copy(c.Kinf.a.begin(), c.Kinf.a.end(), Kinf);
        if (Pinf) std::copy(c.Pinf.a.begin(), c.Pinf.a.end(), Pinf);
        if (Quu_inv) std::copy(c.Quu_inv.a.begin(), c.Quu_inv.a.end(), Quu_inv);
        if (AmBKt) std::copy(c.AmBKt.a.begin(), c.AmBKt.a.end(), AmBKt);
        return 0;
    });
}

int tinympc_host_precompute_sweeps(const double *A, const double *B, const double *Q, const double *R, double rho, int nx, int nu) {
    int sweeps = -1;
    (void)guarded("host_precompute_sweeps", [&]() -> int {
        if (!A || !B || !Q || !R || nx < 1 || nu < 1) return -1;
        tmpc::Cache c;
        if (tmpc::precompute_cache(tmpc::Mat(nx, nx, A), tmpc::Mat(nx, nu, B), tmpc::Mat(nx, nx, Q), tmpc::Mat(nu, nu, R), rho, c)) {
            set_error("Riccati precompute failed: R + B'PB is singular");
            return -1;
        }
        sweeps = c.riccati_iters;
        return 0;
    });
    return sweeps;
}

int tinympc_host_family_cache(const double *A, const double *B, const double *Q, const double *R, double rho, int nx, int nu,
                              double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps) {
    return guarded("host_family_cache", [&]() -> int {
        if (!A || !B || !Q || !R || nx < 1 || nu < 1) return -1;
        std::vector<double> qd((size_t)nx), rd((size_t)nu), K((size_t)nu * nx), P((size_t)nx * nx), Qi((size_t)nu * nu), At((size_t)nx * nx);
        for (int i = 0; i < nx; ++i) qd[i] = Q[i + (size_t)i * nx];
        for (int a = 0; a < nu; ++a) rd[a] = R[a + (size_t)a * nu];
        const int st = tmpc::families_host_cache(nx, nu, A, B, qd.data(), rd.data(), rho, K.data(), P.data(), Qi.data(), At.data(), sweeps);
        if (st) {
            set_error(st == 1 ? "Riccati precompute failed: R + B'PB is singular"
                              : "host_family_cache: the rule is built for nx in {2,3,4,6,8,10,12}, nu <= 4");
            return -1;
        }
        if (Kinf) std::copy(K.begin(), K.end(), Kinf);
        if (Pinf) std::copy(P.begin(), P.end(), Pinf);
        if (Quu_inv) std::copy(Qi.begin(), Qi.end(), Quu_inv);
        if (AmBKt) std::copy(At.begin(), At.end(), AmBKt);
        return 0;
    });
}

int tinympc_host_sensitivity(const double *A, const double *B, const double *Q, const double *R, double rho, int nx,
                             int nu, double *dKinf, double *dPinf, double *dC1, double *dC2) {
    return guarded("host_sensitivity", [&]() -> int {
        if (!A || !B || !Q || !R || nx < 1 || nu < 1) return -1;
        tmpc::Mat dK, dP, d1, d2;
        if (tmpc::compute_sensitivity(tmpc::Mat(nx, nx, A), tmpc::Mat(nx, nu, B), tmpc::Mat(nx, nx, Q),
                                      tmpc::Mat(nu, nu, R), rho, dK, dP, d1, d2)) {
            set_error("host_sensitivity: singular R + rho I + B'PB");
            return -1;
        }
        if (dKinf) std::copy(dK.a.begin(), dK.a.end(), dKinf);
        if (dPinf) std::copy(dP.a.begin(), dP.a.end(), dPinf);
        if (dC1) std::copy(d1.a.begin(), d1.a.end(), dC1);
        if (dC2) std::copy(d2.a.begin(), d2.a.end(), dC2);
        return 0;
    });
}

/* --------------------- process-global solver (drop-in) --------------------- */

int setup_solver(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols,
                 double *fdyn_data, int fdyn_rows, int fdyn_cols, double *Q_data, int Q_rows,
                 int Q_cols, double *R_data, int R_rows, int R_cols, double rho, int nx, int nu,
                 int N, int verbose) {
    return guarded("setup_solver", [&]() -> int {
        g_sharded.reset();
        g_verbose = verbose;
        if (!A_data || !B_data || !Q_data || !R_data) {
            set_error("setup_solver: null matrix");
            g_solver.reset();
            return -1;
        }
        if (!dims_ok("A", A_rows, A_cols, nx, nx) || !dims_ok("B", B_rows, B_cols, nx, nu) ||
            !dims_ok("Q", Q_rows, Q_cols, nx, nx) || !dims_ok("R", R_rows, R_cols, nu, nu)) {
            g_solver.reset();
            return -1;
        }
        if (fdyn_data && (long)fdyn_rows * fdyn_cols != nx) {
            set_error("setup_solver: fdyn must have nx entries");
            g_solver.reset();
            return -1;
        }
        tinympc_solver *s = nullptr;
        if (tinympc_create(&s, A_data, B_data, Q_data, R_data, rho, nx, nu, N, 1, -1, verbose)) {
            g_solver.reset();
            return -1;
        }
        if (fdyn_data && tinympc_set_fdyn(s, fdyn_data)) {
            tinympc_destroy(s);
            g_solver.reset();
            return -1;
        }
        g_solver.reset(s);  // a second setup replaces the first (bindings.cpp:63)
        return 0;
    });
}

int set_batch_size(int batch) {
    if (need_global("set_batch_size")) return -1;
    return guarded("set_batch_size", [&] {
        return g_sharded ? reshard_global(batch, tinympc_sharded_n_shards(g_sharded.get())) : g_solver->s.alloc_batch(batch);
    });
}
int get_batch_size(void) { return global_batch(); }

int set_gpus(int n_gpus) {
    if (need_global("set_gpus")) return -1;
    if (n_gpus < 1) {
        set_error("set_gpus: n_gpus must be >= 1");
        return -1;
    }
    return guarded("set_gpus", [&] { return reshard_global(global_batch(), n_gpus); });
}
int get_gpus(void) { return g_sharded ? tinympc_sharded_n_shards(g_sharded.get()) : (g_solver ? 1 : 0); }

// warm_start = 0: every solve() of the global solver starts from the zero workspace and keeps none ("one-shot": the
// benchmark configs' regime, and what lets the on-chip kernels run); 1 (default): the reference's semantics, the
// workspace persists between solves (admm.cpp:112-115 resets only the counters)
int set_warm_start(int warm_start) {
    if (need_global("set_warm_start")) return -1;
    return each_global([&](tinympc_solver *h) { return tinympc_set_warm_start(h, warm_start); });
}
// recurrence / state precision of the global solver (tinympc_set_precision): 0 default, 1 all fp32, 2 all fp64 like the reference
int set_precision(int precision) {
    if (need_global("set_precision")) return -1;
    return each_global([&](tinympc_solver *h) { return tinympc_set_precision(h, precision); });
}
const char *get_kernel_name(void) {
    if (!g_solver) return "";
    return (g_sharded ? global_shard(0)->s : g_solver->s).kernel_name.c_str();
}
int get_cone_mode(void) {
    if (!g_solver) return -1;
    return (g_sharded ? global_shard(0)->s : g_solver->s).cone_mode;
}

int set_x0(double *x0_data, int x0_rows, int x0_cols, int verbose) {
    (void)verbose;
    if (need_global("set_x0")) return -1;
    if (x0_rows != g_solver->s.nx) {
        set_error("set_x0: x0 is not the correct length");
        return -1;
    }
    if (g_sharded) return guarded("set_x0", [&] { return tinympc_sharded_set_x0(g_sharded.get(), x0_data, x0_cols); });
    return tinympc_set_x0(g_solver.get(), x0_data, x0_cols);
}
int set_x_ref(double *x_ref_data, int x_ref_rows, int x_ref_cols, int verbose) {
    (void)verbose;
    if (need_global("set_x_ref")) return -1;
    if (x_ref_rows != g_solver->s.nx) {
        set_error("set_x_ref: wrong number of rows");
        return -1;
    }
    if (g_sharded) return guarded("set_x_ref", [&] { return tinympc_sharded_set_x_ref(g_sharded.get(), x_ref_data, x_ref_cols); });
    return tinympc_set_x_ref(g_solver.get(), x_ref_data, x_ref_cols);
}
int set_u_ref(double *u_ref_data, int u_ref_rows, int u_ref_cols, int verbose) {
    (void)verbose;
    if (need_global("set_u_ref")) return -1;
    if (u_ref_rows != g_solver->s.nu) {
        set_error("set_u_ref: wrong number of rows");
        return -1;
    }
    if (g_sharded) return guarded("set_u_ref", [&] { return tinympc_sharded_set_u_ref(g_sharded.get(), u_ref_data, u_ref_cols); });
    return tinympc_set_u_ref(g_solver.get(), u_ref_data, u_ref_cols);
}

int solve_mpc(int verbose) {
    if (need_global("solve_mpc")) return -1;
    const int st = g_sharded ? guarded("solve_mpc", [&] { return tinympc_sharded_solve(g_sharded.get()); })
                             : tinympc_solve(g_solver.get());
    if (verbose) std::printf("Solve completed with status: %d\n", st);
    return st;
}

int get_states(double *states_buffer, int *rows, int *cols) {
    if (!g_solver || !states_buffer || !rows || !cols) return -1;
    *rows = g_solver->s.nx;
    *cols = g_solver->s.N * global_batch();
    if (g_sharded) return guarded("get_states", [&] { return tinympc_sharded_get_states(g_sharded.get(), states_buffer); });
    return tinympc_get_states(g_solver.get(), states_buffer);
}
int get_controls(double *controls_buffer, int *rows, int *cols) {
    if (!g_solver || !controls_buffer || !rows || !cols) return -1;
    *rows = g_solver->s.nu;
    *cols = (g_solver->s.N - 1) * global_batch();
    if (g_sharded) return guarded("get_controls", [&] { return tinympc_sharded_get_controls(g_sharded.get(), controls_buffer); });
    return tinympc_get_controls(g_solver.get(), controls_buffer);
}

// fp32 forms of the three per-solve transfers for a Julia host that keeps Float32 arrays (not in bindings.cpp: an addition
// next to its names; one device only — a sharded global solver takes the fp64 forms)
int set_x0_f32(float *x0_data, int x0_rows, int x0_cols, int verbose) {
    (void)verbose;
    if (need_global("set_x0_f32")) return -1;
    if (x0_rows != g_solver->s.nx || g_sharded) {
        set_error(g_sharded ? "set_x0_f32: not available on a sharded solver" : "set_x0_f32: x0 is not the correct length");
        return -1;
    }
    return tinympc_set_x0_f32(g_solver.get(), x0_data, x0_cols);
}
int get_states_f32(float *states_buffer, int *rows, int *cols) {
    if (!g_solver || g_sharded || !states_buffer || !rows || !cols) return -1;
    *rows = g_solver->s.nx;
    *cols = g_solver->s.N * global_batch();
    return tinympc_get_states_f32(g_solver.get(), states_buffer);
}
int get_controls_f32(float *controls_buffer, int *rows, int *cols) {
    if (!g_solver || g_sharded || !controls_buffer || !rows || !cols) return -1;
    *rows = g_solver->s.nu;
    *cols = (g_solver->s.N - 1) * global_batch();
    return tinympc_get_controls_f32(g_solver.get(), controls_buffer);
}

// page-lock / release a host array the Julia caller owns and reuses with the fp32 forms (tinympc_pin_host); the caller
// unpins before the array can be collected
int pin_host_buffer(void *ptr, size_t bytes) {
    if (need_global("pin_host_buffer")) return -1;
    if (g_sharded) {
        set_error("pin_host_buffer: not available on a sharded solver");
        return -1;
    }
    return tinympc_pin_host(g_solver.get(), ptr, bytes);
}
int unpin_host_buffer(void *ptr) {
    if (need_global("unpin_host_buffer")) return -1;
    if (g_sharded) {
        set_error("unpin_host_buffer: not available on a sharded solver");
        return -1;
    }
    return tinympc_unpin_host(g_solver.get(), ptr);
}

void cleanup_solver(void) {
    g_sharded.reset();
    g_solver.reset();
}

int update_settings(double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                    int en_state_bound, int en_input_bound, int en_state_soc, int en_input_soc,
                    int en_state_linear, int en_input_linear, int adaptive_rho,
                    double adaptive_rho_min, double adaptive_rho_max,
                    int adaptive_rho_enable_clipping, int verbose) {
    (void)verbose;
    if (need_global("update_settings")) return -1;
    return each_global([&](tinympc_solver *h) -> int {
        tinympc_enable_cones(h, en_state_soc, en_input_soc);
        tinympc_enable_linear(h, en_state_linear, en_input_linear);
        if (tinympc_set_adaptive_rho(h, adaptive_rho, adaptive_rho_min, adaptive_rho_max, adaptive_rho_enable_clipping))
            return -1;
        return tinympc_update_settings(h, abs_pri_tol, abs_dua_tol, max_iter, check_termination, en_state_bound,
                                       en_input_bound);
    });
}

int set_bound_constraints(double *x_min_data, int x_min_rows, int x_min_cols, double *x_max_data,
                          int x_max_rows, int x_max_cols, double *u_min_data, int u_min_rows,
                          int u_min_cols, double *u_max_data, int u_max_rows, int u_max_cols,
                          int verbose) {
    (void)verbose;
    if (need_global("set_bound_constraints")) return -1;
    const tmpc::Solver &v = g_solver->s;
    // the batch dimension rides on the column counts, as set_x_ref's does: nx x (N*batch) with nu x ((N-1)*batch) is one bound
    // set per instance and knot ([batch][N][nx] / [batch][N-1][nu] in memory)
    const int gb = global_batch();
    const int xc[2] = {x_min_cols, x_max_cols}, uc[2] = {u_min_cols, u_max_cols};
    int wide = 0;
    for (int i = 0; i < 2; ++i) wide += (gb > 1 && (long)xc[i] == (long)v.N * gb) + (gb > 1 && (long)uc[i] == (long)(v.N - 1) * gb);
    if (wide > 0) {
        if (wide != 4 || x_min_rows != v.nx || x_max_rows != v.nx || u_min_rows != v.nu || u_max_rows != v.nu) {
            set_error("set_bound_constraints: mixed widths — per-instance bounds need all four arrays per instance (x_min, x_max nx x (N*batch) "
                      "and u_min, u_max nu x ((N-1)*batch)); shared bounds need nx x N and nu x (N-1)");
            return -1;
        }
        if (!x_min_data || !x_max_data || !u_min_data || !u_max_data) return -1;
        if (g_sharded) {
            if (g_solver->s.st.adaptive_rho) {
                set_error("set_bound_constraints: per-instance bounds are not available with adaptive rho");
                return -1;
            }
            g_solver->s.st.en_state_bound = g_solver->s.st.en_input_bound = 1;   // (the master keeps the family-level state)
            return guarded("set_bound_constraints", [&] {
                return tinympc_sharded_set_instance_bounds(g_sharded.get(), x_min_data, x_max_data, u_min_data, u_max_data, 1);
            });
        }
        return tinympc_set_instance_bounds(g_solver.get(), x_min_data, x_max_data, u_min_data, u_max_data, 1);
    }
    if (!dims_ok("x_min", x_min_rows, x_min_cols, v.nx, v.N) ||
        !dims_ok("x_max", x_max_rows, x_max_cols, v.nx, v.N) ||
        !dims_ok("u_min", u_min_rows, u_min_cols, v.nu, v.N - 1) ||
        !dims_ok("u_max", u_max_rows, u_max_cols, v.nu, v.N - 1))
        return -1;
    return each_global(
        [&](tinympc_solver *h) { return tinympc_set_bound_constraints(h, x_min_data, x_max_data, u_min_data, u_max_data); });
}

int set_cache_terms(double *Kinf_data, int Kinf_rows, int Kinf_cols, double *Pinf_data,
                    int Pinf_rows, int Pinf_cols, double *Quu_inv_data, int Quu_inv_rows,
                    int Quu_inv_cols, double *AmBKt_data, int AmBKt_rows, int AmBKt_cols,
                    int verbose) {
    (void)verbose;
    if (need_global("set_cache_terms")) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (!dims_ok("Kinf", Kinf_rows, Kinf_cols, v.nu, v.nx) ||
        !dims_ok("Pinf", Pinf_rows, Pinf_cols, v.nx, v.nx) ||
        !dims_ok("Quu_inv", Quu_inv_rows, Quu_inv_cols, v.nu, v.nu) ||
        !dims_ok("AmBKt", AmBKt_rows, AmBKt_cols, v.nx, v.nx))
        return -1;
    return each_global(
        [&](tinympc_solver *h) { return tinympc_set_cache_terms(h, Kinf_data, Pinf_data, Quu_inv_data, AmBKt_data); });
}

int set_sensitivity(double *dK_data, int dK_rows, int dK_cols, double *dP_data, int dP_rows, int dP_cols,
                    double *dC1_data, int dC1_rows, int dC1_cols, double *dC2_data, int dC2_rows, int dC2_cols,
                    int verbose) {
    (void)verbose;
    if (need_global("set_sensitivity")) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (!dims_ok("dK", dK_rows, dK_cols, v.nu, v.nx) || !dims_ok("dP", dP_rows, dP_cols, v.nx, v.nx) ||
        (dC1_data && !dims_ok("dC1", dC1_rows, dC1_cols, v.nu, v.nu)) ||
        (dC2_data && !dims_ok("dC2", dC2_rows, dC2_cols, v.nx, v.nx)))
        return -1;
    return each_global([&](tinympc_solver *h) { return tinympc_set_sensitivity(h, dK_data, dP_data, dC1_data, dC2_data); });
}

int get_adaptive_rho(double *rho_buffer, int *count) {
    if (need_global("get_adaptive_rho") || !rho_buffer || !count) return -1;
    *count = global_batch();
    if (g_sharded) {
        for (int i = 0; i < tinympc_sharded_n_shards(g_sharded.get()); ++i) {
            int lo = 0;
            tinympc_sharded_shard(g_sharded.get(), i, nullptr, &lo, nullptr, nullptr);
            if (tinympc_get_adaptive_state(global_shard(i), rho_buffer + lo, nullptr, nullptr)) return -1;
        }
        return 0;
    }
    return tinympc_get_adaptive_state(g_solver.get(), rho_buffer, nullptr, nullptr);
}

int print_problem_data(int verbose) {
    if (need_global("print_problem_data")) return -1;
    const tmpc::Solver &v = g_solver->s;
    std::printf("=== TinyMPC Problem Data ===\n");
    std::printf("Problem: nx=%d, nu=%d, N=%d, batch=%d, gpus=%d, kernel=%s\n", v.nx, v.nu, v.N, global_batch(), get_gpus(),
                (g_sharded ? global_shard(0)->s : v).kernel_name.c_str());
    std::printf("Cache: rho=%g\n", v.cache.rho);
    std::printf("Settings: max_iter=%d, abs_pri_tol=%g, abs_dua_tol=%g, check_termination=%d\n",
                v.st.max_iter, v.st.abs_pri_tol, v.st.abs_dua_tol, v.st.check_termination);
    if (verbose) {
        std::printf("Cache Kinf (%d x %d):\n", v.nu, v.nx);
        for (int i = 0; i < v.nu; ++i) {
            for (int j = 0; j < v.nx; ++j) std::printf(" %.10g", v.cache.Kinf(i, j));
            std::printf("\n");
        }
    }
    return 0;
}

int set_linear_constraints(double *Alin_x_data, int Alin_x_rows, int Alin_x_cols, double *blin_x_data,
                           int blin_x_len, double *Alin_u_data, int Alin_u_rows, int Alin_u_cols,
                           double *blin_u_data, int blin_u_len, int verbose) {
    (void)verbose;
    if (need_global("set_linear_constraints")) return -1;
    const tmpc::Solver &v = g_solver->s;
    // an empty side arrives as 0 x n (TinyMPC.jl:264 zeros(0, nu)); a non-empty one must match nx / nu
    const bool has_x = Alin_x_rows > 0 && blin_x_len > 0, has_u = Alin_u_rows > 0 && blin_u_len > 0;
    // the batch dimension rides on the widths, as set_bound_constraints' does: Alin_x rows_x x (nx*batch) with blin_x of
    // rows_x*batch entries is one row set per instance ([batch] blocks of rows_x x nx, [batch][rows_x] in memory)
    const int gb = global_batch();
    const bool wide_x = has_x && gb > 1 && (long)Alin_x_cols == (long)v.nx * gb, wide_u = has_u && gb > 1 && (long)Alin_u_cols == (long)v.nu * gb;
    if (wide_x || wide_u) {
        if ((has_x && !wide_x) || (has_u && !wide_u) || (has_x && (long)blin_x_len != (long)Alin_x_rows * gb) ||
            (has_u && (long)blin_u_len != (long)Alin_u_rows * gb)) {
            set_error("set_linear_constraints: mixed widths — per-instance rows need every non-empty side per instance (Alin_x m x (nx*batch) "
                      "with m*batch entries in blin_x, Alin_u m x (nu*batch) likewise); shared rows need m x nx and m x nu");
            return -1;
        }
        const int mx = has_x ? Alin_x_rows : 0, mu = has_u ? Alin_u_rows : 0;
        if (g_sharded) {
            if (g_solver->s.st.adaptive_rho) {
                set_error("set_linear_constraints: per-instance linear rows are not available with adaptive rho");
                return -1;
            }
            if (mx > 0) g_solver->s.st.en_state_linear = 1;   // (the master keeps the family-level state)
            if (mu > 0) g_solver->s.st.en_input_linear = 1;
            return guarded("set_linear_constraints", [&] {
                return tinympc_sharded_set_instance_linear(g_sharded.get(), Alin_x_data, mx, blin_x_data, Alin_u_data, mu, blin_u_data);
            });
        }
        return tinympc_set_instance_linear(g_solver.get(), Alin_x_data, mx, blin_x_data, Alin_u_data, mu, blin_u_data);
    }
    if ((has_x && (Alin_x_cols != v.nx || blin_x_len != Alin_x_rows)) ||
        (has_u && (Alin_u_cols != v.nu || blin_u_len != Alin_u_rows))) {
        set_error("set_linear_constraints: Alin_x must be (m x nx) with m entries in blin_x, Alin_u (m x nu) likewise");
        return -1;
    }
    return each_global([&](tinympc_solver *h) {
        return tinympc_set_linear_constraints(h, Alin_x_data, has_x ? Alin_x_rows : 0, blin_x_data, Alin_u_data,
                                              has_u ? Alin_u_rows : 0, blin_u_data);
    });
}

int set_cone_constraints(int *Acu_data, int Acu_len, int *qcu_data, int qcu_len, double *cu_data,
                         int cu_len, int *Acx_data, int Acx_len, int *qcx_data, int qcx_len,
                         double *cx_data, int cx_len, int verbose) {
    (void)verbose;
    if (need_global("set_cone_constraints")) return -1;
    if (Acu_len != qcu_len || Acx_len != qcx_len) {
        set_error("set_cone_constraints: Ac, qc and c of one side must have the same length");
        return -1;
    }
    // the batch dimension rides on the widths, as set_linear_constraints' does: cu of Acu_len*batch entries, [batch][cone] in
    // memory, is one coefficient set per instance (+inf: a cone the instance does not have)
    const int gb = global_batch();
    const bool has_u = Acu_len > 0, has_x = Acx_len > 0;
    const bool wide_u = has_u && gb > 1 && (long)cu_len == (long)Acu_len * gb, wide_x = has_x && gb > 1 && (long)cx_len == (long)Acx_len * gb;
    if (wide_u || wide_x) {
        if ((has_u && !wide_u) || (has_x && !wide_x)) {
            set_error("set_cone_constraints: mixed widths — per-instance cones need every non-empty side per instance (cu with n*batch entries "
                      "for n input cones, cx likewise); shared cones need n entries");
            return -1;
        }
        if (g_sharded) {
            if (g_solver->s.st.adaptive_rho) {
                set_error("set_cone_constraints: per-instance cones are not available with adaptive rho");
                return -1;
            }
            const int rc = guarded("set_cone_constraints", [&] {
                return tinympc_sharded_set_instance_cones(g_sharded.get(), Acu_data, qcu_data, cu_data, Acu_len, Acx_data, qcx_data, cx_data, Acx_len);
            });
            if (rc == 0) {
                // the master keeps the family-level state, which a later set_gpus / set_batch_size replays on fresh shards: the
                // per-instance coefficients replace whatever shared set it held and do not survive a re-batch, so it holds no cones
                g_solver->s.drop_instance_cones();
                g_solver->s.ncx = g_solver->s.ncu = 0;
                if (has_x) g_solver->s.st.en_state_soc = 1;
                if (has_u) g_solver->s.st.en_input_soc = 1;
            }
            return rc;
        }
        return tinympc_set_instance_cones(g_solver.get(), Acu_data, qcu_data, cu_data, Acu_len, Acx_data, qcx_data, cx_data, Acx_len);
    }
    if (Acu_len != cu_len || Acx_len != cx_len) {
        set_error("set_cone_constraints: Ac, qc and c of one side must have the same length");
        return -1;
    }
    // bindings.cpp:478-483: the flags of the non-empty halves are switched on
    return each_global([&](tinympc_solver *h) {
        return tinympc_set_cone_constraints(h, Acu_data, qcu_data, cu_data, Acu_len, Acx_data, qcx_data, cx_data, Acx_len);
    });
}

int get_status(int *iter, int *solved, double *residuals4) {
    if (need_global("get_status")) return -1;
    if (g_sharded) return guarded("get_status", [&] { return tinympc_sharded_get_status(g_sharded.get(), iter, solved, residuals4); });
    return tinympc_get_status(g_solver.get(), iter, solved, residuals4);
}
int reset_workspace(void) {
    if (need_global("reset_workspace")) return -1;
    return each_global([&](tinympc_solver *h) { return tinympc_reset(h); });
}
// The fused closed loop on the process-global solver (one device): what examples/cartpole_example_mpc.jl:35-51 and
// examples/rocket_landing_constraints.jl:97-134 do with one solve per host iteration, as one launch.
int set_ref_sequence(double *x_ref_seq, int x_rows, int x_cols, double *u_ref_seq, int u_rows, int u_cols, int steps) {
    if (need_global("set_ref_sequence")) return -1;
    if (g_sharded) {
        set_error("set_ref_sequence: not available on a sharded solver");
        return -1;
    }
    return tinympc_set_ref_sequence(g_solver.get(), x_ref_seq, x_rows, x_cols, u_ref_seq, u_rows, u_cols, steps);
}
// ... against a plant of its own and under a disturbance (tinympc_set_plant / tinympc_set_disturbance), shapes checked here
int set_plant(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols, double *f_data, int f_len, int per_instance) {
    if (need_global("set_plant")) return -1;
    if (g_sharded) {
        set_error("set_plant: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    const tmpc::Solver &v = g_solver->s;
    if (A_data || B_data) {
        const int n = per_instance ? v.batch : 1;
        if (!A_data || !B_data || (per_instance != 0 && per_instance != 1) || A_rows != v.nx || A_cols != v.nx * n || B_rows != v.nx ||
            B_cols != v.nu * n || (f_data && f_len != v.nx * n)) {
            set_error("set_plant: expected A nx x nx, B nx x nu, f nx (shared), or A nx x (nx batch), B nx x (nu batch), f nx batch (per instance); here nx = " +
                      std::to_string(v.nx) + ", nu = " + std::to_string(v.nu) + ", batch = " + std::to_string(v.batch));
            return -1;
        }
    }
    return tinympc_set_plant(g_solver.get(), A_data, B_data, f_data, per_instance);
}
int set_disturbance(double *w_data, int w_rows, int w_cols, int per_instance) {
    if (need_global("set_disturbance")) return -1;
    if (g_sharded) {
        set_error("set_disturbance: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    const tmpc::Solver &v = g_solver->s;
    if (!w_data || w_cols == 0) return tinympc_set_disturbance(g_solver.get(), nullptr, 0, 0);
    const int n = per_instance ? v.batch : 1;
    if ((per_instance != 0 && per_instance != 1) || w_rows != v.nx || w_cols < 0 || w_cols % n != 0) {
        set_error("set_disturbance: expected w nx x steps (shared) or nx x (steps batch) (per instance); here nx = " + std::to_string(v.nx) +
                  ", batch = " + std::to_string(v.batch));
        return -1;
    }
    return tinympc_set_disturbance(g_solver.get(), w_data, w_cols / n, per_instance);
}
int plant_mode(void) {
    if (need_global("plant_mode")) return -1;
    if (g_sharded) {
        set_error("plant_mode: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    return tinympc_plant_mode(g_solver.get());
}
// ... and under noise drawn on the device (tinympc_set_process_noise / _set_measurement_noise): G nx x nx column-major (shared) or
// nx x (nx batch), instance after instance; shapes checked here.  A sharded solver takes none of it.
static int need_unsharded(const char *what) {
    if (need_global(what)) return -1;
    if (g_sharded) {
        set_error(std::string(what) + ": not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    return 0;
}
static int set_noise_global(const char *what, int which, double *G_data, int G_rows, int G_cols, int per_instance, unsigned long long seed) {
    if (need_unsharded(what)) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (G_data && ((per_instance != 0 && per_instance != 1) || G_rows != v.nx || (long)G_cols != (long)v.nx * (per_instance ? v.batch : 1))) {
        set_error(std::string(what) + ": expected G nx x nx (per_instance 0) or nx x (nx batch) (per_instance 1); here nx = " + std::to_string(v.nx) +
                  ", batch = " + std::to_string(v.batch));
        return -1;
    }
    return which == tmpc::NOISE_PROCESS ? tinympc_set_process_noise(g_solver.get(), G_data, per_instance, seed)
                                        : tinympc_set_measurement_noise(g_solver.get(), G_data, per_instance, seed);
}
int set_process_noise(double *G_data, int G_rows, int G_cols, int per_instance, unsigned long long seed) {
    return set_noise_global("set_process_noise", tmpc::NOISE_PROCESS, G_data, G_rows, G_cols, per_instance, seed);
}
int set_measurement_noise(double *G_data, int G_rows, int G_cols, int per_instance, unsigned long long seed) {
    return set_noise_global("set_measurement_noise", tmpc::NOISE_MEASUREMENT, G_data, G_rows, G_cols, per_instance, seed);
}
int set_noise_cursor(int t) { return need_unsharded("set_noise_cursor") ? -1 : tinympc_set_noise_cursor(g_solver.get(), t); }
int noise_cursor(void) { return need_unsharded("noise_cursor") ? -1 : tinympc_noise_cursor(g_solver.get()); }
int noise_mode(void) { return need_unsharded("noise_mode") ? -1 : tinympc_noise_mode(g_solver.get()); }
int get_noise(int which, int t0, int steps, double *buf) { return need_unsharded("get_noise") ? -1 : tinympc_get_noise(g_solver.get(), which, t0, steps, buf); }
int get_mpc_measured(double *y) { return need_unsharded("get_mpc_measured") ? -1 : tinympc_get_mpc_measured(g_solver.get(), y); }
// ... and through a state estimator (tinympc_set_estimator): C ny x nx and L nx x ny column-major (shared), or ny x (nx batch) and
// nx x (ny batch), instance after instance; ny is C's row count; shapes checked here
int set_estimator(double *C_data, int C_rows, int C_cols, double *L_data, int L_rows, int L_cols, int per_instance) {
    if (need_unsharded("set_estimator")) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (!C_data && !L_data) return tinympc_set_estimator(g_solver.get(), nullptr, 0, nullptr, 0);
    const long n = per_instance ? v.batch : 1;
    if (C_data && L_data && ((per_instance != 0 && per_instance != 1) || (long)C_cols != (long)v.nx * n || L_rows != v.nx || (long)L_cols != (long)C_rows * n)) {
        set_error("set_estimator: expected C ny x nx and L nx x ny (per_instance 0), or ny x (nx batch) and nx x (ny batch) (per_instance 1); here nx = " +
                  std::to_string(v.nx) + ", batch = " + std::to_string(v.batch));
        return -1;
    }
    return tinympc_set_estimator(g_solver.get(), C_data, C_rows, L_data, per_instance);
}
// One family per instance on the global solver (julia/TinyMPC.jl: setup_families, set_families!, family_cache): the handle
// entry points behind the process-global one.  A (nx, nx batch), B (nx, nu batch), Q (nx, nx batch), R (nu, nu batch): the
// handle API's [batch] blocks seen as one column-major matrix; rho [batch].
int setup_families(double *A_data, int A_rows, int A_cols, double *B_data, int B_rows, int B_cols, double *Q_data, int Q_rows, int Q_cols,
                   double *R_data, int R_rows, int R_cols, double *rho_data, int rho_len, int nx, int nu, int N, int batch, int on_device,
                   int verbose) {
    return guarded("setup_families", [&]() -> int {
        if (!A_data || !B_data || !Q_data || !R_data || !rho_data || batch < 1 || A_rows != nx || (long)A_cols != (long)nx * batch || B_rows != nx ||
            (long)B_cols != (long)nu * batch || Q_rows != nx || (long)Q_cols != (long)nx * batch || R_rows != nu || (long)R_cols != (long)nu * batch ||
            rho_len != batch) {
            set_error("setup_families: expected A (nx, nx batch), B (nx, nu batch), Q (nx, nx batch), R (nu, nu batch) and rho of batch entries");
            return -1;
        }
        g_sharded.reset();
        tinympc_solver *s = nullptr;
        if ((on_device ? tinympc_create_families_device : tinympc_create_families)(&s, A_data, B_data, Q_data, R_data, rho_data, nx, nu, N, batch, -1,
                                                                                verbose)) {
            g_solver.reset();
            return -1;
        }
        g_solver.reset(s);   // (a second setup replaces the first, as setup_solver's does)
        return 0;
    });
}
int set_families(double *A_data, double *B_data, double *Q_data, double *R_data, double *rho_data) {
    return need_unsharded("set_families") ? -1 : tinympc_set_families(g_solver.get(), A_data, B_data, Q_data, R_data, rho_data);
}
int get_family_cache(int first, int count, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps) {
    return need_unsharded("get_family_cache") ? -1 : tinympc_get_family_cache(g_solver.get(), first, count, Kinf, Pinf, Quu_inv, AmBKt, sweeps);
}
int families_setup_mode(void) { return need_unsharded("families_setup_mode") ? -1 : tinympc_families_setup_mode(g_solver.get()); }
int set_estimator_state(double *xhat_data, int xhat_rows, int xhat_cols) {
    if (need_unsharded("set_estimator_state")) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (!xhat_data) return tinympc_set_estimator_state(g_solver.get(), nullptr, 0);
    if (xhat_rows != v.nx || (xhat_cols != 1 && xhat_cols != v.batch)) {
        set_error("set_estimator_state: expected xhat nx x 1 (shared) or nx x batch; here nx = " + std::to_string(v.nx) + ", batch = " + std::to_string(v.batch));
        return -1;
    }
    return tinympc_set_estimator_state(g_solver.get(), xhat_data, xhat_cols == v.batch && v.batch > 1 ? 1 : 0);
}
int estimator_mode(void) { return need_unsharded("estimator_mode") ? -1 : tinympc_estimator_mode(g_solver.get()); }
int estimator_outputs(void) { return need_unsharded("estimator_outputs") ? -1 : tinympc_estimator_outputs(g_solver.get()); }
int get_estimator_state(double *xhat) { return need_unsharded("get_estimator_state") ? -1 : tinympc_get_estimator_state(g_solver.get(), xhat); }
int get_mpc_estimate(double *xhat) { return need_unsharded("get_mpc_estimate") ? -1 : tinympc_get_mpc_estimate(g_solver.get(), xhat); }
int get_mpc_outputs(double *y) { return need_unsharded("get_mpc_outputs") ? -1 : tinympc_get_mpc_outputs(g_solver.get(), y); }
// ... and scored on the device (tinympc_set_rollout_metrics): the weights ride with their lengths, which are checked here
int set_rollout_metrics(int enable, double *qw_data, int qw_len, double *rw_data, int rw_len, double *x_lo, double *x_hi, double *u_lo, double *u_hi) {
    if (need_unsharded("set_rollout_metrics")) return -1;
    const tmpc::Solver &v = g_solver->s;
    if (enable && ((qw_data && qw_len != v.nx) || (rw_data && rw_len != v.nu))) {
        set_error("set_rollout_metrics: expected qw of nx and rw of nu weights (or none: the diagonal of Q / R); here nx = " + std::to_string(v.nx) +
                  ", nu = " + std::to_string(v.nu));
        return -1;
    }
    return tinympc_set_rollout_metrics(g_solver.get(), enable, qw_data, rw_data, x_lo, x_hi, u_lo, u_hi);
}
int reset_rollout_metrics(void) { return need_unsharded("reset_rollout_metrics") ? -1 : tinympc_reset_rollout_metrics(g_solver.get()); }
int get_rollout_metrics(double *per_instance) { return need_unsharded("get_rollout_metrics") ? -1 : tinympc_get_rollout_metrics(g_solver.get(), per_instance); }
int get_rollout_summary(double *summary) { return need_unsharded("get_rollout_summary") ? -1 : tinympc_get_rollout_summary(g_solver.get(), summary); }
// ... and along a reference trajectory (tinympc_set_ref_trajectory): x nx x Lx and u nu x Lu column-major (shared), or
// nx x (Lx batch) and nu x (Lu batch), instance after instance — the batch rides on the column count; shapes checked here
int set_ref_trajectory(double *x_data, int x_rows, int x_cols, double *u_data, int u_rows, int u_cols, int per_instance, int verbose) {
    (void)verbose;
    if (need_global("set_ref_trajectory")) return -1;
    if (g_sharded) {
        set_error("set_ref_trajectory: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    const tmpc::Solver &v = g_solver->s;
    if (!x_data) return tinympc_set_ref_trajectory(g_solver.get(), nullptr, 0, nullptr, 0, 0);
    const int n = per_instance ? v.batch : 1;
    if ((per_instance != 0 && per_instance != 1) || x_rows != v.nx || x_cols < 1 || x_cols % n != 0 ||
        (u_data && (u_rows != v.nu || u_cols < 1 || u_cols % n != 0))) {
        set_error("set_ref_trajectory: expected x_traj nx x Lx and u_traj nu x Lu (shared), or nx x (Lx batch) and nu x (Lu batch) (per instance), Lx, Lu >= 1; here nx = " +
                  std::to_string(v.nx) + ", nu = " + std::to_string(v.nu) + ", batch = " + std::to_string(v.batch));
        return -1;
    }
    return tinympc_set_ref_trajectory(g_solver.get(), x_data, x_cols / n, u_data, u_data ? u_cols / n : 0, per_instance);
}
int set_ref_cursor(int cursor) {
    if (need_global("set_ref_cursor")) return -1;
    if (g_sharded) {
        set_error("set_ref_cursor: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    return tinympc_set_ref_cursor(g_solver.get(), cursor);
}
int ref_cursor(void) {
    if (need_global("ref_cursor")) return -1;
    if (g_sharded) {
        set_error("ref_cursor: not available on a sharded solver (which has no mpc_rollout)");
        return -1;
    }
    return tinympc_ref_cursor(g_solver.get());
}
int mpc_rollout(int steps, double *x_log, double *u_log, int *iter_log) {
    if (need_global("mpc_rollout")) return -1;
    if (g_sharded) {
        set_error("mpc_rollout: not available on a sharded solver");
        return -1;
    }
    const int st = tinympc_mpc_rollout(g_solver.get(), steps, nullptr);
    if (st < 0) return -1;
    if ((x_log || u_log || iter_log) && tinympc_get_mpc_log(g_solver.get(), x_log, u_log, iter_log)) return -1;
    return st;
}

}  // extern "C"
