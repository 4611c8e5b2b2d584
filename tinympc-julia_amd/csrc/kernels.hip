// Kernel table, generic-kernel launcher and its host-side pack builders.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>

#include "admm_generic.hip.h"
#include "host_setup.h"
#include "solver.h"

namespace tmpc {

// Shapes with a specialised kernel: the BASELINE.json configs plus the shapes the
// reference's own tests/examples use (tests/test_basic.jl N=10, test_settings.jl N=2,
// examples/*: cartpole N=20, quadrotor N=20, rocket N=10).
// Table order = preference: the first entry matching (nx, nu, N) is the shape's default variant.
#define TMPC_ENTRY(NX, NU, NN, GG) const KernelEntry *quad_entry_##NX##_##NU##_##NN##_g##GG();
TMPC_ENTRY(4, 1, 20, 4) TMPC_ENTRY(4, 1, 20, 2) TMPC_ENTRY(4, 1, 20, 1)
TMPC_ENTRY(4, 1, 10, 4) TMPC_ENTRY(4, 1, 10, 2) TMPC_ENTRY(4, 1, 10, 1) TMPC_ENTRY(4, 1, 2, 4)
TMPC_ENTRY(4, 1, 5, 4) TMPC_ENTRY(4, 1, 5, 1) TMPC_ENTRY(4, 1, 15, 4) TMPC_ENTRY(4, 1, 15, 1) TMPC_ENTRY(4, 1, 30, 4) TMPC_ENTRY(4, 1, 30, 1)
TMPC_ENTRY(12, 4, 30, 4) TMPC_ENTRY(12, 4, 20, 4)
TMPC_ENTRY(6, 3, 10, 4) TMPC_ENTRY(6, 3, 10, 2) TMPC_ENTRY(6, 3, 50, 4)
#undef TMPC_ENTRY

const KernelEntry *find_quad_kernel(int nx, int nu, int N, int group) {
    static const KernelEntry *const table[] = {
        quad_entry_4_1_20_g4(),  quad_entry_4_1_20_g2(),  quad_entry_4_1_20_g1(), quad_entry_4_1_10_g4(),
        quad_entry_4_1_10_g2(),  quad_entry_4_1_10_g1(),  quad_entry_4_1_2_g4(),  quad_entry_12_4_30_g4(),
        quad_entry_12_4_20_g4(), quad_entry_6_3_10_g4(),  quad_entry_6_3_10_g2(), quad_entry_6_3_50_g4(),
        // further cartpole horizons (tests/test_codegen.jl:15 uses N = 5): without them these fall to the HBM-streaming kernel
        quad_entry_4_1_5_g4(),   quad_entry_4_1_5_g1(),   quad_entry_4_1_15_g4(), quad_entry_4_1_15_g1(),
        quad_entry_4_1_30_g4(),  quad_entry_4_1_30_g1(),
    };
    for (const KernelEntry *e : table)
        if (e->nx == nx && e->nu == nu && e->N == N && (group < 0 || e->G == group)) return e;
    return jit_find(false, nx, nu, N, group);   // ... or one specialised at setup (jit.cpp)
}

const KernelEntry *mfma_entry_12_4_30();
const KernelEntry *mfma_entry_12_4_25();
const KernelEntry *mfma_entry_12_4_20();
const KernelEntry *mfma_entry_12_4_15();
const KernelEntry *mfma_entry_12_4_10();

// matrix-core kernels (admm_mfma.hip.h): one-shot solves of the shapes instantiated.  The kernel is fully unrolled with its
// state in registers: rocket N=50 (347 state floats per lane with finite state bounds) spills ~1 000 registers and runs
// 18 ms against the quad kernel's 5.5, and rocket N=10 fills only 9 of a tile's 16 rows (1.13 ms against 0.74):
// neither is instantiated.  Quadrotor ([A; -Kinf] is a full 16 x 12): N=30 4.13 against 11.6 ms, N=20 2.7 against 5.9
const KernelEntry *find_mfma_kernel(int nx, int nu, int N) {
    static const KernelEntry *const table[] = {mfma_entry_12_4_30(), mfma_entry_12_4_25(), mfma_entry_12_4_20(), mfma_entry_12_4_15(),
                                               mfma_entry_12_4_10()};
    for (const KernelEntry *e : table)
        if (e->nx == nx && e->nu == nu && e->N == N) return e;
    return jit_find(true, nx, nu, N, -1);   // ... or one specialised at setup (jit.cpp)
}

const LeanEntry *lean_entry_4_1_20();
const LeanEntry *lean_entry_4_1_15();
const LeanEntry *lean_entry_4_1_10();
const LeanEntry *lean_entry_4_1_5();

const LeanEntry *find_lean_kernel(int nx, int nu, int N) {
    static const LeanEntry *const table[] = {lean_entry_4_1_20(), lean_entry_4_1_15(), lean_entry_4_1_10(), lean_entry_4_1_5()};
    for (const LeanEntry *e : table)
        if (e->nx == nx && e->nu == nu && e->N == N) return e;
    return nullptr;
}

// The diagonal scaling x^ = S x under which a kernel of the scaled pattern lean_pattern_scaled(built) computes the model
// (A [nx][nx], B [nx][nu], row-major): each chosen entry A^[i][j] = s_i A[i][j] / s_j = 1 fixes a ratio along the forest of
// chosen entries (a component's root has s = 1), B's unit the scale of its component.  Returns the scaled pattern and fills
// s [nx], or 0 — the launch then keeps the unscaled sparse kernel — where `built` does not cover the model, a chosen entry is
// zero in it (the ratio does not exist), or the scaled sweeps cost no less than the sparse ones.
uint64_t lean_scale_model(uint64_t built, int nx, int nu, const double *A, const double *B, double *s) {
    const uint64_t sz = lean_pattern_scaled(built, nx, nu);
    if (!sz || !lean_pattern_covers(built, lean_pattern_rm(nx, nu, A, B))) return 0;
    if (lean_cost_scaled(sz, nx, nu) >= lean_cost_sparse(built, nx, nu)) return 0;
    bool known[4] = {false, false, false, false};
    int comp[4] = {0, 1, 2, 3};
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j)
            if (i != j && lsp_one(sz, nx, i, j)) {
                if (A[i * nx + j] == 0.0) return 0;
                const int ci = comp[i], cj = comp[j];
                for (int q = 0; q < nx; ++q)
                    if (comp[q] == cj) comp[q] = ci;
            }
    for (int r = 0; r < nx; ++r) {
        if (known[r]) continue;
        s[r] = 1.0, known[r] = true;                                     // the root of a component not reached yet
        for (int pass = 0; pass < nx; ++pass)
            for (int i = 0; i < nx; ++i)
                for (int j = 0; j < nx; ++j) {
                    if (i == j || !lsp_one(sz, nx, i, j)) continue;
                    if (known[j] && !known[i]) s[i] = s[j] / A[i * nx + j], known[i] = true;
                    else if (known[i] && !known[j]) s[j] = s[i] * A[i * nx + j], known[j] = true;
                }
    }
    for (int i = 0; i < nx; ++i)
        for (int a = 0; a < nu; ++a)
            if (lsp_b_one(sz, nu, i, a)) {
                if (B[i * nu + a] == 0.0) return 0;
                const double f = 1.0 / (B[i * nu + a] * s[i]);
                for (int q = 0; q < nx; ++q)
                    if (comp[q] == comp[i]) s[q] *= f;
            }
    for (int i = 0; i < nx; ++i)
        if (!std::isfinite(s[i]) || s[i] == 0.0 || !std::isfinite(1.0 / (s[i] * s[i]))) return 0;
    return sz;
}
// ... and the scaled model's coefficients: A^ = S A S^-1 and B^ = S B with exact units where sz says so, K^ = Kinf S^-1
void lean_scaled_coefficients(uint64_t sz, int nx, int nu, const double *A, const double *B, const double *K, const double *s,
                              double *Ah, double *Bh, double *Kh) {
    for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j)
            Ah[i * nx + j] = i == j ? A[i * nx + j] : (lsp_one(sz, nx, i, j) ? 1.0 : s[i] * A[i * nx + j] / s[j]);
        for (int a = 0; a < nu; ++a) Bh[i * nu + a] = lsp_b_one(sz, nu, i, a) ? 1.0 : s[i] * B[i * nu + a];
    }
    if (K && Kh)
        for (int a = 0; a < nu; ++a)
            for (int j = 0; j < nx; ++j) Kh[a * nx + j] = K[a * nx + j] / s[j];
}
// ... and the pack's scaled block z = [A^, K^, B^, C, w] (admm_params.h: LeanLayout, oM .. oW relative to it) of the model's
// A, B, Kinf and C = -rho Quu_inv.  w = diag(S)^-2 — and, at nu = 1, c diag(S)^-2 with the scalar c = C: the kernel then carries
// the costate as c p^ and never multiplies by C (admm_lean.hip.h: FOLD; C itself stays in the block, the product c r~ reads it).
// false — the launch keeps the unscaled kernel — where a w is not finite, or at nu = 1 zero (c = 0: no such scale)
bool lean_scaled_block(uint64_t sz, int nx, int nu, const double *A, const double *B, const double *K, const double *C, const double *s,
                       double *z) {
    const LeanLayout L = lean_layout(nx, nu);
    lean_scaled_coefficients(sz, nx, nu, A, B, K, s, z + L.oM, z + L.oB, z + L.oK);
    for (int i = 0; i < nu * nu; ++i) z[L.oC + i] = C[i];
    for (int i = 0; i < nx; ++i) {
        z[L.oW + i] = nu == 1 ? C[0] / (s[i] * s[i]) : 1.0 / (s[i] * s[i]);
        if (!std::isfinite(z[L.oW + i]) || (nu == 1 && z[L.oW + i] == 0.0)) return false;
    }
    return true;
}

bool build_lean_pack(const Solver &sv, std::vector<double> &out, bool *scaled) {
    const int nx = sv.nx, nu = sv.nu;
    if (scaled) *scaled = false;
    const LeanLayout L = lean_layout(nx, nu);
    out.assign((size_t)L.total, 0.0);
    const Cache &c = sv.cache;
    // the kernel reads ONE matrix as A - B Kinf (rollout) and, transposed, as AmBKt (gradient recursion): only valid while
    // the cache's AmBKt is that transpose (tiny_api.cpp:170; set_cache_terms can install anything)
    double scale = 0.0, diff = 0.0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            double m = sv.A(i, j);
            for (int a = 0; a < nu; ++a) m -= sv.B(i, a) * c.Kinf(a, j);
            out[L.oM + i * nx + j] = m;
            scale = std::max(scale, std::fabs(m));
            diff = std::max(diff, std::fabs(m - c.AmBKt(j, i)));
        }
    if (!(diff <= 1e-12 * std::max(scale, 1.0))) return false;
    for (int i = 0; i < nx; ++i)      // (bit for bit the cache's own values where the two agree to rounding)
        for (int j = 0; j < nx; ++j) out[L.oM + i * nx + j] = c.AmBKt(j, i);
    for (int a = 0; a < nu; ++a)
        for (int j = 0; j < nx; ++j) out[L.oK + a * nx + j] = c.Kinf(a, j);
    for (int i = 0; i < nx; ++i)
        for (int a = 0; a < nu; ++a) out[L.oB + i * nu + a] = sv.B(i, a);
    for (int a = 0; a < nu; ++a)
        for (int b2 = 0; b2 < nu; ++b2) out[L.oC + a * nu + b2] = -c.rho * c.Quu_inv(a, b2);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) out[L.oP + i * nx + j] = c.Pinf(i, j);
    // the same coefficients in controller-Hessenberg coordinates x = T x^ (T orthogonal): M^ = T' M T, b^ = T' B, k^ = Kinf T;
    // the input-space C does not change
    std::vector<double> Mh((size_t)nx * nx), Bh((size_t)nx * nu);
    staircase_form(nx, nu, out.data() + L.oM, out.data() + L.oB, out.data() + L.oT, Mh.data(), Bh.data());
    const double *T = out.data() + L.oT;
    for (int i = 0; i < nx * nx; ++i) out[L.oH + L.oM + i] = Mh[i];
    for (int i = 0; i < nx * nu; ++i) out[L.oH + L.oB + i] = Bh[i];
    for (int a = 0; a < nu; ++a)
        for (int j = 0; j < nx; ++j) {
            double s = 0.0;
            for (int l = 0; l < nx; ++l) s += c.Kinf(a, l) * T[l * nx + j];
            out[L.oH + L.oK + a * nx + j] = s;
        }
    for (int i = 0; i < nu * nu; ++i) out[L.oH + L.oC + i] = out[L.oC + i];
    // the sparse variants' block: the model's A where M is, Kinf, B and C as in the plain one
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) out[L.oS + L.oM + i * nx + j] = sv.A(i, j);
    for (int i = L.oK; i < L.len; ++i) out[L.oS + i] = out[i];
    // the scaled block, where the built-in entry has kernels of its scaled pattern and this model takes them
    if (sv.le && sv.le->sp_scaled && nx <= 4 && nu <= 4) {
        double s[4];
        const uint64_t sz = lean_scale_model(sv.le->sp, nx, nu, out.data() + L.oS + L.oM, out.data() + L.oS + L.oB, s);
        if (sz && sz == sv.le->sp_scaled) {
            const bool ok = lean_scaled_block(sz, nx, nu, out.data() + L.oS + L.oM, out.data() + L.oS + L.oB, out.data() + L.oS + L.oK,
                                              out.data() + L.oC, s, out.data() + L.oZ);
            for (int i = 0; i < nx; ++i) {
                out[L.oSc + i] = s[i];
                out[L.oSi + i] = 1.0 / s[i];
            }
            if (scaled) *scaled = ok;
        }
    }
    return true;
}

// The one-lane-per-instance bound pack — [knot][x_min x_max u_min u_max], then diag(Q) + rho, diag(R) + rho (quad_entry.hip.h:
// build_quad_bounds with G = 1) — behind the coefficient doubles of `out`, for a solver whose selected entry keeps its bounds
// in another layout (four lanes per instance, the stream kernel's): launch_pass points P.bounds there
void append_lean_bounds(const Solver &sv, std::vector<double> &out) {
    constexpr float kInf = std::numeric_limits<float>::infinity();
    const int nx = sv.nx, nu = sv.nu, N = sv.N, BW = 2 * nx + 2 * nu;
    std::vector<float> lb((size_t)N * BW + nx + nu + 1, 0.f);
    for (int k = 0; k < N; ++k) {
        float *p = lb.data() + (size_t)k * BW;
        for (int r = 0; r < nx; ++r) {
            p[r] = sv.st.en_state_bound ? (float)sv.x_min[r + (size_t)k * nx] : -kInf;
            p[nx + r] = sv.st.en_state_bound ? (float)sv.x_max[r + (size_t)k * nx] : kInf;
        }
        for (int a = 0; a < nu; ++a) {
            const bool on = sv.st.en_input_bound && k < N - 1;
            p[2 * nx + a] = on ? (float)sv.u_min[a + (size_t)k * nu] : -kInf;
            p[2 * nx + nu + a] = on ? (float)sv.u_max[a + (size_t)k * nu] : kInf;
        }
    }
    for (int r = 0; r < nx; ++r) lb[(size_t)N * BW + r] = (float)sv.cache.Qd[r];
    for (int a = 0; a < nu; ++a) lb[(size_t)N * BW + nx + a] = (float)sv.cache.Rd[a];
    const size_t at = out.size();
    out.resize(at + (lb.size() + 1) / 2, 0.0);
    std::memcpy(out.data() + at, lb.data(), lb.size() * sizeof(float));
}

// The lean kernel takes the launches of a one-lane-per-instance quad entry (fp64 recurrences, fp32 state), or — precision 2, no
// quad entry — of a shape it holds in its fp64-state form, when the family's pack qualifies, the references are zero or shared,
// rho is the family's, every slot is an instance and there is an iteration to run:
//   one-shot solves (cold start, nothing of the workspace kept): always;
//   every other solve: TINYMPC_HIP_LEAN_WS, on the workspace-keeping form (fp32 state only), where the entry has it or a
//     specialised variant fits the LDS (lean_ws_fits) — a shape beyond it stays on its quad kernel, fused closed loop included;
//   mpc_steps in one launch: TINYMPC_HIP_LEAN_LOOP beside it and the caller asking for the loop (in.loop), which in turn
//     gets the loop kernel or nothing.
// The variant then follows, every normalisation once:
//   XB    a finite state bound, or a kept workspace whose state dual may hold something (the kernels without a state bound
//         take g for zero; the state-bounded form's clamps then clamp nothing);
//   LIVE  positive tolerances; every in-kernel loop; the WS pattern XB + shared references + per-knot input bounds, whose
//         fixed-iteration kernel is not built (lean_entry.hip.h);
//   ONE   the 512-register form: at most one workgroup per CU (= one wavefront per SIMD); every LIVE, WS and fp64-state
//         kernel; TINYMPC_HIP_LEAN_ONE; a specialised shape the 256-register form does not hold.  (Fixed-iteration solves of
//         batch 131 072 in the 256- / 512-register form: 0.46 / 0.69 against 0.47 / 0.61 ms — scripts/lean_time.py "big")
//   SPARSE where a kernel's (A, B) pattern covers the model's and costs less per knot than the dense form it replaces
//         (lean_pick_form; TINYMPC_HIP_LEAN_DENSE: never).  The built-in sparse kernels take zero references and uniform
//         input bounds; a specialised variant carries the model's own pattern, any calling pattern.
LeanPlan lean_plan(const LeanPlanIn &in) {
    LeanPlan p;
    const int nx = in.nx, nu = in.nu, N = in.N;
    const bool f64 = in.precision == 2 && in.quad_G == 0 && in.lean_jit && !in.stream_ext;
    if (!(in.quad_G ? in.precision == 0 : f64) || !in.lean_ok || !(in.builtin || in.lean_jit)) return p;
    if (in.indexed || in.ref_mode == REF_PER_INSTANCE || in.adaptive_rho || in.iters < 1) return p;
    const bool ws = !(in.cold && !in.save);
    if (ws && !(in.sw_ws && in.quad_G > 0 && in.quad_G < 16 && in.precision == 0 && (!in.builtin || (in.kinds & LK_WS)))) return p;
    const bool mpc = in.loop && in.sw_loop && ws && in.mpc_steps > 0;
    if ((in.loop || in.mpc_steps > 0) && !mpc) return p;
    const bool xb = in.state_bounds || (ws && in.g_maybe_nonzero), shared = in.ref_mode == REF_SHARED;
    const bool live = in.live || mpc || (ws && xb && shared && in.knot_bounds);
    const bool one = live || ws || f64 || in.sw_one || (in.slots + 255) / 256 <= in.cus ||
                     (!in.builtin && 2 * N * nx + 3 * N * nu + 50 > 250);
    if (ws && !in.builtin && !lean_ws_fits(nx, nu, N, live, xb, shared, in.knot_bounds)) return p;
    bool sparse_allowed = !in.sw_dense;
    p.sp = in.model_sp;
    if (in.builtin) {
        const bool has = (in.kinds & (mpc ? LK_SPARSE_MPC : (ws ? LK_SPARSE_WS : LK_SPARSE))) != 0;
        p.sp = has ? in.builtin_sp : 0;
        sparse_allowed = sparse_allowed && has && in.ref_mode == REF_ZERO && !in.knot_bounds;
    }
    p.form = lean_pick_form(nx, nu, p.sp, in.model_sp, one, live, xb, sparse_allowed);
    if (mpc && in.builtin && !(in.kinds & (p.form == LF_SPARSE ? LK_SPARSE_MPC : LK_MPC))) return LeanPlan();
    p.take = true;
    p.variant = (live ? LV_LIVE : 0) | (in.knot_bounds ? 0 : LV_UBK) | (one ? LV_ONE : 0) | (xb ? LV_XB : 0) | (shared ? LV_SHARED : 0) |
                (f64 ? LV_F64 : 0) | (p.form == LF_SPARSE ? LV_SPARSE : 0) | (ws ? LV_WS : 0) | (mpc ? LV_MPC : 0);
    p.cost_sparse = p.sp ? lean_cost_sparse(p.sp, nx, nu) : 0;
    p.cost_dense = (one && !live && !xb) ? lean_cost_hessenberg(nx, nu) : lean_cost_dense(nx, nu);
    return p;
}

uint64_t lean_pattern(const Mat &A, const Mat &B) {
    const int nx = A.r, nu = B.c;
    if (nx < 1 || nu < 1 || nx > 4 || nu > 4) return 0;
    double a[16], b[16];
    for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j) a[i * nx + j] = A(i, j);
        for (int c = 0; c < nu; ++c) b[i * nu + c] = B(i, c);
    }
    return lean_pattern_rm(nx, nu, a, b);
}

}  // namespace tmpc

// (test hooks, not part of the public boundary include/tinympc_hip.h: the lean kernel's routing, lean_plan)
// the pattern of row-major A [nx][nx], B [nx][nu]; the per-knot fp64 costs {sparse of sp, Hessenberg, dense}; the coverage
// rule; the form a launch would take; the pattern of the built-in entry of a shape (0: none, or no sparse kernels)
extern "C" unsigned long long tmpc_lean_pattern(int nx, int nu, const double *A, const double *B) {
    return (A && B) ? tmpc::lean_pattern_rm(nx, nu, A, B) : 0;
}
extern "C" int tmpc_lean_costs(int nx, int nu, unsigned long long sp, int *out3) {
    if (nx < 1 || nu < 1 || nx > 4 || nu > 4 || !out3) return 1;
    out3[0] = tmpc::lean_cost_sparse(sp, nx, nu), out3[1] = tmpc::lean_cost_hessenberg(nx, nu), out3[2] = tmpc::lean_cost_dense(nx, nu);
    return 0;
}
// the scaled pattern of a pattern (admm_params.h: lean_pattern_scaled) and its per-knot fp64 cost; the scaling a kernel of
// lean_pattern_scaled(built) takes a model under (built = 0: the model's own pattern) — returns the scaled pattern, 0 where the
// model keeps the unscaled sweeps, and fills s [nx], A^ [nx][nx], B^ [nx][nu]
extern "C" unsigned long long tmpc_lean_scaled_pattern(int nx, int nu, unsigned long long sp) { return tmpc::lean_pattern_scaled(sp, nx, nu); }
extern "C" int tmpc_lean_scaled_cost(int nx, int nu, unsigned long long sz) {
    return (nx < 1 || nu < 1 || nx > 4 || nu > 4 || !tmpc::lsp_scaled(sz)) ? -1 : tmpc::lean_cost_scaled(sz, nx, nu);
}
extern "C" unsigned long long tmpc_lean_scale_model(int nx, int nu, const double *A, const double *B, unsigned long long built, double *s,
                                                    double *Ah, double *Bh) {
    if (nx < 1 || nu < 1 || nx > 4 || nu > 4 || !A || !B || !s || !Ah || !Bh) return 0;
    if (!built) built = tmpc::lean_pattern_rm(nx, nu, A, B);
    const uint64_t sz = tmpc::lean_scale_model(built, nx, nu, A, B, s);
    if (sz) tmpc::lean_scaled_coefficients(sz, nx, nu, A, B, nullptr, s, Ah, Bh, nullptr);
    return sz;
}
// the per-knot fp64 cost of the form the scaled kernels run (admm_params.h: lean_cost_folded); the scaled block [A^, K^, B^, C, w]
// build_lean_pack writes for a model — row-major A, B, Kinf [nu][nx], C = -rho Quu_inv [nu][nu] — under the kernel of
// lean_pattern_scaled(built) (built = 0: the model's own pattern): returns its length nx nx + 2 nu nx + nu nu + nx and fills
// out, 0 where the model keeps the unscaled sweeps, -1 on bad arguments or cap too small
extern "C" int tmpc_lean_folded_cost(int nx, int nu, unsigned long long sz) {
    return (nx < 1 || nu < 1 || nx > 4 || nu > 4 || !tmpc::lsp_scaled(sz)) ? -1 : tmpc::lean_cost_folded(sz, nx, nu);
}
extern "C" int tmpc_lean_scaled_block(int nx, int nu, const double *A, const double *B, const double *K, const double *C,
                                      unsigned long long built, double *out, int cap) {
    if (nx < 1 || nu < 1 || nx > 4 || nu > 4 || !A || !B || !K || !C || !out) return -1;
    const tmpc::LeanLayout L = tmpc::lean_layout(nx, nu);
    if (cap < L.len + nx) return -1;
    if (!built) built = tmpc::lean_pattern_rm(nx, nu, A, B);
    double s[4];
    const uint64_t sz = tmpc::lean_scale_model(built, nx, nu, A, B, s);
    if (!sz || !tmpc::lean_scaled_block(sz, nx, nu, A, B, K, C, s, out)) return 0;
    return L.len + nx;
}
extern "C" int tmpc_lean_covers(unsigned long long built, unsigned long long model) { return tmpc::lean_pattern_covers(built, model) ? 1 : 0; }
extern "C" int tmpc_lean_pick_form(int nx, int nu, unsigned long long built, unsigned long long model, int one, int live, int xb) {
    return tmpc::lean_pick_form(nx, nu, built, model, one != 0, live != 0, xb != 0, true);
}
extern "C" unsigned long long tmpc_lean_builtin_pattern(int nx, int nu, int N) {
    const tmpc::LeanEntry *e = tmpc::find_lean_kernel(nx, nu, N);
    return (e && (e->kinds & tmpc::LK_SPARSE)) ? e->sp : 0;
}
// lean_plan on LeanPlanIn's fields in their order, the two patterns apart; out: take, variant, form, the two costs
extern "C" int tmpc_lean_plan(const int *in, int n_in, unsigned long long builtin_sp, unsigned long long model_sp, int *out5,
                              unsigned long long *weighed) {
    if (!in || n_in != 28 || !out5) return -1;
    tmpc::LeanPlanIn q;
    int i = 0;
    q.nx = in[i++], q.nu = in[i++], q.N = in[i++];
    q.builtin = in[i++] != 0, q.kinds = in[i++], q.builtin_sp = builtin_sp;
    q.lean_jit = in[i++] != 0, q.lean_ok = in[i++] != 0, q.model_sp = model_sp, q.knot_bounds = in[i++] != 0;
    q.quad_G = in[i++], q.precision = in[i++];
    q.sw_one = in[i++] != 0, q.sw_dense = in[i++] != 0, q.sw_ws = in[i++] != 0, q.sw_loop = in[i++] != 0;
    q.slots = in[i++], q.iters = in[i++], q.mpc_steps = in[i++];
    q.cold = in[i++] != 0, q.save = in[i++] != 0, q.indexed = in[i++] != 0, q.adaptive_rho = in[i++] != 0;
    q.ref_mode = in[i++];
    q.loop = in[i++] != 0, q.state_bounds = in[i++] != 0, q.g_maybe_nonzero = in[i++] != 0, q.live = in[i++] != 0, q.stream_ext = in[i++] != 0;
    q.cus = in[i++];
    const tmpc::LeanPlan p = tmpc::lean_plan(q);
    out5[0] = p.take ? 1 : 0, out5[1] = p.variant, out5[2] = p.form, out5[3] = p.cost_sparse, out5[4] = p.cost_dense;
    if (weighed) *weighed = p.sp;
    return 0;
}

namespace tmpc {

// Lanes per instance for a batch size.  Fewer lanes per instance means fewer cross-lane moves and no redundant
// work, but also fewer wavefronts.  A launch with at most one wavefront per SIMD takes about the same time
// whatever the batch (the instances' serial chains run side by side), so one lane per instance wins as soon as four
// lanes would need more than 1 024 wavefronts.  Measured on cartpole N=20, MI355X (scripts/group_sweep.sh), kernel ms
// for 1 / 2 / 4 lanes: batch 16 384: 0.326 / 0.331 / 0.272; 24 576: 0.331 / 0.348 / 0.383; 65 536: 0.370 / 0.512 / 0.748.
const KernelEntry *select_quad_kernel(int nx, int nu, int N, int batch) {
    const int pref[2][3] = {{1, 2, 4}, {4, 2, 1}};
    const int *order = batch >= 20480 ? pref[0] : pref[1];
    for (int i = 0; i < 3; ++i)
        if (const KernelEntry *e = find_quad_kernel(nx, nu, N, order[i])) return e;
    return nullptr;
}

const ConeEntry *mfmac_entry_6_3();
const ConeEntry *mfmar_entry_6_3_50();
const ConeEntry *mfmar_entry_6_3_10();
const ConeEntry *mfmar_entry_6_3_20();
const ConeEntry *mfmar_entry_6_3_30();

// matrix-core kernels for one-shot solves with the affine term / cones, instantiated for the rocket's shape: the
// register-resident one where the horizon is compiled in (admm_mfmar.hip.h), else the LDS-resident one with a run-time
// horizon (admm_mfmac.hip.h)
const ConeEntry *find_cone_kernel(int nx, int nu, int N) {
    static const ConeEntry *const table[] = {mfmar_entry_6_3_50(), mfmar_entry_6_3_30(), mfmar_entry_6_3_20(), mfmar_entry_6_3_10(), mfmac_entry_6_3()};
    for (const ConeEntry *e : table)
        if (e->nx == nx && e->nu == nu && e->N == N) return e;
    return nullptr;
}

const ConeEntry *mfmat_entry_6_3_50();
const ConeEntry *mfmat_entry_6_3_30();
const ConeEntry *mfmat_entry_6_3_20();
const ConeEntry *mfmat_entry_6_3_10();

// the transposed-sets matrix-core kernel (admm_mfmat.hip.h): every kind of solve of the shapes instantiated — one-shot,
// warm-started, workspace-keeping, chunked, closed loop — with box bounds, the affine term and one cone per side
const ConeEntry *find_trans_kernel(int nx, int nu, int N) {
    static const ConeEntry *const table[] = {mfmat_entry_6_3_50(), mfmat_entry_6_3_30(), mfmat_entry_6_3_20(), mfmat_entry_6_3_10()};
    for (const ConeEntry *e : table)
        if (e->nx == nx && e->nu == nu && e->N == N) return e;
    return nullptr;
}

int device_cu_count() {
    static std::atomic<int> cus[64];   // (a sharded handle's worker threads may ask for several devices at once)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int c = cus[dev & 63].load(std::memory_order_relaxed);
    if (c <= 0) {
        hipDeviceProp_t prop;
        c = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        cus[dev & 63].store(c, std::memory_order_relaxed);
    }
    return c;
}

const StreamEntry *stream4_entry_2_1();
const StreamEntry *stream4_entry_2_2();
const StreamEntry *stream4_entry_3_1();
const StreamEntry *stream4_entry_3_2();
const StreamEntry *stream4_entry_3_3();
const StreamEntry *stream4_entry_4_1();
const StreamEntry *stream4_entry_4_2();
const StreamEntry *stream4_entry_4_3();
const StreamEntry *stream4_entry_4_4();
const StreamEntry *stream4_entry_6_1();
const StreamEntry *stream4_entry_6_2();
const StreamEntry *stream4_entry_6_3();
const StreamEntry *stream4_entry_6_4();
const StreamEntry *stream4_entry_8_1();
const StreamEntry *stream4_entry_8_2();
const StreamEntry *stream4_entry_8_3();
const StreamEntry *stream4_entry_8_4();
const StreamEntry *stream4_entry_10_1();
const StreamEntry *stream4_entry_10_2();
const StreamEntry *stream4_entry_10_3();
const StreamEntry *stream4_entry_10_4();
const StreamEntry *stream4_entry_12_1();
const StreamEntry *stream4_entry_12_2();
const StreamEntry *stream4_entry_12_3();
const StreamEntry *stream4_entry_12_4();

// The run-time-horizon kernel (admm_streamg.hip.h) is instantiated with 4 lanes per instance: measured on MI355X
// (rocket N=50 with cones, batch 4 096 .. 65 536) 1 and 2 lanes per instance are no faster at any batch size - all
// three are bound by the scratch traffic from ~32 768 instances up - and slower below.
const StreamEntry *find_stream_kernel(int nx, int nu) {
    static const StreamEntry *const table[] = {stream4_entry_2_1(), stream4_entry_2_2(), stream4_entry_3_1(), stream4_entry_3_2(), stream4_entry_3_3(), stream4_entry_4_1(), stream4_entry_4_2(), stream4_entry_4_3(), stream4_entry_4_4(), stream4_entry_6_1(), stream4_entry_6_2(), stream4_entry_6_3(), stream4_entry_6_4(), stream4_entry_8_1(), stream4_entry_8_2(), stream4_entry_8_3(), stream4_entry_8_4(), stream4_entry_10_1(), stream4_entry_10_2(), stream4_entry_10_3(), stream4_entry_10_4(), stream4_entry_12_1(), stream4_entry_12_2(), stream4_entry_12_3(), stream4_entry_12_4()};
    for (const StreamEntry *e : table)
        if (e->nx == nx && e->nu == nu) return e;
    return nullptr;
}

hipError_t launch_generic(const AdmmParams &P, int precision, hipStream_t stream) {
    const int threads = 256;
    const int grid = (P.batch + threads - 1) / threads;
    if (P.ic_cx || P.ic_cu) {   // per-instance cone coefficients: the `ic` forms (bounds and rows per instance as the `il` forms read them)
        if (precision == 2)
            hipLaunchKernelGGL((admm_generic_ic_kernel<double, double>), dim3(grid), dim3(threads), 0, stream, P);
        else if (precision == 0)
            hipLaunchKernelGGL((admm_generic_ic_kernel<double, float>), dim3(grid), dim3(threads), 0, stream, P);
        else
            hipLaunchKernelGGL((admm_generic_ic_kernel<float, float>), dim3(grid), dim3(threads), 0, stream, P);
        return hipGetLastError();
    }
    if (P.il_bx) {   // per-instance linear rows: the `il` forms (bounds read per instance as the `ib` forms do; fixed rho)
        if (precision == 2)
            hipLaunchKernelGGL((admm_generic_il_kernel<double, double>), dim3(grid), dim3(threads), 0, stream, P);
        else if (precision == 0)
            hipLaunchKernelGGL((admm_generic_il_kernel<double, float>), dim3(grid), dim3(threads), 0, stream, P);
        else
            hipLaunchKernelGGL((admm_generic_il_kernel<float, float>), dim3(grid), dim3(threads), 0, stream, P);
        return hipGetLastError();
    }
    if (P.ibx) {   // per-instance bounds: the `ib` forms (fixed rho: the solver refuses adaptive rho beside them)
        if (precision == 2)
            hipLaunchKernelGGL((admm_generic_kernel<double, double, true>), dim3(grid), dim3(threads), 0, stream, P);
        else if (precision == 0)
            hipLaunchKernelGGL((admm_generic_kernel<double, float, true>), dim3(grid), dim3(threads), 0, stream, P);
        else
            hipLaunchKernelGGL((admm_generic_kernel<float, float, true>), dim3(grid), dim3(threads), 0, stream, P);
        return hipGetLastError();
    }
    if (precision == 2)
        hipLaunchKernelGGL((admm_generic_kernel<double, double>), dim3(grid), dim3(threads), 0, stream, P);
    else if (precision == 0)
        hipLaunchKernelGGL((admm_generic_kernel<double, float>), dim3(grid), dim3(threads), 0, stream, P);
    else
        hipLaunchKernelGGL((admm_generic_kernel<float, float>), dim3(grid), dim3(threads), 0, stream, P);
    return hipGetLastError();
}

template <class RT>
static void fill_generic_coef(const Solver &sv, std::vector<unsigned char> &out) {
    const int nx = sv.nx, nu = sv.nu;
    const GenericPack pk(nx, nu);
    out.assign((size_t)pk.len * sizeof(RT), 0);
    auto put = [&](size_t idx, double val) {
        const RT v = (RT)val;
        std::memcpy(out.data() + idx * sizeof(RT), &v, sizeof(RT));
    };
    const Cache &c = sv.cache;
    for (int j = 0; j < nx; ++j)
        for (int i = 0; i < nx; ++i) {
            put(pk.oA + i + j * nx, sv.A(i, j));
            put(pk.oP + i + j * nx, c.Pinf(i, j));
            put(pk.oAt + i + j * nx, c.AmBKt(i, j));
        }
    for (int a = 0; a < nu; ++a)
        for (int i = 0; i < nx; ++i) {
            put(pk.oB + i + a * nx, sv.B(i, a));
            put(pk.oK + a + i * nu, c.Kinf(a, i));
        }
    for (int a = 0; a < nu; ++a)
        for (int b2 = 0; b2 < nu; ++b2) put(pk.oQi + a + b2 * nu, c.Quu_inv(a, b2));
    // affine dynamics (UNPINNED): f, APf = AmBKt Pinf f, BPf = B^T Pinf f, all formed in fp64
    std::vector<double> Pf(nx, 0.0);
    for (int i = 0; i < nx; ++i)
        for (int l = 0; l < nx; ++l) Pf[i] += c.Pinf(i, l) * sv.fdyn[l];
    for (int i = 0; i < nx; ++i) {
        double apf = 0.0;
        for (int j = 0; j < nx; ++j) apf += c.AmBKt(i, j) * Pf[j];
        put(pk.oF + i, sv.fdyn[i]);
        put(pk.oAPf + i, apf);
    }
    for (int a = 0; a < nu; ++a) {
        double bpf = 0.0;
        for (int j = 0; j < nx; ++j) bpf += sv.B(j, a) * Pf[j];
        put(pk.oBPf + a, bpf);
    }
}

void build_generic_coef(const Solver &sv, std::vector<unsigned char> &out) {
    if (sv.precision != 1)
        fill_generic_coef<double>(sv, out);
    else
        fill_generic_coef<float>(sv, out);
}

void build_generic_bounds(const Solver &sv, std::vector<float> &out) {
    constexpr float kInf = std::numeric_limits<float>::infinity();
    const int EX = sv.ex(), EU = sv.eu();
    out.assign((size_t)2 * EX + 2 * EU + sv.nx + sv.nu, 0.f);
    for (int e = 0; e < EX; ++e) {
        out[e] = sv.st.en_state_bound ? (float)sv.x_min[e] : -kInf;
        out[EX + e] = sv.st.en_state_bound ? (float)sv.x_max[e] : kInf;
    }
    for (int e = 0; e < EU; ++e) {
        out[2 * EX + e] = sv.st.en_input_bound ? (float)sv.u_min[e] : -kInf;
        out[2 * EX + EU + e] = sv.st.en_input_bound ? (float)sv.u_max[e] : kInf;
    }
    for (int i = 0; i < sv.nx; ++i) out[2 * EX + 2 * EU + i] = (float)sv.cache.Qd[i];
    for (int a = 0; a < sv.nu; ++a) out[2 * EX + 2 * EU + sv.nx + a] = (float)sv.cache.Rd[a];
}

}  // namespace tmpc
