// Shared host/device definitions for the fused ADMM kernels.
#pragma once
#include <stdint.h>

namespace tmpc {

// How reference trajectories reach the kernel.
enum RefMode : int {
    REF_ZERO = 0,          // Xref = Uref = 0 (what tiny_setup leaves, tiny_api.cpp:102-103)
    REF_SHARED = 1,        // one (nx,N)/(nu,N-1) pair broadcast over the batch
    REF_PER_INSTANCE = 2,  // [B][N][nx] / [B][N-1][nu]
};

// Longest horizon at which the lanes-per-instance (quad) kernels' in-kernel closed loop takes per-step references
// (admm_quad.hip.h: REF_STEP; solver.hip refuses a reference sequence on a longer quad entry)
enum { QUAD_REF_SEQ_MAX_N = 20 };

// Slots of the per-solve device status block (uint32 each).
//   [0..3] max over instances of (pri_x, dua_x, pri_u, dua_u), float bits (non-negative
//          floats order like unsigned ints, so atomicMax on the bits is a float max)
//   [4]    number of instances that hit max_iter without converging
//   [5]    number of instances whose solution contains a non-finite value
enum { GSTAT_WORDS = 8 };
// A workgroup's record of the status fold: the four maxima as float bits, its unsolved count, padding — 32 bytes, aligned
enum { GSLOT_WORDS = 8, GSLOT_DEFAULT_CAP = 1024 };

// generic (runtime-shape) kernel limits
constexpr int LIN_MAX_ROWS = 8, GEN_MAX_NX = 64;
constexpr int GEN_MAX_NU = 32;

struct AdmmParams {
    // family constants (device pointers)
    const float *coef;    // lane-role-major coefficient pack, layout in QuadShape / generic kernel
    const float *bounds;  // per-knot bounds pack
    // per-instance inputs
    const float *x0;    // [B][nx]
    const double *x0d;  // matrix-core kernel, closed loop: the plant state in fp64 (NULL: x0)
    const float *xref;  // REF_SHARED: [N][nx]   REF_PER_INSTANCE: [B][N][nx]
    const float *uref;  // REF_SHARED: [N-1][nu] REF_PER_INSTANCE: [B][N-1][nu]
    // per-instance outputs
    float *xout;   // [B][N][nx]    projected slack vnew (admm.cpp:187,204)
    float *uout;   // [B][N-1][nu]  projected slack znew (admm.cpp:188,205)
    int *iter;     // [B]
    int *solved;   // [B]
    float *res;    // [B][4] pri_x, dua_x, pri_u, dua_u
    // warm-start state, persists between solves: d,y,z [B][N-1][nu]; g,v [B][N][nx]
    float *sd, *sy, *sz, *sg, *sv;
    uint32_t *gstat;  // [GSTAT_WORDS] status block of the launch: max residual bits [0..3], unsolved count [4]
    uint32_t *gacc;   // [GSTAT_WORDS] accumulator behind it (fold_status); zero between launches
    // stream / generic kernels: per-instance scratch in HBM
    float *scratch;
    // chunked solves with compaction (Solver::solve_chunked): launch slot j works on instance idx[j] (NULL: j) and
    // reports iter_offset + its own iteration count; `batch` is then the number of slots of this launch
    const int *idx;
    int iter_offset;
    int batch;
    int max_iter;
    int check_termination;  // <= 0: never check (the reference divides by it, admm.cpp:91)
    int ref_mode;
    int cold_start;  // 1: start from the zero workspace, do not read sd..sv
    int save_state;  // 1: write sd..sv back at exit
    float abs_pri_tol, abs_dua_tol, rho;
    int nx, nu, N;  // run-time shape (stream kernel: N; generic kernel: all three)
    // fused closed loop (0 = plain solve): steps per launch and per-step logs
    int mpc_steps;
    float *mpc_x;    // [B][steps][nx]  plant state after each step
    float *mpc_u;    // [B][steps][nu]  control applied at each step
    int *mpc_iter;   // [B][steps]      ADMM iterations of each step, negative if it hit max_iter
    float *x0_out;   // [B][nx]         plant state after the last step (aliases x0)
    // ---- stream / generic kernels: affine dynamics + second-order cones (parity UNPINNED) ----
    int xb_active;           // some enabled state bound is finite (else vnew = x + g is never clamped)
    int has_fdyn;            // coef pack carries fdyn, APf, BPf behind the matrices
    int ncx, ncu;            // number of state / input cones per knot (0: disabled), at most 8 each
    int Acx[8], qcx[8], Acu[8], qcu[8];  // first row and dimension of each cone block
    float cx[8], cu[8];                  // mu of each cone: ||head|| <= mu * (last row)
    float *sgc, *svc, *syc, *szc;        // warm-start state of the cone slack/dual pairs
    // ---- linear inequalities Alin_x x <= blin_x, Alin_u u <= blin_u at every knot (parity UNPINNED) ----
    int mlx, mlu;                        // rows per side (0: disabled), at most LIN_MAX_ROWS each
    const float *lin;                    // [mlx][nx] rows | b[mlx] | |a|^2[mlx] | [mlu][nu] rows | b[mlu] | |a|^2[mlu]
    float *sgl, *svl, *syl, *szl;        // warm-start state of the linear-inequality slack/dual pairs
    // ---- stream / generic kernels: adaptive rho (admm.cpp:147-174, rho_benchmark.cpp) ----
    int adaptive_rho;                    // every 5th iteration each instance re-predicts its rho and Taylor-updates Kinf, Pinf
    int rho_clip;
    double rho_family;                   // the family's rho as a double (the adaptive state's reset value; `rho` above is a float)
    float rho_min, rho_max;
    const double *sens;                  // dKinf/drho [nu*nx] then dPinf/drho [nx*nx], column-major
    double *adapt;                       // [1 + nu*nx + nx*nx][batch]: rho, Kinf, Pinf of each instance; solver state, it
                                         // persists between solves like the reference's cache
    long adapt_stride;                   // instances per row of `adapt` (the solver's batch)
    void *adp_cols;                      // stream kernel, adaptive rho: [ADP_LEN][G * batch] scratch columns (kernel-local)
    // ---- stream kernel only: one problem family PER INSTANCE ----
    const float *het_aux;                // [nx + nu + 1][batch]: diag(Q)+rho, diag(R)+rho, rho of each instance
    // ---- mfmac kernel only: 0 = the bounds pack holds one knot's bounds (they do not depend on the knot) ----
    int bounds_stride;
    // ---- mfmat kernel, fused closed loop: shared references of every step, [steps][N][nx] / [steps][N-1][nu] (NULL: the
    // references stay as set) — the per-step shift of rocket_landing_constraints.jl:107-115 ----
    const float *xref_seq, *uref_seq;
    // ---- lean kernel (admm_lean.hip.h): its fp64 coefficient pack (LeanPack), wave-uniform ----
    const double *lean;
    // ---- launcher-side switches (read from the environment once per solver: Switches), not read by any kernel ----
    int host_flags;   // HF_NO_REFILL | HF_NO_UNI | HF_NO_OS | HF_LEAN_SCALED
    // ---- generic kernel, precision 2 (fp64 end to end): the workspace kept between solves (Ws64) and the tolerances in fp64 ----
    double *ws64;
    double abs_pri_tol64, abs_dua_tol64;
    // ---- lean kernel, one-shot forms: the status fold's records (fold_status_records) ----
    uint32_t *gslot;  // [gslot_cap][GSLOT_WORDS] one status record per workgroup; never zeroed.  NULL: none
    int gslot_cap;    // workgroups with blockIdx.x below it write a record, the others accumulate in gacc
    // ---- stream / generic kernels, `ib` forms: box bounds PER INSTANCE (tinympc_set_instance_bounds), fp32, in the scratch
    // block's layout [min | max][knot][instance][real row], indexed by the INSTANCE (P.idx[slot] under compaction), never by
    // the launch's dense slot.  The knot strides are batch * nx / batch * nu elements of the solver's whole batch for bounds
    // given per knot and 0 for bounds constant over the horizon (one line per instance, re-read at every knot); the max
    // half starts ib_hx / ib_hu elements behind the min half.  NULL: the bounds are the shared pack's ----
    const float *ibx, *ibu;
    long ib_kx, ib_ku, ib_hx, ib_hu;
    int ib_on;        // IB_STATE | IB_INPUT: the sides the settings leave switched on (the other clamps against -+inf, unread)
    // ---- stream / generic kernels, `il` forms: linear rows PER INSTANCE (tinympc_set_instance_linear), fp32, P.mlx / P.mlu
    // rows a side as for the shared set.  Coefficients [row][instance][real entry] — the scratch block's layout, a row il_rx /
    // il_ru elements (batch * nx / batch * nu of the solver's whole batch) behind the one before; right-hand sides and |a|^2
    // [row][instance], a row il_rb elements apart.  Indexed by the INSTANCE, as the `ib` bounds are.  An instance's absent row
    // is a = 0, b = FLT_MAX, |a|^2 = 1: `dot > b` never holds.  The `il` forms read their bounds from ibx / ibu (a solver with
    // shared bounds uploads them replicated).  NULL: the rows are the shared pack's (P.lin) ----
    const float *il_ax, *il_au, *il_bx, *il_n2x, *il_bu, *il_n2u;
    long il_rx, il_ru, il_rb;
    // ---- stream / generic kernels, `ic` forms: the cone coefficient mu PER INSTANCE (tinympc_set_instance_cones), fp32,
    // [cone][instance], a cone ic_rc elements (the solver's whole batch) behind the one before; P.ncx / P.ncu cones a side
    // and the layout Acx .. qcu as for the shared set.  Indexed by the INSTANCE, as the `ib` bounds are.  +inf: the instance
    // does not have the cone (no projection; its rows stay as they are).  The `ic` forms are `il` forms: they read their
    // bounds from ibx / ibu and their rows from il_* (a solver with shared ones uploads them replicated).  NULL: the
    // coefficients are cx / cu above ----
    const float *ic_cx, *ic_cu;
    long ic_rc;
};
enum : int { IB_STATE = 1, IB_INPUT = 2 };
enum : int { HF_NO_REFILL = 1, HF_NO_UNI = 2, HF_NO_OS = 4, HF_LEAN_SCALED = 8 };   // (HF_LEAN_SCALED: the lean pack's scaled block is valid)

// Coefficient pack of the lean kernel (admm_lean.hip.h), fp64, all wave-uniform; filled by build_lean_pack (kernels.hip).
// Three coefficient blocks of the same layout: the plain one (what the tolerance-terminated and state-bounded variants read);
// at oH, the same four matrices in controller-Hessenberg coordinates x = T x^ (host_setup.h: staircase_form) — T' M T
// with lower bandwidth nu, T' B upper trapezoidal, Kinf T, and the input-space -rho Quu_inv unchanged — which the
// fixed-iteration variants' sweeps read; at oS, the model's own A where M is (the sparse variants, lean_pattern below).
struct LeanLayout {
    int oM;      // A - B Kinf     [nx][nx] row-major (its transpose is the AmBKt the backward sweep reads); A in the oS block
    int oK;      // Kinf           [nu][nx]
    int oB;      // B              [nx][nu]
    int oC;      // -rho Quu_inv   [nu][nu]
    int len;
    int padded;  // rounded up to whole 8-double scalar loads (what the kernel keeps in SGPRs)
    int oH;      // the transformed block (oM .. oC relative to it), padded likewise
    int oS;      // the sparse variants' block [A, Kinf, B, C] (oM .. oC relative to it), padded likewise
    int oP;      // Pinf           [nx][nx] row-major, behind the padded blocks (read once, for the terminal reference term)
    int oT;      // T              [nx][nx] row-major, orthogonal (read at entry, at the residual iteration and at the store)
    int total;
    // appended behind everything above (no earlier offset moves): the block of the diagonally scaled model x^ = S x
    // (lean_pattern_scaled below) — [S A S^-1, Kinf S^-1, S B, C] in the layout of the others, w = diag(S)^-2 [nx] behind C at
    // oW (nu = 1: c diag(S)^-2 with the scalar c = C, which the costate's scale takes in — admm_lean.hip.h: FOLD), padded to whole
    // scalar loads (padZ) — then s [nx] and 1 / s [nx], read at entry, at the residuals and at the store
    int oZ, oW, padZ, oSc, oSi;
};
constexpr LeanLayout lean_layout(int nx, int nu) {
    const int len = nx * nx + 2 * nu * nx + nu * nu, pad = (len + 7) / 8 * 8, padz = (len + nx + 7) / 8 * 8;
    const int old_total = 3 * pad + 2 * nx * nx, oz = (old_total + 7) / 8 * 8;
    return LeanLayout{0, nx * nx, nx * nx + nu * nx, nx * nx + 2 * nu * nx, len, pad, pad, 2 * pad, 3 * pad, 3 * pad + nx * nx,
                      oz + padz + 2 * nx, oz, len, padz, oz + padz, oz + padz + nx};
}

// Zero / unit pattern of a model's (A, B), nx, nu <= 4, as a lean kernel's compile-time parameter SP: bits 0-15 the nonzeros
// of A (bit i * nx + j: A[i][j]), bits 16-31 the entries of A that are exactly 1.0 (a subset of the nonzeros), bits 32-47
// the nonzeros of B (bit i * nu + a), bit 48 set in every pattern.  SP == 0: no pattern, the dense sweeps.
enum : int { LSP_UNIT = 16, LSP_B = 32, LSP_ON = 48 };
constexpr bool lsp_a(uint64_t sp, int nx, int i, int j) { return (sp >> (i * nx + j)) & 1; }
constexpr bool lsp_one(uint64_t sp, int nx, int i, int j) { return (sp >> (LSP_UNIT + i * nx + j)) & 1; }
constexpr bool lsp_b(uint64_t sp, int nu, int i, int a) { return (sp >> (LSP_B + i * nu + a)) & 1; }
// the pattern of A [nx][nx] and B [nx][nu], row-major: nonzero is != 0.0, unit is == 1.0 exactly (0: nx or nu above 4)
constexpr uint64_t lean_pattern_rm(int nx, int nu, const double *A, const double *B) {
    if (nx < 1 || nu < 1 || nx > 4 || nu > 4) return 0;
    uint64_t sp = 1ull << LSP_ON;
    for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j) {
            if (A[i * nx + j] != 0.0) sp |= 1ull << (i * nx + j);
            if (A[i * nx + j] == 1.0) sp |= 1ull << (LSP_UNIT + i * nx + j);
        }
        for (int a = 0; a < nu; ++a)
            if (B[i * nu + a] != 0.0) sp |= 1ull << (LSP_B + i * nu + a);
    }
    return sp;
}
// fp64 instructions per knot of each form (both sweeps, zero references): the sparse sweeps of pattern sp — u = -Kinf x - d,
// x+ = A x + B u with a row's chain started from x_j where A[i][j] is a unit; t = B' p~ + r~, d = C t, p~ = x + A' p~ - Kinf' t
constexpr int lean_cost_sparse(uint64_t sp, int nx, int nu) {
    int c = 2 * nx * nu + nu * nu;                  // u, Kinf' t, C t
    for (int i = 0; i < nx; ++i) {
        int terms = 0;
        bool unit = false;
        for (int j = 0; j < nx; ++j) terms += lsp_a(sp, nx, i, j), unit = unit || lsp_one(sp, nx, i, j);
        for (int a = 0; a < nu; ++a) terms += 2 * lsp_b(sp, nu, i, a);   // (B u forward, B' p~ backward)
        for (int j = 0; j < nx; ++j) terms += lsp_a(sp, nx, j, i);       // (A' p~: a unit is an add)
        c += terms - (unit ? 1 : 0);
    }
    return c;
}
// ... controller-Hessenberg (band of T'MT, trapezoid of T'B) and plain dense (A - B Kinf, B)
constexpr int lean_cost_hessenberg(int nx, int nu) {
    int band = 0, trap = 0;
    for (int m = 0; m < nx; ++m) {
        for (int j = 0; j < nx; ++j) band += j >= m - nu;
        for (int a = 0; a < nu; ++a) trap += m <= a;
    }
    return 2 * band + 2 * trap + 2 * nx * nu + nu * nu;
}
constexpr int lean_cost_dense(int nx, int nu) { return 2 * nx * nx + 4 * nx * nu + nu * nu; }
// a kernel built for pattern `built` computes a model of pattern `model` exactly when the model's nonzeros lie inside the
// built pattern's and every entry the kernel takes as 1 is 1 in the model (the kernel never reads those entries)
constexpr bool lean_pattern_covers(uint64_t built, uint64_t model) {
    const uint64_t nz = 0xFFFFull | (0xFFFFull << LSP_B), one = 0xFFFFull << LSP_UNIT;
    return built != 0 && model != 0 && (model & nz & ~built) == 0 && ((built & one) & ~(model & one)) == 0;
}

// Pattern of a diagonally scaled model.  x^ = S x, S = diag(s), turns (A, B) into (S A S^-1, S B): the zeros and the diagonal of
// A stay, and the nx free ratios of s make up to nx - 1 off-diagonal nonzeros of A and one nonzero of B exactly 1 — a forward
// row may then start from a free operand where the model's own row has none.  The backward recursion keeps its form with
// p^ = S^-1 p~: p^_k = W x^_k + A^' p^_{k+1} - K^' t_k, t_k = r~_k + B^' p^_{k+1}, W = S^-2 diagonal, K^ = Kinf S^-1; the
// input-space u, d, t, r~, y, z and C are unchanged.  Bit 49 marks such a pattern: its unit bits (16-31) are the model's
// DIAGONAL units and the chosen off-diagonal entries, bit 54 says that B has a unit and bits 50-53 which (i * nu + a).
enum : int { LSP_SCALED = 49, LSP_BU = 50, LSP_BU_ON = 54 };
constexpr bool lsp_scaled(uint64_t sp) { return (sp >> LSP_SCALED) & 1; }
constexpr bool lsp_b_one(uint64_t sp, int nu, int i, int a) {
    return ((sp >> LSP_BU_ON) & 1) && (int)((sp >> LSP_BU) & 15) == i * nu + a;
}
// fp64 instructions per knot of the scaled sparse sweeps of pattern sp^ (both sweeps, zero references): u = -K^ x^ - d costs
// nx nu; a forward row its terms of A^ and B^, one fewer where it holds a unit of either (the chain's free start); t the
// nonzeros of B^ (from r~; a unit is an add); d = C t costs nu^2; a backward column 1 (w x^) + its nonzeros of A^ + nu
// (K^' t), one fewer where the column holds a unit of A^ (fma(w, x^, p^_j) starts the chain)
constexpr int lean_cost_scaled(uint64_t sp, int nx, int nu) {
    int c = nx * nu + nu * nu;
    for (int i = 0; i < nx; ++i) {
        int row = 0, col = 1 + nu;
        bool ru = false, cu = false;
        for (int j = 0; j < nx; ++j) {
            row += lsp_a(sp, nx, i, j), ru = ru || lsp_one(sp, nx, i, j);
            col += lsp_a(sp, nx, j, i), cu = cu || lsp_one(sp, nx, j, i);
        }
        for (int a = 0; a < nu; ++a) {
            row += lsp_b(sp, nu, i, a), ru = ru || lsp_b_one(sp, nu, i, a);
            c += lsp_b(sp, nu, i, a);                                    // (t)
        }
        c += row - (ru && row > 0 ? 1 : 0) + col - (cu ? 1 : 0);
    }
    return c;
}
// ... and of the form the kernel runs at nu = 1, where C is a scalar c folded into the costate's scale (admm_lean.hip.h: FOLD;
// the pack's w is then c s^-2): d = c r~ + B^' pv starts from a product it needed anyway, so the product by C goes.  The choice of
// the pattern (lean_pattern_scaled, lean_scale_model) stays on lean_cost_scaled: the two differ by a constant per nu
constexpr int lean_cost_folded(uint64_t sp, int nx, int nu) { return lean_cost_scaled(sp, nx, nu) - (nu == 1 ? 1 : 0); }
// The scaled pattern of a model's pattern sp (positions only, not values): the off-diagonal nonzeros of A made units — a set
// that is acyclic as an undirected graph on the states (a cycle's product is invariant under the scaling), so at most
// nx - 1 of them — and at most one nonzero of B, chosen by plain enumeration (at most 12 candidates at nx <= 4) to minimise
// lean_cost_scaled; among equal costs the choice with the most units wins (a unit is a coefficient the kernel never reads, and
// its term an add without a product's rounding), then the lowest mask (the A bits, then the B choice: none, then by index).
// Diagonal units of A carry over; an off-diagonal unit of the model is a candidate like any other nonzero.  0: no pattern.
constexpr uint64_t lean_pattern_scaled(uint64_t sp, int nx, int nu) {
    if (sp == 0 || lsp_scaled(sp) || nx < 1 || nu < 1 || nx > 4 || nu > 4) return 0;
    uint64_t base = (sp & (0xFFFFull | (0xFFFFull << LSP_B))) | (1ull << LSP_ON) | (1ull << LSP_SCALED);
    uint32_t cand = 0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            if (i == j && lsp_one(sp, nx, i, i)) base |= 1ull << (LSP_UNIT + i * nx + i);
            if (i != j && lsp_a(sp, nx, i, j)) cand |= 1u << (i * nx + j);
        }
    uint64_t best = 0;
    int best_cost = 0, best_units = 0;
    for (uint32_t m = 0, done = 0; !done; done = (m == cand), m = (m - cand) & cand) {   // the subsets of cand, ascending
        int comp[4] = {0, 1, 2, 3};
        bool ok = true;
        for (int e = 0; e < nx * nx && ok; ++e) {
            if (!((m >> e) & 1)) continue;
            const int ci = comp[e / nx], cj = comp[e % nx];
            if (ci == cj) ok = false;                                    // (closes a cycle; a forest has at most nx - 1 edges)
            for (int q = 0; q < nx; ++q)
                if (comp[q] == cj) comp[q] = ci;
        }
        for (int b = -1; ok && b < nx * nu; ++b) {
            if (b >= 0 && !((sp >> (LSP_B + b)) & 1)) continue;
            uint64_t s = base | ((uint64_t)m << LSP_UNIT);
            if (b >= 0) s |= (1ull << LSP_BU_ON) | ((uint64_t)b << LSP_BU);
            int units = b >= 0 ? 1 : 0;
            for (int e = 0; e < nx * nx; ++e) units += (m >> e) & 1;
            const int cost = lean_cost_scaled(s, nx, nu);
            if (best == 0 || cost < best_cost || (cost == best_cost && units > best_units)) best = s, best_cost = cost, best_units = units;
        }
    }
    return best;
}

#ifdef __HIPCC__
// Folds a workgroup's residual maxima / unsolved count into the launch's status block without a host-side clear: the
// wavefronts of a workgroup (at most four) meet in LDS, ONE lane per workgroup accumulates in P.gacc (per-wavefront atomics
// queue on five words when a thousand wavefronts finish together: round 4, lean kernel timeline); the last workgroup to
// finish (ticket in gacc[7]) publishes the totals to P.gstat and hands the accumulator back zeroed to the next launch.
// Every thread of the workgroup must call it; lane 0 of each wavefront carries that wavefront's values.
__device__ __forceinline__ void fold_status(const AdmmParams &P, float m0, float m1, float m2, float m3,
                                            int unsolved_in_wave, int tid) {
    __shared__ float s_fold_m[4][4];
    __shared__ int s_fold_u[4];
    const int w = tid >> 6, nw = ((int)blockDim.x + 63) >> 6;
    const bool merged = nw <= 4;
    if ((tid & 63) == 0) {
        if (merged) {
            s_fold_m[w][0] = m0, s_fold_m[w][1] = m1, s_fold_m[w][2] = m2, s_fold_m[w][3] = m3;
            s_fold_u[w] = unsolved_in_wave;
        } else {
            atomicMax(&P.gacc[0], __float_as_uint(m0));
            atomicMax(&P.gacc[1], __float_as_uint(m1));
            atomicMax(&P.gacc[2], __float_as_uint(m2));
            atomicMax(&P.gacc[3], __float_as_uint(m3));
            if (unsolved_in_wave) atomicAdd(&P.gacc[4], (uint32_t)unsolved_in_wave);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (merged) {
            int un = 0;
            for (int i = 0; i < nw; ++i) {
                m0 = i ? fmaxf(m0, s_fold_m[i][0]) : s_fold_m[0][0];
                m1 = i ? fmaxf(m1, s_fold_m[i][1]) : s_fold_m[0][1];
                m2 = i ? fmaxf(m2, s_fold_m[i][2]) : s_fold_m[0][2];
                m3 = i ? fmaxf(m3, s_fold_m[i][3]) : s_fold_m[0][3];
                un += s_fold_u[i];
            }
            atomicMax(&P.gacc[0], __float_as_uint(m0));
            atomicMax(&P.gacc[1], __float_as_uint(m1));
            atomicMax(&P.gacc[2], __float_as_uint(m2));
            atomicMax(&P.gacc[3], __float_as_uint(m3));
            if (un) atomicAdd(&P.gacc[4], (uint32_t)un);
        }
        __threadfence();  // this workgroup's contributions before its ticket
        if (atomicAdd(&P.gacc[7], 1u) == gridDim.x - 1) {
            __threadfence();
            uint32_t tot[5];              // (the swaps issued together and waited for once: this is the tail of the launch)
#pragma unroll
            for (int i = 0; i < 5; ++i) tot[i] = atomicExch(&P.gacc[i], 0u);
            atomicExch(&P.gacc[6], 0u);   // (persistent kernels' tile counter)
            atomicExch(&P.gacc[7], 0u);
#pragma unroll
            for (int i = 0; i < 5; ++i) P.gstat[i] = tot[i];
        }
    }
}

// fold_status with one record per workgroup: what the one-shot lean kernels call (admm_lean.hip.h).  Same contract, same
// accumulator block and ticket, so launches of either kind may follow each other on one solver.  The wavefronts of a
// workgroup (at most four) meet in LDS and ONE lane per workgroup reports; the last workgroup to finish (ticket in gacc[7])
// publishes the totals to P.gstat and hands the accumulator back zeroed to the next launch.
// How a workgroup reports:
//   * record (P.gslot set, blockIdx.x < P.gslot_cap, at most four wavefronts): the lane writes the five values to the
//     workgroup's own 32-byte record with agent-scope write-through stores, waits for them (s_waitcnt vmcnt(0)) and takes its
//     ticket with ONE relaxed atomic — no fence (a fence writes the L2 back, behind megabytes of solution stores that nothing
//     here needs ordered) and one atomic on the shared line where the accumulator path has six.  Records are overwritten, not
//     accumulated, and never zeroed: every workgroup below min(gridDim.x, cap) rewrites its record in every launch before
//     its ticket, and the last arriver reads that range only (records beyond it may be older launches');
//   * accumulator (every other workgroup): atomicMax / atomicAdd on gacc[0..4], a fence, the ticket.
// The last arriver — wavefront 0 of its workgroup, told by lane 0's ticket — executes one agent-scope acquire, lane 0 swaps
// the accumulator words out (issued together), all lanes load the records `lane, lane + 64, ...` with agent-scope loads,
// four rounds in flight, the wavefront reduces and lane 0 stores the block.
// EVERY thread of the workgroup must call it, EXACTLY ONCE per launch (a second call would overwrite the record where the
// accumulator tolerated it, and take a second ticket): the lean kernel calls it once, outside its loops, either ahead of the
// final store or behind it (TMPC_LEAN_FOLD_FIRST).  Lane 0 of each wavefront carries that wavefront's values.
__device__ __forceinline__ void fold_status_records(const AdmmParams &P, float m0, float m1, float m2, float m3,
                                            int unsolved_in_wave, int tid) {
    __shared__ float s_fold_m[4][4];
    __shared__ int s_fold_u[4];
    const int w = tid >> 6, nw = ((int)blockDim.x + 63) >> 6;
    const bool merged = nw <= 4;
    if ((tid & 63) == 0) {
        if (merged) {
            s_fold_m[w][0] = m0, s_fold_m[w][1] = m1, s_fold_m[w][2] = m2, s_fold_m[w][3] = m3;
            s_fold_u[w] = unsolved_in_wave;
        } else {
            atomicMax(&P.gacc[0], __float_as_uint(m0));
            atomicMax(&P.gacc[1], __float_as_uint(m1));
            atomicMax(&P.gacc[2], __float_as_uint(m2));
            atomicMax(&P.gacc[3], __float_as_uint(m3));
            if (unsolved_in_wave) atomicAdd(&P.gacc[4], (uint32_t)unsolved_in_wave);
        }
    }
    __syncthreads();
    if (tid >= 64) return;                                    // wavefront 0 goes on: its lane 0 reports, all of it may reduce
    const int nrec = P.gslot ? min((int)gridDim.x, P.gslot_cap) : 0;   // the records of this launch
    int last = 0;
    if (tid == 0) {
        bool recorded = false;
        if (merged) {
            int un = 0;
            for (int i = 0; i < nw; ++i) {
                m0 = i ? fmaxf(m0, s_fold_m[i][0]) : s_fold_m[0][0];
                m1 = i ? fmaxf(m1, s_fold_m[i][1]) : s_fold_m[0][1];
                m2 = i ? fmaxf(m2, s_fold_m[i][2]) : s_fold_m[0][2];
                m3 = i ? fmaxf(m3, s_fold_m[i][3]) : s_fold_m[0][3];
                un += s_fold_u[i];
            }
            if ((int)blockIdx.x < nrec) {
                unsigned long long *rec = reinterpret_cast<unsigned long long *>(P.gslot + (size_t)blockIdx.x * GSLOT_WORDS);
                __hip_atomic_store(rec + 0, (unsigned long long)__float_as_uint(m0) | ((unsigned long long)__float_as_uint(m1) << 32),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(rec + 1, (unsigned long long)__float_as_uint(m2) | ((unsigned long long)__float_as_uint(m3) << 32),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(rec + 2, (unsigned long long)(uint32_t)un, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the record is written through before the ticket says so
                recorded = true;
            } else {
                atomicMax(&P.gacc[0], __float_as_uint(m0));
                atomicMax(&P.gacc[1], __float_as_uint(m1));
                atomicMax(&P.gacc[2], __float_as_uint(m2));
                atomicMax(&P.gacc[3], __float_as_uint(m3));
                if (un) atomicAdd(&P.gacc[4], (uint32_t)un);
            }
        }
        if (!recorded) __threadfence();  // this workgroup's contributions before its ticket
        last = __hip_atomic_fetch_add(&P.gacc[7], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    }
    if (!__shfl(last, 0, 64)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    uint32_t tot[5] = {0, 0, 0, 0, 0};
    if (tid == 0) {                   // (the swaps issued together and waited for once: this is the tail of the launch)
#pragma unroll
        for (int i = 0; i < 5; ++i) tot[i] = atomicExch(&P.gacc[i], 0u);
        atomicExch(&P.gacc[6], 0u);   // (persistent kernels' tile counter)
        atomicExch(&P.gacc[7], 0u);
    }
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, ru = 0;   // (non-negative floats order like their bits)
    for (int base = 0; base < nrec; base += 4 * 64) {
        unsigned long long a[4], b[4], c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // (a lane beyond the last record re-reads that record and drops it: no branch between the loads, all twelve in flight)
            const int s = min(base + q * 64 + tid, nrec - 1);
            unsigned long long *rec = reinterpret_cast<unsigned long long *>(P.gslot + (size_t)s * GSLOT_WORDS);
            a[q] = __hip_atomic_load(rec + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b[q] = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c[q] = __hip_atomic_load(rec + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (base + q * 64 + tid >= nrec) a[q] = b[q] = c[q] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r0 = max(r0, (uint32_t)a[q]), r1 = max(r1, (uint32_t)(a[q] >> 32));
            r2 = max(r2, (uint32_t)b[q]), r3 = max(r3, (uint32_t)(b[q] >> 32));
            ru += (uint32_t)c[q];
        }
    }
    if (nrec) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            r0 = max(r0, (uint32_t)__shfl_xor((int)r0, off, 64)), r1 = max(r1, (uint32_t)__shfl_xor((int)r1, off, 64));
            r2 = max(r2, (uint32_t)__shfl_xor((int)r2, off, 64)), r3 = max(r3, (uint32_t)__shfl_xor((int)r3, off, 64));
            ru += (uint32_t)__shfl_xor((int)ru, off, 64);
        }
    }
    if (tid == 0) {
        tot[0] = max(tot[0], r0), tot[1] = max(tot[1], r1), tot[2] = max(tot[2], r2), tot[3] = max(tot[3], r3), tot[4] += ru;
#pragma unroll
        for (int i = 0; i < 5; ++i) P.gstat[i] = tot[i];
    }
}
#endif

}  // namespace tmpc
