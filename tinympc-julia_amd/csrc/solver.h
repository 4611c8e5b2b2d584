// Batched TinyMPC solver object behind the C-ABI (include/tinympc_hip.h).
// Host side of the drop-in boundary that replaces the reference's global
// `g_solver` + tiny_* calls (reference: src/bindings.cpp:15-490).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "admm_params.h"
#include "devbuf.h"
#include "host_setup.h"

namespace tmpc {

struct Solver;

// One specialised quad-kernel instantiation (admm_quad.hip.h) and its pack builders.
struct KernelEntry {
    int nx, nu, N, G;  // G = lanes per instance
    const char *name;
    void (*build_coef)(const Solver &, std::vector<unsigned char> &);  // typed by Solver::precision
    void (*build_bounds)(const Solver &, std::vector<float> &);
    hipError_t (*launch)(const AdmmParams &, int precision, bool state_bounds_active, hipStream_t);
    bool adp = false;  // the entry also carries the adaptive-rho kernels (QuadShape::ADP_OK)
    bool jit = false;  // specialised at setup (jit.cpp): fp64-recurrence kernels only, no adaptive-rho variants
};
// Specialisation at setup (jit.cpp): compiles / loads the on-chip kernel of a shape the library was not built with and adds
// it to what find_quad_kernel / find_mfma_kernel return; nullptr when nothing could be specialised (no compiler, no
// sources, the state does not fit, TINYMPC_HIP_NO_JIT)
const KernelEntry *jit_kernel_for(int nx, int nu, int N, int verbose);
const KernelEntry *jit_find(bool mfma, int nx, int nu, int N, int group);
// ... and the transposed-sets matrix-core kernel for exactly a solver's constraint layout (two cones per side, linear rows, a
// horizon the library was not built with): the unit already loaded that takes this solver / compile it now
struct ConeEntry;
const ConeEntry *jit_trans_find(const Solver &);
const ConeEntry *jit_trans_for(const Solver &, int verbose);
// group < 0: the shape's default group size; otherwise that exact variant (nullptr if not built)
const KernelEntry *find_quad_kernel(int nx, int nu, int N, int group = -1);
// the variant best suited to `batch` instances (nullptr: no specialised kernel for the shape)
const KernelEntry *select_quad_kernel(int nx, int nu, int N, int batch);
// the matrix-core kernel of the shape, for one-shot solves (nullptr: not instantiated)
const KernelEntry *find_mfma_kernel(int nx, int nu, int N);
// One entry of the lean kernel (admm_lean.hip.h): the one-lane-per-instance quad entry's solves with zero or shared
// references and fp64 recurrences run there — the benchmark's calling pattern.  Which of its instantiations
// admm_lean_kernel<LIVE, UBK, ONE, XB, REFS, ST, SP, WS, MPC> a launch runs is the variant, a set of LV_* bits that lean_plan
// (below) decides and nothing else: LV_LIVE tolerance-terminated, LV_UBK the input bounds do not depend on the knot, LV_ONE the
// 512-register form (one wavefront per SIMD), LV_XB the state-bounded form, LV_SHARED shared references, LV_F64 slack / dual
// state in fp64 (precision 2), LV_SPARSE the sweeps on the pattern sp, LV_WS the workspace-keeping form (warm starts, kept
// workspace, the chained closed loop), LV_MPC its in-kernel closed loop (P.mpc_steps warm solves and plant steps in one launch).
enum { LV_LIVE = 1, LV_UBK = 2, LV_ONE = 4, LV_XB = 8, LV_SHARED = 16, LV_F64 = 32, LV_SPARSE = 64, LV_WS = 128, LV_MPC = 256, LV_COUNT = 512 };
// the kinds of kernel a built-in entry carries beside its dense one-shot ones
enum { LK_SPARSE = 1, LK_WS = 2, LK_SPARSE_WS = 4, LK_MPC = 8, LK_SPARSE_MPC = 16, LK_ALL = 31 };
using LeanLaunch = hipError_t (*)(const AdmmParams &, int variant, hipStream_t, hipEvent_t ev0, hipEvent_t ev1);
struct LeanEntry {
    int nx, nu, N;
    const char *name;
    uint64_t sp;   // the (A, B) pattern of its sparse kernels (admm_params.h: lean_pattern_rm), 0: none
    int kinds;     // LK_*; a specialised unit: 0 (it carries the one variant it was compiled for)
    // runs the kernel of `variant`; hipErrorNotSupported: the entry has no such kernel (lean_plan sends none).  ev0 / ev1:
    // timing events carried by the kernel's own dispatch packet (its start and its end); null: none
    LeanLaunch launch;
    // the scaled pattern (admm_params.h: lean_pattern_scaled) its scaled sparse kernels are built for, 0: it has none.  A launch
    // runs them where P.host_flags carries HF_LEAN_SCALED and the (LIVE, ONE, XB) case has one (lean_entry.hip.h)
    uint64_t sp_scaled = 0;
};
// The (LIVE, ONE, XB) cases of the one-shot sparse kernels that exist in the scaled form: without a state bound, the
// 512-register kernels, fixed-iteration and tolerance-terminated (they must agree bit for bit).  The 256-register
// fixed-iteration kernel is not built: at 246 of 256 registers today, it spills 63 with the scaled sweeps.  THE rule: the
// built-in entry's launcher (lean_entry.hip.h) and the test hook tmpc_lean_last_scaled both ask it.
inline bool lean_runs_scaled(const LeanEntry *e, int variant, int host_flags) {
    if (!e || !e->sp_scaled || !(host_flags & HF_LEAN_SCALED)) return false;
    if ((variant & (LV_SPARSE | LV_UBK | LV_SHARED | LV_F64 | LV_WS | LV_MPC | LV_XB)) != (LV_SPARSE | LV_UBK)) return false;
    return (variant & LV_ONE) != 0;
}
const LeanEntry *find_lean_kernel(int nx, int nu, int N);
// ... or ONE variant of it specialised at the first launch that needs it (jit.cpp; nullptr: the shape does not fit the kernel);
// sp: the model's own pattern with LV_SPARSE, else 0
const LeanEntry *jit_lean_for(int nx, int nu, int N, int variant, uint64_t sp, int verbose);
// whether a workspace-keeping variant of the shape fits a workgroup's LDS (jit.cpp: the one rule)
bool lean_ws_fits(int nx, int nu, int N, bool live, bool xb, bool shared, bool knot_bounds);
int device_cu_count();   // CU count of the current device (cached per device: a sharded handle launches on several)
// The sweeps a lean launch runs: the dense plain form, controller-Hessenberg (fixed iterations, no state bound, 512 registers)
// or the sparse form of a pattern.  A kernel built for pattern `built` takes a model of pattern `model` when it covers it and
// costs fewer fp64 instructions per knot than the form it replaces.
enum { LF_NONE = 0, LF_PLAIN = 1, LF_HB = 2, LF_SPARSE = 3 };
inline int lean_pick_form(int nx, int nu, uint64_t built, uint64_t model, bool one, bool live, bool xb, bool sparse_allowed) {
    const bool hb = one && !live && !xb;
    const int dense = hb ? lean_cost_hessenberg(nx, nu) : lean_cost_dense(nx, nu);
    if (sparse_allowed && lean_pattern_covers(built, model) && lean_cost_sparse(built, nx, nu) < dense) return LF_SPARSE;
    return hb ? LF_HB : LF_PLAIN;
}
// THE routing of the lean kernel: whether a launch runs there and as which variant — the one place that decides it
// (kernels.hip).  Scalars in, scalars out; nothing is allocated and nothing asked of the device (cus comes in).
struct LeanPlanIn {
    int nx = 0, nu = 0, N = 0;
    // what the solver holds
    bool builtin = false;            // a built-in entry of the shape, with
    int kinds = 0;                   // ... these kinds of kernel (LK_*) and
    uint64_t builtin_sp = 0;         // ... this pattern; otherwise
    bool lean_jit = false;           // ... single variants are specialised at the launches that need them
    bool lean_ok = false;            // the family qualifies (build_lean_pack)
    uint64_t model_sp = 0;           // the model's pattern (lean_pattern)
    bool knot_bounds = false;        // the input bounds depend on the knot
    int quad_G = 0;                  // lanes per instance of the selected quad entry, 0: none is selected
    int precision = 0;
    bool sw_one = false, sw_dense = false, sw_ws = false, sw_loop = false;   // TINYMPC_HIP_LEAN_ONE / _DENSE / _WS / _LOOP
    // the launch
    int slots = 0, iters = 0, mpc_steps = 0;
    bool cold = false, save = false, indexed = false, adaptive_rho = false;
    int ref_mode = REF_ZERO;
    bool loop = false;               // the in-kernel closed loop or nothing (Pass::loop)
    bool state_bounds = false;       // some enabled state bound is finite
    bool g_maybe_nonzero = false;    // the kept workspace's state dual may hold something
    bool live = false;               // both tolerances positive
    bool stream_ext = false;         // the stream entry is selected and extensions are active (precision 2: they go there)
    int cus = 256;
};
struct LeanPlan {
    bool take = false;
    int variant = 0;                 // LV_*
    int form = LF_NONE;              // LF_*
    uint64_t sp = 0;                 // the pattern weighed against the model's: the built-in sparse kernels' or the model's own
    int cost_sparse = 0, cost_dense = 0;   // per-knot fp64 costs: of sp, and of the dense form it replaces (tmpc_lean_last_form)
};
LeanPlan lean_plan(const LeanPlanIn &);
// the (A, B) pattern of a solver's model (0: nx or nu above 4)
uint64_t lean_pattern(const Mat &A, const Mat &B);
// the lean kernel's fp64 pack (lean_layout); false when the family does not qualify (cache.AmBKt is not (A - B Kinf)')
// scaled (may be null): whether the pack's scaled block is valid for this model (lean_scale_model)
bool build_lean_pack(const Solver &, std::vector<double> &, bool *scaled = nullptr);
uint64_t lean_scale_model(uint64_t built, int nx, int nu, const double *A, const double *B, double *s);
void lean_scaled_coefficients(uint64_t sz, int nx, int nu, const double *A, const double *B, const double *K, const double *s,
                              double *Ah, double *Bh, double *Kh);
// ... and the one-lane-per-instance bound pack appended to it, for a solver whose selected entry keeps another layout
void append_lean_bounds(const Solver &, std::vector<double> &);
// One (nx, nu) instantiation of the run-time-horizon stream kernel (admm_streamg.hip.h).
struct StreamEntry {
    int nx, nu;
    int lanes;  // lanes per instance
    const char *name;
    void (*build_coef)(const Solver &, std::vector<unsigned char> &);
    void (*build_bounds)(const Solver &, std::vector<float> &);
    size_t (*lds_bytes)(int N, int precision);
    size_t (*scratch_floats)(int N, int sets);  // per instance; sets: 1 box, 2 + cones, 3 + linear
    hipError_t (*launch)(const AdmmParams &, int precision, int ext, bool het, hipStream_t);  // ext: 0 | 1 fdyn, cones | 2 + linear
    // the fp64-state form (precision 2: scratch, knot buffers, duals and the kept workspace in doubles; one family, fixed
    // rho) and the name it reports, "stream4<NX,NU;f64>" — both null where the form is not built (sinst_f64_*.hip)
    hipError_t (*launch_f64)(const AdmmParams &, int ext, hipStream_t) = nullptr;
    const char *name_f64 = nullptr;
    // the in-kernel closed loop (TINYMPC_HIP_STREAM_LOOP; sinst_mpc_*.hip), null where it is not built.  hipErrorNotSupported:
    // no loop kernel for that precision / family kind, nothing launched
    hipError_t (*launch_mpc)(const AdmmParams &, int precision, int ext, bool het, hipStream_t) = nullptr;
    bool (*has_mpc)(int precision, int ext, bool het) = nullptr;   // whether launch_mpc has a kernel for the call
    // the per-instance-bounds form (tinympc_set_instance_bounds; precision 0, one family or one per instance, fixed rho) and
    // the name it reports, "stream4<NX,NU;ib>" — both null where the form is not built (sinst_ib_*.hip)
    hipError_t (*launch_ib)(const AdmmParams &, int ext, bool het, hipStream_t) = nullptr;
    const char *name_ib = nullptr;
    // the per-instance-rows form (tinympc_set_instance_linear; the `ib` form with the instance's own rows), the name it
    // reports, "stream4<NX,NU;il>", and the LDS bytes its rows take behind the image of lds_bytes — null where the form is
    // not built (sinst_il_*.hip)
    hipError_t (*launch_il)(const AdmmParams &, bool het, hipStream_t) = nullptr;
    const char *name_il = nullptr;
    size_t (*il_lds_bytes)(int mlx, int mlu) = nullptr;
    // the per-instance-cones form (tinympc_set_instance_cones; the `il` form with the instance's own cone coefficients), the
    // name it reports, "stream4<NX,NU;ic>", and the LDS bytes its coefficients take behind the rows' slice — null where the
    // form is not built (sinst_ic_*.hip)
    hipError_t (*launch_ic)(const AdmmParams &, bool het, hipStream_t) = nullptr;
    const char *name_ic = nullptr;
    size_t (*ic_lds_bytes)(int ncx, int ncu) = nullptr;
};
const StreamEntry *find_stream_kernel(int nx, int nu);
// Per-instance families set up on the device (families_setup.hip; the rule: riccati.h).  The inputs are device pointers: A
// [batch][nx*nx] and B [batch][nx*nu] column-major as the caller gave them, the diagonals of Q and R [batch][nx] / [batch][nu]
// (rho not added) and rho [batch].
struct FamilyInputs {
    const double *A, *B, *Qdiag, *Rdiag, *rho;
};
bool families_shape_built(int nx, int nu);             // the stream kernel's grid: nx in {2,3,4,6,8,10,12}, nu <= 4
int families_cache_elems(int nx, int nu);              // doubles of one instance's cache image
size_t families_pack_elems(int nx, int nu, int lanes); // elements per column of the stream kernel's pack (0: not built for that)
// every instance's cache into img [element][batch], its sweep count (-1: singular) into sweeps [batch]
hipError_t families_riccati_launch(int nx, int nu, const FamilyInputs &in, int batch, double *img, int *sweeps, hipStream_t stream);
// the stream kernel's per-instance pack (fp64 rows, precision 1: fp32) into coef and [Qd | Rd | rho] into aux; fdyn: host, nx
hipError_t families_fill_launch(int nx, int nu, const double *img, const FamilyInputs &in, const double *fdyn, int batch, int precision,
                                void *coef, float *aux, hipStream_t stream);
// the rule on the host for one family: 0, 1 singular, -2 a shape outside the grid
int families_host_cache(int nx, int nu, const double *A, const double *B, const double *Qdiag, const double *Rdiag, double rho, double *Kinf,
                        double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps);
// One (nx, nu) instantiation of the LDS-resident matrix-core kernel with a run-time horizon (admm_mfmac.hip.h):
// one-shot solves with box bounds, the affine term and cones.
struct ConeEntry {
    int nx, nu;
    int N;                                      // compile-time horizon of the entry, 0: any (run-time horizon)
    bool (*supports)(const Solver &);           // further conditions of the entry (null: none)
    bool plain;                                 // box-only one-shot solves of the shape run here too (measured faster than the quad kernel)
    const char *name;
    void (*build_coef)(const Solver &, std::vector<unsigned char> &);
    void (*build_bounds)(const Solver &, std::vector<float> &);
    size_t (*lds_bytes)(const Solver &);        // per workgroup (one wavefront = 16 instances)
    size_t (*scratch_floats)(const Solver &);   // for the whole batch
    bool (*bounds_vary)(const Solver &);
    hipError_t (*launch)(const AdmmParams &, bool ext, size_t lds, hipStream_t);
    bool ws = false;                            // takes every kind of solve: warm starts, kept workspace, chunks, the fused closed loop
};
const ConeEntry *find_cone_kernel(int nx, int nu, int N);   // N = 0: the run-time-horizon entry only
const ConeEntry *find_trans_kernel(int nx, int nu, int N);  // the transposed-sets kernel of the shape (admm_mfmat.hip.h), or null
hipError_t launch_generic(const AdmmParams &, int precision, hipStream_t);
void build_generic_coef(const Solver &, std::vector<unsigned char> &);
void build_generic_bounds(const Solver &, std::vector<float> &);

// Environment switches (tuning / test aids), read once per solver at creation (read_switches)
struct Switches {
    int group = 0;          // TINYMPC_HIP_GROUP = 1 | 2 | 4: that lanes-per-instance variant, no matrix-core kernels
    bool strict_fp32 = false, no_quad = false, no_quad_adp = false, no_quad_adp1 = false, no_mfma = false, no_mfma_adp = false,
         mfma_oneshot_only = false, no_stream = false, no_stream_adp = false, no_mfmar = false, no_mfmac = false, mfmac_all = false,
         no_mfmat = false, mfmat_all = false, mfmat_ws_only = false, no_lean = false, no_refill = false,
         no_uni = false, no_os = false, lean_one = false,   // lean_one: TINYMPC_HIP_LEAN_ONE — the lean kernel's 512-register variant at any batch
         no_jit = false,                                    // TINYMPC_HIP_NO_JIT: no unit specialised at setup, loaded or not
         lean_dense = false,                                // TINYMPC_HIP_LEAN_DENSE: the lean kernel's dense sweeps only (no sparse form)
         lean_unscaled = false,                             // TINYMPC_HIP_LEAN_UNSCALED: the lean kernel's sparse sweeps on the model as given, never the diagonally scaled one (the A/B switch)
         lean_ws = false,                                   // TINYMPC_HIP_LEAN_WS: warm / kept-workspace solves and mpc_rollout on the lean kernel
         lean_loop = false,                                 // TINYMPC_HIP_LEAN_LOOP: with lean_ws, mpc_rollout as one launch of the lean kernel's in-kernel loop
         stream_f64 = false,                                // TINYMPC_HIP_STREAM_F64: precision 2 on the stream kernel's fp64-state form where it is built
         stream_mpc = false,                                // TINYMPC_HIP_STREAM_MPC: mpc_rollout on the stream and generic kernels (every precision), as the chain of launches
         stream_loop = false,                               // TINYMPC_HIP_STREAM_LOOP: with stream_mpc, one launch of the stream kernel's in-kernel loop where it is built
         event_markers = false,                             // TINYMPC_HIP_EVENT_MARKERS: profiled lean launches between separate event records
         noise_split = false,                               // TINYMPC_HIP_NOISE_SPLIT: measurement noise by a kernel of its own ahead of every launch (timing aid)
         estimator_split = false;                           // TINYMPC_HIP_ESTIMATOR_SPLIT: the estimator's predict and correct as two launches a step (the A/B arm of the fused form)
    int mfmac_debug = 0;    // timing probe builds only
    int fold_slots = -1;    // TINYMPC_HIP_FOLD_SLOTS = n: the status fold's records for the first n workgroups only (at most
                            // GSLOT_DEFAULT_CAP; 0: none, the accumulator path for all — the A/B switch); unset: all of them
};
Switches read_switches();

struct Settings {
    double abs_pri_tol = 1e-3, abs_dua_tol = 1e-3;  // TinyMPC.jl:57-58
    int max_iter = 100;                              // TinyMPC.jl:59
    int check_termination = 1;                       // TinyMPC.jl:59,202
    int en_state_bound = 0, en_input_bound = 0;      // TinyMPC.jl:94-95
    int en_state_soc = 0, en_input_soc = 0;          // TinyMPC.jl:96-97 (parity unpinned)
    int en_state_linear = 0, en_input_linear = 0;    // TinyMPC.jl:98-99 (parity unpinned)
    int adaptive_rho = 0, adaptive_rho_clip = 1;     // TinyMPC.jl:59-61,100-103
    double adaptive_rho_min = 0.1, adaptive_rho_max = 10.0;
};

// The device buffers sized by the batch.  A buffer declared HERE dies at a re-batch (Solver::free_batch assigns a fresh
// BatchBuffers over this part of the solver); one declared in Solver itself lives until the solver goes.
struct BatchBuffers {
    DevBuf<float> d_x0, d_xref, d_uref;   // (the reference arrays grow on demand: upload_refs, set_ref_trajectory)
    DevBuf<float> d_xout, d_uout, d_res;
    DevBuf<int> d_iter, d_solved;
    DevBuf<float> d_sd, d_sy, d_sz, d_sg, d_sv;
    DevBuf<float> d_scratch;
    DevBuf<double> d_ws64;                // precision 2: the fp64 workspace block (admm_generic.hip.h, Ws64)
    DevBuf<float> d_het_aux;
    DevBuf<float> d_ibx, d_ibu, d_il;     // per-instance bounds and rows in the kernels' layout
    DevBuf<float> d_ic;                   // per-instance cone coefficients, [state cones | input cones][instance]
    DevBuf<float> d_sgc, d_svc, d_syc, d_szc;
    DevBuf<int> d_idx[2], d_count;        // chunked solves: the index lists of the instances still iterating
    DevBuf<float> d_lin, d_sgl, d_svl, d_syl, d_szl;
    DevBuf<double> d_adapt;
    DevBuf<unsigned char> d_adp_cols;     // stream kernel, adaptive rho: per-lane coefficient columns (scratch)
    DevBuf<double> d_x0d;                 // [B][nx] plant state
    DevBuf<float> d_mpc_x, d_mpc_u;       // closed-loop logs
    DevBuf<int> d_mpc_iter;
    DevBuf<float> d_mpc_y, d_mpc_yout;
    DevBuf<float> d_xref_seq, d_uref_seq; // shared references of every step of a fused closed loop
    DevBuf<double> d_metrics, d_metric_cfg, d_metric_part;
    DevBuf<double> d_est_C, d_est_L, d_xhat;
};

struct Solver : BatchBuffers {
    int nx = 0, nu = 0, N = 0, batch = 1, device = 0;
    int verbose = 0;
    Mat A, B, Q, R;
    Cache cache;
    Settings st;
    // per-knot bounds, column-major fp64 (nx x N, nu x (N-1)); +-1e17 until set
    std::vector<double> x_min, x_max, u_min, u_max;
    // Box bounds PER INSTANCE (tinympc_set_instance_bounds).  bounds_mode 0: the shared set above; 1: one column per instance,
    // constant over the horizon (ib_x* nx x batch, ib_u* nu x batch); 2: per instance and knot (ib_x* [batch][N][nx], ib_u*
    // [batch][N-1][nu]).  The host copies are the caller's fp64 arrays as given (they survive a change of precision or of the
    // settings); the device arrays hold them transposed to the kernels' layout (AdmmParams::ibx).  Such a solver runs on the
    // `ib` forms of the stream and generic kernels only: the on-chip families' packs hold one bound image.
    int bounds_mode = 0;
    std::vector<double> ib_xmin, ib_xmax, ib_umin, ib_umax;
    int set_instance_bounds(const double *xmin, const double *xmax, const double *umin, const double *umax, int per_knot);
    void drop_instance_bounds();
    int upload_instance_bounds();
    bool ib_by_knot = false;   // the device arrays' layout as last uploaded: per knot, or one line per instance
    // Linear rows PER INSTANCE (tinympc_set_instance_linear).  lin_mode 0: the shared set below (or none); 1: mlx / mlu rows a
    // side, every instance its own — il_Ax [batch] blocks of mlx x nx column-major, il_bx [batch][mlx], the input side alike,
    // the caller's fp64 arrays as given (they survive a change of precision or of the settings); d_il holds them rounded and
    // transposed to the kernels' layout (AdmmParams::il_ax).  An all-zero row of an instance is that instance's absent row; a
    // side that is enabled carries its slack and dual for every instance, those without a row on it included (so does a
    // shared set whose rows never act).  Such a solver runs on the `il` forms of the stream and generic kernels only, which
    // read their bounds per instance as the `ib` forms do (shared bounds are uploaded replicated).
    int lin_mode = 0;
    std::vector<double> il_Ax, il_bx, il_Au, il_bu;
    int set_instance_linear(const double *Ax, int mx, const double *bx, const double *Au, int mu, const double *bu);
    void drop_instance_linear();
    int upload_instance_linear();
    // Cone coefficients PER INSTANCE (tinympc_set_instance_cones).  cone_mode 0: the shared set below (or none); 1: the layout
    // below (ncx / ncu, Acx .. qcu) is the batch's and every instance has its own mu — ic_cx [batch][ncx], ic_cu [batch][ncu],
    // the caller's fp64 arrays as given (they survive a change of precision or of the settings; cx[] / cu[] below then hold
    // nothing the kernels read); d_ic holds them rounded and transposed to the kernels' layout (AdmmParams::ic_cx).  +inf: the
    // instance does not have the cone; a side that is enabled carries its slack and dual for every instance, those without a
    // cone on it included (so does a shared set whose cones never act).  Such a solver runs on the `ic` forms of the stream
    // and generic kernels only, which are `il` forms: they read their bounds and their rows per instance (shared ones are
    // uploaded replicated: upload_instance_bounds, upload_instance_linear).
    int cone_mode = 0;
    std::vector<double> ic_cx, ic_cu;
    int set_instance_cones(const int *Acu, const int *qcu, const double *cu, int ncu, const int *Acx, const int *qcx,
                           const double *cx, int ncx);
    void drop_instance_cones();
    int upload_instance_cones();
    // affine dynamics term and cone constraints (parity UNPINNED: they exist only in the absent
    // TinyMPC submodule; run on the stream kernel, or the generic one for shapes outside its grid)
    std::vector<double> fdyn;  // nx, all zero by default
    bool has_fdyn = false;
    int ncx = 0, ncu = 0;
    int Acx[8] = {0}, qcx[8] = {0}, Acu[8] = {0}, qcu[8] = {0};
    double cx[8] = {0}, cu[8] = {0};
    bool cones_active() const { return (st.en_state_soc && ncx > 0) || (st.en_input_soc && ncu > 0); }
    // linear inequalities Alin_x x <= blin_x, Alin_u u <= blin_u at every knot (bindings.cpp:413-450; UNPINNED):
    // rows row-major fp64, at most LIN_MAX_ROWS per side
    int mlx = 0, mlu = 0;
    std::vector<double> lin_Ax, lin_bx, lin_Au, lin_bu;
    bool lin_dirty = false;
    bool lin_active() const { return (st.en_state_linear && mlx > 0) || (st.en_input_linear && mlu > 0); }
    // constraint sets whose arrays the stream / generic scratch lays out: box | + cones | + linear
    int constraint_sets() const { return lin_active() ? 3 : (cones_active() ? 2 : 1); }
    // adaptive rho (admm.cpp:147-174): sensitivities d(Kinf | Pinf)/d rho of the family (column-major, set by the
    // caller or computed on first use as TinyMPC.jl:301-352 does) and each instance's own (rho, Kinf, Pinf) on the
    // device; generic kernel only
    std::vector<double> sens;
    bool sens_set = false, sens_dirty = true, adapt_dirty = true;
    // the adaptive state on the device is `family + (rho_b - rho_family) x tables` with the CURRENT tables (what every
    // adaptive kernel leaves; false once the tables change under a live state): the matrix-core variant rebuilds an instance's
    // Kinf / Pinf from rho_b alone
    bool adapt_pure = true;
    DevBuf<double> d_sens;
    int set_sensitivity(const double *dK, const double *dP);
    int get_adaptive_state(double *rho, double *Kinf, double *Pinf);
    // one problem family PER INSTANCE: per-instance A, B (column-major, concatenated),
    // Riccati caches and diag/rho scalars; runs on the stream kernel with per-lane coefficient columns
    bool hetero = false;
    bool no_specialise = false;   // init() does not compile an on-chip unit for the shape (jit.cpp)
    bool layout_final = false;    // a constraint layout is specialised (jit_trans_for) from the first solve on, not while the setters run
    std::vector<double> het_A, het_B;
    std::vector<Cache> het_cache;
    // Where the families were set up.  Host (tinympc_create_families): het_cache holds every instance's cache
    // and upload_packs builds the coefficient pack from it on the host.  Device (tinympc_create_families_device,
    // tinympc_set_families): het_cache is EMPTY; the caches are the fp64 image d_het_cache [element][batch] (riccati.h:
    // Riccati<NX,NU>::E_*) written by riccati_families_kernel, d_het_sweeps [batch] its sweep counts, d_fam_* the inputs it read
    // (A, B as given, the diagonals of Q and R, rho), and upload_packs has fill_family_pack_kernel write d_coef and d_het_aux
    // from them (families_setup.hip).  In both modes the host keeps A and B (the plant image and the estimator's predict read
    // them), the diagonals of Q and R as given and rho (what a partial set_families keeps).
    enum { FAM_NONE = 0, FAM_HOST = 1, FAM_DEVICE = 2 };
    int fam_mode = FAM_NONE;
    std::vector<double> het_Qdiag, het_Rdiag, het_rho;   // [batch][nx], [batch][nu], [batch]
    DevBuf<double> d_het_cache, d_fam_A, d_fam_B, d_fam_Qdiag, d_fam_Rdiag, d_fam_rho;
    DevBuf<int> d_het_sweeps;
    float fam_ms[2] = {-1.f, -1.f};   // kernel times of the last device setup and the last device pack fill (-1: none has run)
    // replaces every instance's family (null pairs / rho: kept) by a device setup; commits only if no instance is singular
    int set_families(const double *A_, const double *B_, const double *Q_, const double *R_, const double *rho_);
    int get_family_cache(int first, int count, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps);
    int fill_family_pack();   // device mode's part of upload_packs
    void family_diagonals(const double *Q_, const double *R_, const double *rho_);   // het_Qdiag / het_Rdiag / het_rho from what is given
    // references as last set by the host API: kind 0 zero / 1 shared / 2 per instance
    std::vector<float> h_xref, h_uref;
    int xref_kind = 0, uref_kind = 0;
    bool refs_dirty = true;
    bool refs_device_owned = false;  // caller writes d_xref/d_uref itself (tinympc_set_ref_mode)
    // the references the next launch will see are per instance ([B][N][nx] / [B][N-1][nu], upload_refs)
    bool refs_per_instance() const { return refs_device_owned ? ref_mode == REF_PER_INSTANCE : (xref_kind >= 2 || uref_kind >= 2); }
    int ref_mode = REF_ZERO;
    bool warm_start = true;
    bool cache_overridden = false;  // set_cache_terms replaced the host Riccati's terms
    bool packs_dirty = true;
    bool state_bounds_active = false;  // any finite (|b| < 1e17) enabled state bound
    const KernelEntry *ke = nullptr;  // specialised quad kernel, or
    const StreamEntry *se = nullptr;  // run-time-horizon stream kernel, or
    const ConeEntry *ce = nullptr;    // LDS-resident matrix-core kernel (one-shot solves), or (all null) the generic kernel
    std::string kernel_name;
    // the lean kernel of the shape (admm_lean.hip.h; lean_plan decides per launch); its pack, and whether the family
    // qualifies (build_lean_pack)
    const LeanEntry *le = nullptr;
    bool lean_jit = false;                // no built-in lean instantiation: single variants specialised at the launches that need them
    const LeanEntry *le_var[LV_COUNT] = {};
    bool le_var_tried[LV_COUNT] = {};
    DevBuf<double> d_lean;
    bool lean_ok = false, lean_knot_bounds = false;
    bool lean_enabled = true;             // TINYMPC_HIP_NO_LEAN, read once at creation
    uint64_t lean_sp = 0;                 // the (A, B) pattern of the model (lean_pattern), set with the pack
    bool lean_scaled_ok = false;          // the pack's scaled block is valid for this model (build_lean_pack)
    bool last_lean_scaled = false;        // the most recent launch ran a scaled sparse kernel
    int last_lean_form = LF_NONE;         // the sweeps of the most recent launch (LF_*), and the per-knot fp64 costs it
    int last_lean_cost[2] = {0, 0};       // weighed: the sparse form's (its pattern's), the form it replaces
    std::string last_launch_name;         // the kernel the most recent launch actually ran (family or its lean variant)
    // device buffers that survive a re-batch (those that do not: BatchBuffers)
    DevBuf<unsigned char> d_coef;
    DevBuf<float> d_bounds;
    DevBuf<uint32_t> d_gstat;     // [2 * GSTAT_WORDS]: the public status block, then the kernels' accumulator
    DevBuf<uint32_t> d_gslot;     // [GSLOT_DEFAULT_CAP][GSLOT_WORDS]: the workgroups' status records (fold_status), never zeroed
    PinnedBuf<uint32_t> h_gstat;
    // host round trips (fp64 caller buffers <-> fp32 device buffers): pinned staging, copy stream, two chunk slots
    PinnedBuf<float> h_stage;
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_copy[2] = {nullptr, nullptr};
    int d2h_double(const float *d, double *out, size_t n);
    // fp32 host buffers of the *_f32 entry points: page-locked on first sight (at most 8 ranges, of at least 1 MB) so that
    // the copies of a caller who reuses its buffers are direct DMAs; unlocked when the solver is destroyed
    std::vector<std::pair<void *, size_t>> pinned_ranges;
    int pin_host_range(void *p, size_t bytes);
    int unpin_host_range(void *p);
    int h2d_float(float *d, const double *in, size_t n);
    int mpc_cap = 0, mpc_steps_last = 0;
    bool solved_once = false;
    bool g_maybe_nonzero = false;  // the workspace's state dual may hold non-zeros (see launch_pass)
    bool profiling = false;
    static constexpr int EV_RING = 256;  // event pairs around the most recent launches (profiling mode)
    std::vector<hipEvent_t> ev_ring;     // [2 * EV_RING], created on first use
    long launches = 0;                   // launches recorded since profiling was switched on
    int precision = 0;  // 0: fp64 recurrences, fp32 state (default), 1: all fp32, 2: all fp64 (lean / stream / generic kernel's fp64-state form)

    int ex() const { return nx * N; }
    int eu() const { return nu * (N - 1); }

    ~Solver();
    int init(const double *A_, const double *B_, const double *Q_, const double *R_, double rho,
             int nx_, int nu_, int N_, int batch_, int device_, int verbose_);
    int init_families(const double *A_, const double *B_, const double *Q_, const double *R_, const double *rho_,
                      int nx_, int nu_, int N_, int batch_, int device_, int verbose_, bool on_device = false);
    int alloc_batch(int batch_);
    // family-level state of another solver of the SAME family (settings, bounds, affine term, cones, linear rows, cache,
    // sensitivities, precision / warm-start / compaction switches): what set_gpus() replays onto fresh shards
    int copy_family_state(const Solver &o);
    // last launch of this solver, whatever stream it went to: every getter waits for it first
    // (a profiled lean launch carries its timing events in its own packet: its stop event is then the one waited for)
    hipEvent_t ev_done = nullptr, ev_wait = nullptr;
    bool ev_done_pending = false;
    int wait_last_launch();
    int select_kernel(bool rollout = false);  // rollout: for a closed loop (plan_rollout)
    // routing (solver.hip, "kernel routing"): switches, the families' routes, the cached decision
    Switches sw;
    bool strict_precision = false;            // tinympc_set_strict_precision: precision = 1 really means fp32 recurrences
    bool strict_fp32() const { return precision != 0 && (sw.strict_fp32 || strict_precision); }
    bool extensions_active() const { return has_fdyn || cones_active() || lin_active(); }
    bool rollout_on_quad() const { return sw.mfma_oneshot_only || !warm_start; }
    const KernelEntry *route_quad(bool rollout) const;
    const KernelEntry *route_mfma(bool rollout, const KernelEntry *quad) const;
    const StreamEntry *route_stream() const;
    const StreamEntry *route_stream_f64() const;   // precision 2, TINYMPC_HIP_STREAM_F64
    const ConeEntry *route_cone(bool rollout, bool have_quad, bool have_stream) const;
    const ConeEntry *route_trans(bool rollout, const ConeEntry *oneshot) const;
    std::vector<long> routing_key(bool rollout) const;
    bool bounds_vary_by_knot() const;   // do the enabled box bounds depend on the knot?
    std::vector<long> routed_key;
    bool routed = false;
    unsigned route_gen = 0;                   // bumped by setters whose effect on routing the key's scalars do not show
    void free_batch();
    int upload_packs();
    int upload_refs();
    int set_x0(const double *x0, int cols);
    int set_ref(bool is_x, const double *ref, int cols);
    int set_ref_sequence(const double *x_seq, const double *u_seq, int steps);
    int ref_seq_steps = 0;
    int set_bounds(const double *xmin, const double *xmax, const double *umin, const double *umax);
    int set_fdyn(const double *f);
    int set_cones(const int *Acu_, const int *qcu_, const double *cu_, int ncu_, const int *Acx_, const int *qcx_,
                  const double *cx_, int ncx_);
    int set_linear(const double *Ax, int mx, const double *bx, const double *Au, int mu, const double *bu);
    int ensure_extension_buffers();
    int reset();
    int solve_async(hipStream_t stream, int mpc_steps = 0);
    // one kernel launch over `slots` instances (idx: their ids, NULL = 0..slots-1) for at most `iters` iterations, the
    // instances having done `iter_offset` already
    struct Pass {
        const int *idx = nullptr;
        int slots = 0, iter_offset = 0, iters = 0;
        bool cold = false, save = false;
        int mpc_steps = 0;
        const double *x0d = nullptr;                        // the fp64 plant state of a closed loop stepped outside the quad kernel
        const float *xref = nullptr, *uref = nullptr;       // shared references where not the solver's own (a step of a reference sequence)
        bool loop = false;                                  // the lean kernel's in-kernel closed loop (plan_rollout found its kernel)
        bool stream_loop = false;                           // the stream kernel's in-kernel closed loop (likewise)
    };
    Pass whole_batch(bool cold, bool save, int mpc_steps = 0) const;
    int launch_pass(hipStream_t stream, const Pass &);
    LeanPlan plan_lean(const Pass &) const;                 // lean_plan of this solver and that launch
    // the lean entry and variant that take a launch (null: the selected family's kernel runs it), and whether the stream kernel's
    // in-kernel loop is built for it: asked by launch_pass for the launch, by plan_rollout before anything is launched
    struct Pick {
        LeanPlan plan;
        const LeanEntry *lean = nullptr;
        bool stream_loop = false;
    };
    Pick pick_kernel(const Pass &);
    void fill_params(AdmmParams &P, const Pass &) const;
    int ensure_mpc_log(int mpc_steps);                      // the closed loops' log buffers
    int record_done(hipStream_t stream, hipEvent_t carried = nullptr);   // the completion event every getter waits for
    // tolerance-terminated solves of big batches in chunks of `chunk_iters` iterations: after each chunk the
    // instances still iterating are compacted, so wavefronts do not idle behind their slowest instance
    int solve_chunked(hipStream_t stream);
    // mpc_rollout.  plan_rollout decides the route, once and before anything is launched — every condition and every refusal
    // of a closed loop is there (solver.hip) — and solve_async launches it:
    //   Fused       the loop inside the selected kernel (the lanes-per-instance kernels, mfmat): one launch_pass
    //   Chain       per step one workspace-carrying launch and the plant step (plant_step_kernel), stream-ordered, the plant
    //               state kept in fp64 on the device between steps: rollout_chain.  mfma and the lean kernel under
    //               TINYMPC_HIP_LEAN_WS, whose launches read the fp64 state; from_x0 — the stream / generic kernels under
    //               TINYMPC_HIP_STREAM_MPC, and an own-plant solver or one with a reference trajectory on whatever kernel a
    //               kept-workspace solve of it takes, no switch — every launch from the fp32 state, the fp64 state resumed
    //   LeanLoop    ONE launch of the lean kernel's in-kernel loop (TINYMPC_HIP_LEAN_LOOP)
    //   StreamLoop  ONE launch of the stream kernel's (TINYMPC_HIP_STREAM_LOOP)
    //   Refused     the reason is the last error
    enum class Rollout { Refused, Fused, Chain, LeanLoop, StreamLoop };
    struct RolloutPlan {
        Rollout route = Rollout::Refused;
        bool from_x0 = false;   // Chain: the launches start from the fp32 d_x0 (Pass::x0d null) and the fp64 plant state resumes (plant_start)
    };
    RolloutPlan plan_rollout(int mpc_steps);
    int rollout_chain(hipStream_t stream, int mpc_steps, bool from_x0);
    int rollout_loop(hipStream_t stream, int mpc_steps, Rollout route);   // LeanLoop | StreamLoop
    int stream_ext() const { return lin_active() ? 2 : ((has_fdyn || cones_active()) ? 1 : 0); }   // the stream kernel's EXT of this solver
    int last_rollout_launches = -1;               // solve-kernel launches of the last mpc_rollout enqueued (-1: none has run)
    // The plant of every chain, one image: d_plant is [A | B | f] column-major fp64, one block or [batch] blocks plant_stride()
    // apart — the installed plant (set_plant), else the model's A, B and affine term (a family solver: every instance's A_b, B_b
    // and the shared f).  plant_dirty: to be (re)written by ensure_plant before the next chain — set_plant, set_fdyn, a re-batch.
    DevBuf<double> d_plant;
    bool plant_dirty = true;
    bool x0d_live = false;                        // d_x0d holds the plant state a from_x0 chain or the stream loop left (plant_start)
    int plant_start(hipStream_t stream, bool resume);   // x0d <- x0, or (resume, x0d_live) the state the last loop left where x0 still is its rounding
    int ensure_plant();
    // A plant of its own (tinympc_set_plant) and an additive disturbance (tinympc_set_disturbance): what mpc_rollout steps when it
    // is not the model, x+ = f_p + A_p x + B_p u0 (+ w).  plant_kind / dist_kind 0: none, 1: shared, 2: per instance.  Host copies
    // are the caller's fp64 arrays as given (own_A [batch][nx*nx] etc. when per instance; dist_w nx x steps or [batch][steps][nx]);
    // on the device the plant is d_plant's content and d_dist is the disturbance as given.  Either makes the solver an own-plant
    // solver, whose closed loop is the chain on the kernel a kept-workspace solve takes (plan_rollout).
    int plant_kind = 0, dist_kind = 0, dist_steps = 0;
    std::vector<double> own_A, own_B, own_f, dist_w;
    DevBuf<double> d_dist;
    bool own_plant() const { return plant_kind != 0 || dist_kind != 0 || noisy() || estimating(); }
    bool own_plant_per_instance() const { return plant_kind == 2 || (plant_kind == 0 && hetero); }
    long plant_stride() const { return own_plant_per_instance() ? (long)nx * nx + (long)nx * nu + nx : 0L; }
    int plant_mode() const { return plant_kind | (dist_kind == 1 ? 4 : (dist_kind == 2 ? 8 : 0)); }
    int set_plant(const double *A_, const double *B_, const double *f_, int per_instance);
    int set_disturbance(const double *w, int steps, int per_instance);
    void drop_own_plant();   // both pieces (a re-batch)
    // Seeded process and measurement noise drawn on the device (tinympc_set_process_noise / _set_measurement_noise; the draw rule:
    // noise.h).  Index 0 process, 1 measurement; noise_kind 0: none, 1: a shared factor, 2: one per instance.  The factors G (nx x nx
    // column-major fp64, or [batch][nx*nx]) are kept as given on the host and the device; a draw is a pure function of (seed, kind,
    // instance, step t), t = noise_cursor + loop step, so nothing else is stored.  Either kind makes the solver an own-plant solver:
    // the solve of step t starts from (float)(x_t + G_v xi_v[b][t]) — logged in d_mpc_y [batch][steps][nx], allocated only while
    // measurement noise is installed — and the plant step ends with (acc + w) + (G_w xi_w[b][t]) (plant_step_kernel's noise form); x0d, the
    // x log and x0 after the loop hold the true state.  One cursor serves both kinds; a loop leaves it steps further on.
    int noise_kind[2] = {0, 0};
    unsigned long long noise_seed[2] = {0, 0};
    int noise_cursor = 0;
    std::vector<double> noise_G[2];
    DevBuf<double> d_noise_G[2];
    int mpc_y_cap = 0, mpc_y_steps = 0;   // steps allocated; steps of the loop that wrote it (0: none)
    bool noisy() const { return noise_kind[0] != 0 || noise_kind[1] != 0; }
    int noise_mode() const { return noise_kind[0] | (noise_kind[1] == 1 ? 4 : (noise_kind[1] == 2 ? 8 : 0)); }
    int set_noise(int which, const double *G, int per_instance, unsigned long long seed);
    void drop_noise();   // both kinds (a re-batch)
    int get_noise(int which, int t0, int steps, double *buf);
    int get_mpc_measured(double *y);
    // Output feedback through a fixed-gain state estimator stepped on the device (tinympc_set_estimator; the rule: estimator.h; the
    // kernels and this block's functions: estimator.hip).  est_kind 0: none, 1: shared C (ny x nx) and L (nx x ny), 2: [batch] of
    // each, column-major fp64, kept as given on the host and the device.  Such a solver is an own-plant solver (the from_x0 chain):
    // the solve of step t starts from (float)(xhat_t), xhat_t = xhat-_t + L (y_t - C xhat-_t), y_t = C x_t + v_t (v_t: the first ny
    // rows of the measurement noise, where installed), and behind the plant step xhat-_{t+1} = f + A xhat_t + B u_t with the MODEL
    // (d_model: the model's image where a plant is installed, built by ensure_plant; else d_plant is the model).  d_xhat [batch][nx]
    // fp64: xhat- of the next step between rollouts (xhat_t between a step's correct and its predict); xhat_live false: the next
    // rollout takes xhat-_0 = (double)x0.  Logs: d_mpc_y takes (float)xhat_t, d_mpc_yout [batch][steps][ny] (float)y_t.
    int est_kind = 0, est_ny = 0;
    std::vector<double> est_C, est_L;
    DevBuf<double> d_model;
    bool xhat_live = false;
    int mpc_yout_cap = 0, mpc_yout_steps = 0;   // steps x ny floats allocated per instance / ny; steps of the loop that wrote it
    bool estimating() const { return est_kind != 0; }
    long model_stride() const { return hetero ? (long)nx * nx + (long)nx * nu + nx : 0L; }
    int set_estimator(const double *C, int ny, const double *L, int per_instance);
    void drop_estimator();   // (a re-batch)
    int set_estimator_state(const double *xhat, int per_instance);
    int get_estimator_state(double *xhat);
    int get_mpc_estimate(double *xhat);
    int get_mpc_outputs(double *y);
    int ensure_estimator_logs(int mpc_steps);
    // one launch of estimator_step_kernel<predict, correct> on the chain's stream; step: the loop step whose solve the correct part
    // feeds (its log row, its draw t = noise_cursor + step)
    int estimator_step(hipStream_t stream, bool predict, bool correct, int mpc_steps, int step);
    // A reference trajectory (tinympc_set_ref_trajectory): x_traj Lx rows of nx and optionally u_traj Lu rows of nu, shared or
    // [batch][L][n] per instance, rounded to fp32 once when set; the references of a solve are its window at the cursor,
    // x_ref[k] = x_traj[min(c + k, Lx - 1)], u_ref[k] = u_traj[min(c + k, Lu - 1)] (no u_traj: zero).  traj_kind 0: none, 1: shared,
    // 2: per instance.  While one is installed the references are device-owned in the trajectory's mode (refs_device_owned with
    // ref_mode, what every route already keys on) and ref_window_kernel cuts the window into d_xref / d_uref whenever the one
    // there (traj_dev_cursor, -1: none) is not the one the next launch needs: before a plain solve's launch, and per step in
    // the chain — such a solver's mpc_rollout is the own-plant chain against the model (or the installed plant), and leaves the
    // cursor steps further on.  The host copies serve the drop, which installs the window at the cursor as ordinary references.
    int traj_kind = 0, traj_Lx = 0, traj_Lu = 0;   // traj_Lu 0: no u_traj
    int ref_cursor = 0, traj_dev_cursor = -1;
    std::vector<float> h_xtraj, h_utraj;
    DevBuf<float> d_xtraj, d_utraj;
    int set_ref_trajectory(const double *x_traj, int Lx, const double *u_traj, int Lu, int per_instance);
    int drop_ref_trajectory(bool install_window);   // install_window: the window at the cursor becomes the ordinary references
    int ensure_ref_window(hipStream_t stream, int cursor);
    // Per-instance closed-loop metrics folded on the device (tinympc_set_rollout_metrics; the rule: metrics.h; the kernels:
    // metrics.hip).  While enabled every mpc_rollout enqueues rollout_metrics_kernel on its stream behind its route, whatever the
    // route: it reads the log the route wrote and the references its solves used, and updates d_metrics [batch][11] fp64, which
    // therefore accumulates across rollouts until reset_rollout_metrics.  d_metric_cfg: the weights and limits ([qw | rw | x_lo |
    // x_hi | u_lo | u_hi], metric_limits bit 0..3: that limit array was given); d_metric_part: the summary's partials and result.
    // A solver without them launches what it launched before.  set_precision keeps them, a re-batch drops them (free_batch).
    bool metrics_on = false;
    int metric_limits = 0;
    int set_rollout_metrics(int enable, const double *qw, const double *rw, const double *x_lo, const double *x_hi, const double *u_lo,
                            const double *u_hi);
    int reset_rollout_metrics();
    void drop_rollout_metrics();
    int fold_rollout_metrics(hipStream_t stream, int mpc_steps, int cursor0);
    int get_rollout_metrics(double *per_instance);
    int get_rollout_summary(double *summary);
    int chunk_iters = 0;  // 0: off
    int get_mpc_log(double *x, double *u, int *iter);
    int solve_status();
    double kernel_elapsed_ms();
    double kernel_elapsed_mean_ms(int last_n);
    int get_traj(bool states, double *buf);
    int get_status(int *iter, int *solved, double *res4);
    int get_workspace(double *d, double *y, double *g, double *v, double *z);
    int set_workspace(const double *d, const double *y, const double *g, const double *v,
                      const double *z);
};

void set_error(const std::string &msg);
const char *last_error();
bool hip_ok(hipError_t e, const char *what);

}  // namespace tmpc

struct tinympc_solver {
    tmpc::Solver s;
};
