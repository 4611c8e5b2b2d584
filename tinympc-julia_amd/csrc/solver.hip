// Host side of the batched solver: device memory, pack uploads, launches.
#include "solver.h"
#include "admm_generic.hip.h"   // Ws64 (layout of the precision-2 workspace)
#include "noise.h"              // the draw rule of the closed loop's noise (host and device)
#include "riccati.h"            // the Riccati rule's constants (families set up on the device: families_setup.hip)

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cstring>
#include <thread>


namespace tmpc {

static thread_local std::string g_err;
void set_error(const std::string &msg) {
    g_err = msg;
    std::fprintf(stderr, "tinympc_hip: %s\n", msg.c_str());
}
const char *last_error() { return g_err.c_str(); }
bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
#define HIP_TRY(expr)                       \
    do {                                    \
        if (!hip_ok((expr), #expr)) return -1; \
    } while (0)

// fp32 <-> fp64 conversion of the host-side staging buffers, spread over a few threads: at batch 65 536
// a solution is 6.5 M elements and a single-threaded loop costs more than the kernel that produced it.
// The workers are started once and parked on a condition variable: spawning 16 threads per call costs ~0.5 ms,
// more than the copy they help with.
class HostPool {
public:
    static HostPool &get() {
        static HostPool pool;
        return pool;
    }
    // runs f(lo, hi) over [0, n) in `parts` contiguous ranges, part 0 on the calling thread
    void run(size_t n, size_t parts, const std::function<void(size_t, size_t)> &f) {
        std::unique_lock<std::mutex> outer(call_);  // one parallel region at a time
        parts = std::min(parts, workers_.size() + 1);
        const size_t chunk = (n + parts - 1) / parts;
        {
            std::lock_guard<std::mutex> lk(m_);
            fn_ = &f;
            n_ = n;
            chunk_ = chunk;
            next_ = 1;
            parts_ = parts;
            pending_ = parts - 1;
        }
        cv_.notify_all();
        f(0, std::min(n, chunk));
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    HostPool() {
        const unsigned hw = std::thread::hardware_concurrency();
        const unsigned nt = std::min<unsigned>(hw ? hw : 1, 16);
        for (unsigned i = 1; i < nt; ++i) workers_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }
    void loop() {
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return stop_ || next_ < parts_; });  // parked until a region has an unclaimed part
            if (stop_) return;
            const size_t part = next_++;
            const auto *f = fn_;
            const size_t lo = part * chunk_, hi = std::min(n_, lo + chunk_);
            lk.unlock();
            if (lo < hi) (*f)(lo, hi);
            lk.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_, call_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t n_ = 0, chunk_ = 0, next_ = 0, parts_ = 0, pending_ = 0;
    bool stop_ = false;
};

template <class F>
static void parallel_chunks(size_t n, F &&f, size_t min_parallel = (size_t)1 << 16) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = n < min_parallel ? 1 : std::min<size_t>(hw ? hw : 1, 16);
    if (nt <= 1) {
        f((size_t)0, n);
        return;
    }
    HostPool::get().run(n, nt, std::function<void(size_t, size_t)>(f));
}
static void widen(const float *src, double *dst, size_t n) {
    parallel_chunks(n, [=](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) dst[i] = (double)src[i];
    });
}
static void narrow(const double *src, float *dst, size_t n) {
    parallel_chunks(n, [=](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) dst[i] = (float)src[i];
    });
}

// every device allocation of the library (devbuf.h), and the bytes of them that are live (tmpc_device_bytes_live)
static std::atomic<long long> g_device_bytes{0};
int device_alloc_bytes(void **p, size_t bytes) {
    *p = nullptr;
    HIP_TRY(hipMalloc(p, bytes));
    g_device_bytes += (long long)bytes;
    return 0;
}
void device_free_bytes(void *p, size_t bytes) {
    (void)hipFree(p);
    g_device_bytes -= (long long)bytes;
}

// (the buffers go with the members that own them)
Solver::~Solver() {
    for (const auto &r : pinned_ranges) (void)hipHostUnregister(r.first);
    pinned_ranges.clear();
    free_batch();
    for (hipEvent_t e : ev_ring)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_copy)
        if (e) (void)hipEventDestroy(e);
    if (s_copy) (void)hipStreamDestroy(s_copy);
    if (ev_done) (void)hipEventDestroy(ev_done);
}

// Getters are synchronous, and a solve may have been enqueued on any stream (tinympc_solve_async): they wait for the
// event recorded behind the last launch rather than relying on null-stream ordering, which a non-blocking stream escapes.
int Solver::wait_last_launch() {
    if (ev_done_pending) {
        HIP_TRY(hipEventSynchronize(ev_wait));
        ev_done_pending = false;
    }
    return 0;
}

int Solver::copy_family_state(const Solver &o) {
    if (o.nx != nx || o.nu != nu || o.N != N || hetero || o.hetero) {
        set_error("copy_family_state: solvers of different shape");
        return -1;
    }
    // per-instance rows and cone coefficients are per-instance inputs, not family state, on either side: this solver's own go
    // first, and a source that carries them hands over no rows / no cones (its shared cx[] / cu[] hold nothing valid then)
    drop_instance_linear();
    drop_instance_cones();
    st = o.st;
    x_min = o.x_min, x_max = o.x_max, u_min = o.u_min, u_max = o.u_max;
    fdyn = o.fdyn, has_fdyn = o.has_fdyn;
    ncx = o.cone_mode ? 0 : o.ncx, ncu = o.cone_mode ? 0 : o.ncu;
    for (int i = 0; i < 8; ++i) {
        Acx[i] = o.Acx[i], qcx[i] = o.qcx[i], cx[i] = o.cx[i];
        Acu[i] = o.Acu[i], qcu[i] = o.qcu[i], cu[i] = o.cu[i];
    }
    mlx = o.lin_mode ? 0 : o.mlx, mlu = o.lin_mode ? 0 : o.mlu;
    lin_Ax = o.lin_Ax, lin_bx = o.lin_bx, lin_Au = o.lin_Au, lin_bu = o.lin_bu;
    lin_dirty = true;
    cache = o.cache;
    sens = o.sens, sens_set = o.sens_set, sens_dirty = true, adapt_dirty = true;
    warm_start = o.warm_start;
    cache_overridden = o.cache_overridden;
    precision = o.precision;
    strict_precision = o.strict_precision;
    chunk_iters = o.chunk_iters;
    packs_dirty = true;
    return select_kernel() || ensure_extension_buffers();
}

void Solver::free_batch() {
    static_cast<BatchBuffers &>(*this) = BatchBuffers{};
    x0d_live = false;
    adapt_dirty = true;
    mpc_y_steps = 0;
    ref_seq_steps = 0;
    mpc_cap = 0;
    drop_rollout_metrics();   // (per-instance accumulators, and their configuration with them)
    drop_estimator();         // (the estimate is per instance, the matrices may be)
}

int Solver::init(const double *A_, const double *B_, const double *Q_, const double *R_, double rho,
                 int nx_, int nu_, int N_, int batch_, int device_, int verbose_) {
    if (nx_ < 1 || nu_ < 1 || N_ < 2 || batch_ < 1) {
        set_error("invalid dimensions (need nx >= 1, nu >= 1, N >= 2, batch >= 1)");
        return -1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return -1;
    }
    if (device_ < 0) HIP_TRY(hipGetDevice(&device_));
    device = device_;
    HIP_TRY(hipSetDevice(device));
    sw = read_switches();   // the environment, once per solver
    lean_enabled = !sw.no_lean;
    nx = nx_;
    nu = nu_;
    N = N_;
    verbose = verbose_;
    A = Mat(nx, nx, A_);
    B = Mat(nx, nu, B_);
    Q = Mat(nx, nx, Q_);
    R = Mat(nu, nu, R_);
    if (precompute_cache(A, B, Q, R, rho, cache) != 0) {
        set_error("Riccati precompute failed: R + B'PB is singular");
        return -1;
    }
    // a shape without an on-chip kernel in the library: specialise one now (jit.cpp; one-off, cached on disk)
    if (!no_specialise && !find_quad_kernel(nx, nu, N, -1) && !find_mfma_kernel(nx, nu, N) && !find_trans_kernel(nx, nu, N))
        (void)jit_kernel_for(nx, nu, N, verbose);
    if (verbose)
        std::printf("tinympc_hip: setup nx=%d nu=%d N=%d rho=%g batch=%d (Riccati %d sweeps)\n", nx, nu,
                    N, rho, batch_, cache.riccati_iters);
    fdyn.assign((size_t)nx, 0.0);
    x_min.assign((size_t)ex(), -1e17);
    x_max.assign((size_t)ex(), 1e17);
    u_min.assign((size_t)eu(), -1e17);
    u_max.assign((size_t)eu(), 1e17);
    batch = batch_;
    if (select_kernel()) return -1;
    if (d_gstat.alloc_zero((size_t)2 * GSTAT_WORDS)) return -1;
    if (d_gslot.alloc((size_t)GSLOT_DEFAULT_CAP * GSLOT_WORDS)) return -1;   // (written before it is read: fold_status)
    if (h_gstat.alloc(GSTAT_WORDS)) return -1;
    std::memset(h_gstat, 0, GSTAT_WORDS * sizeof(uint32_t));
    packs_dirty = true;
    return alloc_batch(batch_);
}

// One family per instance: B independent (A, B, Q, R, rho) sets, each with its own Riccati cache computed on
// the host in fp64 (threaded); bounds, settings and references behave as in the single-family solver.
int Solver::init_families(const double *A_, const double *B_, const double *Q_, const double *R_, const double *rho_,
                          int nx_, int nu_, int N_, int batch_, int device_, int verbose_, bool on_device) {
    no_specialise = true;   // (a per-instance-family solver runs on the stream kernel: nothing to specialise at setup)
    if (init(A_, B_, Q_, R_, rho_[0], nx_, nu_, N_, batch_, device_, verbose_)) return -1;
    hetero = true, plant_dirty = true;   // (the plant image holds every instance's A_b, B_b)
    const size_t Bn = (size_t)batch, nxx = (size_t)nx * nx, nxu = (size_t)nx * nu, nuu = (size_t)nu * nu;
    if (on_device) {   // every instance's cache by riccati_families_kernel: the setter's path on a solver that has no family yet
        if (select_kernel() || set_families(A_, B_, Q_, R_, rho_)) return -1;
        return ensure_extension_buffers();
    }
    het_A.assign(A_, A_ + Bn * nxx);
    het_B.assign(B_, B_ + Bn * nxu);
    family_diagonals(Q_, R_, rho_);
    fam_mode = FAM_HOST;
    het_cache.assign(Bn, Cache());
    std::vector<int> bad(1, 0);
    parallel_chunks(Bn, [&](size_t lo, size_t hi) {
        for (size_t b = lo; b < hi; ++b)
            if (precompute_cache(Mat(nx, nx, A_ + b * nxx), Mat(nx, nu, B_ + b * nxu), Mat(nx, nx, Q_ + b * nxx),
                                 Mat(nu, nu, R_ + b * nuu), rho_[b], het_cache[b]))
                bad[0] = 1;
    }, 64);
    if (bad[0]) {
        set_error("Riccati precompute failed for at least one instance (R + B'PB singular)");
        return -1;
    }
    std::vector<float> aux((size_t)(nx + nu + 1) * Bn);
    for (size_t b = 0; b < Bn; ++b) {
        for (int i = 0; i < nx; ++i) aux[(size_t)i * Bn + b] = (float)het_cache[b].Qd[i];
        for (int a = 0; a < nu; ++a) aux[(size_t)(nx + a) * Bn + b] = (float)het_cache[b].Rd[a];
        aux[(size_t)(nx + nu) * Bn + b] = (float)het_cache[b].rho;
    }
    if (d_het_aux.upload(aux)) return -1;
    packs_dirty = true;
    return select_kernel() || ensure_extension_buffers();
}

void Solver::family_diagonals(const double *Q_, const double *R_, const double *rho_) {
    const size_t Bn = (size_t)batch, nxx = (size_t)nx * nx, nuu = (size_t)nu * nu;
    if (Q_) {
        het_Qdiag.resize(Bn * nx);
        for (size_t b = 0; b < Bn; ++b)
            for (int i = 0; i < nx; ++i) het_Qdiag[b * nx + i] = Q_[b * nxx + (size_t)i * nx + i];
    }
    if (R_) {
        het_Rdiag.resize(Bn * nu);
        for (size_t b = 0; b < Bn; ++b)
            for (int a = 0; a < nu; ++a) het_Rdiag[b * nu + a] = R_[b * nuu + (size_t)a * nu + a];
    }
    if (rho_) het_rho.assign(rho_, rho_ + Bn);
}

// Every instance's family replaced on a live solver (tinympc_set_families), and the device route of creation: the inputs —
// the caller's, or for a null pair the ones the solver holds — go to staging buffers, riccati_families_kernel writes a staging
// image, and only an image without a singular instance is committed.  A refusal leaves the solver exactly as it was.
int Solver::set_families(const double *A_, const double *B_, const double *Q_, const double *R_, const double *rho_) {
    if (!hetero) {
        set_error("set_families: not a per-instance-family solver (tinympc_create_families and tinympc_create_families_device make one)");
        return -1;
    }
    if ((A_ == nullptr) != (B_ == nullptr) || (Q_ == nullptr) != (R_ == nullptr)) {
        set_error("set_families: A and B come together, and so do Q and R (NULL for both keeps them)");
        return -1;
    }
    if (!families_shape_built(nx, nu)) {
        set_error("set_families: the device setup is built for the stream kernel's grid (nx in {2,3,4,6,8,10,12}, nu <= 4)");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;   // (a launch still in flight reads the pack the next upload_packs overwrites)
    const size_t Bn = (size_t)batch, nxx = (size_t)nx * nx, nxu = (size_t)nx * nu;
    // the diagonals and rho as they will be: the caller's, else the solver's
    std::vector<double> keepQ, keepR, keepRho;
    if (Q_) keepQ.swap(het_Qdiag), keepR.swap(het_Rdiag);
    if (rho_) keepRho.swap(het_rho);
    family_diagonals(Q_, R_, rho_);
    auto restore = [&] {
        if (Q_) het_Qdiag.swap(keepQ), het_Rdiag.swap(keepR);
        if (rho_) het_rho.swap(keepRho);
    };
    // staging: what was given (or is not on the device yet) is uploaded, what is kept and already there is read in place
    DevBuf<double> sA, sB, sQ, sR, sRho, sImg;
    DevBuf<int> sSw;
    const bool upA = A_ || !d_fam_A, upQ = Q_ || !d_fam_Qdiag, upRho = rho_ || !d_fam_rho;
    if ((upA && (sA.upload(A_ ? A_ : het_A.data(), Bn * nxx) || sB.upload(B_ ? B_ : het_B.data(), Bn * nxu))) ||
        (upQ && (sQ.upload(het_Qdiag) || sR.upload(het_Rdiag))) || (upRho && sRho.upload(het_rho)) ||
        sImg.alloc((size_t)families_cache_elems(nx, nu) * Bn) || sSw.alloc(Bn)) {
        restore();
        return -1;
    }
    const FamilyInputs in = {upA ? sA : d_fam_A, upA ? sB : d_fam_B, upQ ? sQ : d_fam_Qdiag, upQ ? sR : d_fam_Rdiag, upRho ? sRho : d_fam_rho};
    std::vector<int> sweeps(Bn);
    float ms = -1.f;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool launched = hip_ok(hipEventCreate(&e0), "hipEventCreate") && hip_ok(hipEventCreate(&e1), "hipEventCreate") &&
                          hip_ok(hipEventRecord(e0, nullptr), "hipEventRecord") &&
                          hip_ok(families_riccati_launch(nx, nu, in, batch, sImg, sSw, nullptr), "riccati_families_kernel") &&
                          hip_ok(hipEventRecord(e1, nullptr), "hipEventRecord") &&
                          hip_ok(hipMemcpy(sweeps.data(), sSw, Bn * sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy (sweeps)") &&
                          hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (!launched) {
        restore();
        return -1;
    }
    long bad = 0, first = -1;
    for (size_t b = 0; b < Bn; ++b)
        if (sweeps[b] < 0) {
            if (first < 0) first = (long)b;
            ++bad;
        }
    if (bad) {
        restore();
        set_error("set_families: R + B'PB is singular for instance " + std::to_string(first) + " (" + std::to_string(bad) + " of " +
                  std::to_string(batch) + " instances singular); the solver keeps the families it had");
        return -1;
    }
    // commit
    if (A_) {
        het_A.assign(A_, A_ + Bn * nxx);
        het_B.assign(B_, B_ + Bn * nxu);
        A = Mat(nx, nx, A_), B = Mat(nx, nu, B_);   // (instance 0's, as creation leaves them; no kernel of a family solver reads them)
    }
    if (Q_) Q = Mat(nx, nx, Q_), R = Mat(nu, nu, R_);
    cache.rho = het_rho[0];
    for (int i = 0; i < nx; ++i) cache.Qd[i] = het_Qdiag[i] + het_rho[0];
    for (int a = 0; a < nu; ++a) cache.Rd[a] = het_Rdiag[a] + het_rho[0];
    if (upA) d_fam_A = std::move(sA), d_fam_B = std::move(sB);
    if (upQ) d_fam_Qdiag = std::move(sQ), d_fam_Rdiag = std::move(sR);
    if (upRho) d_fam_rho = std::move(sRho);
    d_het_cache = std::move(sImg);
    d_het_sweeps = std::move(sSw);
    std::vector<Cache>().swap(het_cache);
    fam_mode = FAM_DEVICE;
    fam_ms[0] = ms;
    packs_dirty = true;
    plant_dirty = true;   // (the plant image and the estimator's model hold every instance's A_b, B_b)
    if (verbose) {
        long cap = 0;
        for (size_t b = 0; b < Bn; ++b) cap += sweeps[b] >= RICCATI_MAX_SWEEPS;
        std::printf("tinympc_hip: %d families set up on the device in %.3f ms (%ld at the %d-sweep cap)\n", batch, ms, cap, RICCATI_MAX_SWEEPS);
    }
    return 0;
}

// device mode's part of upload_packs: the stream kernel's per-instance pack and het_aux written on the device
int Solver::fill_family_pack() {
    const size_t cols = (size_t)(se ? se->lanes : 0) * batch, cp = se ? families_pack_elems(nx, nu, se->lanes) : 0;
    if (!cp || !d_het_cache) {
        set_error("per-instance families set up on the device need the stream kernel's four-lane instantiation of (nx, nu)");
        return -1;
    }
    if (d_coef.alloc(cp * cols * (precision == 1 ? sizeof(float) : sizeof(double))) || d_het_aux.reserve((size_t)(nx + nu + 1) * batch)) return -1;
    const FamilyInputs in = {d_fam_A, d_fam_B, d_fam_Qdiag, d_fam_Rdiag, d_fam_rho};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = -1.f;
    const bool ok = hip_ok(hipEventCreate(&e0), "hipEventCreate") && hip_ok(hipEventCreate(&e1), "hipEventCreate") &&
                    hip_ok(hipEventRecord(e0, nullptr), "hipEventRecord") &&
                    hip_ok(families_fill_launch(nx, nu, d_het_cache, in, fdyn.data(), batch, precision, d_coef, d_het_aux, nullptr),
                           "fill_family_pack_kernel") &&
                    hip_ok(hipEventRecord(e1, nullptr), "hipEventRecord") &&
                    hip_ok(hipEventSynchronize(e1), "hipEventSynchronize") &&   // (the next launch may go to any stream)
                    hip_ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    fam_ms[1] = ms;
    return ok ? 0 : -1;
}

// every block column-major, instance after instance; any output may be null
int Solver::get_family_cache(int first, int count, double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, int *sweeps) {
    if (!hetero) {
        set_error("get_family_cache: not a per-instance-family solver");
        return -1;
    }
    if (first < 0 || count < 0 || (long)first + count > batch) {
        set_error("get_family_cache: the range [first, first + count) leaves the batch");
        return -1;
    }
    const size_t n = (size_t)count, sz[4] = {(size_t)nu * nx, (size_t)nx * nx, (size_t)nu * nu, (size_t)nx * nx};
    double *out[4] = {Kinf, Pinf, Quu_inv, AmBKt};
    if (fam_mode != FAM_DEVICE) {
        for (size_t i = 0; i < n; ++i) {
            const Cache &c = het_cache[first + i];
            const Mat *m[4] = {&c.Kinf, &c.Pinf, &c.Quu_inv, &c.AmBKt};
            for (int k = 0; k < 4; ++k)
                if (out[k]) std::copy(m[k]->a.begin(), m[k]->a.end(), out[k] + i * sz[k]);
            if (sweeps) sweeps[i] = c.riccati_iters;
        }
        return 0;
    }
    HIP_TRY(hipSetDevice(device));
    if (!n) return 0;
    const size_t elems = (size_t)families_cache_elems(nx, nu);
    std::vector<double> h;   // [element][count]
    if (Kinf || Pinf || Quu_inv || AmBKt) {   // (the sweep counts alone: nothing of the image travels)
        h.resize(elems * n);
        HIP_TRY(hipMemcpy2D(h.data(), n * sizeof(double), (const double *)d_het_cache + first, (size_t)batch * sizeof(double), n * sizeof(double),
                            elems, hipMemcpyDeviceToHost));
    }
    size_t e0 = 0;
    for (int k = 0; k < 4; ++k) {   // (the image's blocks in the order K, P, Quu_inv, AmBKt: Riccati<NX,NU>::E_*)
        if (out[k])
            for (size_t i = 0; i < n; ++i)
                for (size_t e = 0; e < sz[k]; ++e) out[k][i * sz[k] + e] = h[(e0 + e) * n + i];
        e0 += sz[k];
    }
    if (sweeps) HIP_TRY(hipMemcpy(sweeps, (const int *)d_het_sweeps + first, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ---- kernel routing ------------------------------------------------------------------------------------------------------
// The environment switches (tuning / test aids) are read ONCE, when the solver is created; nothing on
// the solve path calls getenv.
Switches read_switches() {
    auto on = [](const char *name) { return std::getenv(name) != nullptr; };
    Switches w;
    if (const char *g = std::getenv("TINYMPC_HIP_GROUP")) w.group = std::atoi(g);
    w.strict_fp32 = on("TINYMPC_HIP_STRICT_FP32");
    w.no_quad = on("TINYMPC_HIP_NO_QUAD");
    w.no_quad_adp = on("TINYMPC_HIP_NO_QUAD_ADP");
    w.no_quad_adp1 = on("TINYMPC_HIP_NO_QUAD_ADP1");
    w.no_mfma = on("TINYMPC_HIP_NO_MFMA");
    w.no_mfma_adp = on("TINYMPC_HIP_NO_MFMA_ADP");
    w.mfma_oneshot_only = on("TINYMPC_HIP_MFMA_ONESHOT_ONLY");
    w.no_stream = on("TINYMPC_HIP_NO_STREAM");
    w.no_stream_adp = on("TINYMPC_HIP_NO_STREAM_ADP");
    w.no_mfmar = on("TINYMPC_HIP_NO_MFMAR");
    w.no_mfmac = on("TINYMPC_HIP_NO_MFMAC");
    w.mfmac_all = on("TINYMPC_HIP_MFMAC_ALL");
    w.no_jit = on("TINYMPC_HIP_NO_JIT");
    w.no_mfmat = on("TINYMPC_HIP_NO_MFMAT");
    w.mfmat_all = on("TINYMPC_HIP_MFMAT_ALL");
    w.mfmat_ws_only = on("TINYMPC_HIP_MFMAT_WS_ONLY");
    w.no_lean = on("TINYMPC_HIP_NO_LEAN");
    w.no_refill = on("TINYMPC_HIP_NO_REFILL");
    w.no_uni = on("TINYMPC_HIP_NO_UNI");
    w.no_os = on("TINYMPC_HIP_NO_OS");
    w.lean_one = on("TINYMPC_HIP_LEAN_ONE");
    w.lean_dense = on("TINYMPC_HIP_LEAN_DENSE");
    w.lean_unscaled = on("TINYMPC_HIP_LEAN_UNSCALED");
    w.lean_ws = on("TINYMPC_HIP_LEAN_WS");
    w.lean_loop = on("TINYMPC_HIP_LEAN_LOOP");
    w.stream_f64 = on("TINYMPC_HIP_STREAM_F64");
    w.stream_mpc = on("TINYMPC_HIP_STREAM_MPC");
    w.stream_loop = on("TINYMPC_HIP_STREAM_LOOP");
    w.event_markers = on("TINYMPC_HIP_EVENT_MARKERS");
    w.noise_split = on("TINYMPC_HIP_NOISE_SPLIT");
    w.estimator_split = on("TINYMPC_HIP_ESTIMATOR_SPLIT");
    if (const char *d = std::getenv("TINYMPC_HIP_MFMAC_DEBUG")) w.mfmac_debug = std::atoi(d);
    if (const char *f = std::getenv("TINYMPC_HIP_FOLD_SLOTS")) w.fold_slots = std::max(0, std::atoi(f));
    return w;
}

// Capability table.  A kernel family is a route: `route_*` says whether the family takes the solver's shape, options and
// calling pattern (its "supports"), and — within the family — which instantiation costs least for the batch (lanes per
// instance by batch size: select_quad_kernel).  select_kernel asks the routes in order of preference, last word first:
//   transposed-sets matrix-core kernel (mfmat: every calling pattern of its shapes)
//   > one-shot matrix-core kernels with the affine term / cones (mfmar, compiled horizon; mfmac, LDS, any horizon)
//   > matrix-core kernel of the box-only shapes (mfma, and its adaptive-rho variant)
//   > lanes-per-instance kernels (quad, and their adaptive-rho variants)  > run-time-horizon stream kernel  > generic kernel.
// The result is cached under the key of everything the routes read; a solve re-routes only when that key has changed.

// lanes-per-instance family, its adaptive-rho variants included (precision = 1 — fp32 recurrences, asked for to save time —
// stays here only where no matrix-core kernel exists, or with TINYMPC_HIP_STRICT_FP32: route_mfma)
const KernelEntry *Solver::route_quad(bool rollout) const {
    if (sw.no_quad || extensions_active() || hetero || bounds_mode || lin_mode || cone_mode) return nullptr;   // (per-instance bounds / rows / cones: the pack holds one image)
    if (!st.adaptive_rho) {
        const KernelEntry *k = sw.group ? find_quad_kernel(nx, nu, N, sw.group) : nullptr;
        if (!k) k = select_quad_kernel(nx, nu, N, batch);
        // (a unit specialised at setup carries fp64 recurrences only; TINYMPC_HIP_NO_JIT on this solver: not a unit another one loaded either)
        return (k && k->jit && (precision != 0 || sw.no_jit)) ? nullptr : k;
    }
    // adaptive rho: the ADP variant where the shape has one (4 lanes per instance, coefficient rows in registers: the
    // cartpole shapes) ...
    const KernelEntry *ka = sw.no_quad_adp ? nullptr : find_quad_kernel(nx, nu, N, 4);
    if (!(ka && ka->adp && chunk_iters == 0 && !rollout && !cache_overridden)) return nullptr;
    // ... with ONE lane per instance — the benched variant of large batches — in the correction form (admm_quad.hip.h:
    // dK = (rho_b - rho_family) dKinf/drho next to the family's wave-uniform coefficients): zero or shared references,
    // fp64 recurrences, the adaptive state in closed form
    if (batch >= 20480 && precision == 0 && !sw.group && !refs_device_owned && xref_kind <= 1 && uref_kind <= 1 &&
        (adapt_pure || adapt_dirty) && !sw.no_quad_adp1)
        if (const KernelEntry *k1 = find_quad_kernel(nx, nu, N, 1))
            if (k1->adp) return k1;
    return ka;
}

// matrix-core kernel of the box-only shapes: plain solves with fp64 recurrences (horizons the shape has no
// lanes-per-instance kernel for — quadrotor N = 10, 15, 25 — included; the fused closed loop of a cold-started solver stays
// on the quad kernel), and the adaptive-rho variant (the instance's own Kinf as a correction to the shared products) where
// the quad family has none
const KernelEntry *Solver::route_mfma(bool rollout, const KernelEntry *quad) const {
    if (strict_fp32() || sw.group || sw.no_mfma || sw.no_quad || bounds_mode || lin_mode || cone_mode) return nullptr;
    const KernelEntry *m = find_mfma_kernel(nx, nu, N);
    if (!m || (m->jit && sw.no_jit)) return nullptr;
    if (st.adaptive_rho)
        return (!quad && m->adp && !extensions_active() && chunk_iters == 0 && !rollout && !cache_overridden &&
                (adapt_pure || adapt_dirty) && !sw.no_mfma_adp) ? m : nullptr;
    if (!(quad || !(extensions_active() || hetero))) return nullptr;
    if (rollout && rollout_on_quad()) return nullptr;
    if (!(!sw.mfma_oneshot_only || (!warm_start && chunk_iters == 0))) return nullptr;
    return m;
}

// run-time-horizon stream kernel of (nx, nu): whatever no specialised kernel takes, if its LDS image fits
const StreamEntry *Solver::route_stream() const {
    const bool adp_ok = !extensions_active() && chunk_iters == 0 && !sw.no_stream_adp;
    if ((st.adaptive_rho && !adp_ok) || sw.no_stream) return nullptr;
    const StreamEntry *s2 = find_stream_kernel(nx, nu);
    if (s2 && 16.0 * batch * std::max(nx, nu) >= 4.0e9) s2 = nullptr;   // 32-bit lane byte offsets into one knot's rows
    if (s2 && s2->lds_bytes(N, precision) > 150 * 1024) s2 = nullptr;   // LDS image of coefficients + bounds
    // per-instance bounds: the `ib` form, built for the benchmark shapes with fp64 recurrences (the 32-bit guard above covers
    // its bound arrays: an instance's rows of one knot lie below 4 batch max(nx, nu) bytes)
    if (s2 && bounds_mode && (precision != 0 || !s2->launch_ib)) s2 = nullptr;
    // per-instance rows: the `il` form, the same three shapes; its rows take LDS behind the image
    if (s2 && lin_mode && (precision != 0 || !s2->launch_il || s2->lds_bytes(N, precision) + s2->il_lds_bytes(mlx, mlu) > 150 * 1024)) s2 = nullptr;
    // per-instance cones: the `ic` form, the `il` form with the coefficients behind the rows
    if (s2 && cone_mode && (precision != 0 || !s2->launch_ic || s2->lds_bytes(N, precision) + s2->il_lds_bytes(mlx, mlu) + s2->ic_lds_bytes(ncx, ncu) > 150 * 1024))
        s2 = nullptr;
    return s2;
}

// precision 2 with TINYMPC_HIP_STREAM_F64: the stream kernel's fp64-state form where the shape has one — any horizon, the
// affine term, cones, linear rows, cold or kept workspace.  One family, fixed rho, the whole batch in one launch (no
// chunks): everything else stays on the generic kernel's fp64-state form.
const StreamEntry *Solver::route_stream_f64() const {
    if (!sw.stream_f64 || sw.no_stream || st.adaptive_rho || hetero || chunk_iters != 0 || bounds_mode || lin_mode || cone_mode) return nullptr;
    const StreamEntry *s2 = find_stream_kernel(nx, nu);
    if (!s2 || !s2->launch_f64) return nullptr;
    if (32.0 * batch * std::max(nx, nu) >= 4.0e9) return nullptr;   // 32-bit lane byte offsets, 8-byte elements
    if (s2->lds_bytes(N, 2) > 150 * 1024) return nullptr;
    return s2;
}

// one-shot solves (cold start, workspace not kept) with the affine term and / or cones: the register-resident matrix-core
// kernel where the horizon is compiled in (mfmar; box-only solves too where the entry says so: rocket N = 50, 4.3 ms
// against 5.5 on the quad kernel), else the LDS-resident one (mfmac, any horizon).  Only where a workspace-carrying
// kernel exists to fall back to (`fallback`).
const ConeEntry *Solver::route_cone(bool rollout, bool have_quad, bool have_stream) const {
    if (bounds_mode || lin_mode || cone_mode) return nullptr;
    const ConeEntry *cn = sw.no_mfmar ? nullptr : find_cone_kernel(nx, nu, N);
    if (cn && cn->supports && !cn->supports(*this)) cn = nullptr;
    const bool plain_ok = sw.mfmac_all || (cn != nullptr && cn->plain);
    if (!((have_stream || (have_quad && plain_ok)) && !warm_start && chunk_iters == 0 && !rollout && !strict_fp32() && !hetero &&
          !st.adaptive_rho && (extensions_active() || plain_ok) && xref_kind < 2 && uref_kind < 2 &&
          !(refs_device_owned && ref_mode == REF_PER_INSTANCE) && !sw.no_mfmac && !sw.group && !sw.no_mfma))
        return nullptr;
    const ConeEntry *c2 = cn ? cn : find_cone_kernel(nx, nu, 0);
    if (c2 && c2->lds_bytes(*this) > 160 * 1024 - 1024) c2 = nullptr;   // horizon too long for one tile's LDS
    // (two cones per side / linear rows: the transposed-sets kernel specialised for the layout, route_trans, or the stream kernel)
    if ((st.en_state_soc && ncx > 1) || (st.en_input_soc && ncu > 1) || lin_active()) c2 = nullptr;
    return c2;
}

// transposed-sets matrix-core kernel: every kind of solve (one-shot, warm-started, workspace kept, chunked, the fused closed
// loop) of a shape that has it, with the affine term / at most one cone per side (box-only problems where the entry says so)
const ConeEntry *Solver::route_trans(bool rollout, const ConeEntry *oneshot) const {
    if (sw.no_mfmat || sw.no_mfma || sw.group || bounds_mode || lin_mode || cone_mode) return nullptr;
    if (strict_fp32() || hetero || st.adaptive_rho || (rollout && refs_per_instance() && ref_seq_steps > 0) || st.max_iter < 1 || (double)batch * ex() >= 2.0e9)
        return nullptr;
    const ConeEntry *ct = find_trans_kernel(nx, nu, N);
    if (ct && (lin_active() || (ct->supports && !ct->supports(*this)))) ct = nullptr;
    if (ct && !(has_fdyn || cones_active() || ct->plain || sw.mfmat_all)) return nullptr;
    // a layout the built-in entries do not have — two cones on a side, linear rows, a horizon the library was not built with:
    // the unit specialised for exactly this layout (jit.cpp; compiled on first use, cached on disk)
    if (!ct && extensions_active() && !sw.no_jit) {
        ct = jit_trans_find(*this);
        if (!ct && !no_specialise && layout_final) ct = jit_trans_for(*this, verbose);   // (not for every intermediate layout of a setter sequence)
    }
    if (!ct || ct->lds_bytes(*this) > 160 * 1024 - 1024) return nullptr;
    if (sw.mfmat_ws_only && !warm_start && chunk_iters == 0 && !rollout && oneshot) return nullptr;   // (tests hold the families against each other)
    return ct;
}

bool Solver::bounds_vary_by_knot() const {
    if (st.en_state_bound)
        for (int k = 1; k < N; ++k)
            for (int r = 0; r < nx; ++r)
                if (x_min[r + (size_t)k * nx] != x_min[r] || x_max[r + (size_t)k * nx] != x_max[r]) return true;
    if (st.en_input_bound)
        for (int k = 1; k < N - 1; ++k)
            for (int a = 0; a < nu; ++a)
                if (u_min[a + (size_t)k * nu] != u_min[a] || u_max[a + (size_t)k * nu] != u_max[a]) return true;
    return false;
}

// everything the routes read, in one comparable value
std::vector<long> Solver::routing_key(bool rollout) const {
    return {nx, nu, N, batch, precision, warm_start, chunk_iters, has_fdyn, cones_active(), lin_active(), hetero, st.adaptive_rho,
            cache_overridden, refs_device_owned, xref_kind, uref_kind, ref_mode, adapt_pure, adapt_dirty, ref_seq_steps,
            st.max_iter < 1, st.en_state_soc, st.en_input_soc, ncx, ncu, Acx[0], qcx[0], Acu[0], qcu[0], mlx, mlu, rollout, strict_precision,
            (long)route_gen, Acx[1], qcx[1], Acu[1], qcu[1], st.en_state_linear, st.en_input_linear,
            extensions_active() && bounds_vary_by_knot(), layout_final, bounds_mode, lin_mode, cone_mode};   // (a unit specialised at setup is compiled for one bound kind)
}

int Solver::select_kernel(bool rollout) {
    std::vector<long> key = routing_key(rollout);
    if (routed && key == routed_key) return 0;
    if (st.adaptive_rho && hetero) {
        set_error("adaptive_rho is not available on a per-instance-family solver");
        return -1;
    }
    if (st.adaptive_rho && bounds_mode) {
        set_error("adaptive_rho is not available with per-instance bounds (set_instance_bounds); shared bounds (set_bound_constraints) drop them");
        return -1;
    }
    if (st.adaptive_rho && cone_mode) {
        set_error("adaptive_rho is not available with per-instance cones (set_instance_cones); shared cones (set_cone_constraints) drop them");
        return -1;
    }
    if (st.adaptive_rho && lin_mode) {
        set_error("adaptive_rho is not available with per-instance linear rows (set_instance_linear); shared rows (set_linear_constraints) drop them");
        return -1;
    }
    if (precision == 2) {   // fp64 end to end: the stream kernel's fp64-state form (route_stream_f64), else the generic kernel's, whatever the shape
        if (hetero || (rollout && !sw.stream_mpc)) {   // (TINYMPC_HIP_STREAM_MPC: the closed loop as a chain of these launches, plan_rollout)
            set_error(hetero ? "precision 2 is not available on a per-instance-family solver" : "precision 2 has no fused closed loop (step it from the host)");
            return -1;
        }
        if (nx > GEN_MAX_NX || nu > GEN_MAX_NU) {
            set_error("problem shape exceeds the generic kernel limits (nx <= 64, nu <= 32)");
            return -1;
        }
        const StreamEntry *s2 = route_stream_f64();
        // (the key moved: whether the lean kernel's fp64-state form takes the one-shot solves — lean_jit, its pack — is decided
        // with the packs, from the extensions as they are now, also where the entries stay what they were)
        packs_dirty = true;
        ke = nullptr, se = s2, ce = nullptr;
        kernel_name = se ? se->name_f64 : (cone_mode ? "generic<f64;ic>" : lin_mode ? "generic<f64;il>" : (bounds_mode ? "generic<f64;ib>" : "generic<f64>"));
        routed_key = std::move(key);
        routed = true;
        return 0;
    }
    const KernelEntry *q = route_quad(rollout), *m = route_mfma(rollout, q), *k = m ? m : q;
    if (!k && (nx > GEN_MAX_NX || nu > GEN_MAX_NU)) {
        set_error("problem shape exceeds the generic kernel limits (nx <= 64, nu <= 32)");
        return -1;
    }
    const StreamEntry *s2 = k ? nullptr : route_stream();
    if (hetero && !s2) {
        set_error(cone_mode ? "per-instance families with per-instance cones need the stream kernel's ic form: (nx, nu) in {(4,1), (6,3), (12,4)}, precision 0" :
                  lin_mode ? "per-instance families with per-instance linear rows need the stream kernel's il form: (nx, nu) in {(4,1), (6,3), (12,4)}, precision 0" :
                  bounds_mode ? "per-instance families with per-instance bounds need the stream kernel's ib form: (nx, nu) in {(4,1), (6,3), (12,4)}, precision 0" :
                  "per-instance families need a stream-kernel instantiation for (nx, nu) (nx in {2,3,4,6,8,10,12}, nu <= 4)");
        return -1;
    }
    const ConeEntry *c2 = route_cone(rollout, k != nullptr, s2 != nullptr), *ct = route_trans(rollout, c2);
    if (ct) c2 = ct;
    if (c2) k = nullptr, s2 = nullptr;
    if (k != ke || s2 != se || c2 != ce) packs_dirty = true;
    ke = k, se = s2, ce = c2;
    kernel_name = ke ? ke->name : (se ? (cone_mode ? se->name_ic : lin_mode ? se->name_il : (bounds_mode ? se->name_ib : se->name)) : (ce ? ce->name : (cone_mode ? "generic<ic>" : lin_mode ? "generic<il>" : (bounds_mode ? "generic<ib>" : "generic"))));
    routed_key = std::move(key);
    routed = true;
    return 0;
}

int Solver::alloc_batch(int batch_) {
    if (hetero && batch_ != batch) {
        set_error("set_batch_size: a per-instance-family solver has a fixed batch");
        return -1;
    }
    if (batch_ < 1) {
        set_error("batch must be >= 1");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    free_batch();
    drop_instance_bounds();   // (per-instance inputs do not survive a re-batch: back to the shared bounds)
    drop_instance_linear();   // (... and to no rows)
    drop_instance_cones();    // (... and to no cones)
    drop_own_plant();         // (... and back to the model plant)
    (void)drop_ref_trajectory(false);   // (... and to the references set below)
    drop_noise();             // (... and no noise: a factor may be per instance)
    batch = batch_;
    if (select_kernel()) return -1;
    const size_t Bn = (size_t)batch, EX = (size_t)ex(), EU = (size_t)eu();
    // (the workspace and the residuals are zeroed by reset() below)
    if (d_x0.alloc_zero(Bn * nx) || d_xout.alloc_zero(Bn * EX) || d_uout.alloc_zero(Bn * EU) ||
        d_res.alloc(Bn * 4) || d_iter.alloc_zero(Bn) || d_solved.alloc_zero(Bn) ||
        d_sd.alloc(Bn * EU) || d_sy.alloc(Bn * EU) || d_sz.alloc(Bn * EU) ||
        d_sg.alloc(Bn * EX) || d_sv.alloc(Bn * EX))
        return -1;
    // shared-size reference buffers up front; per-instance ones on demand
    if (d_xref.alloc_zero(EX) || d_uref.alloc_zero(EU)) return -1;
    h_xref.clear();
    h_uref.clear();
    xref_kind = uref_kind = 0;
    ref_mode = REF_ZERO;
    refs_dirty = false;
    refs_device_owned = false;
    if (ensure_extension_buffers()) return -1;
    solved_once = false;
    return reset();
}

int Solver::reset() {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    if (d_sd.zero() || d_sy.zero() || d_sz.zero() || d_sg.zero() || d_sv.zero() || d_res.zero()) return -1;
    if (d_sgc && (d_sgc.zero() || d_svc.zero() || d_syc.zero() || d_szc.zero())) return -1;
    if (d_sgl && (d_sgl.zero() || d_svl.zero() || d_syl.zero() || d_szl.zero())) return -1;
    if (d_ws64 && d_ws64.zero()) return -1;
    adapt_dirty = true;  // adapted (rho, Kinf, Pinf) go back to the family's cache
    g_maybe_nonzero = false;
    return 0;
}

__global__ void adapt_fill_kernel(double *adapt, const double *family, int n, long batch) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)n * batch) adapt[i] = family[i / batch];
}

int Solver::set_sensitivity(const double *dK, const double *dP) {
    sens.assign((size_t)nu * nx + (size_t)nx * nx, 0.0);
    std::copy(dK, dK + (size_t)nu * nx, sens.begin());
    std::copy(dP, dP + (size_t)nx * nx, sens.begin() + (size_t)nu * nx);
    if (d_adapt && !adapt_dirty && sens_set) adapt_pure = false;   // new tables under a live adaptive state
    sens_set = true;
    sens_dirty = true;
    packs_dirty = true;   // (the matrix-core kernel's adaptive variant carries dPinf' as an operand)
    return 0;
}

int Solver::get_adaptive_state(double *rho, double *Kinf, double *Pinf) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const size_t Bn = (size_t)batch, nk = (size_t)nu * nx, np = (size_t)nx * nx;
    if (!d_adapt || adapt_dirty) {  // nothing adapted yet: every instance holds the family's values
        for (size_t b = 0; b < Bn; ++b) {
            if (rho) rho[b] = cache.rho;
            if (Kinf) std::copy(cache.Kinf.a.begin(), cache.Kinf.a.end(), Kinf + b * nk);
            if (Pinf) std::copy(cache.Pinf.a.begin(), cache.Pinf.a.end(), Pinf + b * np);
        }
        return 0;
    }
    std::vector<double> h((1 + nk + np) * Bn);
    HIP_TRY(hipMemcpy(h.data(), d_adapt, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < Bn; ++b) {
        if (rho) rho[b] = h[b];
        if (Kinf)
            for (size_t e = 0; e < nk; ++e) Kinf[b * nk + e] = h[(1 + e) * Bn + b];
        if (Pinf)
            for (size_t e = 0; e < np; ++e) Pinf[b * np + e] = h[(1 + nk + e) * Bn + b];
    }
    return 0;
}

int Solver::upload_packs() {
    if (wait_last_launch()) return -1;   // (a launch still in flight on another stream reads the packs this overwrites)
    state_bounds_active = false;
    const std::vector<double> &sxmin = bounds_mode ? ib_xmin : x_min, &sxmax = bounds_mode ? ib_xmax : x_max;
    if (st.en_state_bound)
        for (size_t i = 0; i < sxmin.size(); ++i)
            if (sxmin[i] > -1e17 || sxmax[i] < 1e17) {
                state_bounds_active = true;
                break;
            }
    if ((bounds_mode || lin_mode || cone_mode) && upload_instance_bounds()) return -1;   // (the `il` and `ic` forms read their bounds per instance too)
    if ((lin_mode || cone_mode) && !d_il && upload_instance_linear()) return -1;              // (... and the `ic` forms their rows)
    if (cone_mode && !d_ic && upload_instance_cones()) return -1;
    std::vector<unsigned char> coef;
    std::vector<float> bnd;
    if (ke) {
        ke->build_coef(*this, coef);
        ke->build_bounds(*this, bnd);
    } else if (ce) {
        ce->build_coef(*this, coef);
        ce->build_bounds(*this, bnd);
    } else if (se) {
        if (fam_mode != FAM_DEVICE) se->build_coef(*this, coef);
        se->build_bounds(*this, bnd);
    } else {
        build_generic_coef(*this, coef);
        build_generic_bounds(*this, bnd);
    }
    if (fam_mode == FAM_DEVICE) {   // (select_kernel leaves a family solver on the stream kernel or refuses)
        if (fill_family_pack() || d_bounds.upload(bnd)) return -1;
    } else if (d_coef.upload(coef) || d_bounds.upload(bnd)) return -1;
    // the lean kernel's own pack where the selected entry has one lane per instance and the shape a lean instantiation
    le = (ke && ke->G == 1 && lean_enabled) ? find_lean_kernel(nx, nu, N) : nullptr;
    // (a shape without one — cartpole at another horizon, a unit specialised at setup with four lanes per instance: where one
    // lane per instance is the batch's variant, launch_pass specialises the variant lean_plan asks for, jit_lean_for)
    lean_jit = !le && ke && lean_enabled && !sw.no_jit && !no_specialise && (ke->G == 1 || (ke->jit && ke->G < 16 && batch >= 20480));
    // precision 2 (the generic kernel's fp64-state form, one lane per instance like this one): one-shot solves of a shape the lean
    // kernel holds run on ITS fp64-state form, specialised on request — the reference's digits at the headline kernel's speed
    // (`se` at precision 2 is the stream kernel's fp64-state form: it takes what the lean kernel leaves)
    if (precision == 2 && !ke && !ce && !hetero && !extensions_active() && lean_enabled && !sw.no_jit && !no_specialise && !bounds_mode && !lin_mode && !cone_mode) lean_jit = true;
    std::fill(le_var_tried, le_var_tried + LV_COUNT, false);
    lean_ok = false;
    lean_scaled_ok = false;
    lean_sp = lean_pattern(A, B);
    if (le || lean_jit) {
        std::vector<double> lp;
        if (build_lean_pack(*this, lp, &lean_scaled_ok)) {
            if (!le && (!ke || ke->G != 1)) append_lean_bounds(*this, lp);   // (the selected entry's bound pack is not the one-lane one)
            if (d_lean.upload(lp)) return -1;
            lean_ok = true;
            lean_knot_bounds = false;
            if (st.en_input_bound)
                for (int k = 1; k < N - 1 && !lean_knot_bounds; ++k)
                    for (int a = 0; a < nu; ++a)
                        if (u_min[a + (size_t)k * nu] != u_min[a] || u_max[a + (size_t)k * nu] != u_max[a]) lean_knot_bounds = true;
        }
    }
    packs_dirty = false;
    return 0;
}

int Solver::set_x0(const double *x0, int cols) {
    if (cols != 1 && cols != batch) {
        set_error("set_x0: expected nx x 1 or nx x batch");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    std::vector<float> h((size_t)batch * nx);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < nx; ++i) h[(size_t)b * nx + i] = (float)x0[(cols == 1 ? 0 : (size_t)b * nx) + i];
    HIP_TRY(hipMemcpy(d_x0, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int Solver::set_ref(bool is_x, const double *ref, int cols) {
    const int kn = is_x ? N : N - 1;       // knots
    const int rows = is_x ? nx : nu;
    int kind;
    if (cols == kn)
        kind = 1;
    else if ((long)cols == (long)kn * batch)
        kind = 2;
    else {
        set_error(is_x ? "set_x_ref: expected nx x N or nx x (N*batch)"
                       : "set_u_ref: expected nu x (N-1) or nu x ((N-1)*batch)");
        return -1;
    }
    // (a reference trajectory goes: its window at the cursor stays as the ordinary references, of which this call replaces one)
    if (traj_kind && drop_ref_trajectory(true)) return -1;
    std::vector<float> &h = is_x ? h_xref : h_uref;
    const size_t n = (size_t)rows * cols;
    h.resize(n);
    bool all_zero = true;
    for (size_t i = 0; i < n; ++i) {
        h[i] = (float)ref[i];
        all_zero = all_zero && (ref[i] == 0.0);
    }
    if (all_zero) {
        kind = 0;  // identical arithmetic (-(0*Q) - rho(..) == 0 - rho(..)), cheaper kernel
        h.clear();
    }
    (is_x ? xref_kind : uref_kind) = kind;
    // a closed loop's per-step references go with the shared references they replaced; per-instance references replace
    // nothing the sequence installed, and the next mpc_rollout says that the two do not go together
    if (kind != 2) ref_seq_steps = 0;
    refs_dirty = true;
    refs_device_owned = false;
    return 0;
}

// Shared references of every step of the next fused closed loop (rocket_landing_constraints.jl:107-115 shifts x_ref by one
// knot per step): x_seq is nx x (N steps), u_seq nu x ((N-1) steps), column-major like set_x_ref / set_u_ref, step after
// step.  Step 0's become the solver's references; steps = 0 clears the sequence.
int Solver::set_ref_sequence(const double *x_seq, const double *u_seq, int steps) {
    if (steps <= 0) {
        ref_seq_steps = 0;
        return 0;
    }
    if (!x_seq || !u_seq) {
        set_error("set_ref_sequence: null reference sequence");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    if (traj_kind && drop_ref_trajectory(false)) return -1;   // (the sequence replaces a reference trajectory: the later call wins)
    const size_t EX = (size_t)ex(), EU = (size_t)eu();
    std::vector<float> hx(EX * steps), hu(EU * steps);
    for (size_t i = 0; i < hx.size(); ++i) hx[i] = (float)x_seq[i];
    for (size_t i = 0; i < hu.size(); ++i) hu[i] = (float)u_seq[i];
    if (d_xref_seq.upload(hx) || d_uref_seq.upload(hu)) return -1;
    // the solver's own references = step 0's, kept in shared mode even when they are all zero (later steps need not be)
    h_xref.assign(hx.begin(), hx.begin() + EX);
    h_uref.assign(hu.begin(), hu.begin() + EU);
    xref_kind = uref_kind = 1;
    refs_dirty = true;
    refs_device_owned = false;
    ref_seq_steps = steps;
    return 0;
}

// Materialise h_xref/h_uref on the device in one common mode for the kernel.
int Solver::upload_refs() {
    if (refs_device_owned || !refs_dirty) return 0;
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const int mode = xref_kind > uref_kind ? xref_kind : uref_kind;
    const size_t EX = (size_t)ex(), EU = (size_t)eu(), Bn = (size_t)batch;
    auto put = [&](DevBuf<float> &dptr, const std::vector<float> &h, int kind, size_t E) -> int {
        const size_t need = mode == REF_PER_INSTANCE ? Bn * E : E;
        if (dptr.reserve(need)) return -1;
        if (mode == REF_ZERO) return 0;
        std::vector<float> tmp;
        const float *src;
        if (kind == mode) {
            src = h.data();
        } else {
            tmp.assign(need, 0.f);
            if (kind == 1)  // shared -> replicate per instance
                for (size_t b = 0; b < Bn; ++b) std::memcpy(tmp.data() + b * E, h.data(), E * sizeof(float));
            src = tmp.data();
        }
        HIP_TRY(hipMemcpy(dptr, src, need * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    };
    if (put(d_xref, h_xref, xref_kind, EX)) return -1;
    if (put(d_uref, h_uref, uref_kind, EU)) return -1;
    ref_mode = mode;
    refs_dirty = false;
    return 0;
}

int Solver::set_bounds(const double *xmin, const double *xmax, const double *umin, const double *umax) {
    route_gen += 1;   // (array-valued state the routes read: the routing key only carries scalars)
    const bool had_instance_bounds = bounds_mode != 0;
    drop_instance_bounds();   // the shared set replaces a per-instance one
    x_min.assign(xmin, xmin + ex());
    x_max.assign(xmax, xmax + ex());
    u_min.assign(umin, umin + eu());
    u_max.assign(umax, umax + eu());
    st.en_state_bound = 1;  // bindings.cpp:400-404
    st.en_input_bound = 1;
    packs_dirty = true;
    // back from per-instance bounds: the solver returns to the routes of the shared set at once (kernel_name says so)
    return had_instance_bounds ? (select_kernel() || ensure_extension_buffers()) : 0;
}

// Per-instance box bounds.  per_knot = 0: x_* nx x batch, u_* nu x batch (column b: instance b's bound at every knot);
// per_knot = 1: x_* [batch][N][nx], u_* [batch][N-1][nu] (the layout of per-instance references).  Enables both sides, as
// set_bounds does.  The solver leaves the on-chip families for the stream / generic kernels' `ib` forms (select_kernel).
int Solver::set_instance_bounds(const double *xmin, const double *xmax, const double *umin, const double *umax, int per_knot) {
    if (!xmin || !xmax || !umin || !umax) {
        set_error("set_instance_bounds: null bound array");
        return -1;
    }
    if (st.adaptive_rho) {
        set_error("set_instance_bounds: per-instance bounds are not available with adaptive rho");
        return -1;
    }
    if (wait_last_launch()) return -1;
    const int old_mode = bounds_mode;
    const size_t Bn = (size_t)batch, nxe = per_knot ? (size_t)ex() * Bn : (size_t)nx * Bn, nue = per_knot ? (size_t)eu() * Bn : (size_t)nu * Bn;
    route_gen += 1;
    bounds_mode = per_knot ? 2 : 1;
    ib_xmin.assign(xmin, xmin + nxe);
    ib_xmax.assign(xmax, xmax + nxe);
    ib_umin.assign(umin, umin + nue);
    ib_umax.assign(umax, umax + nue);
    const int old_sb = st.en_state_bound, old_ib = st.en_input_bound;
    st.en_state_bound = 1;
    st.en_input_bound = 1;
    packs_dirty = true;
    if (select_kernel() || ensure_extension_buffers()) {   // (no kernel takes the combination: the solver stays as it was)
        const std::string why = last_error();
        st.en_state_bound = old_sb, st.en_input_bound = old_ib;
        if (!old_mode) drop_instance_bounds();
        (void)select_kernel();
        set_error(why);
        return -1;
    }
    return 0;
}

void Solver::drop_instance_bounds() {
    if (!bounds_mode) return;
    (void)wait_last_launch();
    bounds_mode = 0;
    ib_xmin.clear(), ib_xmax.clear(), ib_umin.clear(), ib_umax.clear();
    d_ibx.free();
    d_ibu.free();
    route_gen += 1;
    packs_dirty = true;
}

// the host copies, narrowed to fp32 and transposed from the API's instance-major layout to [min | max][knot][instance][row].
// A solver with shared bounds and per-instance rows or cones (bounds_mode 0 under lin_mode / cone_mode) uploads the shared set replicated: one
// line per instance, constant over the horizon — or per knot, where the shared bounds differ between knots.
int Solver::upload_instance_bounds() {
    HIP_TRY(hipSetDevice(device));
    bool shared_by_knot = false;
    if (!bounds_mode) {
        for (int k = 1; k < N && !shared_by_knot; ++k)
            for (int r = 0; r < nx; ++r)
                if (x_min[r + (size_t)k * nx] != x_min[r] || x_max[r + (size_t)k * nx] != x_max[r]) shared_by_knot = true;
        for (int k = 1; k < N - 1 && !shared_by_knot; ++k)
            for (int a = 0; a < nu; ++a)
                if (u_min[a + (size_t)k * nu] != u_min[a] || u_max[a + (size_t)k * nu] != u_max[a]) shared_by_knot = true;
    }
    ib_by_knot = bounds_mode == 2 || shared_by_knot;
    const size_t Bn = (size_t)batch, kx = ib_by_knot ? (size_t)N : 1, ku = ib_by_knot ? (size_t)(N - 1) : 1;
    const bool rep = !bounds_mode;   // every instance reads the shared arrays ([knot][row])
    auto pack = [&](const std::vector<double> &lo, const std::vector<double> &hi, size_t rows, size_t knots, DevBuf<float> &dptr) -> int {
        const size_t half = knots * Bn * rows;
        std::vector<float> h(2 * half);
        for (size_t b = 0; b < Bn; ++b)
            for (size_t k = 0; k < knots; ++k)
                for (size_t r = 0; r < rows; ++r) {
                    const size_t src = ((rep ? 0 : b) * knots + k) * rows + r, dst = (k * Bn + b) * rows + r;
                    h[dst] = (float)lo[src];
                    h[half + dst] = (float)hi[src];
                }
        return dptr.upload(h);
    };
    if (rep) return pack(x_min, x_max, (size_t)nx, kx, d_ibx) || pack(u_min, u_max, (size_t)nu, ku, d_ibu);
    return pack(ib_xmin, ib_xmax, (size_t)nx, kx, d_ibx) || pack(ib_umin, ib_umax, (size_t)nu, ku, d_ibu);
}

// Linear rows PER INSTANCE.  Ax is [batch] blocks of mx x nx, column-major, bx [batch][mx]; the input side likewise.  An all-zero
// row of an instance is that instance's absent row.  Enables the non-empty sides, as set_linear does; the solver leaves the
// on-chip families for the stream / generic kernels' `il` forms (select_kernel).  Both sides empty: no rows at all.
int Solver::set_instance_linear(const double *Ax, int mx, const double *bx, const double *Au, int mu, const double *bu) {
    if (mx < 0 || mu < 0 || mx > LIN_MAX_ROWS || mu > LIN_MAX_ROWS) {
        set_error("set_instance_linear: at most 8 rows per side");
        return -1;
    }
    if ((mx > 0 && (!Ax || !bx)) || (mu > 0 && (!Au || !bu))) {
        set_error("set_instance_linear: null matrix or right-hand side");
        return -1;
    }
    if (st.adaptive_rho) {
        set_error("set_instance_linear: per-instance linear rows are not available with adaptive rho");
        return -1;
    }
    if (mx == 0 && mu == 0) return set_linear(nullptr, 0, nullptr, nullptr, 0, nullptr);
    if (wait_last_launch()) return -1;
    const size_t Bn = (size_t)batch;
    // what a refusal puts back
    const int o_mode = lin_mode, o_mlx = mlx, o_mlu = mlu, o_sl = st.en_state_linear, o_il = st.en_input_linear;
    std::vector<double> o_ax, o_bx, o_au, o_bu;
    o_ax.swap(il_Ax), o_bx.swap(il_bx), o_au.swap(il_Au), o_bu.swap(il_bu);
    route_gen += 1;
    lin_mode = 1;
    mlx = mx, mlu = mu;
    il_Ax.assign(Ax, Ax + (mx ? Bn * mx * nx : 0));
    il_bx.assign(bx, bx + (mx ? Bn * mx : 0));
    il_Au.assign(Au, Au + (mu ? Bn * mu * nu : 0));
    il_bu.assign(bu, bu + (mu ? Bn * mu : 0));
    if (mlx > 0) st.en_state_linear = 1;
    if (mlu > 0) st.en_input_linear = 1;
    packs_dirty = true;
    if (select_kernel() || ensure_extension_buffers() || upload_instance_linear()) {   // (no kernel takes the combination: the solver stays as it was)
        const std::string why = last_error();
        lin_mode = o_mode, mlx = o_mlx, mlu = o_mlu, st.en_state_linear = o_sl, st.en_input_linear = o_il;
        il_Ax.swap(o_ax), il_bx.swap(o_bx), il_Au.swap(o_au), il_bu.swap(o_bu);
        route_gen += 1;
        d_il.free();   // (re-made from the host copies at the next upload_packs where they are still per instance)
        (void)select_kernel();
        set_error(why);
        return -1;
    }
    return 0;
}

void Solver::drop_instance_linear() {
    if (!lin_mode) return;
    (void)wait_last_launch();
    lin_mode = 0;
    mlx = mlu = 0;   // (the shared host arrays hold no rows while the per-instance ones are installed)
    il_Ax.clear(), il_bx.clear(), il_Au.clear(), il_bu.clear();
    lin_Ax.clear(), lin_bx.clear(), lin_Au.clear(), lin_bu.clear();
    d_il.free();
    if (!bounds_mode && !cone_mode) {
        d_ibx.free();
        d_ibu.free();
    }
    route_gen += 1;
    lin_dirty = true;
    packs_dirty = true;
}

// the host copies, rounded as the shared pack rounds them ((float)a, (float)b, (float) of the fp64 sum of squares of the
// unrounded entries) and laid out as the kernels read them: Ax [row][instance][nx] | Au [row][instance][nu] | bx | |ax|^2 | bu |
// |au|^2, each [row][instance].  An all-zero row: a = 0, b = FLT_MAX, |a|^2 = 1 — `dot > b` never holds.
// A solver with shared rows and per-instance cones (lin_mode 0 under cone_mode) uploads the shared set (row-major, lin_Ax ..
// lin_bu) replicated, every row of either side, switched on or not, as the per-instance ones are.
int Solver::upload_instance_linear() {
    HIP_TRY(hipSetDevice(device));
    const size_t Bn = (size_t)batch, nax = (size_t)mlx * Bn * nx, nau = (size_t)mlu * Bn * nu;
    const bool rep = !lin_mode;
    std::vector<float> h(std::max<size_t>(nax + nau + 2 * Bn * (mlx + mlu), 1));   // (no rows at all: one word, so that the pointer exists)
    auto put = [&](const std::vector<double> &A, const std::vector<double> &bv, size_t m, size_t n, float *a, float *rb, float *rn2) {
        for (size_t b = 0; b < Bn; ++b)
            for (size_t k = 0; k < m; ++k) {
                double n2 = 0.0;
                for (size_t j = 0; j < n; ++j) {
                    const double v = rep ? A[k * n + j] : A[b * m * n + k + j * m];
                    a[(k * Bn + b) * n + j] = (float)v;
                    n2 += v * v;
                }
                const bool absent = !(n2 > 0.0);
                rb[k * Bn + b] = absent ? FLT_MAX : (float)bv[(rep ? 0 : b * m) + k];
                rn2[k * Bn + b] = absent ? 1.f : (float)n2;
            }
    };
    float *bx = h.data() + nax + nau, *n2x = bx + Bn * mlx, *bu = n2x + Bn * mlx, *n2u = bu + Bn * mlu;
    put(rep ? lin_Ax : il_Ax, rep ? lin_bx : il_bx, (size_t)mlx, (size_t)nx, h.data(), bx, n2x);
    put(rep ? lin_Au : il_Au, rep ? lin_bu : il_bu, (size_t)mlu, (size_t)nu, h.data() + nax, bu, n2u);
    return d_il.upload(h);
}

int Solver::set_fdyn(const double *f) {
    route_gen += 1;   // (array-valued state the routes read: the routing key only carries scalars)
    bool nz = false;
    for (int i = 0; i < nx; ++i) {
        fdyn[i] = f ? f[i] : 0.0;
        nz = nz || fdyn[i] != 0.0;
    }
    has_fdyn = nz;
    packs_dirty = true;
    plant_dirty = true;   // (the chained closed loop's plant carries f)
    return select_kernel() || ensure_extension_buffers();
}

// Cone coefficients PER INSTANCE.  The layout (Acu, qcu, Acx, qcx) is one for the batch; cu is [batch][ncu], cx [batch][ncx]: mu
// of every cone for every instance, +inf for a cone the instance does not have.  Enables the non-empty sides, as set_cones
// does; the solver leaves the on-chip families for the stream / generic kernels' `ic` forms (select_kernel).  Both sides
// empty: no cones at all, shared mode.
int Solver::set_instance_cones(const int *Acu_, const int *qcu_, const double *cu_, int ncu_, const int *Acx_, const int *qcx_,
                               const double *cx_, int ncx_) {
    if (ncu_ < 0 || ncx_ < 0 || ncu_ > 8 || ncx_ > 8) {
        set_error("set_instance_cones: at most 8 cones per knot and side");
        return -1;
    }
    if ((ncu_ > 0 && (!Acu_ || !qcu_ || !cu_)) || (ncx_ > 0 && (!Acx_ || !qcx_ || !cx_))) {
        set_error("set_instance_cones: null layout or coefficients");
        return -1;
    }
    for (int i = 0; i < ncu_; ++i)
        if (Acu_[i] < 0 || qcu_[i] < 2 || Acu_[i] + qcu_[i] > nu) {
            set_error("set_instance_cones: input cone out of range (need 0 <= Ac, qc >= 2, Ac + qc <= nu)");
            return -1;
        }
    for (int i = 0; i < ncx_; ++i)
        if (Acx_[i] < 0 || qcx_[i] < 2 || Acx_[i] + qcx_[i] > nx) {
            set_error("set_instance_cones: state cone out of range (need 0 <= Ac, qc >= 2, Ac + qc <= nx)");
            return -1;
        }
    const size_t Bn = (size_t)batch;
    // (+inf: absent; NaN, -inf, <= 0 refused, and so is a finite value that fp32 would round to 0 or to +inf.  Non-finite values
    // are told by their bits: this file is compiled with -fno-honor-nans, under which a comparison does not see a NaN)
    auto bad = [](double mu) {
        uint64_t u;
        std::memcpy(&u, &mu, sizeof u);
        if (((u >> 52) & 0x7ffu) == 0x7ffu) return u != 0x7ff0000000000000ull;   // only +inf passes
        const float f = (float)mu;
        return !(f > 0.f) || f > FLT_MAX;
    };
    for (size_t i = 0; i < Bn * ncu_; ++i)
        if (bad(cu_[i])) {
            set_error("set_instance_cones: mu must be positive and finite, or +inf for a cone the instance does not have (input side)");
            return -1;
        }
    for (size_t i = 0; i < Bn * ncx_; ++i)
        if (bad(cx_[i])) {
            set_error("set_instance_cones: mu must be positive and finite, or +inf for a cone the instance does not have (state side)");
            return -1;
        }
    if (st.adaptive_rho) {
        set_error("set_instance_cones: per-instance cones are not available with adaptive rho");
        return -1;
    }
    if (ncu_ == 0 && ncx_ == 0) return set_cones(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0);
    if (wait_last_launch()) return -1;
    // what a refusal puts back
    const int o_mode = cone_mode, o_ncx = ncx, o_ncu = ncu, o_ss = st.en_state_soc, o_is = st.en_input_soc;
    int o_Acx[8], o_qcx[8], o_Acu[8], o_qcu[8];
    for (int i = 0; i < 8; ++i) o_Acx[i] = Acx[i], o_qcx[i] = qcx[i], o_Acu[i] = Acu[i], o_qcu[i] = qcu[i];
    std::vector<double> o_cx, o_cu;
    o_cx.swap(ic_cx), o_cu.swap(ic_cu);
    route_gen += 1;
    cone_mode = 1;
    ncx = ncx_, ncu = ncu_;
    for (int i = 0; i < ncu; ++i) Acu[i] = Acu_[i], qcu[i] = qcu_[i];
    for (int i = 0; i < ncx; ++i) Acx[i] = Acx_[i], qcx[i] = qcx_[i];
    ic_cu.assign(cu_, cu_ + (ncu ? Bn * ncu : 0));
    ic_cx.assign(cx_, cx_ + (ncx ? Bn * ncx : 0));
    if (ncu > 0) st.en_input_soc = 1;
    if (ncx > 0) st.en_state_soc = 1;
    packs_dirty = true;
    if (select_kernel() || ensure_extension_buffers() || upload_instance_cones()) {   // (no kernel takes the combination: the solver stays as it was)
        const std::string why = last_error();
        cone_mode = o_mode, ncx = o_ncx, ncu = o_ncu, st.en_state_soc = o_ss, st.en_input_soc = o_is;
        for (int i = 0; i < 8; ++i) Acx[i] = o_Acx[i], qcx[i] = o_qcx[i], Acu[i] = o_Acu[i], qcu[i] = o_qcu[i];
        ic_cx.swap(o_cx), ic_cu.swap(o_cu);
        route_gen += 1;
        d_ic.free();   // (re-made from the host copies at the next upload_packs where they are still per instance)
        (void)select_kernel();
        set_error(why);
        return -1;
    }
    return 0;
}

void Solver::drop_instance_cones() {
    if (!cone_mode) return;
    (void)wait_last_launch();
    cone_mode = 0;
    ncx = ncu = 0;   // (the shared cx / cu hold no coefficient while the per-instance ones are installed)
    ic_cx.clear(), ic_cu.clear();
    d_ic.free();
    if (!lin_mode) d_il.free();
    if (!bounds_mode && !lin_mode) {
        d_ibx.free();
        d_ibu.free();
    }
    route_gen += 1;
    packs_dirty = true;
}

// the host copies, rounded to fp32 as the shared set's are and transposed to [cone][instance], state cones then input cones
int Solver::upload_instance_cones() {
    HIP_TRY(hipSetDevice(device));
    const size_t Bn = (size_t)batch;
    std::vector<float> h(Bn * (ncx + ncu));
    for (size_t b = 0; b < Bn; ++b) {
        for (int c = 0; c < ncx; ++c) h[(size_t)c * Bn + b] = (float)ic_cx[b * ncx + c];
        for (int c = 0; c < ncu; ++c) h[((size_t)ncx + c) * Bn + b] = (float)ic_cu[b * ncu + c];
    }
    return d_ic.upload(h);
}

int Solver::set_cones(const int *Acu_, const int *qcu_, const double *cu_, int ncu_, const int *Acx_,
                      const int *qcx_, const double *cx_, int ncx_) {
    route_gen += 1;
    if (ncu_ > 8 || ncx_ > 8) {
        set_error("set_cone_constraints: at most 8 cones per knot and side");
        return -1;
    }
    for (int i = 0; i < ncu_; ++i)
        if (Acu_[i] < 0 || qcu_[i] < 2 || Acu_[i] + qcu_[i] > nu || !(cu_[i] > 0.0)) {
            set_error("set_cone_constraints: input cone out of range (need 0 <= Ac, qc >= 2, Ac + qc <= nu, mu > 0)");
            return -1;
        }
    for (int i = 0; i < ncx_; ++i)
        if (Acx_[i] < 0 || qcx_[i] < 2 || Acx_[i] + qcx_[i] > nx || !(cx_[i] > 0.0)) {
            set_error("set_cone_constraints: state cone out of range (need 0 <= Ac, qc >= 2, Ac + qc <= nx, mu > 0)");
            return -1;
        }
    drop_instance_cones();   // the shared set replaces a per-instance one
    ncu = ncu_;
    ncx = ncx_;
    for (int i = 0; i < ncu; ++i) {
        Acu[i] = Acu_[i];
        qcu[i] = qcu_[i];
        cu[i] = cu_[i];
    }
    for (int i = 0; i < ncx; ++i) {
        Acx[i] = Acx_[i];
        qcx[i] = qcx_[i];
        cx[i] = cx_[i];
    }
    if (ncu > 0) st.en_input_soc = 1;  // bindings.cpp:478-483: only the non-empty halves are enabled
    if (ncx > 0) st.en_state_soc = 1;
    packs_dirty = true;   // (what upload_packs decides from extensions_active(): lean_jit)
    return select_kernel() || ensure_extension_buffers();
}

// UNPINNED (bindings.cpp:413-450): Alin_x (mx x nx), Alin_u (mu x nu) column-major; enables the non-empty halves
int Solver::set_linear(const double *Ax, int mx, const double *bx, const double *Au, int mu, const double *bu) {
    route_gen += 1;   // (array-valued state the routes read: the routing key only carries scalars)
    if (lin_mode && mx >= 0 && mu >= 0 && mx <= LIN_MAX_ROWS && mu <= LIN_MAX_ROWS) drop_instance_linear();   // the shared set replaces a per-instance one
    if (mx < 0 || mu < 0 || mx > LIN_MAX_ROWS || mu > LIN_MAX_ROWS) {
        set_error("set_linear_constraints: at most 8 rows per side");
        return -1;
    }
    if ((mx > 0 && (!Ax || !bx)) || (mu > 0 && (!Au || !bu))) {
        set_error("set_linear_constraints: null matrix or right-hand side");
        return -1;
    }
    auto take = [&](const double *A, const double *b, int m, int n, std::vector<double> &Ar, std::vector<double> &br) {
        Ar.assign((size_t)m * n, 0.0);
        br.assign((size_t)m, 0.0);
        for (int k = 0; k < m; ++k) {
            double n2 = 0.0;
            for (int j = 0; j < n; ++j) {
                Ar[(size_t)k * n + j] = A[k + (size_t)j * m];
                n2 += A[k + (size_t)j * m] * A[k + (size_t)j * m];
            }
            if (!(n2 > 0.0)) return false;
            br[k] = b[k];
        }
        return true;
    };
    std::vector<double> ax, bxv, au, buv;
    if (!take(Ax, bx, mx, nx, ax, bxv) || !take(Au, bu, mu, nu, au, buv)) {
        set_error("set_linear_constraints: a constraint row is all zero");
        return -1;
    }
    if (cone_mode) {   // (the `ic` forms read the shared rows replicated: upload_instance_linear at the next upload_packs)
        (void)wait_last_launch();
        d_il.free();
    }
    mlx = mx;
    mlu = mu;
    lin_Ax.swap(ax);
    lin_bx.swap(bxv);
    lin_Au.swap(au);
    lin_bu.swap(buv);
    lin_dirty = true;
    if (mlx > 0) st.en_state_linear = 1;  // bindings.cpp:438-443: only the non-empty halves are enabled
    if (mlu > 0) st.en_input_linear = 1;
    packs_dirty = true;   // (what upload_packs decides from extensions_active(): lean_jit)
    return select_kernel() || ensure_extension_buffers();
}

// Scratch and cone / linear warm-start buffers of the stream and generic kernels, sized for the current batch / options.
int Solver::ensure_extension_buffers() {
    if (ke && !st.adaptive_rho) return 0;
    HIP_TRY(hipSetDevice(device));
    const size_t Bn = (size_t)batch, EX = (size_t)ex(), EU = (size_t)eu();
    if (st.adaptive_rho) {
        const size_t nk = (size_t)nu * nx, np = (size_t)nx * nx;
        if (!sens_set) {  // what the reference's host would compute and hand over (TinyMPC.jl:301-323)
            Mat dK, dP, dC1, dC2;
            if (compute_sensitivity(A, B, Q, R, cache.rho, dK, dP, dC1, dC2)) {
                set_error("adaptive_rho: sensitivity computation failed (singular R + rho I + B'PB)");
                return -1;
            }
            set_sensitivity(dK.a.data(), dP.a.data());
        }
        if (sens_dirty) {
            if (d_sens.upload(sens.data(), nk + np)) return -1;
            sens_dirty = false;
        }
        if (!d_adapt && d_adapt.alloc((1 + nk + np) * Bn)) return -1;
        if (adapt_dirty) {
            std::vector<double> fam(1 + nk + np);
            fam[0] = cache.rho;
            std::copy(cache.Kinf.a.begin(), cache.Kinf.a.end(), fam.begin() + 1);
            std::copy(cache.Pinf.a.begin(), cache.Pinf.a.end(), fam.begin() + 1 + nk);
            DevBuf<double> d_fam;
            if (d_fam.upload(fam)) return -1;
            const long total = (long)fam.size() * (long)Bn;
            adapt_fill_kernel<<<(unsigned)((total + 255) / 256), 256>>>(d_adapt, d_fam, (int)fam.size(), (long)Bn);
            HIP_TRY(hipDeviceSynchronize());
            adapt_dirty = false;
            adapt_pure = true;
        }
        if (se) {  // stream kernel: the per-lane columns of the rows built from Kinf / Pinf (kernel-local scratch)
            const size_t G = (size_t)se->lanes, rx = (nx + G - 1) / G, ru = (nu + G - 1) / G;
            const size_t len = ru * (G * rx) + rx * (G * ru) + rx * (G * rx);
            const size_t bytes = len * G * Bn * (precision == 0 ? 8 : 4);
            if (d_adp_cols.reserve(bytes)) return -1;
        }
    }
    if (ke) return 0;  // (a quad kernel running an adaptive solve: the adaptive state above is all it needs)
    const size_t sets = (size_t)constraint_sets();
    size_t need = Bn * ((2 + 3 * sets) * EX + (3 + 3 * sets) * EU);  // generic kernel: admm_generic.hip.h
    if (precision == 2) {   // fp64 state: the scratch arrays are doubles, and the workspace kept between solves is the fp64 block
        need *= 2;
        const size_t w = (size_t)Ws64::doubles((long)Bn, (long)EX, (long)EU, 3);
        if (d_ws64.count() < w && d_ws64.alloc_zero(w)) return -1;
    }
    if (se) need = std::max(need, Bn * se->scratch_floats(N, (int)sets) * (precision == 2 ? 2 : 1));   // (fp64 state: doubles)
    if (ce) need = ce->scratch_floats(*this);
    if (d_scratch.reserve(need)) return -1;
    if (cones_active() && !d_sgc) {
        if (d_sgc.alloc_zero(Bn * EX) || d_svc.alloc_zero(Bn * EX) || d_syc.alloc_zero(Bn * EU) || d_szc.alloc_zero(Bn * EU)) return -1;
    }
    if (lin_active() && !d_sgl) {
        if (d_sgl.alloc_zero(Bn * EX) || d_svl.alloc_zero(Bn * EX) || d_syl.alloc_zero(Bn * EU) || d_szl.alloc_zero(Bn * EU)) return -1;
    }
    if (!lin_mode && (lin_dirty || (lin_active() && !d_lin))) {   // (per-instance rows: upload_instance_linear)
        // [mlx][nx] rows | b | |a|^2 | [mlu][nu] rows | b | |a|^2   (fp32)
        std::vector<float> pk;
        auto put = [&](const std::vector<double> &A, const std::vector<double> &b, int m, int n) {
            for (size_t i = 0; i < (size_t)m * n; ++i) pk.push_back((float)A[i]);
            for (int k = 0; k < m; ++k) pk.push_back((float)b[k]);
            for (int k = 0; k < m; ++k) {
                double n2 = 0.0;
                for (int j = 0; j < n; ++j) n2 += A[(size_t)k * n + j] * A[(size_t)k * n + j];
                pk.push_back((float)n2);
            }
        };
        // (a side that has rows but is switched off — tinympc_enable_linear — is left out: the kernels find the input block
        // behind P.mlx state rows)
        put(lin_Ax, lin_bx, st.en_state_linear ? mlx : 0, nx);
        put(lin_Au, lin_bu, st.en_input_linear ? mlu : 0, nu);
        if (pk.empty()) pk.push_back(0.f);
        if (d_lin.upload(pk)) return -1;
        lin_dirty = false;
    }
    return 0;
}

// appends the ids of the instances that have not converged to `out` (order unspecified)
__global__ void compact_unsolved_kernel(const int *solved, const int *idx_in, int n_in, int *idx_out, int *count) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_in) return;
    const int b = idx_in ? idx_in[j] : j;
    if (!solved[b]) idx_out[atomicAdd(count, 1)] = b;
}

// status words 0..3 of a chunked solve: the maxima of every instance's FINAL residuals (what one launch would have
// folded), rebuilt from the per-instance residual array — the chunks' own blocks also hold the larger residuals that
// late-converging instances had at earlier chunk ends
__global__ void residual_max_kernel(const float *res, long batch, uint32_t *gstat) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += (long)gridDim.x * blockDim.x) {
        const float4 r = reinterpret_cast<const float4 *>(res)[b];
        m0 = fmaxf(m0, r.x), m1 = fmaxf(m1, r.y), m2 = fmaxf(m2, r.z), m3 = fmaxf(m3, r.w);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        m0 = fmaxf(m0, __shfl_xor(m0, off, 64));
        m1 = fmaxf(m1, __shfl_xor(m1, off, 64));
        m2 = fmaxf(m2, __shfl_xor(m2, off, 64));
        m3 = fmaxf(m3, __shfl_xor(m3, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&gstat[0], __float_as_uint(m0));
        atomicMax(&gstat[1], __float_as_uint(m1));
        atomicMax(&gstat[2], __float_as_uint(m2));
        atomicMax(&gstat[3], __float_as_uint(m3));
    }
}

// mpc_rollout: WHICH of its routes a closed loop takes — the one place that decides it, before anything is launched.
// Refusals first, each named once: what a reference sequence (set_ref_sequence: per-step shared references) does not go
// with; select_kernel's own; a selection without a closed loop — the stream / generic kernels have none unless
// TINYMPC_HIP_STREAM_MPC is set, and none with adaptive rho; a solver without the persistent workspace.  Then, in order of
// preference:
//   an own-plant solver (set_plant / set_disturbance) or one with a reference trajectory (set_ref_trajectory): the chain on
//     whatever kernel a plain kept-workspace solve of it takes, selected as for a plain solve, every family and precision, no
//     switch, every launch from the fp32 state (RolloutPlan::from_x0); not with adaptive rho;
//   the matrix-core kernel of the box-only shapes (mfma): the chain (rollout_chain, the one driver of every chain) — per step
//     one workspace-carrying launch, here handed the fp64 plant state, and the plant step, stream-ordered;
//   TINYMPC_HIP_LEAN_WS, where lean_plan takes a warm whole-batch launch (the calling pattern, whatever the iteration count):
//     that chain on the lean kernel; with TINYMPC_HIP_LEAN_LOOP beside it ONE launch of the lean kernel's in-kernel loop
//     (admm_lean.hip.h, MPC) — not with a reference sequence (the kernel stages the shared references once per launch), and
//     only where the loop kernel of the calling pattern exists: the entry has it, or its specialisation compiled;
//   the stream / generic kernels under their switch: that chain too, from the fp32 state — every precision, the affine term
//     (in the plant as well), cones, linear rows, per-instance references and families; with TINYMPC_HIP_STREAM_LOOP beside it
//     ONE launch of the stream kernel's in-kernel loop where one is built (admm_streamg.hip.h, MPC; not the generic kernel,
//     precision 1, a shape or form without a loop kernel);
//   else the loop fused into the selected kernel: the lanes-per-instance kernels, mfmat.
// A loop that runs inside one launch takes a reference sequence only as one shared reference set per step.
Solver::RolloutPlan Solver::plan_rollout(int mpc_steps) {
    RolloutPlan rp;
    auto refuse = [&rp](const std::string &why) {
        set_error(why);
        return rp;
    };
    if (ref_seq_steps > 0) {
        if (ref_seq_steps < mpc_steps)
            return refuse("mpc_rollout: the reference sequence holds " + std::to_string(ref_seq_steps) + " steps, the loop asks for " +
                          std::to_string(mpc_steps) + " (one reference set per step)");
        if (refs_per_instance())
            return refuse("mpc_rollout: a reference sequence is shared by the batch and cannot be combined with per-instance references "
                          "(set_ref_sequence with steps = 0 drops the sequence)");
        if (st.adaptive_rho) return refuse("mpc_rollout: a reference sequence is not available with adaptive rho");
        if (precision == 2 && !sw.stream_mpc && !own_plant())
            return refuse("mpc_rollout: a reference sequence is not available at precision 2 (which has no fused closed loop; step it from the host)");
    }
    if (cone_mode && !sw.stream_mpc && !(own_plant() || traj_kind))
        return refuse("mpc_rollout: per-instance cones have no closed loop by default (a plant of its own, or TINYMPC_HIP_STREAM_MPC=1, gives one as a chain of launches; or step it from the host)");
    if (lin_mode && !sw.stream_mpc && !(own_plant() || traj_kind))
        return refuse("mpc_rollout: per-instance linear rows have no closed loop by default (a plant of its own, or TINYMPC_HIP_STREAM_MPC=1, gives one as a chain of launches; or step it from the host)");
    if (bounds_mode && !sw.stream_mpc)
        return refuse("mpc_rollout: per-instance bounds have no closed loop by default (TINYMPC_HIP_STREAM_MPC=1 gives one as a chain of launches; or step it from the host)");
    if (own_plant() || traj_kind) {
        // a plant of its own or a disturbance: the chain on the kernel a plain kept-workspace solve takes (its launches ARE plain
        // solves, every kernel family and precision has them) — ahead of the kernels' own routes.
        // A reference trajectory takes the same chain, against the model where no plant is installed: every launch is handed
        // its step's window by ref_window_kernel, which no loop inside a kernel is
        if (dist_kind && dist_steps < mpc_steps)
            return refuse("mpc_rollout: the disturbance holds " + std::to_string(dist_steps) + " steps, the loop asks for " + std::to_string(mpc_steps) +
                          " (one row per step, read from row 0)");
        if (st.adaptive_rho)
            return refuse(estimating() ? "mpc_rollout: a state estimator is not available with adaptive rho"
                          : noisy() ? "mpc_rollout: process / measurement noise is not available with adaptive rho"
                                  : (own_plant() ? "mpc_rollout: a plant of its own / a disturbance is not available with adaptive rho"
                                                 : "mpc_rollout: a reference trajectory is not available with adaptive rho"));
        if (!warm_start) return refuse("mpc_rollout needs the persistent workspace (set_warm_start(1))");
        if (noisy() && noise_cursor > INT_MAX - mpc_steps)
            return refuse("mpc_rollout: the noise cursor would pass the largest int (the step index is one 32-bit word of the generator's counter; "
                          "set_noise_cursor, or another seed, starts a fresh stream)");
        if (traj_kind && ref_cursor > INT_MAX - mpc_steps)
            return refuse("mpc_rollout: the reference cursor would pass the largest int (set_ref_cursor: every cursor from the longer trajectory's last row on gives the same window)");
        if (select_kernel(false) || ensure_extension_buffers()) return rp;
        if ((packs_dirty && upload_packs()) || upload_refs()) return rp;
        rp.route = Rollout::Chain, rp.from_x0 = true;
        return rp;
    }
    if (select_kernel(true) || ensure_extension_buffers()) return rp;
    const bool fused = ke || (ce && ce->ws);
    const bool stream = sw.stream_mpc && !ke && !ce && !st.adaptive_rho;   // the stream or the generic kernel, under its switch
    if (!fused && !stream) return refuse("mpc_rollout: this problem shape / option set has no kernel with a fused closed loop");
    if (!warm_start) return refuse("mpc_rollout needs the persistent workspace (set_warm_start(1))");
    if ((packs_dirty && upload_packs()) || upload_refs()) return rp;   // (the lean entry and its pack are found there; the reference mode here)
    Pass step = whole_batch(false, true), loop = whole_batch(false, true, mpc_steps);
    step.iters = 1;
    Rollout route = Rollout::Fused;
    if (ke && ke->G == 16) {
        route = Rollout::Chain;
    } else if (sw.lean_ws && plan_lean(step).take) {
        loop.loop = true;
        route = (sw.lean_loop && ref_seq_steps == 0 && pick_kernel(loop).lean) ? Rollout::LeanLoop : Rollout::Chain;
    } else if (stream) {
        loop.stream_loop = true;
        route = (sw.stream_loop && pick_kernel(loop).stream_loop) ? Rollout::StreamLoop : Rollout::Chain;
    }
    if (route != Rollout::Chain && ref_seq_steps > 0 && ref_mode != REF_SHARED)
        return refuse("mpc_rollout: per-step references need one shared reference set per step");
    rp.route = route, rp.from_x0 = stream;
    return rp;
}

// A single solve is one launch_pass (or solve_chunked's); a closed loop is planned (plan_rollout), then launched as its route
// asks.  What a rollout leaves for get_mpc_log and the launch count are set here, once it has been enqueued.
int Solver::solve_async(hipStream_t stream, int mpc_steps) {
    HIP_TRY(hipSetDevice(device));
    layout_final = true;
    if (mpc_steps <= 0) {
        if (select_kernel() || ensure_extension_buffers()) return -1;
        if (traj_kind && ensure_ref_window(stream, ref_cursor)) return -1;   // (a reference trajectory: its window at the cursor)
        const bool chunkable = chunk_iters > 0 && !hetero && (ke || se || (ce && ce->ws)) && st.check_termination > 0 &&
                               st.abs_pri_tol > 0.0 && st.abs_dua_tol > 0.0 && st.max_iter > chunk_iters;
        return chunkable ? solve_chunked(stream) : launch_pass(stream, whole_batch(!warm_start, warm_start));
    }
    const RolloutPlan rp = plan_rollout(mpc_steps);
    if (rp.route == Rollout::Refused || ensure_mpc_log(mpc_steps)) return -1;
    const int cursor0 = ref_cursor;   // (the chain leaves the cursor mpc_steps further on)
    int rc = -1;
    switch (rp.route) {
    case Rollout::Fused: rc = launch_pass(stream, whole_batch(false, true, mpc_steps)); break;
    case Rollout::Chain: rc = rollout_chain(stream, mpc_steps, rp.from_x0); break;
    default: rc = rollout_loop(stream, mpc_steps, rp.route); break;
    }
    if (rc) return rc;
    // the metrics' fold, behind the route on its stream and inside what the done event covers (set_rollout_metrics)
    if (metrics_on && fold_rollout_metrics(stream, mpc_steps, cursor0)) return -1;
    mpc_steps_last = mpc_steps;
    last_rollout_launches = rp.route == Rollout::Chain ? mpc_steps : 1;
    return 0;
}

// Chunks of (a multiple of check_termination) iterations; between chunks the unconverged instances are gathered
// into a dense index list on the device, so the next launch has no idle lanes for the finished ones.  The warm-start
// workspace carries every instance from chunk to chunk exactly (it is what the kernel holds, fp32), so the iterates,
// iteration counts and residuals are those of the single-launch solve.  Synchronises the stream between chunks.
int Solver::solve_chunked(hipStream_t stream) {
    const int ct = st.check_termination;
    const int chunk = std::max(ct, (chunk_iters + ct - 1) / ct * ct);
    if (!d_idx[0]) {
        if (d_idx[0].alloc((size_t)batch) || d_idx[1].alloc((size_t)batch) || d_count.alloc(1)) return -1;
    }
    uint32_t acc[GSTAT_WORDS] = {0};
    const int *idx = nullptr;
    int n = batch, offset = 0, cur = 0;
    for (;;) {
        const int iters = std::min(chunk, st.max_iter - offset);
        Pass chunk_pass;
        chunk_pass.idx = idx, chunk_pass.slots = n, chunk_pass.iter_offset = offset, chunk_pass.iters = iters;
        chunk_pass.cold = offset == 0 && !warm_start, chunk_pass.save = true;
        if (launch_pass(stream, chunk_pass)) return -1;
        offset += iters;
        HIP_TRY(hipMemcpyAsync(h_gstat, d_gstat, GSTAT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        const bool last = offset >= st.max_iter;
        int count = 0;
        if (!last) {
            HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int), stream));
            hipLaunchKernelGGL(compact_unsolved_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_solved, idx, n,
                               d_idx[cur], d_count);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        acc[4] = h_gstat[4];                                                // unsolved: what the latest chunk left
        if (last || count == 0) {
            if (count == 0 && !last) acc[4] = 0;
            break;
        }
        idx = d_idx[cur];
        n = count;
        cur ^= 1;
    }
    // the public block: unsolved count of the last chunk; residual maxima over every instance's final residuals
    HIP_TRY(hipMemcpyAsync(d_gstat, acc, GSTAT_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(residual_max_kernel, dim3((unsigned)std::min<long>(1024, ((long)batch + 255) / 256)), dim3(256), 0,
                       stream, d_res, (long)batch, d_gstat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

Solver::Pass Solver::whole_batch(bool cold, bool save, int mpc_steps) const {
    Pass a;
    a.slots = batch, a.iters = st.max_iter, a.cold = cold, a.save = save, a.mpc_steps = mpc_steps;
    return a;
}

// lean_plan (solver.h) of this solver and one launch: what the solver holds and what the launch asks, as scalars
LeanPlan Solver::plan_lean(const Pass &a) const {
    LeanPlanIn in;
    in.nx = nx, in.nu = nu, in.N = N;
    in.builtin = le != nullptr, in.kinds = le ? le->kinds : 0, in.builtin_sp = le ? le->sp : 0;
    in.lean_jit = lean_jit, in.lean_ok = lean_ok, in.model_sp = lean_sp, in.knot_bounds = lean_knot_bounds;
    in.quad_G = ke ? ke->G : 0, in.precision = precision;
    in.sw_one = sw.lean_one, in.sw_dense = sw.lean_dense, in.sw_ws = sw.lean_ws, in.sw_loop = sw.lean_loop;
    in.slots = a.slots, in.iters = a.iters, in.mpc_steps = a.mpc_steps;
    in.cold = a.cold, in.save = a.save, in.indexed = a.idx != nullptr, in.adaptive_rho = st.adaptive_rho != 0;
    in.ref_mode = ref_mode, in.loop = a.loop;
    in.state_bounds = state_bounds_active, in.g_maybe_nonzero = g_maybe_nonzero;
    in.live = st.abs_pri_tol > 0.0 && st.abs_dua_tol > 0.0;
    // (behind the stream kernel's fp64-state form the lean kernel is asked launch by launch: constraints added since the packs
    // were built go to the stream kernel's EXT forms)
    in.stream_ext = se && extensions_active();
    in.cus = device_cu_count();
    return lean_plan(in);
}

// the kernels' argument block: everything but the bound pack and the events, which depend on the kernel that runs
void Solver::fill_params(AdmmParams &P, const Pass &a) const {
    std::memset(&P, 0, sizeof(P));
    P.coef = reinterpret_cast<const float *>(static_cast<const unsigned char *>(d_coef));
    P.bounds = d_bounds;
    P.x0 = d_x0;
    P.x0d = a.x0d;
    P.xref = a.xref ? a.xref : d_xref;
    P.uref = a.uref ? a.uref : d_uref;
    P.xout = d_xout;
    P.uout = d_uout;
    P.iter = d_iter;
    P.solved = d_solved;
    P.res = d_res;
    P.sd = d_sd;
    P.sy = d_sy;
    P.sz = d_sz;
    P.sg = d_sg;
    P.sv = d_sv;
    P.gstat = d_gstat;
    P.gacc = d_gstat + GSTAT_WORDS;
    P.gslot_cap = sw.fold_slots < 0 ? (int)GSLOT_DEFAULT_CAP : std::min(sw.fold_slots, (int)GSLOT_DEFAULT_CAP);
    P.gslot = P.gslot_cap > 0 ? d_gslot : nullptr;
    P.scratch = d_scratch;
    P.idx = a.idx;
    P.iter_offset = a.iter_offset;
    P.batch = a.slots;
    P.max_iter = a.iters;
    P.check_termination = st.check_termination;
    P.ref_mode = ref_mode;
    P.cold_start = a.cold ? 1 : 0;
    P.save_state = a.save ? 1 : 0;
    P.abs_pri_tol = (float)st.abs_pri_tol;
    P.abs_dua_tol = (float)st.abs_dua_tol;
    P.rho = (float)cache.rho;
    P.nx = nx;
    P.nu = nu;
    P.N = N;
    P.mpc_steps = a.mpc_steps;
    P.mpc_x = d_mpc_x;
    P.mpc_u = d_mpc_u;
    P.mpc_iter = d_mpc_iter;
    P.x0_out = d_x0;
    P.xb_active = state_bounds_active ? 1 : 0;
    P.has_fdyn = has_fdyn ? 1 : 0;
    P.ncx = st.en_state_soc ? ncx : 0;
    P.ncu = st.en_input_soc ? ncu : 0;
    for (int i = 0; i < 8; ++i) {
        P.Acx[i] = Acx[i];
        P.qcx[i] = qcx[i];
        P.cx[i] = (float)cx[i];
        P.Acu[i] = Acu[i];
        P.qcu[i] = qcu[i];
        P.cu[i] = (float)cu[i];
    }
    P.het_aux = d_het_aux;
    P.adaptive_rho = st.adaptive_rho;
    P.rho_clip = st.adaptive_rho_clip;
    P.rho_family = cache.rho;
    P.rho_min = (float)st.adaptive_rho_min;
    P.rho_max = (float)st.adaptive_rho_max;
    P.sens = d_sens;
    P.adapt = d_adapt;
    P.adapt_stride = batch;
    P.adp_cols = d_adp_cols;
    P.sgc = d_sgc;
    P.svc = d_svc;
    P.syc = d_syc;
    P.szc = d_szc;
    P.mlx = st.en_state_linear ? mlx : 0;
    P.mlu = st.en_input_linear ? mlu : 0;
    P.lin = d_lin;
    P.sgl = d_sgl;
    P.svl = d_svl;
    P.syl = d_syl;
    P.szl = d_szl;
    P.bounds_stride = (ce && ce->bounds_vary(*this)) ? 1 : 0;
    // per-step references of a loop that runs inside the launch: mfmat's and the quad kernel's (the chain, rollout_chain,
    // hands every launch its step's slice as P.xref / P.uref instead and arrives here with mpc_steps = 0)
    if (a.mpc_steps > 0 && ref_seq_steps > 0) {
        P.xref_seq = d_xref_seq;
        P.uref_seq = d_uref_seq;
    }
    P.lean = d_lean;
    P.ws64 = d_ws64;
    P.abs_pri_tol64 = st.abs_pri_tol;
    P.abs_dua_tol64 = st.abs_dua_tol;
    if (bounds_mode || lin_mode || cone_mode) {   // (ib_by_knot: upload_instance_bounds — bounds_mode 2, or shared bounds that differ between knots under lin_mode / cone_mode)
        P.ibx = d_ibx, P.ibu = d_ibu;
        P.ib_kx = ib_by_knot ? (long)batch * nx : 0, P.ib_ku = ib_by_knot ? (long)batch * nu : 0;
        P.ib_hx = (long)batch * nx * (ib_by_knot ? N : 1), P.ib_hu = (long)batch * nu * (ib_by_knot ? N - 1 : 1);
        P.ib_on = (st.en_state_bound ? IB_STATE : 0) | (st.en_input_bound ? IB_INPUT : 0);
    }
    if (cone_mode) {
        P.ic_cx = d_ic, P.ic_cu = P.ic_cx + (long)ncx * batch;
        P.ic_rc = batch;
    }
    if (lin_mode || cone_mode) {
        const long Bn = batch;
        P.il_ax = d_il, P.il_au = P.il_ax + (long)mlx * Bn * nx;
        P.il_bx = P.il_au + (long)mlu * Bn * nu, P.il_n2x = P.il_bx + Bn * mlx, P.il_bu = P.il_n2x + Bn * mlx, P.il_n2u = P.il_bu + Bn * mlu;
        P.il_rx = Bn * nx, P.il_ru = Bn * nu, P.il_rb = Bn;
    }
    P.host_flags = (sw.no_refill ? HF_NO_REFILL : 0) | (sw.no_uni ? HF_NO_UNI : 0) | (sw.no_os ? HF_NO_OS : 0) |
                   (lean_ok && lean_scaled_ok && !sw.lean_unscaled ? HF_LEAN_SCALED : 0);
}

int Solver::ensure_mpc_log(int mpc_steps) {
    if (mpc_cap < mpc_steps) {
        const size_t n = (size_t)batch * mpc_steps;
        if (d_mpc_x.alloc(n * nx) || d_mpc_u.alloc(n * nu) || d_mpc_iter.alloc(n)) return -1;
        mpc_cap = mpc_steps;
    }
    return 0;
}

// carried: an event the launch's own dispatch packet already records at its end (a profiled lean launch)
int Solver::record_done(hipStream_t stream, hipEvent_t carried) {
    if (carried) {
        ev_wait = carried;
    } else {
        if (!ev_done) HIP_TRY(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev_done, stream));
        ev_wait = ev_done;
    }
    ev_done_pending = true;
    return 0;
}

// Which kernel beside the selected family's takes a launch: the lean kernel (same arithmetic as the quad entry's, a third fewer
// instructions) where lean_plan takes it — the built-in entry, or the one variant of a shape without one, compiled on first
// use — and, for the stream kernel's in-kernel closed loop, whether that kernel is built for this solver
Solver::Pick Solver::pick_kernel(const Pass &a) {
    Pick k;
    k.plan = plan_lean(a);
    k.lean = k.plan.take ? le : nullptr;
    if (k.plan.take && !le) {
        const int v = k.plan.variant;
        if (!le_var_tried[v]) le_var[v] = jit_lean_for(nx, nu, N, v, k.plan.form == LF_SPARSE ? k.plan.sp : 0, verbose), le_var_tried[v] = true;
        k.lean = le_var[v];
    }
    k.stream_loop = a.stream_loop && !k.lean && se && !bounds_mode && !lin_mode && !cone_mode && se->launch_mpc && se->has_mpc(precision, stream_ext(), hetero);   // (no `ib` loop form)
    return k;
}

int Solver::launch_pass(hipStream_t stream, const Pass &a) {
    // ---- prepare (a closed loop arrives planned: plan_rollout; what is refused here depends on the kernel that runs) ----
    if (packs_dirty && upload_packs()) return -1;
    if (upload_refs()) return -1;
    if (a.mpc_steps > 0 && ref_seq_steps > 0 && ke && ke->N > QUAD_REF_SEQ_MAX_N) {
        set_error("mpc_rollout: the lanes-per-instance kernels take a reference sequence at horizons up to " +
                  std::to_string((int)QUAD_REF_SEQ_MAX_N) + " (this entry: " + ke->name + "); step the loop from the host");
        return -1;
    }
    AdmmParams P;
    fill_params(P, a);
    // the quad and stream kernels keep the status block clean themselves (fold_status); the generic kernel
    // accumulates straight into it
    if (!ke && !se && !ce) HIP_TRY(hipMemsetAsync(d_gstat, 0, GSTAT_WORDS * sizeof(uint32_t), stream));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (profiling) {
        if (ev_ring.empty()) {
            ev_ring.assign(2 * EV_RING, nullptr);
            for (hipEvent_t &e : ev_ring) HIP_TRY(hipEventCreate(&e));
        }
        ev0 = ev_ring[2 * (launches % EV_RING)];
        ev1 = ev_ring[2 * (launches % EV_RING) + 1];
    }
    // the workspace's state dual is non-zero only if some solve since the last reset had a finite state bound (or the
    // caller wrote one in): the matrix-core kernel (G == 16) carries g only then
    if (state_bounds_active && a.save) g_maybe_nonzero = true;
    const bool carry_g = state_bounds_active || (ke && ke->G == 16 && g_maybe_nonzero);
    // ---- plan ----
    const Pick pick = pick_kernel(a);
    const LeanPlan &plan = pick.plan;
    const LeanEntry *lk = pick.lean;
    const bool lean = lk != nullptr, sloop = pick.stream_loop;
    if (lean && !le && (!ke || ke->G != 1)) P.bounds = reinterpret_cast<const float *>(d_lean + lean_layout(nx, nu).total);   // (upload_packs)
    // ---- launch ----
    // A profiled lean launch carries its two timing events in the kernel's own dispatch packet (start and end of the kernel):
    // recorded on their own they are marker packets the command processor handles between two kernels that are already
    // serialised, and a third one for the completion wait — four packets per solve where one does.  The stop event then
    // serves the completion wait too.  TINYMPC_HIP_EVENT_MARKERS: the separate records (timing aid).
    const bool attached = profiling && lean && !sw.event_markers;
    if (profiling && !attached) HIP_TRY(hipEventRecord(ev0, stream));
    if (lean)
        HIP_TRY(lk->launch(P, plan.variant, stream, attached ? ev0 : nullptr, attached ? ev1 : nullptr));
    else
        HIP_TRY(ke ? ke->launch(P, precision, carry_g, stream)
                   : (ce ? ce->launch(P, cones_active(), ce->lds_bytes(*this), stream)
                         : (se ? (sloop ? se->launch_mpc(P, precision, stream_ext(), hetero, stream)
                                        : (precision == 2 ? se->launch_f64(P, stream_ext(), stream)
                                                          : cone_mode ? se->launch_ic(P, hetero, stream)
                                                          : lin_mode ? se->launch_il(P, hetero, stream)
                                                          : (bounds_mode ? se->launch_ib(P, stream_ext(), hetero, stream)
                                                                         : se->launch(P, precision, stream_ext(), hetero, stream))))
                               : launch_generic(P, precision, stream))));
    // ---- record ----
    if (profiling) {
        if (!attached) HIP_TRY(hipEventRecord(ev1, stream));
        launches += 1;
    }
    last_launch_name = lean ? lk->name : kernel_name;
    last_lean_form = lean ? plan.form : LF_NONE;
    last_lean_scaled = lean && lean_runs_scaled(lk, plan.variant, P.host_flags);
    last_lean_cost[0] = lean ? plan.cost_sparse : 0;
    last_lean_cost[1] = lean ? plan.cost_dense : 0;
    // the status block stays on the device; solve_status() fetches it when asked (nothing but the kernel and the
    // 32-byte clear is enqueued per solve)
    solved_once = true;
    return record_done(stream, attached ? ev1 : nullptr);
}

// x0d <- x0 (start of a closed loop)
__global__ void plant_init_kernel(double *x0d, const float *x0, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x0d[i] = (double)x0[i];
}

// ... of a stream / generic closed loop behind an earlier one: where x0 still is the fp32 rounding of the fp64 plant state that
// loop left, the loop goes on from that state — mpc_rollout(a) then mpc_rollout(b) is mpc_rollout(a + b) — and from x0
// wherever the caller has set another one since (on the host or in the device buffer)
__global__ void plant_resume_kernel(double *x0d, const float *x0, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (float)x0d[i] != x0[i]) x0d[i] = (double)x0[i];
}

// the fp64 plant state a closed loop outside the selected kernel starts from.  resume: the from_x0 chains and the stream loop, which go on
// from the state an earlier loop of theirs left (x0d_live); every other route starts from x0
int Solver::plant_start(hipStream_t stream, bool resume) {
    if (!d_x0d && d_x0d.alloc((size_t)batch * nx)) return -1;
    const long n0 = (long)batch * nx;
    (resume && x0d_live ? plant_resume_kernel : plant_init_kernel)<<<(unsigned)((n0 + 255) / 256), 256, 0, stream>>>(d_x0d, d_x0, n0);
    HIP_TRY(hipGetLastError());
    if (resume) x0d_live = true;
    return 0;
}

// The plant every chained closed loop steps, on the device: [A | B | f] column-major fp64, one block or — plant_stride() != 0 —
// [batch] of them.  The installed plant (set_plant) where there is one; else the model: A, B and the affine term as set_fdyn
// left it (zero without one), on a per-instance-family solver every instance's own A_b, B_b beside the shared f.  Whether a
// disturbance, noise or a trajectory is installed does not enter.
int Solver::ensure_plant() {
    if (d_plant && !plant_dirty) return 0;
    if (wait_last_launch()) return -1;   // (a chain still running reads it)
    const size_t na = (size_t)nx * nx, nb = (size_t)nx * nu, blk = na + nb + nx, n = own_plant_per_instance() ? (size_t)batch : 1;
    std::vector<double> h(n * blk);
    for (size_t b = 0; b < n; ++b) {
        double *o = h.data() + b * blk;
        if (plant_kind) {
            std::copy(own_A.begin() + b * na, own_A.begin() + (b + 1) * na, o);
            std::copy(own_B.begin() + b * nb, own_B.begin() + (b + 1) * nb, o + na);
            std::copy(own_f.begin() + b * nx, own_f.begin() + (b + 1) * nx, o + na + nb);
        } else {
            const double *Am = hetero ? het_A.data() + b * na : A.a.data(), *Bm = hetero ? het_B.data() + b * nb : B.a.data();
            std::copy(Am, Am + na, o);
            std::copy(Bm, Bm + nb, o + na);
            for (int r = 0; r < nx; ++r) o[na + nb + r] = has_fdyn ? fdyn[r] : 0.0;
        }
    }
    if (d_plant.upload(h)) return -1;
    // ... and, for an estimator beside an installed plant, the model's image as a second one (its predict never steps the plant)
    if (estimating() && plant_kind) {
        const size_t nm = hetero ? (size_t)batch : 1;
        h.assign(nm * blk, 0.0);
        for (size_t b = 0; b < nm; ++b) {
            double *o = h.data() + b * blk;
            const double *Am = hetero ? het_A.data() + b * na : A.a.data(), *Bm = hetero ? het_B.data() + b * nb : B.a.data();
            std::copy(Am, Am + na, o);
            std::copy(Bm, Bm + nb, o + na);
            for (int r = 0; r < nx; ++r) o[na + nb + r] = has_fdyn ? fdyn[r] : 0.0;
        }
        if (d_model.upload(h)) return -1;
    }
    plant_dirty = false;
    return 0;
}

int Solver::set_plant(const double *A_, const double *B_, const double *f_, int per_instance) {
    if (!A_ && !B_) {
        plant_kind = 0;
        own_A.clear(), own_B.clear(), own_f.clear();
        plant_dirty = true;   // (back to the model's; ensure_plant waits for a chain still reading the image)
        return 0;
    }
    if (!A_ || !B_) {
        set_error("set_plant: expected both A (nx x nx) and B (nx x nu), or neither to drop the plant");
        return -1;
    }
    const size_t n = per_instance ? (size_t)batch : 1, na = (size_t)nx * nx, nb = (size_t)nx * nu;
    own_A.assign(A_, A_ + n * na);
    own_B.assign(B_, B_ + n * nb);
    if (f_)
        own_f.assign(f_, f_ + n * nx);
    else
        own_f.assign(n * nx, 0.0);
    plant_kind = per_instance ? 2 : 1;
    plant_dirty = true;
    return 0;
}

int Solver::set_disturbance(const double *w, int steps, int per_instance) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;   // (a chain still running reads it)
    if (!w || steps <= 0) {
        dist_kind = 0, dist_steps = 0;
        dist_w.clear();
        d_dist.free();
        return 0;
    }
    const size_t n = (per_instance ? (size_t)batch : 1) * (size_t)steps * nx;
    dist_w.assign(w, w + n);
    if (d_dist.upload(dist_w)) return -1;
    dist_kind = per_instance ? 2 : 1, dist_steps = steps;
    return 0;
}

void Solver::drop_own_plant() {
    if (!own_plant()) return;
    (void)wait_last_launch();
    plant_kind = dist_kind = dist_steps = 0;
    own_A.clear(), own_B.clear(), own_f.clear(), dist_w.clear();
    d_dist.free();
    plant_dirty = true;
}

// ---- noise drawn on the device (tinympc_set_process_noise / _set_measurement_noise; the rule: noise.h) ----
// The kernels here share plant_step_kernel's layout — 256 / nx instances per workgroup, lane (instance, r) owns row r — and
// one way to the noise vector: the lanes r < ceil(nx / 2) of an instance draw its pair r (one Philox block and one Box-Muller
// each, nothing drawn twice) into the workgroup's LDS, and after the barrier every lane takes its row of G xi (noise_row).
// G: instance b's factor at G + b * g_stride (0: shared).  Every lane of the workgroup reaches the barrier.
__device__ inline double noise_block_row(double *xi, const double *G, long g_stride, unsigned long long seed, int which, long b, unsigned t,
                                         int nx, int r, bool on) {
    double *mine = xi + ((int)threadIdx.x / nx) * nx;
    if (on && 2 * r < nx) {
        double even, odd;
        noise_pair(seed, which, (uint64_t)b, t, (uint32_t)r, even, odd);
        mine[2 * r] = even;
        if (2 * r + 1 < nx) mine[2 * r + 1] = odd;
    }
    __syncthreads();
    return on ? noise_row(G + b * g_stride, nx, r, mine) : 0.0;
}

// tinympc_get_noise: out[b][s][r] = (G xi[which][b][t0 + s])[r]; workgroup = (step s, 256 / nx instances)
__global__ void noise_fill_kernel(double *out, const double *G, long g_stride, unsigned long long seed, int which, int nx, long batch, int steps,
                                  int t0) {
    __shared__ double xi[256];
    const int per_block = (int)blockDim.x / nx, t = (int)threadIdx.x, r = t % nx;
    const long groups = (batch + per_block - 1) / per_block, s = (long)blockIdx.x / groups;
    const long b = ((long)blockIdx.x - s * groups) * per_block + t / nx;
    const bool on = t < per_block * nx && b < batch;
    const double n = noise_block_row(xi, G, g_stride, seed, which, b, (unsigned)(t0 + (int)s), nx, r, on);
    if (on) out[(b * steps + s) * nx + r] = n;
}

// The measurement a step's solve starts from: x0 = ylog[b][step] = (float)(x0d + G_v xi_v[b][t]); x0d, the true state, is read only
__global__ void measure_kernel(float *x0, float *ylog, const double *x0d, const double *G, long g_stride, unsigned long long seed, int nx, long batch,
                               int steps, int step, int t) {
    __shared__ double xi[256];
    const int per_block = (int)blockDim.x / nx, lane = (int)threadIdx.x, r = lane % nx;
    const long b = (long)blockIdx.x * per_block + lane / nx;
    const bool on = lane < per_block * nx && b < batch;
    const double n = noise_block_row(xi, G, g_stride, seed, NOISE_MEASUREMENT, b, (unsigned)t, nx, r, on);
    if (!on) return;
    const float y = (float)(x0d[b * nx + r] + n);
    x0[b * nx + r] = y;
    ylog[(b * steps + step) * nx + r] = y;
}

// The noise of one step (plant_step_kernel<true>): Gw / Gv null where that kind is not drawn in this launch; t = noise cursor + step
struct StepNoise {
    const double *Gw, *Gv;
    long gw_stride, gv_stride;
    unsigned long long seed_w, seed_v;
    float *ylog;
    int t;
};

// One closed-loop step behind a solve (cartpole_example_mpc.jl:35-51), the one rule of every chained closed loop:
// x+ = f + A x + B u0 (+ w) (+ G_w xi_w) in fp64, u0 = the first column of the solution.  One thread per (instance, row), 256 / nx
// instances per workgroup, lane (instance, r) owns row r: acc = f[r], then A's row by ascending column, then B's, one fma each;
// with a disturbance one fp64 add acc + w[r]; the process draw last, acc + (G_w xi_w[b][t])[r]; every row has read the old state
// at the barrier (which every lane reaches), then x0d = acc, mpc_x = (float)acc — the true state — the control and the iteration
// count, signed by the solved flag, like the quad kernel's fused loop logs them.  x0 = (float)acc too, unless nz.Gv is given:
// then x0 and ylog[b][step + 1] take the NEXT step's measurement (float)(acc + (G_v xi_v[b][t + 1])[r]), what measure_kernel
// would write ahead of that step's launch.
// plant: [A | B | f] column-major fp64, instance b's block at plant + b * plant_stride (0: one shared block; an instance's
// nx (nx + nu + 1) doubles are contiguous and row r of every column is lane r's, so a workgroup reads one contiguous span).
// w: this step's row of the disturbance, instance b's at w + b * w_stride (0: shared); null: none.
// Two forms, because of what the draws cost: NOISE false reads nothing of nz and has no LDS; true holds the two draw buffers.
template <bool NOISE>
__global__ void plant_step_kernel(double *x0d, float *x0, const float *uout, const int *iter, const int *solved, const double *plant,
                                  long plant_stride, const double *w, long w_stride, float *mpc_x, float *mpc_u, int *mpc_iter, StepNoise nz,
                                  int nx, int nu, int N, long batch, int steps, int step) {
    const int per_block = (int)blockDim.x / nx, lane = (int)threadIdx.x, r = lane % nx;
    const long b = (long)blockIdx.x * per_block + lane / nx;
    const bool on = lane < per_block * nx && b < batch;
    double acc = 0.0;
    if (on) {
        const double *A = plant + b * plant_stride, *Bm = A + nx * nx;
        const float *u0 = uout + b * (long)nu * (N - 1);
        acc = Bm[nx * nu + r];
        for (int j = 0; j < nx; ++j) acc = fma(A[r + j * nx], x0d[b * nx + j], acc);
        for (int a = 0; a < nu; ++a) acc = fma(Bm[r + a * nx], (double)u0[a], acc);
        if (w) acc = acc + w[b * w_stride + r];
    }
    double next = acc;
    if constexpr (NOISE) {
        __shared__ double xi_w[256], xi_v[256];
        if (nz.Gw) acc = acc + noise_block_row(xi_w, nz.Gw, nz.gw_stride, nz.seed_w, NOISE_PROCESS, b, (unsigned)nz.t, nx, r, on);
        next = acc;
        if (nz.Gv) next = acc + noise_block_row(xi_v, nz.Gv, nz.gv_stride, nz.seed_v, NOISE_MEASUREMENT, b, (unsigned)nz.t + 1u, nx, r, on);
    }
    __syncthreads();   // (every row has read x0d)
    if (!on) return;
    const long so = b * steps + step;
    x0d[b * nx + r] = acc;
    x0[b * nx + r] = (float)next;
    mpc_x[so * nx + r] = (float)acc;
    if constexpr (NOISE)
        if (nz.Gv) nz.ylog[(so + 1) * nx + r] = (float)next;
    for (int a = r; a < nu; a += nx) mpc_u[so * nu + a] = uout[b * (long)nu * (N - 1) + a];
    if (r == 0) mpc_iter[so] = solved[b] ? iter[b] : -iter[b];
}

// The chain: per step one workspace-carrying launch and the plant step, stream-ordered, the plant state in fp64 on the device
// between them.  from_x0: every launch is the solver's ordinary kept-workspace launch, from the fp32 rounding in d_x0 (Pass::x0d
// null, what a host-stepped loop launches), and the fp64 state goes on from an earlier loop's (plant_start); otherwise — the
// matrix-core and lean kernels' chains — the launch reads the fp64 state itself and the loop starts from x0.
// With a reference sequence every launch reads its step's slice of the sequence as its shared references (step 0's are the
// solver's own, which stay installed: nothing is copied, and the stream is not synchronised between steps).  With a reference
// trajectory every launch is handed its step's window first (ref_window_kernel, where the window on the device is another),
// and the cursor is left mpc_steps further on.
// With noise the step is plant_step_kernel's noise form, t = noise cursor + step: with measurement noise it also writes the NEXT
// step's measurement into x0 (and the y log), so only step 0's comes from measure_kernel ahead of the first launch; the last
// step leaves the true state's rounding in x0.  TINYMPC_HIP_NOISE_SPLIT (timing aid): measure_kernel ahead of every launch,
// the same values.  The noise cursor is left mpc_steps further on.
// With an estimator (set_estimator; estimator.hip) the solves start from its estimate instead: estimator_step_kernel<false, true>
// ahead of the first launch, <true, true> behind every plant step but the last, <true, false> behind the last; no
// measure_kernel, and the plant step draws no measurement (nz.Gv null).  TINYMPC_HIP_ESTIMATOR_SPLIT: predict and correct as
// separate launches, the same bits.
int Solver::rollout_chain(hipStream_t stream, int mpc_steps, bool from_x0) {
    if (ensure_plant() || plant_start(stream, from_x0)) return -1;
    const size_t EX = (size_t)ex(), EU = (size_t)eu(), per_block = 256 / nx;
    const unsigned step_groups = (unsigned)((batch + per_block - 1) / per_block);
    const bool est = estimating();                                 // (the estimator draws the measurement itself: estimator.hip)
    const bool measured = noise_kind[NOISE_MEASUREMENT] != 0 && !est;
    const long gw_stride = noise_kind[NOISE_PROCESS] == 2 ? (long)nx * nx : 0L, gv_stride = noise_kind[NOISE_MEASUREMENT] == 2 ? (long)nx * nx : 0L;
    if (measured) {
        if (mpc_y_cap < mpc_steps) {
            if (d_mpc_y.alloc((size_t)batch * mpc_steps * nx)) return -1;
            mpc_y_cap = mpc_steps;
        }
        mpc_y_steps = mpc_steps;
    }
    if (est && ensure_estimator_logs(mpc_steps)) return -1;
    Pass pass = whole_batch(false, true);
    pass.x0d = from_x0 ? nullptr : d_x0d;
    for (int step = 0; step < mpc_steps; ++step) {
        if (ref_seq_steps > 0 && step > 0) pass.xref = d_xref_seq + step * EX, pass.uref = d_uref_seq + step * EU;
        if (traj_kind && ensure_ref_window(stream, ref_cursor + step)) return -1;
        if (est && (step == 0 || sw.estimator_split) && estimator_step(stream, false, true, mpc_steps, step)) return -1;
        if (measured && (step == 0 || sw.noise_split))
            measure_kernel<<<step_groups, 256, 0, stream>>>(d_x0, d_mpc_y, d_x0d, d_noise_G[NOISE_MEASUREMENT], gv_stride, noise_seed[NOISE_MEASUREMENT], nx,
                                                            (long)batch, mpc_steps, step, noise_cursor + step);
        if (launch_pass(stream, pass)) return -1;
        const double *w = dist_kind ? d_dist + (size_t)step * nx : nullptr;
        const long w_stride = dist_kind == 2 ? (long)dist_steps * nx : 0L;
        StepNoise nz{};
        if (noisy())
            nz = {d_noise_G[NOISE_PROCESS], measured && !sw.noise_split && step + 1 < mpc_steps ? d_noise_G[NOISE_MEASUREMENT] : nullptr,
                  gw_stride, gv_stride, noise_seed[NOISE_PROCESS], noise_seed[NOISE_MEASUREMENT], d_mpc_y, noise_cursor + step};
        (noisy() ? plant_step_kernel<true> : plant_step_kernel<false>)<<<step_groups, 256, 0, stream>>>(
            d_x0d, d_x0, d_uout, d_iter, d_solved, d_plant, plant_stride(), w, w_stride, d_mpc_x, d_mpc_u, d_mpc_iter, nz, nx, nu, N, (long)batch,
            mpc_steps, step);
        // the estimator behind the plant step: the predict with this step's u, fused with the next step's correct (its log row,
        // its draw) on every step but the last, which leaves x0 as the plant step wrote it
        if (est && estimator_step(stream, true, !sw.estimator_split && step + 1 < mpc_steps, mpc_steps, step + 1)) return -1;
    }
    HIP_TRY(hipGetLastError());
    if (traj_kind) ref_cursor += mpc_steps;   // (plan_rollout checked the sum)
    if (noisy()) noise_cursor += mpc_steps;   // (likewise)
    return record_done(stream);
}


// ---- noise: set, drop, read back (the kernels are above the chain) ----
// G: nx x nx column-major fp64, or [batch][nx*nx]; null drops that kind.  The cursor stays where it is.
int Solver::set_noise(int which, const double *G, int per_instance, unsigned long long seed) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;   // (a chain still running reads the factor)
    if (!G) {
        noise_kind[which] = 0;
        noise_G[which].clear();
        d_noise_G[which].free();
        if (which == NOISE_MEASUREMENT) {
            d_mpc_y.free();
            mpc_y_cap = mpc_y_steps = 0;
        }
        return 0;
    }
    const size_t n = (per_instance ? (size_t)batch : 1) * (size_t)nx * nx;
    noise_G[which].assign(G, G + n);
    if (d_noise_G[which].upload(noise_G[which])) return -1;
    noise_kind[which] = per_instance ? 2 : 1;
    noise_seed[which] = seed;
    return 0;
}

void Solver::drop_noise() {
    if (!noisy()) return;
    (void)wait_last_launch();
    for (int k = 0; k < 2; ++k) {
        noise_kind[k] = 0;
        noise_G[k].clear();
        d_noise_G[k].free();
    }
    d_mpc_y.free();
    mpc_y_cap = mpc_y_steps = 0;
}

// the realised G xi of the steps t0 .. t0 + steps - 1, [batch][steps][nx] fp64, by noise_fill_kernel: the device function of the loop
int Solver::get_noise(int which, int t0, int steps, double *buf) {
    if (which < 0 || which > 1 || !noise_kind[which]) {
        set_error("get_noise: which is 0 (process) or 1 (measurement), and that kind has to be installed (set_process_noise / set_measurement_noise)");
        return -1;
    }
    const size_t per_block = 256 / nx, groups = (batch + per_block - 1) / per_block;
    if (t0 < 0 || steps < 1 || t0 > INT_MAX - steps || !buf || groups * (size_t)steps > 0x7fffffffu) {
        set_error("get_noise: expected t0 >= 0, steps >= 1, t0 + steps within an int, and a buffer of batch * steps * nx doubles");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    DevBuf<double> d_out;
    const size_t n = (size_t)batch * steps * nx;
    if (d_out.alloc(n)) return -1;
    noise_fill_kernel<<<(unsigned)(groups * steps), 256>>>(d_out, d_noise_G[which], noise_kind[which] == 2 ? (long)nx * nx : 0L, noise_seed[which], which, nx,
                                                           (long)batch, steps, t0);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(buf, d_out, n * sizeof(double), hipMemcpyDeviceToHost);
    HIP_TRY(e);
    return 0;
}

// what every step's solve of the last loop started from, [batch][steps][nx] (measurement noise installed)
int Solver::get_mpc_measured(double *y) {
    if (estimating()) {
        set_error("get_mpc_measured: an estimator is installed, the solves start from its estimate: get_mpc_estimate (what every solve started "
                  "from) and get_mpc_outputs (the measured outputs y)");
        return -1;
    }
    if (!noise_kind[NOISE_MEASUREMENT] || mpc_steps_last <= 0 || mpc_y_steps != mpc_steps_last || !y) {
        set_error("get_mpc_measured: no mpc_rollout with measurement noise has run (set_measurement_noise, then mpc_rollout)");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    return d2h_double(d_mpc_y, y, (size_t)batch * mpc_steps_last * nx);
}

// The references of one solve cut out of a reference trajectory (tinympc_set_ref_trajectory): the window at `cursor`,
// xref[b][k][r] = xtraj[b][min(cursor + k, Lx - 1)][r] for the N knots, uref[b][k][a] = utraj[b][min(cursor + k, Lu - 1)][a] for the
// N - 1 (utraj null: zero) — the last row held beyond the end.  A flat index over the output, the x part (nxo floats, the first
// ceil(nxo / REF_WINDOW_SPAN) workgroups) then the u part (nuo floats): a workgroup takes REF_WINDOW_SPAN consecutive floats, a
// lane those blockDim.x apart, so at every one of its REF_WINDOW_PER_LANE steps consecutive lanes write consecutive floats and,
// within a row and from one unclamped row to the next, read consecutive floats.  A lane splits its first index into (instance,
// knot, row) by division once (32-bit where the part is indexed in 32 bits) and then steps it by the workgroup-uniform split of
// blockDim.x — the divisions cost as much issue time as the traffic takes when every float pays them.  Instance b's trajectory
// starts at xtraj + b * x_stride / utraj + b * u_stride; the shared form is one "instance" (nxo = N nx, strides 0) written to
// the shared [N][nx] / [N-1][nu] arrays.  Copies only: a window holds the trajectory's own floats.
constexpr int REF_WINDOW_THREADS = 256, REF_WINDOW_PER_LANE = 4, REF_WINDOW_SPAN = REF_WINDOW_THREADS * REF_WINDOW_PER_LANE;
__global__ void ref_window_kernel(float *xref, float *uref, const float *xtraj, const float *utraj, long x_stride, long u_stride,
                                  int Lx, int Lu, int nx, int nu, int N, long nxo, long nuo, int cursor) {
    const long groups_x = (nxo + REF_WINDOW_SPAN - 1) / REF_WINDOW_SPAN;
    const bool is_x = (long)blockIdx.x < groups_x;
    const long count = is_x ? nxo : nuo, j0 = ((long)blockIdx.x - (is_x ? 0 : groups_x)) * REF_WINDOW_SPAN + threadIdx.x;
    if (j0 >= count) return;
    const int n = is_x ? nx : nu, knots = is_x ? N : N - 1, per = n * knots;   // floats per row; per instance
    const float *traj = is_x ? xtraj : utraj;
    float *out = is_x ? xref : uref;
    const long stride = is_x ? x_stride : u_stride, last = (is_x ? Lx : Lu) - 1;
    long b;
    int rem;
    if (count <= 0x7fffffffL) {
        b = (unsigned)j0 / (unsigned)per;
        rem = (int)((unsigned)j0 - (unsigned)b * (unsigned)per);
    } else {
        b = j0 / per;
        rem = (int)(j0 - b * per);
    }
    int k = rem / n, r = rem - k * n;
    // blockDim.x floats further on: sb instances, sk knots and sr rows, each below its radix, so one carry per digit
    const int sb = REF_WINDOW_THREADS / per, sk = (REF_WINDOW_THREADS - sb * per) / n, sr = REF_WINDOW_THREADS - sb * per - sk * n;
    for (int e = 0; e < REF_WINDOW_PER_LANE; ++e) {
        const long j = j0 + (long)e * REF_WINDOW_THREADS;
        if (j >= count) return;
        const long at = (long)cursor + k, row = at < last ? at : last;
        out[j] = traj ? traj[b * stride + row * n + r] : 0.f;
        r += sr;
        if (r >= n) r -= n, ++k;
        k += sk;
        if (k >= knots) k -= knots, ++b;
        b += sb;
    }
}

// x_traj: Lx rows of nx, u_traj (or null: zero input references): Lu rows of nu, row after row — the columns of an nx x Lx /
// nu x Lu column-major matrix — shared, or instance after instance ([batch][L][n], the layout of get_mpc_log's x / u).  Rounded
// to fp32 here, as set_ref rounds.  x_traj null drops the trajectory and leaves its window at the cursor as the ordinary
// references.  A newly installed trajectory starts at cursor 0 (set_ref_cursor moves it, mpc_rollout advances it).
int Solver::set_ref_trajectory(const double *x_traj, int Lx, const double *u_traj, int Lu, int per_instance) {
    if (!x_traj) return traj_kind ? drop_ref_trajectory(true) : 0;
    if (Lx < 1 || (u_traj && Lu < 1)) {
        set_error("set_ref_trajectory: expected Lx >= 1 rows of x_traj, and Lu >= 1 rows of u_traj where one is given");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;   // (a chain still running reads the trajectory and the reference arrays)
    const size_t n = per_instance ? (size_t)batch : 1, EX = (size_t)ex(), EU = (size_t)eu();
    const size_t nxf = n * (size_t)Lx * nx, nuf = u_traj ? n * (size_t)Lu * nu : 0;
    std::vector<float> hx(nxf), hu(nuf);
    for (size_t i = 0; i < nxf; ++i) hx[i] = (float)x_traj[i];
    for (size_t i = 0; i < nuf; ++i) hu[i] = (float)u_traj[i];
    if (d_xtraj.upload(hx)) return -1;
    if (nuf) {
        if (d_utraj.upload(hu)) return -1;
    } else {
        d_utraj.free();
    }
    // the reference arrays in the trajectory's mode, handed to the window kernel: the device-owned path (tinympc_set_ref_mode)
    if (d_xref.reserve(n * EX) || d_uref.reserve(n * EU)) return -1;
    h_xtraj.swap(hx), h_utraj.swap(hu);
    traj_kind = per_instance ? 2 : 1, traj_Lx = Lx, traj_Lu = u_traj ? Lu : 0;
    ref_cursor = 0, traj_dev_cursor = -1;
    h_xref.clear(), h_uref.clear();
    xref_kind = uref_kind = ref_mode = traj_kind;
    refs_dirty = false;
    refs_device_owned = true;
    ref_seq_steps = 0;   // (a reference sequence goes: the later call wins)
    return 0;
}

// The trajectory goes.  install_window: its window at the cursor stays, as references set by set_x_ref / set_u_ref would be —
// the same floats, shared or per instance, an all-zero side in the zero mode as there — and the solver returns to the routes
// that serve those.  Otherwise (the caller installs references of its own next) zero references.
int Solver::drop_ref_trajectory(bool install_window) {
    if (!traj_kind) return 0;
    if (wait_last_launch()) return -1;
    h_xref.clear(), h_uref.clear();
    xref_kind = uref_kind = 0;
    if (install_window) {
        const size_t n = traj_kind == 2 ? (size_t)batch : 1;
        auto cut = [&](std::vector<float> &h, int &kind, const std::vector<float> &traj, int L, int rows, int knots) {
            if (L < 1) return;
            h.resize(n * knots * rows);
            bool all_zero = true;
            for (size_t b = 0; b < n; ++b)
                for (int k = 0; k < knots; ++k) {
                    const size_t row = (size_t)std::min<long>((long)ref_cursor + k, L - 1);
                    for (int r = 0; r < rows; ++r) {
                        const float v = traj[(b * L + row) * rows + r];
                        h[(b * knots + k) * rows + r] = v;
                        all_zero = all_zero && v == 0.f;
                    }
                }
            if (all_zero)
                h.clear();
            else
                kind = traj_kind;
        };
        cut(h_xref, xref_kind, h_xtraj, traj_Lx, nx, N);
        cut(h_uref, uref_kind, h_utraj, traj_Lu, nu, N - 1);
    }
    traj_kind = traj_Lx = traj_Lu = 0;
    traj_dev_cursor = -1;
    h_xtraj.clear(), h_utraj.clear();
    d_xtraj.free();
    d_utraj.free();
    refs_device_owned = false;
    refs_dirty = true;
    return 0;
}

// the window at `cursor` into d_xref / d_uref, stream-ordered, unless it is the one there
int Solver::ensure_ref_window(hipStream_t stream, int cursor) {
    if (traj_dev_cursor == cursor) return 0;
    const long n = traj_kind == 2 ? (long)batch : 1, nxo = n * ex(), nuo = n * eu();
    const long groups = (nxo + REF_WINDOW_SPAN - 1) / REF_WINDOW_SPAN + (nuo + REF_WINDOW_SPAN - 1) / REF_WINDOW_SPAN;
    ref_window_kernel<<<(unsigned)groups, REF_WINDOW_THREADS, 0, stream>>>(
        d_xref, d_uref, d_xtraj, d_utraj, traj_kind == 2 ? (long)traj_Lx * nx : 0L, traj_kind == 2 ? (long)traj_Lu * nu : 0L, traj_Lx,
        traj_Lu, nx, nu, N, nxo, nuo, cursor);
    HIP_TRY(hipGetLastError());
    traj_dev_cursor = cursor;
    return 0;
}

// The closed loop as ONE launch of the lean or the stream kernel's in-kernel loop (plan_rollout found the kernel): the fp64
// plant state set up as the chain's and handed to the launch, which leaves x0 and x0d as the chain leaves them.  (The stream
// kernel reads its plant coefficients from its own pack: the fp64 A, B, f rows, the doubles ensure_plant uploads for the chain.)
int Solver::rollout_loop(hipStream_t stream, int mpc_steps, Rollout route) {
    if (plant_start(stream, route == Rollout::StreamLoop)) return -1;
    Pass pass = whole_batch(false, true, mpc_steps);
    pass.x0d = d_x0d;
    (route == Rollout::StreamLoop ? pass.stream_loop : pass.loop) = true;
    return launch_pass(stream, pass);
}

int Solver::solve_status() {
    if (!solved_once) {
        set_error("solve_status before any solve");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    HIP_TRY(hipMemcpy(h_gstat, d_gstat, GSTAT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return h_gstat[4] == 0 ? 0 : 1;  // admm.cpp:192 / :206 folded over the batch
}

int Solver::get_mpc_log(double *x, double *u, int *iter) {
    if (mpc_steps_last <= 0) {
        set_error("get_mpc_log: no mpc_rollout has run");
        return -1;
    }
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const size_t n = (size_t)batch * mpc_steps_last;
    std::vector<float> h;
    if (x) {
        h.resize(n * nx);
        HIP_TRY(hipMemcpy(h.data(), d_mpc_x, h.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i) x[i] = (double)h[i];
    }
    if (u) {
        h.resize(n * nu);
        HIP_TRY(hipMemcpy(h.data(), d_mpc_u, h.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i) u[i] = (double)h[i];
    }
    if (iter) HIP_TRY(hipMemcpy(iter, d_mpc_iter, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

double Solver::kernel_elapsed_ms() { return kernel_elapsed_mean_ms(1); }

// mean duration of the last `last_n` launches (at most EV_RING), from the event pairs recorded around each
double Solver::kernel_elapsed_mean_ms(int last_n) {
    if (!profiling || ev_ring.empty() || launches == 0 || last_n <= 0) return -1.0;
    const long n = std::min<long>(std::min<long>(last_n, EV_RING), launches);
    double sum = 0.0;
    for (long i = launches - n; i < launches; ++i) {
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, ev_ring[2 * (i % EV_RING)], ev_ring[2 * (i % EV_RING) + 1]) != hipSuccess) return -1.0;
        sum += ms;
    }
    return sum / (double)n;
}

int Solver::get_traj(bool states, double *buf) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    return d2h_double(states ? d_xout : d_uout, buf, (size_t)batch * (states ? ex() : eu()));
}

int Solver::get_status(int *iter, int *solved, double *res4) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const size_t Bn = (size_t)batch;
    if (iter) HIP_TRY(hipMemcpy(iter, d_iter, Bn * sizeof(int), hipMemcpyDeviceToHost));
    if (solved) HIP_TRY(hipMemcpy(solved, d_solved, Bn * sizeof(int), hipMemcpyDeviceToHost));
    if (res4) {
        std::vector<float> h(Bn * 4);
        HIP_TRY(hipMemcpy(h.data(), d_res, Bn * 4 * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < Bn * 4; ++i) res4[i] = (double)h[i];
    }
    return 0;
}

// fp32 device buffer -> fp64 caller buffer.  Chunks travel into pinned staging on a copy stream while the previous
// chunk is widened by the host threads, so the round trip costs about max(PCIe, widening) instead of their sum plus
// a pageable-memory bounce.
int Solver::d2h_double(const float *d, double *out, size_t n) {
    if (!out || n == 0) return 0;
    constexpr size_t CHUNK = (size_t)1 << 21;  // floats per slot (8 MB)
    if (!s_copy) {
        HIP_TRY(hipStreamCreate(&s_copy));  // callers have already waited for the last launch (wait_last_launch)
        for (hipEvent_t &e : ev_copy) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (h_stage.reserve(2 * CHUNK)) return -1;
    const size_t nchunks = (n + CHUNK - 1) / CHUNK;
    for (size_t c = 0; c <= nchunks; ++c) {
        if (c < nchunks) {
            const size_t off = c * CHUNK, len = std::min(CHUNK, n - off);
            HIP_TRY(hipMemcpyAsync(h_stage + (c & 1) * CHUNK, d + off, len * sizeof(float), hipMemcpyDeviceToHost, s_copy));
            HIP_TRY(hipEventRecord(ev_copy[c & 1], s_copy));
        }
        if (c > 0) {
            const size_t pc = c - 1, off = pc * CHUNK, len = std::min(CHUNK, n - off);
            HIP_TRY(hipEventSynchronize(ev_copy[pc & 1]));
            widen(h_stage + (pc & 1) * CHUNK, out + off, len);
        }
    }
    return 0;
}
// Page-lock a caller-owned host range so that the fp32 transfers DMA straight into it.  Only on request
// (tinympc_pin_host): the library does not own these buffers and cannot know when they are freed, so it never registers
// them on its own — the caller unpins (tinympc_unpin_host) before releasing the memory; whatever is still registered
// when the solver is destroyed is unregistered there.
int Solver::pin_host_range(void *p, size_t bytes) {
    if (!p || bytes == 0) {
        set_error("pin_host: null or empty range");
        return -1;
    }
    for (const auto &r : pinned_ranges)
        if (r.first == p) {
            if (r.second >= bytes) return 0;
            set_error("pin_host: this address is already pinned with a smaller size; unpin it first");
            return -1;
        }
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    pinned_ranges.emplace_back(p, bytes);
    return 0;
}
int Solver::unpin_host_range(void *p) {
    for (size_t i = 0; i < pinned_ranges.size(); ++i)
        if (pinned_ranges[i].first == p) {
            HIP_TRY(hipSetDevice(device));
            if (wait_last_launch()) return -1;
            pinned_ranges.erase(pinned_ranges.begin() + i);
            HIP_TRY(hipHostUnregister(p));
            return 0;
        }
    set_error("unpin_host: this address was not pinned through this solver");
    return -1;
}

int Solver::h2d_float(float *d, const double *in, size_t n) {
    if (!in) return 0;
    std::vector<float> h(n);
    narrow(in, h.data(), n);
    HIP_TRY(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int Solver::get_workspace(double *d, double *y, double *g, double *v, double *z) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const size_t Bn = (size_t)batch, EX = (size_t)ex(), EU = (size_t)eu();
    if (precision == 2 && d_ws64) {   // the fp64 block itself: no widening
        const Ws64 w(d_ws64, (long)Bn, (long)EX, (long)EU);
        auto get = [&](double *dst, const double *src, size_t n) { return !dst || hipMemcpy(dst, src, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess; };
        if (!(get(d, w.sd, Bn * EU) && get(y, w.sy, Bn * EU) && get(z, w.sz, Bn * EU) && get(g, w.sg, Bn * EX) && get(v, w.sv, Bn * EX))) {
            set_error("get_workspace: copy failed");
            return -1;
        }
        return 0;
    }
    if (d2h_double(d_sd, d, Bn * EU) || d2h_double(d_sy, y, Bn * EU) || d2h_double(d_sz, z, Bn * EU) ||
        d2h_double(d_sg, g, Bn * EX) || d2h_double(d_sv, v, Bn * EX))
        return -1;
    return 0;
}

int Solver::set_workspace(const double *d, const double *y, const double *g, const double *v,
                          const double *z) {
    HIP_TRY(hipSetDevice(device));
    if (wait_last_launch()) return -1;
    const size_t Bn = (size_t)batch, EX = (size_t)ex(), EU = (size_t)eu();
    if (precision == 2) {
        if (select_kernel() || ensure_extension_buffers()) return -1;
        const Ws64 w(d_ws64, (long)Bn, (long)EX, (long)EU);
        auto put = [&](double *dst, const double *src, size_t n) { return !src || hipMemcpy(dst, src, n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess; };
        if (!(put(w.sd, d, Bn * EU) && put(w.sy, y, Bn * EU) && put(w.sz, z, Bn * EU) && put(w.sg, g, Bn * EX) && put(w.sv, v, Bn * EX))) {
            set_error("set_workspace: copy failed");
            return -1;
        }
        return 0;
    }
    if (h2d_float(d_sd, d, Bn * EU) || h2d_float(d_sy, y, Bn * EU) || h2d_float(d_sz, z, Bn * EU) ||
        h2d_float(d_sg, g, Bn * EX) || h2d_float(d_sv, v, Bn * EX))
        return -1;
    g_maybe_nonzero = true;
    return 0;
}

}  // namespace tmpc

// (test hook, not part of the public boundary include/tinympc_hip.h: the lean sweeps of a solver's most recent launch) the
// model's (A, B) pattern; the per-knot fp64 costs weighed — the sparse form's (0: no sparse kernel was on offer) and that of
// the dense form it replaces; the form taken (LF_*: 0 no lean launch, 1 plain dense, 2 Hessenberg, 3 sparse)
extern "C" int tmpc_lean_last_form(tinympc_solver *s, unsigned long long *pattern, int *cost_sparse, int *cost_dense, int *form) {
    if (!s) return 1;
    if (pattern) *pattern = s->s.lean_sp;
    if (cost_sparse) *cost_sparse = s->s.last_lean_cost[0];
    if (cost_dense) *cost_dense = s->s.last_lean_cost[1];
    if (form) *form = s->s.last_lean_form;
    return 0;
}

// (test hook like the one above) whether the solver's most recent launch ran a scaled sparse kernel of the lean family
// (admm_params.h: lean_pattern_scaled): 1 / 0, -1 without a solver
extern "C" int tmpc_lean_last_scaled(tinympc_solver *s) { return s ? (s->s.last_lean_scaled ? 1 : 0) : -1; }

// (test hook like the one above) the number of solve-kernel launches the solver's last mpc_rollout took: `steps` for the
// chains of launches, 1 for any in-kernel loop, -1 before any rollout
extern "C" int tmpc_last_rollout_launches(tinympc_solver *s) { return s ? s->s.last_rollout_launches : -1; }

// (test hook like the one above) the bytes of device memory the library holds in this process: every allocation goes through
// devbuf.h's two functions above
extern "C" long long tmpc_device_bytes_live(void) { return tmpc::g_device_bytes.load(); }
