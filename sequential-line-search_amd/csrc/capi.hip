// C-ABI of libsls_hip (include/sls_hip.h): host orchestration of the gfx950 kernels.  No CPU fallback.
#include <cstddef>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>

#include "common.hpp"
#include "kernels.hpp"
#include "lbfgs_driver.hpp"
#include "sub_maps.hpp"

using namespace slsk;


namespace slsk {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace slsk

// ---- device block cache (common.hpp) -------------------------------------------------------------------------
namespace slsk {
namespace {
struct Pool {
    std::mutex mtx;
    std::multimap<size_t, void*> free_blocks;
    size_t cached = 0;
    long synced_epoch = -1;
};
// bumped by every C-ABI entry point: "device work may have been queued since the last device-wide synchronisation"
std::atomic<long> g_work_epoch{0};
Pool& pool_of(int dev) {
    static std::mutex m;
    static std::map<int, std::unique_ptr<Pool>> pools;
    std::lock_guard<std::mutex> lock(m);
    auto& p = pools[dev];
    if (!p) p.reset(new Pool());
    return *p;
}
size_t pool_limit() {
    return (size_t)tune(TUNE_POOL_MB, 16384) << 20;
}
}  // namespace

void note_entry() { g_work_epoch.fetch_add(1); }


void* pool_alloc(size_t bytes) {
    if (bytes == 0) bytes = 8;
    int dev = 0;
    (void)hipGetDevice(&dev);
    Pool& P = pool_of(dev);
    {
        std::lock_guard<std::mutex> lock(P.mtx);
        auto it = P.free_blocks.find(bytes);
        if (it != P.free_blocks.end()) {
            void* p = it->second;
            P.free_blocks.erase(it);
            P.cached -= bytes;
            return p;
        }
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {          // out of memory: give the cache back and try once more
        pool_trim(dev);
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        throw HipFail{SLS_ERR_HIP};
    }
    return p;
}

void pool_free(void* p, size_t bytes, bool in_flight) {
    if (!p) return;
    if (bytes == 0) bytes = 8;
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) dev = attr.device;   // freed from another thread / current device
    Pool& P = pool_of(dev);
    {
        std::lock_guard<std::mutex> lock(P.mtx);
        if (P.cached + bytes <= pool_limit()) {
            // A cached block may be handed out again at once (to any stream): everything queued on it must have finished.
            // hipFree would have synchronised implicitly; here ONE device-wide synchronisation covers all the blocks
            // released after the same entry point (a handle's ~30 buffers cost one ~5 us call, normally on an idle device
            // because handles and temporaries are released after their stream has been synchronised).
            const long epoch = g_work_epoch.load();
            // (in_flight: the block is released by the entry point that queued work on it -- a buffer regrown between two
            // launches -- so the epoch's earlier synchronisation does not cover it: synchronise again before it can be reused
            // by another context's stream)
            if (P.synced_epoch != epoch || in_flight) {
                int cur = 0;
                (void)hipGetDevice(&cur);
                if (cur != dev) (void)hipSetDevice(dev);
                (void)hipDeviceSynchronize();
                if (cur != dev) (void)hipSetDevice(cur);
                P.synced_epoch = epoch;
            }
            P.free_blocks.emplace(bytes, p);
            P.cached += bytes;
            return;
        }
    }
    (void)hipFree(p);
}

void pool_trim(int device) {
    Pool& P = pool_of(device);
    std::vector<void*> blocks;
    {
        std::lock_guard<std::mutex> lock(P.mtx);
        for (auto& kv : P.free_blocks) blocks.push_back(kv.second);
        P.free_blocks.clear();
        P.cached = 0;
    }
    for (void* b : blocks) (void)hipFree(b);
}
}  // namespace slsk

// ---- context --------------------------------------------------------------------------------------------
hipEvent_t sls_ctx::get_event() {
    if (!event_pool.empty()) {
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    SLS_HIP(hipEventCreate(&e));
    return e;
}
void sls_ctx::prof_begin(const char*, hipEvent_t& e0) {
    e0 = get_event();
    SLS_HIP(hipEventRecord(e0, stream));
}
void sls_ctx::prof_end(const char* name, hipEvent_t e0) {
    hipEvent_t e1 = get_event();
    (void)hipEventRecord(e1, stream);
    ProfEntry& pe = prof[name];
    pe.pending.emplace_back(e0, e1);
    pe.launches += 1;
}
void sls_ctx::prof_collect() {
    for (auto& kv : prof) {
        for (auto& pr : kv.second.pending) {
            (void)hipEventSynchronize(pr.second);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, pr.first, pr.second);
            kv.second.ms += ms;
            event_pool.push_back(pr.first);
            event_pool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}

void sls_ctx::potrf_tick_rearm() {
    if (!potrf_persistent_ok && potrf_rearm > 0 && --potrf_rearm == 0) potrf_persistent_ok = true;
}

bool sls_ctx::potrf_df_available(int Np) const { return potrf_persistent_ok && slsk::potrf_default_mode(Np) == 3; }
int* sls_ctx::potrf_df_sync(int Np) {
    if (!potrf_df_available(Np)) return nullptr;
    potrf_df.ensure((slsk::potrf_dataflow_sync_ints(Np) + 1) / 2);
    potrf_single_pending = Np >= 384;   // smaller matrices never take the single-launch form (launch_potrf)
    return reinterpret_cast<int*>(potrf_df.p);
}

namespace slsk {
bool potrf_gave_up(sls_ctx* c, int abort_flag, int attempt) {
    if (abort_flag == 0) {
        // a single-launch factorisation ran to the end: the back-off of earlier give-ups starts over (a context that saw a few
        // transient residency failures would otherwise sit on a 4096-fit back-off for the rest of its life)
        if (c->potrf_single_pending && c->potrf_persistent_ok) c->potrf_rearm_next = 16;
        c->potrf_single_pending = false;
        return false;
    }
    c->potrf_single_pending = false;
    if (attempt > 0 || !c->potrf_persistent_ok) {
        set_error("Cholesky factorisation aborted: a device-side wait expired");
        throw HipFail{SLS_ERR_HIP};
    }
    // The single-launch form needs every workgroup resident at once; another kernel on the device (another process, a
    // profiler, RCCL) can prevent that.  This context uses the multi-launch schedule for the next fits and then tries again,
    // backing off (16, 64, 256, ... 4096 fits) while the device stays shared; the count is visible through
    // sls_prof_get("potrf_fallbacks") and in bench.py's line.  The two schedules agree to rounding, not bit for bit.
    c->potrf_persistent_ok = false;
    c->potrf_rearm = c->potrf_rearm_next;
    c->potrf_rearm_next = std::min(4096, c->potrf_rearm_next * 4);
    c->potrf_fallbacks += 1;
    return true;
}
}  // namespace slsk

extern "C" const char* sls_last_error(void) { return slsk::g_err; }
extern "C" int sls_version(void) { return 101; }

extern "C" int sls_ctx_create(int device, sls_ctx** out) {
    SLS_TRY
    SLS_REQUIRE(out != nullptr, "sls_ctx_create: out is NULL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        set_error("sls_ctx_create: no HIP device available (%s); this library has no CPU fallback",
                  e == hipSuccess ? "0 devices" : hipGetErrorString(e));
        return SLS_ERR_NO_DEVICE;
    }
    SLS_REQUIRE(device >= 0 && device < ndev, "sls_ctx_create: device %d out of range (%d devices)", device, ndev);
    SLS_HIP(hipSetDevice(device));
    std::unique_ptr<sls_ctx> c(new sls_ctx());
    c->device = device;
    SLS_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    SLS_HIP(hipMalloc((void**)&c->d_info, 4096));   // ints 0..15: potrf info ([0] pivot, [1] abort); 32..47: acq_gemm generation gates; 64..1023: sync words of the persistent potrf
    *out = c.release();
    SLS_CATCH
}

void* sls_ctx::host_take(size_t bytes, bool mapped, size_t* got) {
    int best = -1;
    for (int i = 0; i < (int)host_free.size(); ++i)
        if (host_free[i].mapped == mapped && host_free[i].bytes >= bytes && (best < 0 || host_free[i].bytes < host_free[best].bytes)) best = i;
    if (best >= 0) {
        HostBlock b = host_free[best];
        host_free.erase(host_free.begin() + best);
        *got = b.bytes;
        return b.p;
    }
    void* p = nullptr;
    const size_t sz = std::max<size_t>(bytes, 4096);
    if (hipHostMalloc(&p, sz, mapped ? hipHostMallocMapped : hipHostMallocDefault) != hipSuccess) {
        slsk::set_error("hipHostMalloc(%zu) failed", sz);
        throw slsk::HipFail{SLS_ERR_HIP};
    }
    *got = sz;
    return p;
}
void sls_ctx::host_give(void* p, size_t bytes, bool mapped) {
    if (!p) return;
    if (host_free.size() >= 16) {
        (void)hipHostFree(p);
        return;
    }
    host_free.push_back(HostBlock{p, bytes, mapped});
}

static void ctx_destroy_now(sls_ctx* ctx);
namespace slsk {
void ctx_retain(sls_ctx* c) { ++c->live_handles; }
void ctx_release(sls_ctx* c) {
    bool last;
    {
        std::unique_lock<std::recursive_mutex> lock(c->mtx);
        last = --c->live_handles == 0 && c->destroy_requested;
    }
    if (last) ctx_destroy_now(c);
}
}  // namespace slsk

extern "C" int sls_ctx_destroy(sls_ctx* ctx) {
    if (!ctx) return SLS_OK;
    {
        std::unique_lock<std::recursive_mutex> lock(ctx->mtx);
        if (ctx->live_handles > 0) {       // handles outlive the context: the last one frees it (slsk::ctx_release)
            ctx->destroy_requested = true;
            return SLS_OK;
        }
    }
    ctx_destroy_now(ctx);
    return SLS_OK;
}
static void ctx_destroy_now(sls_ctx* ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->slots) {   // the evaluation slots: their streams, their mapped blocks back to the pool that is freed next
        if (s->stream) {
            (void)hipStreamSynchronize(s->stream);
            (void)hipStreamDestroy(s->stream);
        }
    }
    ctx->slots.clear();
    for (auto& b : ctx->host_free) (void)hipHostFree(b.p);
    ctx->host_free.clear();
    ctx->prof_collect();
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->d_info) (void)hipFree(ctx->d_info);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" int sls_tuning_reload(void) {
    slsk::tuning_reload();
    return SLS_OK;
}

extern "C" int sls_device_trim_cache(int device) {
    slsk::note_entry();
    (void)hipDeviceSynchronize();
    slsk::pool_trim(device);
    return SLS_OK;
}

extern "C" int sls_ctx_set_stream(sls_ctx* ctx, void* hip_stream) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx, "ctx is NULL");
    SLS_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    SLS_CATCH
}
extern "C" int sls_ctx_synchronize(sls_ctx* ctx) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx, "ctx is NULL");
    SLS_HIP(hipStreamSynchronize(ctx->stream));
    SLS_CATCH
}
extern "C" int sls_ctx_set_candidate_chunk(sls_ctx* ctx, int chunk) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx && chunk >= 128, "candidate chunk must be >= 128");
    ctx->cand_chunk = round_up(chunk, 128);
    SLS_CATCH
}
extern "C" int sls_prof_enable(sls_ctx* ctx, int on) {
    if (!ctx) return SLS_ERR_INVALID;
    CtxCall call_(ctx);
    ctx->prof_on = on != 0;
    return SLS_OK;
}
extern "C" int sls_prof_reset(sls_ctx* ctx) {
    if (!ctx) return SLS_ERR_INVALID;
    CtxCall call_(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->prof_collect();
    ctx->prof.clear();
    return SLS_OK;
}
extern "C" int sls_prof_get(sls_ctx* ctx, const char* name, double* total_ms, long* launches) {
    if (!ctx || !name) return SLS_ERR_INVALID;
    CtxCall call_(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->prof_collect();
    if (std::string(name) == "potrf_fallbacks") {          // not a timing: how often a single-launch Cholesky gave up
        if (total_ms) *total_ms = 0.0;
        if (launches) *launches = ctx->potrf_fallbacks;
        return SLS_OK;
    }
    auto it = ctx->prof.find(name);
    if (total_ms) *total_ms = it == ctx->prof.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == ctx->prof.end() ? 0 : it->second.launches;
    return SLS_OK;
}

// ---- helpers --------------------------------------------------------------------------------------------
static void sync(sls_ctx* c) { SLS_HIP(hipStreamSynchronize(c->stream)); }
// Up to this many doubles of query points / results / matrices go through a handle's page-locked staging block (32 MB); larger
// transfers take the plain (pageable, blocking) copies.
static const size_t IO_STAGE_MAX = (size_t)4 << 20;

static void check_theta(const double* theta, int D) {
    SLS_REQUIRE(theta != nullptr, "theta is NULL");
    SLS_REQUIRE(theta[0] > 0.0, "theta[0] (signal variance) must be positive");
    for (int d = 0; d < D; ++d) SLS_REQUIRE(theta[1 + d] > 0.0, "length scale %d must be positive", d);
}

// copies a padded (ld = Np) device matrix region [N x N] into a dense host N x N
static void d2h_matrix(sls_ctx* c, double* dst, const double* src, int N, int Np) {
    SLS_HIP(hipMemcpy2DAsync(dst, (size_t)N * 8, src, (size_t)Np * 8, (size_t)N * 8, N, hipMemcpyDeviceToHost, c->stream));
}
static void h2d_matrix(sls_ctx* c, double* dst, const double* src, int N, int Np) {
    SLS_HIP(hipMemcpy2DAsync(dst, (size_t)Np * 8, src, (size_t)N * 8, (size_t)N * 8, N, hipMemcpyHostToDevice, c->stream));
}

// ---- GP handle --------------------------------------------------------------------------------------------
struct sls_gp {
    sls_ctx* ctx = nullptr;
    int D = 0, N = 0, Np = 0, Dp = 0, Dcols = 0, kernel = 0;
    double a = 0, b = 0;
    std::vector<double> theta, Xh, yh;
    std::vector<double> il_h, ypad_h;   // upload staging that lives with the handle: no synchronisation between the uploads and the fit
    bool host_stale = false;   // sls_gp_refit_dev replaced the device X / y: Xh / yh are refreshed before their next use
    DBuf X, y, inv_ell, XT, XaT, nx, L, Linv, Kinv, U, alpha, tvec, mu_data, scal, gemv_part, idx_buf;   // U = (L^-1)^T, needed by the fit only
    const double* linv_clean_p = nullptr;   // the Linv buffer / leading dimension whose blocks above the diagonal are known to be zero
    int linv_clean_np = 0;
    long* d_idx = nullptr;             // idx_buf's block (pooled: a hipMalloc / hipFree pair per handle synchronised the device)
    // what the host reads after a fit -- max mu, log|K_y|, arg max, the factorisation's two info words -- in a page-locked block the
    // last kernel of the fit writes directly (mapped): one synchronisation, no copies back (they were three blocking pageable copies)
    HostBuf sum;
    int best_index = 0;
    double mu_best = 0, logdet = 0;
    // evaluation workspace (grown on demand)
    DBuf Ks, Cs, P, Vs, parts, Gs, Gm, Gpart, XsT, ns, raw, outv;
    int ws_chunk = 0;
    // L-BFGS state
    DBuf pair_mu, pair_sg, pair_dmu, pair_dsg;
    LbfgsWs lb;   // pooled blocks that live with the handle: a repeated maximisation costs no allocation
    // the second option's evaluation workspace of the pair objective (sls_eubo_*; the first option uses the blocks above) and the
    // difference Kd of the two cross-covariance blocks; grown on demand, sized for eubo_np / eubo_chunk
    DBuf eubo_Ks, eubo_Cs, eubo_XsT, eubo_ns, eubo_parts, eubo_Gs, eubo_Gm, eubo_Kd;
    int eubo_chunk = 0, eubo_np = 0;
    HostBuf eubo_best;   // mapped: the pair maximiser's best start (8 + 2D doubles; `sum` holds 8 + D)
    // the *_sub entry points: the expanded points x = c + A z and their gradient, D x round_up(columns, 128) doubles each, grown on demand
    DBuf sub_x, sub_gx;
    // 0: sigma^2 = a - k^T K^-1 k with the explicit inverse (GaussianProcessRegressor); 1: a - |L^-1 k|^2, the Cholesky solve of
    // PreferenceRegressor (sls_gp_set_sigma_mode)
    int sigma_mode = 0;
    // changes whenever the predictor this handle stands for changes (fit, refit, appended point, sigma mode); process-wide unique, so
    // a new handle at a recycled address never repeats a number (sls_gp_generation: the host layer keys its replicas on it)
    long generation = 0;
    // this fit is beyond the guard of the norm expansion (gram_direct_form, kernels.hpp): every Gram route of the handle forms q from
    // the raw coordinate differences (set by gp_fit_device from the length scales)
    bool gram_direct = false;
    // statistics of the last sls_acq_maximize* call on this handle (sls_acq_last_stats)
    long stat_issued = 0, stat_cap = 0;
    int stat_rounds = 0, stat_live_end = 0;
    // page-locked, device-mapped block for small value-only evaluations (query points in, values out: no copy calls)
    HostBuf zc;
    // page-locked staging of host-supplied query points and their results (predict / acquisition entry points on the tiled path):
    // uploads and downloads are truly asynchronous, one synchronisation per call (pageable buffers: blocking staged copies, a
    // synchronisation behind each, and a fresh 0.5 MB temporary per transfer)
    HostBuf io;
    double* io_stage(size_t doubles) {
        if (io.host && doubles * 8 > io.bytes) (void)hipStreamSynchronize(ctx->stream);   // an upload from the old block may still be in flight (growth is rare)
        io.ensure(ctx, doubles * 8, false);
        return io.host;
    }
    // Concurrent const evaluations (src/acquisition-function.cpp:125-144: Predict* of ONE regressor from hardware_concurrency worker
    // threads).  A small evaluation (a few query points on a wave-path handle) does not take the context's lock: it borrows a SLOT of
    // the handle -- a stream of its own and a page-locked, device-mapped block for the query points and the results -- under a
    // SHARED lock on the fitted state; everything that changes the state (refit, appended point, sigma mode) holds it exclusively.
    // The slots belong to the CONTEXT (sls_ctx::slots): a stream costs ~1 ms to create and the facade builds a new handle per submit.
    std::shared_mutex state_mtx;
    // Laplace posterior of the goodness values (sls_gp_set_laplace): while set, every sigma route of the handle reads M in the place
    // of K_y^-1 on the tiled evaluation, and the fit is frozen.  laplace_on mirrors `lap != nullptr` for readers that have not taken
    // a lock yet (the slot path asks before it takes the state lock, and again under it).
    struct LaplaceState {
        double btl_scale = 0.0;
        DBuf W, M, T, LBinv, Binv;   // Np x Np each: the BTL Hessian, the effective inverse, T = I - B^-1, chol(B)^-1 (path draws), B^-1 (Sigma_g)
        double log_lik = 0.0, logdet_B = 0.0, quad = 0.0;   // sum_t log p_t0, log|B|, y . alpha
    };
    std::unique_ptr<LaplaceState> lap;
    std::atomic<bool> laplace_on{false};
};

// An entry point that neither honours the Laplace state nor may silently use the plain variance refuses the handle.
static void refuse_laplace(const sls_gp* g, const char* who) {
    if (g && g->lap) {
        set_error("%s: the handle carries a Laplace posterior (sls_gp_set_laplace); this entry point does not support it -- "
                  "sls_gp_clear_laplace first", who);
        throw HipFail{SLS_ERR_UNSUPPORTED};
    }
}

// N <= 128: the whole fit is one single-workgroup launch (kernels_small.hip); SLS_FIT_SMALL=0 forces the tiled pipeline (A/B, tests)
static bool gp_fit_small_ok(const sls_gp* g) {
    if (g->N > NLL_SMALL_MAX_N || g->Np != 128 || g->D > 128) return false;
    return tune_on(TUNE_FIT_SMALL);
}

static std::atomic<long> g_gp_generation{0};
static void gp_fit_device(sls_gp* g) {
    g->generation = ++g_gp_generation;
    sls_ctx* c = g->ctx;
    const int N = g->N, Np = g->Np, D = g->D;
    g->gram_direct = gram_direct_form(g->theta.data() + 1, D);
    if (gp_fit_small_ok(g)) {
        GpFitSmallArgs f;
        f.X = g->X.p; f.y = g->y.p; f.inv_ell = g->inv_ell.p;
        f.D = D; f.N = N; f.Dcols = g->Dcols; f.a = g->a; f.b = g->b;
        f.XT = g->XT.p; f.nx = g->nx.p; f.XaT = g->XaT.p; f.L = g->L.p; f.Linv = g->Linv.p; f.U = g->U.p; f.Kinv = g->Kinv.p;
        f.alpha = g->alpha.p; f.mu_data = g->mu_data.p; f.scal = g->scal.p; f.d_idx = g->d_idx; f.info = c->d_info;
        f.summary = g->sum.dev;
        f.x_lds = tune_on(TUNE_SMALL_XLDS) ? 1 : 0;
        SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
        ProfScope ps(c, "fit_small");
        launch_gp_fit_small(c->stream, g->kernel, f);
        return;
    }
    KernelSpec ks{g->kernel, g->a};
    {
        ProfScope ps(c, "gram");
        launch_prep_points(c->stream, g->X.p, D, N, g->inv_ell.p, g->XT.p, Np, Np, g->Dcols, g->nx.p);
        if (g->gram_direct) launch_gram_sym_direct(c->stream, g->X.p, D, g->inv_ell.p, Np, N, ks, g->b, g->L.p, true);
        else launch_gram_sym(c->stream, g->XT.p, Np, g->Dp, g->nx.p, Np, N, ks, g->b, g->L.p, true);
    }
    SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
    // L^-1 is read as a full matrix (gemv, the plain-product predict): its blocks above the diagonal must be zero.  Nothing ever
    // writes them -- the factorisation, the inverse and the rank-1 growth touch blocks on and below the diagonal only -- so they are
    // cleared when the buffer is new or its leading dimension changed, not on every refit (a 512 MB sweep, 91 us, at N = 8192).
    if (g->linv_clean_p != g->Linv.p || g->linv_clean_np != Np) {
        launch_fill(c->stream, g->Linv.p, (long)Np * Np, 0.0);
        g->linv_clean_p = g->Linv.p;
        g->linv_clean_np = Np;
    }
    c->potrf_tick_rearm();
    int* df_sync = c->potrf_df_sync(Np);
    if (potri_fused_applies(Np, df_sync != nullptr)) {
        // N <= 4096: factorisation, L^-1, its transpose and K_y^-1 in ONE launch (the inverse is built behind the chain by the CUs the
        // factorisation leaves idle)
        ProfScope ps(c, "potri");
        if (!launch_potri(c->stream, g->L.p, Np, g->Linv.p, g->U.p, g->Kinv.p, c->d_info, df_sync))
            ps.rename("potrf+trtri+lauum");   // the fused launch declined (too few CUs resident): the three separate launches ran
    } else {
        {
            ProfScope ps(c, "potrf");
            launch_potrf(c->stream, g->L.p, Np, g->Linv.p, c->d_info, 0, df_sync);
        }
        {
            ProfScope ps(c, "trtri");
            launch_trtri(c->stream, g->L.p, Np, g->Linv.p, g->Kinv.p, g->U.p);
        }
        {
            ProfScope ps(c, "lauum");
            launch_lauum(c->stream, g->U.p, Np, g->Kinv.p);
        }
    }
    // alpha = Linv^T (Linv y);  mu at the data points = y - b alpha;  x_best = first argmax  (regressor.cpp:29-43 hoisted)
    launch_gemv_n(c->stream, g->Linv.p, Np, g->y.p, g->tvec.p, g->gemv_part.p, true);
    launch_gemv_t(c->stream, g->Linv.p, Np, g->tvec.p, g->alpha.p, true);
    launch_scale_rows(c->stream, g->XT.p, g->alpha.p, g->XaT.p, Np, Np, g->Dcols);
    if (g->sigma_mode == 1) launch_transpose_full(c->stream, g->Linv.p, g->U.p, Np);   // every block of U = (L^-1)^T
    // mu at the data points, its first maximum, log|K_y| and the info words: one launch, results straight into the mapped block
    launch_fit_summary(c->stream, g->y.p, g->alpha.p, g->b, N, g->mu_data.p, g->L.p, Np, c->d_info, g->scal.p, g->d_idx, g->sum.dev);
}

static void gp_fetch_summary(sls_gp* g, int attempt = 0) {
    sls_ctx* c = g->ctx;
    sync(c);                         // the fit's last kernel has written the mapped block
    const double* sm = g->sum.host;
    const int info[2] = {(int)sm[3], (int)sm[4]};
    if (potrf_gave_up(c, info[1], attempt)) {
        gp_fit_device(g);            // once more, on the multi-launch schedule (the fit rebuilds K_y from X)
        gp_fetch_summary(g, 1);
        return;
    }
    if (info[0] != 0) {
        set_error("Cholesky failed: K_y is not positive definite (pivot %d)", info[0] - 1);
        throw HipFail{SLS_ERR_NOT_SPD};
    }
    g->best_index = (int)sm[2];
    g->mu_best = sm[0];
    g->logdet = sm[1];
}
// (re)size every per-handle buffer for the host copies g->Xh / g->yh, upload and fit
static void gp_setup(sls_gp* g) {
    sls_ctx* ctx = g->ctx;
    const int D = g->D, N = (int)g->yh.size();
    g->N = N;
    g->Np = round_up(N, 128); g->Dp = round_up(D, 16); g->Dcols = round_up(D, 128);
    const size_t Np = g->Np;
    g->X.ensure((size_t)D * N); g->y.ensure(Np); g->inv_ell.ensure(g->Dcols);
    g->XT.ensure(Np * g->Dcols); g->XaT.ensure(Np * g->Dcols); g->nx.ensure(Np);
    g->L.ensure(Np * Np); g->Linv.ensure(Np * Np); g->Kinv.ensure(Np * Np); g->U.ensure(Np * Np);
    g->alpha.ensure(Np); g->tvec.ensure(Np); g->mu_data.ensure(Np); g->scal.ensure(8);
    g->gemv_part.ensure((Np / 128) * Np);
    g->ws_chunk = 0;   // the evaluation workspace depends on Np
    g->idx_buf.ensure(8);
    g->d_idx = reinterpret_cast<long*>(g->idx_buf.p);
    g->sum.ensure(ctx, (size_t)(16 + D) * 8, true);   // [0..5) the fit's summary, [8..16 + D) the maximiser's best start
    g->il_h.assign(g->Dcols, 0.0);
    g->ypad_h.assign(Np, 0.0);
    for (int d = 0; d < D; ++d) g->il_h[d] = 1.0 / g->theta[1 + d];
    std::copy(g->yh.begin(), g->yh.end(), g->ypad_h.begin());
    h2d(ctx, g->X.p, g->Xh.data(), (size_t)D * N);
    h2d(ctx, g->y.p, g->ypad_h.data(), Np);
    h2d(ctx, g->inv_ell.p, g->il_h.data(), g->Dcols);
    gp_fit_device(g);            // enqueued behind the uploads; the staging vectors are members
    gp_fetch_summary(g);         // the one synchronisation of the fit
}

extern "C" int sls_gp_create(sls_ctx* ctx, const double* X, int D, int N, const double* y, const double* theta, double b,
                             int kernel, sls_gp** out) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx && out, "sls_gp_create: NULL argument");
    SLS_REQUIRE(D >= 1 && N >= 1, "sls_gp_create: need D >= 1 and N >= 1 (got D=%d N=%d)", D, N);
    SLS_REQUIRE(X && y, "sls_gp_create: X / y is NULL");
    SLS_REQUIRE(kernel == SLS_KERNEL_ARD_SQUARED_EXPONENTIAL || kernel == SLS_KERNEL_ARD_MATERN52, "unknown kernel %d", kernel);
    SLS_REQUIRE(b >= 0.0, "noise level must be >= 0");
    check_theta(theta, D);
    SLS_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<sls_gp> g(new sls_gp());
    g->ctx = ctx; g->D = D; g->kernel = kernel; g->a = theta[0]; g->b = b;
    g->theta.assign(theta, theta + D + 1);
    g->Xh.assign(X, X + (size_t)D * N);
    g->yh.assign(y, y + N);
    gp_setup(g.get());
    slsk::ctx_retain(ctx);
    *out = g.release();
    SLS_CATCH
}

extern "C" int sls_gp_refit_dev(sls_gp* g, const double* X_dev, const double* y_dev) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && X_dev && y_dev, "sls_gp_refit_dev: NULL argument");
    refuse_laplace(g, "sls_gp_refit_dev");
    std::unique_lock<std::shared_mutex> state_(g->state_mtx);
    sls_ctx* c = g->ctx;
    SLS_HIP(hipMemcpyAsync(g->X.p, X_dev, (size_t)g->D * g->N * 8, hipMemcpyDeviceToDevice, c->stream));
    SLS_HIP(hipMemcpyAsync(g->y.p, y_dev, (size_t)g->N * 8, hipMemcpyDeviceToDevice, c->stream));
    g->host_stale = true;
    gp_fit_device(g);
    gp_fetch_summary(g);
    SLS_CATCH
}

extern "C" int sls_gp_destroy(sls_gp* gp) {
    if (!gp) return SLS_OK;
    slsk::note_entry();
    // evaluations that run on the context's slots without its lock (eval_in_slot) hold the state lock shared until their slot's
    // stream has drained: taking it exclusively waits for them
    destroy_handle(gp, &gp->state_mtx);
    return SLS_OK;
}

namespace slsk {
GpView gp_view(sls_gp* g) {
    GpView v;
    v.ctx = g->ctx;
    v.D = g->D; v.N = g->N; v.Np = g->Np; v.Dp = g->Dp; v.Dcols = g->Dcols; v.kernel = g->kernel;
    v.a = g->a; v.b = g->b;
    v.XT = g->XT.p; v.nx = g->nx.p; v.inv_ell = g->inv_ell.p; v.alpha = g->alpha.p; v.Linv = g->Linv.p;
    v.y = g->y.p; v.L = g->L.p;
    v.X = g->X.p; v.gram_direct = g->gram_direct;
    v.generation = g->generation;
    v.laplace = g->lap != nullptr;
    v.lap_T = g->lap ? g->lap->T.p : nullptr;
    v.lap_LBinv = g->lap ? g->lap->LBinv.p : nullptr;
    v.state = &g->state_mtx;
    return v;
}
bool gp_has_laplace(sls_gp* g) {
    CtxCall call_(g);
    return g->lap != nullptr;
}
void gp_set_acq_stats(sls_gp* g, long issued, long cap, int rounds, int live_end) {
    g->stat_issued = issued; g->stat_cap = cap; g->stat_rounds = rounds; g->stat_live_end = live_end;
}
}  // namespace slsk

extern "C" int sls_gp_generation(sls_gp* g, long* generation) {
    if (!g || !generation) return SLS_ERR_INVALID;
    CtxCall call_(g->ctx);
    *generation = g->generation;
    return SLS_OK;
}

extern "C" int sls_gp_get_summary(sls_gp* g, int* best_index, double* mu_best, double* logdet) {
    if (!g) return SLS_ERR_INVALID;
    CtxCall call_(g->ctx);
    if (best_index) *best_index = g->best_index;
    if (mu_best) *mu_best = g->mu_best;
    if (logdet) *logdet = g->logdet;
    return SLS_OK;
}

namespace slsk {
int gp_export_inputs(sls_gp* g, int* D, int* N, int* kernel, int* sigma_mode, int* device, double* b, std::vector<double>* X,
                     std::vector<double>* y, std::vector<double>* theta) {
    SLS_TRY
    CtxCall call_(g);
    refuse_laplace(g, "sls_multi_gp_create_from");
    *D = g->D; *N = g->N; *kernel = g->kernel; *sigma_mode = g->sigma_mode; *device = g->ctx->device; *b = g->b;
    *theta = g->theta;
    X->resize((size_t)g->D * g->N);
    y->resize(g->N);
    d2h(g->ctx, X->data(), g->X.p, X->size());
    d2h(g->ctx, y->data(), g->y.p, y->size());
    sync(g->ctx);
    SLS_CATCH
}
}  // namespace slsk

extern "C" int sls_gp_set_sigma_mode(sls_gp* g, int mode) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && (mode == SLS_SIGMA_EXPLICIT_INVERSE || mode == SLS_SIGMA_CHOLESKY_SOLVE), "sls_gp_set_sigma_mode: bad argument");
    refuse_laplace(g, "sls_gp_set_sigma_mode");
    std::unique_lock<std::shared_mutex> state_(g->state_mtx);
    if (mode == SLS_SIGMA_CHOLESKY_SOLVE && g->sigma_mode != mode)
        launch_transpose_full(g->ctx->stream, g->Linv.p, g->U.p, g->Np);   // every block of U = (L^-1)^T (trtri writes the upper ones only)
    if (g->sigma_mode != mode) g->generation = ++g_gp_generation;
    g->sigma_mode = mode;
    sync(g->ctx);   // slot streams are not ordered behind the context's stream: the state is complete before the lock goes
    SLS_CATCH
}

// ---- Laplace posterior of the goodness values (include/sls_hip.h "Laplace posterior") ---------------------------------------------
// Everything on the context's stream; nothing N^2-sized passes through the host.  With L = chol(K_y) (a copy with its upper triangle
// cleared), W the BTL Hessian at the handle's y:
//   "laplace_w"      W: probabilities per tuple, one lane per row in a fixed order, the upper triangle mirrored from the lower
//   "laplace_b"      T1 = W L,  A = L^T T1 (lower tiles, mirrored),  B = A + I
//   "laplace_potri"  B = L_B L_B^T and B^-1 (launch_potri at the handle's padding)
//   "laplace_m"      G = B^-1 T1^T (= T L^-1),  M = L^-T G and T = G L (lower tiles, mirrored)
// M = L^-T B^-1 (L^T W L) L^-1 is a product throughout: no two K_y^-1-sized quantities are ever differenced.
static void laplace_clean_factor(sls_gp* g, DBuf& Lc) {
    const size_t n2 = (size_t)g->Np * g->Np;
    Lc.ensure(n2);
    SLS_HIP(hipMemcpyAsync(Lc.p, g->L.p, n2 * sizeof(double), hipMemcpyDeviceToDevice, g->ctx->stream));
    launch_zero_upper(g->ctx->stream, Lc.p, g->Np);
}
static void laplace_build(sls_gp* g, sls_gp::LaplaceState& st, const std::vector<int>& off, const std::vector<int>& flat) {
    sls_ctx* c = g->ctx;
    const int N = g->N, Np = g->Np, nt = Np / 128, n_prefs = (int)off.size() - 1, E = (int)flat.size();
    const size_t n2 = (size_t)Np * Np;
    // the transposed CSR (point -> flat positions, increasing) and the tuple of every flat position
    std::vector<int> ints;
    ints.reserve((size_t)n_prefs + 1 + 3 * (size_t)E + N + 1);
    ints.insert(ints.end(), off.begin(), off.end());
    ints.insert(ints.end(), flat.begin(), flat.end());
    std::vector<int> csc_off(N + 1, 0), csc_ent(E), tuple_of(E);
    for (int e = 0; e < E; ++e) ++csc_off[flat[e] + 1];
    for (int i = 0; i < N; ++i) csc_off[i + 1] += csc_off[i];
    {
        std::vector<int> at(csc_off.begin(), csc_off.end() - 1);
        for (int e = 0; e < E; ++e) csc_ent[at[flat[e]]++] = e;
    }
    for (int t = 0; t < n_prefs; ++t)
        for (int e = off[t]; e < off[t + 1]; ++e) tuple_of[e] = t;
    ints.insert(ints.end(), csc_off.begin(), csc_off.end());
    ints.insert(ints.end(), csc_ent.begin(), csc_ent.end());
    ints.insert(ints.end(), tuple_of.begin(), tuple_of.end());
    DBuf ibuf, P, logp0, Lc, T1, A, U, G, scal, LB;   // LB: B, then its factor (read by the summary only)
    ibuf.ensure((ints.size() + 1) / 2);
    SLS_HIP(hipMemcpyAsync(ibuf.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int* d_off = reinterpret_cast<const int*>(ibuf.p);
    const int* d_flat = d_off + n_prefs + 1;
    const int* d_csc_off = d_flat + E;
    const int* d_csc_ent = d_csc_off + N + 1;
    const int* d_tuple_of = d_csc_ent + E;
    P.ensure(E); logp0.ensure(n_prefs); T1.ensure(n2); A.ensure(n2); U.ensure(n2); G.ensure(n2); scal.ensure(4);
    st.W.ensure(n2); st.M.ensure(n2); st.T.ensure(n2); LB.ensure(n2); st.LBinv.ensure(n2); st.Binv.ensure(n2);
    {
        ProfScope ps(c, "laplace_w");
        launch_laplace_w(c->stream, d_off, d_flat, d_csc_off, d_csc_ent, d_tuple_of, n_prefs, g->y.p, st.btl_scale, N, Np, P.p, logp0.p,
                         st.W.p);
        launch_mirror_lower(c->stream, st.W.p, Np);
    }
    {
        ProfScope ps(c, "laplace_b");
        laplace_clean_factor(g, Lc);
        launch_gemm_plain(c->stream, st.W.p, Np, false, Lc.p, Np, true, T1.p, Np, nt, nt, Np, 1.0, 0.0);          // T1 = W L
        launch_gemm_lower_tiles(c->stream, Lc.p, Np, true, T1.p, Np, true, A.p, Np, nt, Np, 1.0, 0.0);           // A = L^T T1
        launch_mirror_lower(c->stream, A.p, Np);
    }
    for (int attempt = 0;; ++attempt) {
        SLS_HIP(hipMemcpyAsync(LB.p, A.p, n2 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        launch_add_diag(c->stream, LB.p, Np, Np, 1.0);   // B = I + L^T W L (the padding of A is zero: identity there)
        SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
        c->potrf_tick_rearm();
        int* df_sync = c->potrf_df_sync(Np);
        {
            ProfScope ps(c, "laplace_potri");
            launch_fill(c->stream, st.LBinv.p, (long)n2, 0.0);   // L_B^-1 is kept and read as a full matrix: zero above the diagonal
            launch_potri(c->stream, LB.p, Np, st.LBinv.p, U.p, st.Binv.p, c->d_info, df_sync);
        }
        int info[2] = {0, 0};
        SLS_HIP(hipMemcpyAsync(info, c->d_info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        if (potrf_gave_up(c, info[1], attempt)) continue;   // once more, on the multi-launch schedule
        if (info[0] != 0) {
            set_error("sls_gp_set_laplace: I + L^T W L is not positive definite (pivot %d): y or the fit is not finite", info[0] - 1);
            throw HipFail{SLS_ERR_NOT_SPD};
        }
        break;
    }
    {
        ProfScope ps(c, "laplace_m");
        launch_gemm_plain(c->stream, st.Binv.p, Np, false, T1.p, Np, false, G.p, Np, nt, nt, Np, 1.0, 0.0);      // G = B^-1 T1^T
        launch_gemm_lower_tiles(c->stream, g->Linv.p, Np, true, G.p, Np, true, st.M.p, Np, nt, Np, 1.0, 0.0);    // M = L^-T G
        launch_mirror_lower(c->stream, st.M.p, Np);
        launch_gemm_lower_tiles(c->stream, G.p, Np, false, Lc.p, Np, true, st.T.p, Np, nt, Np, 1.0, 0.0);        // T = G L
        launch_mirror_lower(c->stream, st.T.p, Np);
    }
    launch_laplace_summary(c->stream, logp0.p, n_prefs, LB.p, Np, N, g->y.p, g->alpha.p, scal.p);
    double sm[3] = {0, 0, 0};
    d2h(c, sm, scal.p, 3);
    sync(c);   // also: the temporaries of this call are idle before they go back to the pool
    st.log_lik = sm[0]; st.logdet_B = sm[1]; st.quad = sm[2];
}

extern "C" int sls_gp_set_laplace(sls_gp* g, const unsigned* prefs_flat, const int* pref_offsets, int n_prefs, double btl_scale) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && prefs_flat && pref_offsets, "sls_gp_set_laplace: NULL argument");
    SLS_REQUIRE(n_prefs >= 1, "sls_gp_set_laplace: n_prefs = %d (need at least one tuple)", n_prefs);
    SLS_REQUIRE(std::isfinite(btl_scale) && btl_scale > 0.0, "sls_gp_set_laplace: btl_scale = %g (must be > 0)", btl_scale);
    SLS_REQUIRE(pref_offsets[0] == 0, "sls_gp_set_laplace: pref_offsets[0] = %d (must be 0)", pref_offsets[0]);
    for (int t = 0; t < n_prefs; ++t)
        SLS_REQUIRE(pref_offsets[t + 1] - pref_offsets[t] >= 2 && pref_offsets[t + 1] - pref_offsets[t] <= (1 << 20),
                    "sls_gp_set_laplace: tuple %d has %d members (need at least 2)", t, pref_offsets[t + 1] - pref_offsets[t]);
    const int E = pref_offsets[n_prefs];
    for (int e = 0; e < E; ++e)
        SLS_REQUIRE(prefs_flat[e] < (unsigned)g->N, "sls_gp_set_laplace: index %u at flat position %d (N = %d)", prefs_flat[e], e, g->N);
    std::unique_lock<std::shared_mutex> state_(g->state_mtx);
    std::vector<int> off(pref_offsets, pref_offsets + n_prefs + 1), flat(prefs_flat, prefs_flat + E);
    std::unique_ptr<sls_gp::LaplaceState> st(new sls_gp::LaplaceState());
    st->btl_scale = btl_scale;
    laplace_build(g, *st, off, flat);   // a failure leaves the handle as it was
    g->lap = std::move(st);
    g->laplace_on.store(true);
    g->generation = ++g_gp_generation;
    SLS_CATCH
}

extern "C" int sls_gp_clear_laplace(sls_gp* g) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g, "sls_gp_clear_laplace: NULL handle");
    std::unique_lock<std::shared_mutex> state_(g->state_mtx);
    if (!g->lap) return SLS_OK;
    sync(g->ctx);
    g->lap.reset();
    g->laplace_on.store(false);
    g->generation = ++g_gp_generation;
    SLS_CATCH
}

extern "C" int sls_gp_laplace_get(sls_gp* g, int what, double* out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && out, "sls_gp_laplace_get: NULL argument");
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    SLS_REQUIRE(g->lap != nullptr, "sls_gp_laplace_get: the handle has no Laplace posterior (sls_gp_set_laplace)");
    sls_ctx* c = g->ctx;
    const int N = g->N, Np = g->Np, nt = Np / 128;
    switch (what) {
        case SLS_LAPLACE_W: d2h_matrix(c, out, g->lap->W.p, N, Np); break;
        case SLS_LAPLACE_M: d2h_matrix(c, out, g->lap->M.p, N, Np); break;
        case SLS_LAPLACE_COV: {
            // Sigma_g = L B^-1 L^T, formed on demand: S1 = B^-1 L^T, Sigma = L S1 (lower tiles, mirrored)
            DBuf Lc, S1, Sg;
            laplace_clean_factor(g, Lc);
            S1.ensure((size_t)Np * Np); Sg.ensure((size_t)Np * Np);
            launch_gemm_plain(c->stream, g->lap->Binv.p, Np, false, Lc.p, Np, false, S1.p, Np, nt, nt, Np, 1.0, 0.0);
            launch_gemm_lower_tiles(c->stream, Lc.p, Np, false, S1.p, Np, true, Sg.p, Np, nt, Np, 1.0, 0.0);
            launch_mirror_lower(c->stream, Sg.p, Np);
            d2h_matrix(c, out, Sg.p, N, Np);
            sync(c);
            break;
        }
        default: SLS_REQUIRE(false, "sls_gp_laplace_get: unknown selector %d", what);
    }
    sync(c);
    SLS_CATCH
}

extern "C" int sls_gp_laplace_summary(sls_gp* g, double* log_lik, double* logdet_B, double* log_evidence) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g, "sls_gp_laplace_summary: NULL handle");
    SLS_REQUIRE(g->lap != nullptr, "sls_gp_laplace_summary: the handle has no Laplace posterior (sls_gp_set_laplace)");
    const sls_gp::LaplaceState& st = *g->lap;
    if (log_lik) *log_lik = st.log_lik;
    if (logdet_B) *logdet_B = st.logdet_B;
    if (log_evidence) *log_evidence = st.log_lik - 0.5 * st.quad - 0.5 * st.logdet_B;
    SLS_CATCH
}

extern "C" int sls_gp_get_matrix(sls_gp* g, int what, double* out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && out, "sls_gp_get_matrix: NULL argument");
    sls_ctx* c = g->ctx;
    const int N = g->N, Np = g->Np;
    // Up to Np = 2048 the padded matrix comes back as ONE contiguous copy into the handle's page-locked staging block and the N x N
    // part is taken out on the host (a strided copy into pageable memory is executed row by row, blocking; the factor's upper
    // triangle is cleared on the way out instead of by a device copy + launch).  PreferenceRegressor fetches K and L after every fit.
    const bool staged = (size_t)Np * Np <= IO_STAGE_MAX;
    auto fetch_staged = [&](const double* dev, bool lower_only) {
        double* st = g->io_stage((size_t)Np * Np);
        d2h(c, st, dev, (size_t)Np * Np);
        sync(c);
        for (int j = 0; j < N; ++j) {
            const double* col = st + (size_t)j * Np;
            double* o = out + (size_t)j * N;
            if (lower_only) {
                std::fill(o, o + std::min(j, N), 0.0);
                std::copy(col + j, col + N, o + j);
            } else {
                std::copy(col, col + N, o);
            }
        }
    };
    switch (what) {
        case SLS_GP_K_Y: {
            // m_K_y is not kept resident (the Cholesky factor overwrites it): rebuild the full symmetric matrix
            DBuf K;
            K.ensure((size_t)Np * Np);
            if (g->gram_direct) launch_gram_sym_direct(c->stream, g->X.p, g->D, g->inv_ell.p, Np, N, KernelSpec{g->kernel, g->a}, g->b, K.p, false);
            else launch_gram_sym(c->stream, g->XT.p, Np, g->Dp, g->nx.p, Np, N, KernelSpec{g->kernel, g->a}, g->b, K.p, false);
            if (staged) fetch_staged(K.p, false);
            else {
                d2h_matrix(c, out, K.p, N, Np);
                sync(c);
            }
            break;
        }
        case SLS_GP_K_Y_INV:
            if (staged) fetch_staged(g->Kinv.p, false);
            else {
                d2h_matrix(c, out, g->Kinv.p, N, Np);
                sync(c);
            }
            break;
        case SLS_GP_CHOL_L: {
            if (staged) {
                fetch_staged(g->L.p, true);
                break;
            }
            DBuf T;
            T.ensure((size_t)Np * Np);
            SLS_HIP(hipMemcpyAsync(T.p, g->L.p, (size_t)Np * Np * 8, hipMemcpyDeviceToDevice, c->stream));
            launch_zero_upper(c->stream, T.p, Np);
            d2h_matrix(c, out, T.p, N, Np);
            sync(c);
            break;
        }
        case SLS_GP_ALPHA: d2h(c, out, g->alpha.p, N); sync(c); break;
        case SLS_GP_MU_DATA: d2h(c, out, g->mu_data.p, N); sync(c); break;
        default: SLS_REQUIRE(false, "sls_gp_get_matrix: unknown selector %d", what);
    }
    SLS_CATCH
}

// ---- batched evaluation -------------------------------------------------------------------------------------
static void ensure_eval_ws(sls_gp* g, int chunk) {
    if (chunk <= g->ws_chunk) return;
    const size_t Np = g->Np, C = chunk;
    const size_t nbt = Np / 128;
    g->Ks.ensure(C * Np);
    if (g->kernel == SLS_KERNEL_ARD_MATERN52) g->Cs.ensure(C * Np);
    g->P.ensure(C * Np);
    g->parts.ensure(10 * nbt * C);  // mu, ca: one per row tile; kw, cw: one per half row tile; + kw, cw of the solve-based sigma
    g->Gs.ensure(C * g->Dcols);
    g->Gm.ensure(C * g->Dcols);
    g->XsT.ensure(C * g->Dcols);
    g->ns.ensure(C);
    g->ws_chunk = chunk;
}

// What one evaluation wants; any output may be NULL.  At the entry points the pointers are the caller's host arrays (row outputs
// dmu, dsigma, grad: D x M column-major); below them, candidate-major device outputs with leading dimension ldo (eval_block).
struct EvalOut {
    long ldo = 0;
    double *mu = nullptr, *sigma = nullptr, *dmu = nullptr, *dsigma = nullptr, *val = nullptr, *grad = nullptr;
    int acq = SLS_ACQ_EXPECTED_IMPROVEMENT;
    double ucb_h = 1.0;
};

// value-only evaluations take the triangular L^-1 contraction (half the flops); SLS_TRI_PREDICT=0 forces the K^-1 form
static bool tri_predict() {
    return tune_on(TUNE_TRI_PREDICT);
}

// xr: raw candidate coordinates, S candidates: candidate-major xr[n + d*ldr], or (point_major) xr[d + n*D] as the host hands them
// over (the device transposes: prep_kernel<false>, same arithmetic and same bits as the candidate-major form).
static void eval_candidates(sls_gp* g, const double* xr, long ldr, int S, const EvalOut& o, bool point_major = false) {
    sls_ctx* c = g->ctx;
    const int Np = g->Np, N = g->N, D = g->D;
    const bool want_grad = o.dmu || o.dsigma || o.grad;
    const int chunk_max = std::min(round_up(S, 128), c->cand_chunk);
    ensure_eval_ws(g, chunk_max);
    const int nbt = Np / 128;
    KernelSpec ks{g->kernel, g->a};
    for (int s0 = 0; s0 < S; s0 += chunk_max) {
        const int sc = std::min(chunk_max, S - s0);
        const int Sp = round_up(sc, 128);
        const long ldk = Sp;
        double* Cs = (g->kernel == SLS_KERNEL_ARD_MATERN52) ? g->Cs.p : g->Ks.p;
        double* mu_part = g->parts.p;
        double* ca_part = mu_part + (size_t)nbt * ldk;
        double* kw_part = ca_part + (size_t)nbt * ldk;
        double* cw_part = kw_part + (size_t)2 * nbt * ldk;
        {
            ProfScope ps(c, "cross_gram");
            if (point_major) launch_prep_points(c->stream, xr + (size_t)s0 * D, D, sc, g->inv_ell.p, g->XsT.p, ldk, Sp, g->Dcols, g->ns.p);
            else launch_prep_cands(c->stream, xr + s0, ldr, D, sc, g->inv_ell.p, g->XsT.p, ldk, Sp, g->Dcols, g->ns.p);
            if (g->gram_direct)
                launch_cross_gram_direct(c->stream, point_major ? xr + (size_t)s0 * D : xr + s0, point_major ? D : 1, point_major ? 1 : ldr, sc,
                                         Sp, g->X.p, D, g->inv_ell.p, Np, N, ks, g->alpha.p, g->Ks.p, Cs, ldk, mu_part, ca_part);
            else
                launch_cross_gram(c->stream, g->XsT.p, ldk, g->ns.p, Sp, g->XT.p, Np, g->nx.p, Np, N, g->Dp, ks, g->alpha.p, g->Ks.p, Cs,
                                  ldk, mu_part, ca_part);
        }
        int split_first = 0x7fffffff;
        // a Laplace handle: the explicit-inverse route with M = L^-T T L^-1 in the place of K_y^-1, in either sigma mode
        const bool lap = g->lap != nullptr;
        const double* Kinv = lap ? g->lap->M.p : g->Kinv.p;
        const bool solve_grad = !lap && g->sigma_mode == 1 && (want_grad || !tri_predict());
        {
            ProfScope ps(c, want_grad ? "acq_gemm" : "var_gemm");
            if (solve_grad) {
                // handles of a PreferenceRegressor: w = K^-1 k as L^-T (L^-1 k) (LLT.solve, src/preference-regressor.cpp:299-330) --
                // V = K* L^-T as a plain product, then the acq_gemm tile kernel with (L^-1)^T in the place of K^-1 and V in the
                // place of K*: P = C* o W and the c.w partial sums come out as usual (its k.w sums are not used: sigma below)
                g->Vs.ensure((size_t)chunk_max * Np);
                launch_gemm_plain(c->stream, g->Ks.p, ldk, false, g->Linv.p, Np, false, g->Vs.p, ldk, Sp / 128, Np / 128, Np, 1.0, 0.0);
                split_first = launch_acq_gemm(c->stream, g->Vs.p, Cs, ldk, Sp, g->U.p, Np, g->P.p, kw_part, cw_part, c->d_info + 32);
            } else if (lap || want_grad || !tri_predict())
                split_first = launch_acq_gemm(c->stream, g->Ks.p, Cs, ldk, Sp, Kinv, Np, g->P.p, kw_part, cw_part, c->d_info + 32);
            else
                launch_var_gemm(c->stream, g->Ks.p, ldk, Sp, g->Linv.p, Np, kw_part, cw_part);
        }
        // ... and sigma from the triangular form |L^-1 k|^2
        double* kw_solve = nullptr;
        if (solve_grad) {
            kw_solve = cw_part + (size_t)2 * nbt * ldk;
            ProfScope ps(c, "var_gemm");
            launch_var_gemm(c->stream, g->Ks.p, ldk, Sp, g->Linv.p, Np, kw_solve, kw_solve + (size_t)2 * nbt * ldk);
        }
        if (want_grad && g->gram_direct) {
            // beyond the guard: the contractions over raw coordinate differences; finalize's x~* ca and x~* cw terms are then zero
            ProfScope ps(c, "grad_gemm");
            launch_grad_direct(c->stream, g->P.p, Cs, ldk, Sp, point_major ? xr + (size_t)s0 * D : xr + s0, point_major ? D : 1,
                               point_major ? 1 : ldr, sc, g->X.p, D, g->inv_ell.p, N, g->alpha.p, g->Gs.p, g->Gm.p);
            SLS_HIP(hipMemsetAsync(ca_part, 0, (size_t)nbt * ldk * 8, c->stream));
            SLS_HIP(hipMemsetAsync(cw_part, 0, (size_t)2 * nbt * ldk * 8, c->stream));
        } else if (want_grad) {
            ProfScope ps(c, "grad_gemm");
            launch_grad_gemm(c->stream, g->P.p, Cs, ldk, Sp, g->XT.p, g->XaT.p, Np, Np, D <= 64 ? -g->Dcols : g->Dcols, g->Gs.p, g->Gm.p,
                             grad_split_scratch(g->Gpart, D, Sp));
        }
        {
            ProfScope ps(c, "finalize");
            FinalizeArgs f;
            f.S = sc; f.D = D; f.nbt = nbt; f.ldk = ldk; f.ntm = Sp / 128; f.split_first = split_first;
            f.mu_part = mu_part; f.ca_part = ca_part; f.kw_part = kw_part; f.cw_part = cw_part;
            f.kw_solve_part = kw_solve;
            f.Gs = g->Gs.p; f.Gm = g->Gm.p; f.XsT = g->XsT.p; f.inv_ell = g->inv_ell.p;
            f.a = g->a; f.mu_best = g->mu_best; f.ucb_h = o.ucb_h; f.acq = o.acq;
            f.ldo = o.ldo;
            f.mu = o.mu ? o.mu + s0 : nullptr;
            f.sigma = o.sigma ? o.sigma + s0 : nullptr;
            f.dmu = o.dmu ? o.dmu + s0 : nullptr;
            f.dsigma = o.dsigma ? o.dsigma + s0 : nullptr;
            f.val = o.val ? o.val + s0 : nullptr;
            f.grad = o.grad ? o.grad + s0 : nullptr;
            launch_finalize(c->stream, f);
        }
    }
}

// Small problems: one wavefront per query point / start (kernels_wave.hip) instead of the tiled pipeline.  The answer depends
// only on the fitted state and the count, so repeated / sharded calls take the same path.  D never changes for a handle
// (wave_path_dims); Np grows with appended points, so whoever works without the context's lock asks under the state lock.
constexpr int WAVE_PATH_MAX_POINTS = 4096;   // query points / starts per launch
// A handle beyond the guard of the norm expansion (gram_direct) takes the tiled pipeline: the wavefront kernels difference scaled coordinates.
// So does a Laplace handle: the wavefront kernels read K_y^-1 / L^-1.
static bool wave_path_dims(const sls_gp* g) {
    return tune_on(TUNE_WAVE_PATH) && g->D <= WAVE_PATH_MAX_D && !g->gram_direct && !g->laplace_on.load();
}
static bool wave_path_applies(const sls_gp* g, int count) {
    return wave_path_dims(g) && g->Np <= WAVE_PATH_MAX_NP && count <= WAVE_PATH_MAX_POINTS;
}
// the model half of WaveArgs: everything that comes from the fitted state
static void wave_model_args(const sls_gp* g, WaveArgs& w) {
    w.D = g->D; w.N = g->N; w.Np = g->Np;
    w.matern = g->kernel == SLS_KERNEL_ARD_MATERN52;
    w.a = g->a; w.mu_best = g->mu_best;
    w.XT = g->XT.p; w.inv_ell = g->inv_ell.p; w.Kinv = g->Kinv.p; w.alpha = g->alpha.p;
    w.solve_sigma = g->sigma_mode == 1; w.Linv = g->Linv.p; w.U = g->U.p;
    w.useful = nullptr;
}
// evaluation-only mode on stream s.  Xs_dev: D x M column-major device copy of the query points; outputs as in EvalOut (device).
static void wave_eval(const sls_gp* g, hipStream_t s, const double* Xs_dev, int M, const EvalOut& o) {
    WaveArgs w;
    wave_model_args(g, w);
    w.S = M; w.m = 1; w.n_local = 0; w.acq = o.acq; w.ucb_h = o.ucb_h;
    w.c1 = 0; w.shrink = 0; w.gtol = 0; w.max_backtracks = 0;
    w.starts = Xs_dev; w.x_out = nullptr; w.f_out = nullptr; w.ld = o.ldo;
    w.ev_mu = o.mu; w.ev_sigma = o.sigma; w.ev_dmu = o.dmu; w.ev_dsigma = o.dsigma; w.ev_val = o.val; w.ev_grad = o.grad;
    launch_maximize_wave(s, w);
}
// ... on the context's stream (the caller has asked wave_path_applies)
static void eval_small(sls_gp* g, const double* Xs_dev, int M, const EvalOut& o) {
    ProfScope ps(g->ctx, "acq_wave");
    wave_eval(g, g->ctx->stream, Xs_dev, M, o);
}

// host rows x M column-major (rows = D; 2D for query pairs) -> the handle's candidate-major raw coordinates (clamping is NOT
// applied here)
static void upload_candidates(sls_gp* g, const double* Xs, int rows, int M, int Mp) {
    const std::vector<double> t = host_to_cm(Xs, rows, M, Mp);
    g->raw.ensure(t.size());
    h2d(g->ctx, g->raw.p, t.data(), t.size());
    sync(g->ctx);
}

// evaluate M host-supplied query points (D x M column-major) into the candidate-major device outputs of `o`
static void eval_host_points(sls_gp* g, const double* Xs, int M, int Mp, const EvalOut& o) {
    sls_ctx* c = g->ctx;
    const size_t n = (size_t)g->D * M;
    const bool wave = wave_path_applies(g, M);
    const bool staged = n <= IO_STAGE_MAX && tune_on(TUNE_IO_STAGE);
    if (!wave && !staged) {   // SLS_IO_STAGE=0: the transposing pageable upload of rounds 1-3 (A/B, tests)
        upload_candidates(g, Xs, g->D, M, Mp);
        eval_candidates(g, g->raw.p, Mp, M, o);
        return;
    }
    // as handed over (point-major): no transposition on the host, no synchronisation behind the upload
    g->raw.ensure(n);
    const double* src = Xs;
    if (staged) {   // through the page-locked block: a copy from pageable memory blocks the host
        double* st = g->io_stage(n);
        std::memcpy(st, Xs, n * sizeof(double));
        src = st;
    }
    h2d(c, g->raw.p, src, n);
    if (wave) eval_small(g, g->raw.p, M, o);
    else eval_candidates(g, g->raw.p, 0, M, o, true);
}

// ---- result blocks ---------------------------------------------------------------------------------------------
// The outputs a call asked for, one behind the other in ONE block: mu | sigma | val | dmu | dsigma | grad, the absent ones left
// out, each candidate-major with leading dimension ld (1 row, or D rows for dmu / dsigma / grad).  The same layout serves the
// device outputs of the general path, the mapped blocks of the small paths and the host's copy of either.
static size_t eval_block_doubles(const EvalOut& want, int D, long ld) {
    const int vecs = (want.mu != nullptr) + (want.sigma != nullptr) + (want.val != nullptr);
    const int mats = (want.dmu != nullptr) + (want.dsigma != nullptr) + (want.grad != nullptr);
    return (size_t)(vecs + (size_t)mats * D) * ld;
}
static EvalOut eval_block(const EvalOut& want, double* base, int D, long ld) {
    EvalOut b = want;
    b.ldo = ld;
    auto place = [&](double* asked, int rows) {
        double* at = asked ? base : nullptr;
        if (asked) base += (size_t)rows * ld;
        return at;
    };
    b.mu = place(want.mu, 1); b.sigma = place(want.sigma, 1); b.val = place(want.val, 1);
    b.dmu = place(want.dmu, D); b.dsigma = place(want.dsigma, D); b.grad = place(want.grad, D);
    return b;
}
// a block `at` (eval_block over host-readable memory) into the arrays the caller named in `want`
static void eval_block_to_host(const EvalOut& want, const EvalOut& at, int D, int M) {
    cm_to_host(at.mu, at.ldo, 1, M, want.mu); cm_to_host(at.sigma, at.ldo, 1, M, want.sigma); cm_to_host(at.val, at.ldo, 1, M, want.val);
    cm_to_host(at.dmu, at.ldo, D, M, want.dmu); cm_to_host(at.dsigma, at.ldo, D, M, want.dsigma); cm_to_host(at.grad, at.ldo, D, M, want.grad);
}
// where a call's downloads land: the handle's page-locked staging block when n doubles fit, `pageable` otherwise
static double* host_stage(sls_gp* g, size_t n, std::vector<double>& pageable) {
    if (n <= IO_STAGE_MAX) return g->io_stage(n);
    pageable.resize(n);
    return pageable.data();
}
// n doubles of device memory where the host can read them on return; ONE synchronisation
static double* fetch(sls_gp* g, const double* dev, size_t n, std::vector<double>& pageable) {
    double* t = host_stage(g, n, pageable);
    d2h(g->ctx, t, dev, n);
    sync(g->ctx);
    return t;
}
// every output of a call back to the host: the device block behind eval_block(want, dev, rows, Mp) in one copy
static void download_block(sls_gp* g, const EvalOut& want, const double* dev, int rows, int M, int Mp) {
    const size_t n = eval_block_doubles(want, rows, Mp);
    if (n == 0) {
        sync(g->ctx);   // nothing to fetch, but the evaluation in flight reads the staging block the next call writes into
        return;
    }
    std::vector<double> pageable;
    eval_block_to_host(want, eval_block(want, fetch(g, dev, n, pageable), rows, Mp), rows, M);
}

// Small evaluations through a device-mapped block: [D x M query points][eval_block with ld = M].  The kernel reads the points from
// and writes the results to host memory: no copy calls.  mapped_in fills the block and returns the device's view of the outputs;
// mapped_out, behind the stream's synchronisation, hands the results to the caller.
static size_t mapped_bytes(const EvalOut& want, int D, int M) { return ((size_t)D * M + eval_block_doubles(want, D, M)) * sizeof(double); }
static EvalOut mapped_in(const HostBuf& blk, const double* Xs, int D, int M, const EvalOut& want) {
    std::memcpy(blk.host, Xs, sizeof(double) * (size_t)D * M);
    return eval_block(want, blk.dev + (size_t)D * M, D, M);
}
static void mapped_out(const HostBuf& blk, int D, int M, const EvalOut& want) {
    eval_block_to_host(want, eval_block(want, blk.host + (size_t)D * M, D, M), D, M);
}

// ---- concurrent small evaluations (sls_ctx::EvalSlot) ---------------------------------------------------------
constexpr int SLOT_MAX_POINTS = 64;
// true: evaluated (results are in the caller's arrays).  false: not applicable -- the caller takes the context's lock and the
// general path.  Holds no lock of the context; the caller must NOT hold it either (a mutator waiting for the state lock would
// then wait for this call, not the other way round -- there is no inversion, but the point of the path is to stay off that lock).
static bool eval_in_slot(sls_gp* g, const double* Xs, int M, const EvalOut& want) {
    sls_ctx* c = g->ctx;
    if (M < 1 || M > SLOT_MAX_POINTS || !tune_on(TUNE_EVAL_SLOTS) || c->prof_on) return false;
    if (!wave_path_dims(g)) return false;              // D never changes for a handle
    (void)hipSetDevice(c->device);
    const int D = g->D;
    // Lock order: the slot (and, for the rare growth of its block, the context's lock, released again) FIRST, the shared lock on the
    // fitted state LAST and on its own.  Mutators hold the context's lock and then the state lock exclusively: taking the context's
    // lock under the shared state lock here would deadlock against them.
    // ---- borrow a slot ----
    sls_ctx::EvalSlot* slot = nullptr;
    {
        std::unique_lock<std::mutex> lk(c->slot_mtx);
        for (;;) {
            for (auto& s : c->slots)
                if (!s->busy) { slot = s.get(); break; }
            if (slot) break;
            if ((int)c->slots.size() < sls_ctx::MAX_SLOTS) {
                c->slots.emplace_back(new sls_ctx::EvalSlot());
                slot = c->slots.back().get();
                break;
            }
            c->slot_cv.wait(lk);
        }
        slot->busy = true;
    }
    struct Release {
        sls_ctx* c;
        sls_ctx::EvalSlot* s;
        ~Release() {
            {
                std::lock_guard<std::mutex> lk(c->slot_mtx);
                s->busy = false;
            }
            c->slot_cv.notify_one();
        }
    } release{c, slot};
    if (!slot->stream) SLS_HIP(hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking));
    const size_t need = mapped_bytes(want, D, M);
    if (need > slot->block.bytes) {
        std::lock_guard<std::recursive_mutex> ctx_lock(c->mtx);   // the context's page-locked pool is not thread safe; growth is rare
        slot->block.ensure(c, need, true, (size_t)(4 + 4 * D) * SLOT_MAX_POINTS * sizeof(double));
    }
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    if (!wave_path_applies(g, M)) return false;        // grown past the wave path by appended points: the general path
    const EvalOut od = mapped_in(slot->block, Xs, D, M, want);
    wave_eval(g, slot->stream, slot->block.dev, M, od);
    SLS_HIP(hipStreamSynchronize(slot->stream));
    mapped_out(slot->block, D, M, want);
    return true;
}

// mu / dmu of g and sigma / dsigma of gs (of g when there is no gs) at the S points into g's pair blocks, leading dimension ldo
static void eval_pair_blocks(sls_gp* g, sls_gp* gs, const double* xr, long ldr, int S, bool want_grad, long ldo) {
    const size_t D = g->D;
    g->pair_mu.ensure(ldo); g->pair_sg.ensure(ldo);
    if (want_grad) { g->pair_dmu.ensure(ldo * D); g->pair_dsg.ensure(ldo * D); }
    EvalOut a, b;
    a.ldo = b.ldo = ldo;
    a.mu = g->pair_mu.p; a.dmu = want_grad ? g->pair_dmu.p : nullptr;
    EvalOut& sg = gs ? b : a;
    sg.sigma = g->pair_sg.p; sg.dsigma = want_grad ? g->pair_dsg.p : nullptr;
    eval_candidates(g, xr, ldr, S, a);
    if (gs) eval_candidates(gs, xr, ldr, S, b);
}
// value (+ gradient) of the acquisition at candidate-major points xr; gs != nullptr: sigma / dsigma come from gs
// (objective_for_multiple_points, src/acquisition-function.cpp:63-110)
// acq_type SLS_ACQ_LOG_EXPECTED_IMPROVEMENT: mu / dmu of g and sigma / dsigma of gs (of g if there is none) in g's pair blocks, then the
// LogEI combiner with g's mu_best
static void eval_acq(sls_gp* g, sls_gp* gs, const double* xr, long ldr, int S, int acq_type, double ucb_h, double* val,
                     double* grad, long ldo) {
    sls_ctx* c = g->ctx;
    if (!gs && acq_type != SLS_ACQ_LOG_EXPECTED_IMPROVEMENT) {   // EI / UCB of one handle: finalize forms them itself
        EvalOut eo;
        eo.ldo = ldo; eo.val = val; eo.grad = grad; eo.acq = acq_type; eo.ucb_h = ucb_h;
        eval_candidates(g, xr, ldr, S, eo);
        return;
    }
    eval_pair_blocks(g, gs, xr, ldr, S, grad != nullptr, ldo);
    const double *mu = g->pair_mu.p, *sg = g->pair_sg.p, *dmu = g->pair_dmu.p, *dsg = g->pair_dsg.p;
    if (acq_type == SLS_ACQ_LOG_EXPECTED_IMPROVEMENT) {
        ProfScope ps(c, "logei");
        launch_logei_combine(c->stream, S, g->D, ldo, mu, sg, dmu, dsg, g->mu_best, val, grad);
    } else {
        launch_combine(c->stream, S, g->D, ldo, mu, sg, dmu, dsg, acq_type, g->mu_best, ucb_h, val, grad);
    }
}

// ---- objectives on a handle and their front ends ---------------------------------------------------------------------------------
// What the two front ends (eval_points, maximize_starts) need to know of an acquisition.  A new acquisition constructs one of these
// and has its eval / maximize entry points, and through sub_objective its *_sub ones.
template <class Eval>
struct Objective {
    sls_gp* g;        // the handle whose workspace (raw, outv, lb, io), statistics and locks the call uses
    int nvar;         // rows of the caller's points / starts: D; 2D for query pairs; d for a subspace
    BestBlock best;   // the winner's block of a maximisation, 8 + nvar doubles
    // eval(xr, ldr, count, live, val, grad, ldo): value and gradient (may be nullptr) at the candidate-major points xr[n + r*ldr],
    // n < count, on the context's stream; live: as lockstep_rounds hands it over (only sub_objective reads it)
    Eval eval;
    int wave_acq;     // plain EI / UCB of the handle: the acq_type of the one-launch search (maximize_wave); -1 for everything else
    double ucb_h;
};
template <class Eval>
static Objective<Eval> objective(sls_gp* g, int nvar, BestBlock best, Eval eval, int wave_acq = -1, double ucb_h = 0.0) {
    return Objective<Eval>{g, nvar, best, eval, wave_acq, ucb_h};
}
static BestBlock sum_best(sls_gp* g) { return BestBlock{g->sum.dev + 8, g->sum.host + 8, false}; }   // nvar <= D

static bool known_acq(int acq_type) {
    return acq_type == SLS_ACQ_EXPECTED_IMPROVEMENT || acq_type == SLS_ACQ_GP_UCB || acq_type == SLS_ACQ_LOG_EXPECTED_IMPROVEMENT;
}
// EI / UCB / LogEI of g, with sigma from gs when there is one (the *_pair entry points)
static auto acq_objective(sls_gp* g, sls_gp* gs, int acq_type, double ucb_h) {
    SLS_REQUIRE(known_acq(acq_type), "unknown acquisition type %d", acq_type);
    // (the wave kernel has neither the pair nor the LogEI objective)
    const bool plain = !gs && acq_type != SLS_ACQ_LOG_EXPECTED_IMPROVEMENT;
    return objective(
        g, g->D, sum_best(g),
        [=](const double* xr, long ldr, int n, const int*, double* val, double* grad, long ldo) {
            eval_acq(g, gs, xr, ldr, n, acq_type, ucb_h, val, grad, ldo);
        },
        plain ? acq_type : -1, ucb_h);
}

// One more block of a point call: rows x Mp candidate-major doubles at dev->p once the evaluation has run (it may grow the block), back
// to the caller as rows x M column-major (transposed) or as they are, [m + r*M]
struct ExtraBlock {
    const DBuf* dev = nullptr;
    int rows = 0;
    double* host = nullptr;   // NULL: not asked for
    bool transposed = false;
};

// THE LOCKING RULE of every route through the two front ends: the context's lock and the handle's device first (the entry point's
// CtxCall), then the handle's state_mtx shared (here).  Mutators take the same two in the same order, state_mtx exclusively; only the
// slot path (eval_in_slot) has an order of its own, written down there.  Objects derived from a handle (sls_jes, sls_kg) check its
// generation under the context's lock, which every mutator holds.
//
// The objective at M >= 1 host points (nvar x M column-major) through the transposing upload; value (val == NULL: computed into
// scratch, the combiners always write it), gradient (nvar x M, may be NULL) and `extra` to the caller's arrays.  Two synchronisations:
// behind the upload, and ONE behind every download.
template <class Obj>
static void eval_points(const Obj& f, const double* pts, int M, double* val, double* grad, const ExtraBlock& extra = ExtraBlock()) {
    sls_gp* g = f.g;
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    const int Mp = round_up(M, 128), nvar = f.nvar;
    upload_candidates(g, pts, nvar, M, Mp);
    std::vector<double> unused;
    if (!val) unused.resize(M);
    EvalOut want;
    want.val = val ? val : unused.data(); want.grad = grad;
    const size_t n = eval_block_doubles(want, nvar, Mp), ne = extra.host ? (size_t)extra.rows * Mp : 0;
    g->outv.ensure(n);
    const EvalOut o = eval_block(want, g->outv.p, nvar, Mp);
    f.eval(g->raw.p, (long)Mp, M, nullptr, o.val, o.grad, (long)Mp);
    std::vector<double> pageable;
    double* t = host_stage(g, n + ne, pageable);
    d2h(g->ctx, t, g->outv.p, n);
    if (ne) d2h(g->ctx, t + n, extra.dev->p, ne);
    sync(g->ctx);
    eval_block_to_host(want, eval_block(want, t, nvar, Mp), nvar, M);
    if (ne && extra.transposed) cm_to_host(t + n, Mp, extra.rows, M, extra.host);
    else
        for (int r = 0; ne && r < extra.rows; ++r) std::copy(t + n + (size_t)r * Mp, t + n + (size_t)r * Mp + M, extra.host + (size_t)r * M);
}

// The body of sls_gp_predict, sls_gp_predict_grad and sls_acq_eval: `want` names the caller's arrays (any may be NULL).
static int eval_entry(const char* who, sls_gp* g, const double* Xs, int M, const EvalOut& want) {
    SLS_TRY
    // LogEI has no objective in the one-wavefront-per-start kernel: neither the slots nor the zero-copy path, always the tiled one
    const bool logei = want.acq == SLS_ACQ_LOG_EXPECTED_IMPROVEMENT;
    const bool slot_acq = want.acq == SLS_ACQ_EXPECTED_IMPROVEMENT || want.acq == SLS_ACQ_GP_UCB;
    if (g && Xs && M >= 1 && M <= SLOT_MAX_POINTS && slot_acq && eval_in_slot(g, Xs, M, want)) return SLS_OK;
    CtxCall call_(g);
    SLS_REQUIRE(g && Xs && M >= 0, "%s: bad argument", who);
    SLS_REQUIRE(known_acq(want.acq), "unknown acquisition type %d", want.acq);
    if (M == 0) return SLS_OK;
    if (logei) {
        eval_points(acq_objective(g, nullptr, want.acq, want.ucb_h), Xs, M, want.val, want.grad);
        return SLS_OK;
    }
    sls_ctx* c = g->ctx;
    const int Mp = round_up(M, 128), D = g->D;
    // Value-only evaluation of a small batch on a small problem -- one iteration of DIRECT (host/direct.cpp; the reference's
    // default global phase, src/acquisition-function.cpp:155-165) -- : the query points are read from, and the values written to,
    // a page-locked block the device maps: ONE launch + one synchronisation per call instead of upload + launch + download
    // (~60 -> ~30 us per call; ten calls per SubmitFeedbackData).  SLS_EVAL_ZEROCOPY=0: the copying path.
    const bool value_only = want.val && eval_block_doubles(want, D, 1) == 1;
    if (value_only && tune_on(TUNE_EVAL_ZEROCOPY) && wave_path_applies(g, M)) {
        const size_t need = mapped_bytes(want, D, M);
        g->zc.ensure(c, need, true, need * 2);
        eval_small(g, g->zc.dev, M, mapped_in(g->zc, Xs, D, M, want));
        sync(c);
        mapped_out(g->zc, D, M, want);
        return SLS_OK;
    }
    g->outv.ensure(eval_block_doubles(want, D, Mp));
    eval_host_points(g, Xs, M, Mp, eval_block(want, g->outv.p, D, Mp));
    download_block(g, want, g->outv.p, D, M, Mp);
    SLS_CATCH
}

extern "C" int sls_gp_predict(sls_gp* g, const double* Xs, int M, double* mu, double* sigma) {
    EvalOut want;
    want.mu = mu; want.sigma = sigma;
    return eval_entry("sls_gp_predict", g, Xs, M, want);
}

extern "C" int sls_gp_predict_grad(sls_gp* g, const double* Xs, int M, double* dmu, double* dsigma) {
    EvalOut want;
    want.dmu = dmu; want.dsigma = dsigma;
    return eval_entry("sls_gp_predict_grad", g, Xs, M, want);
}

extern "C" int sls_acq_eval(sls_gp* g, int acq_type, double ucb_h, const double* Xs, int M, double* val, double* grad) {
    EvalOut want;
    want.val = val; want.grad = grad; want.acq = acq_type; want.ucb_h = ucb_h;
    return eval_entry("sls_acq_eval", g, Xs, M, want);
}

// ---- multi-start maximiser -------------------------------------------------------------------------------------
extern "C" void sls_lbfgs_default_opts(sls_lbfgs_opts* o) {
    o->struct_size = (int)sizeof(sls_lbfgs_opts);
    o->history = 6; o->c1 = 1e-4; o->shrink = 0.5; o->gtol = 0.0; o->max_backtracks = 20; o->ftol_rel = 0.0; o->xtol_rel = 0.0;
}
// the caller's struct may be shorter than this library's (an older header): its struct_size bytes over the defaults
sls_lbfgs_opts slsk::read_lbfgs_opts(const sls_lbfgs_opts* in) {
    sls_lbfgs_opts o;
    sls_lbfgs_default_opts(&o);
    if (!in) return o;
    const int min_size = (int)(offsetof(sls_lbfgs_opts, max_backtracks) + sizeof(int));   // the members of the first version
    SLS_REQUIRE(in->struct_size >= min_size && in->struct_size <= (int)sizeof(sls_lbfgs_opts),
                "sls_lbfgs_opts.struct_size = %d: expected %d .. %d (call sls_lbfgs_default_opts first)", in->struct_size, min_size,
                (int)sizeof(sls_lbfgs_opts));
    memcpy(&o, in, (size_t)in->struct_size);
    o.struct_size = (int)sizeof(sls_lbfgs_opts);
    return o;
}

// The whole multi-start search in one launch, one wavefront per start (the caller has asked wave_path_applies).  Returns the device
// counter of useful evaluations: those of starts that were still moving (finished starts run idle to keep the barriers uniform),
// counted by the kernel into the live-count words of the integer scratch.
static const unsigned long long* maximize_wave(sls_gp* g, int acq_type, double ucb_h, const double* starts_dev,
                                               const MultistartRun& r) {
    sls_ctx* c = g->ctx;
    const sls_lbfgs_opts& o = r.o;
    const LbfgsState& st = r.st;
    const int S = st.S;
    WaveArgs w;
    wave_model_args(g, w);
    w.S = S; w.m = o.history; w.n_local = r.n_local; w.acq = acq_type; w.ucb_h = ucb_h;
    w.c1 = o.c1; w.shrink = o.shrink; w.gtol = o.gtol; w.max_backtracks = o.max_backtracks;
    w.ftol_rel = o.ftol_rel; w.xtol_rel = o.xtol_rel;
    w.starts = starts_dev; w.x_out = st.x; w.f_out = st.f; w.ld = st.ld;
    w.ev_mu = w.ev_sigma = w.ev_dmu = w.ev_dsigma = w.ev_val = w.ev_grad = nullptr;
    unsigned long long* d_useful = g->lb.wave_useful();
    SLS_HIP(hipMemsetAsync(d_useful, 0, sizeof(unsigned long long), c->stream));
    w.useful = d_useful;
    long long* d_trace = nullptr;
    if (tune_set(TUNE_WAVE_TRACE)) {
        d_trace = g->lb.wave_trace();
        SLS_HIP(hipMemsetAsync(d_trace, 0, 9 * sizeof(long long), c->stream));
        w.trace = d_trace;
    }
    {
        ProfScope ps(c, "acq_wave");
        launch_maximize_wave(c->stream, w);
    }
    if (d_trace) {
        long long tr[9] = {};
        SLS_HIP(hipMemcpyAsync(tr, d_trace, sizeof(tr), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        fprintf(stderr, "wave trace (us): S %d N %d D %d evals %lld | kvec %.1f  Kinv.k %.1f  sums %.1f  grad+acq %.1f  direction %.1f  "
                "bookkeeping %.1f  total %.1f  (shader clock %.0f MHz)\n", S, g->N, g->D, tr[6], tr[0] * 0.01, tr[1] * 0.01, tr[2] * 0.01, tr[3] * 0.01, tr[4] * 0.01,
                tr[5] * 0.01, tr[7] * 0.01, tr[7] > 0 ? (double)tr[8] / (tr[7] * 0.01) : 0.0);
    }
    return d_useful;
}

// fetch of maximize_finish on the sls_gp routes: through the handle's page-locked stage
static auto staged_fetch(sls_gp* g, std::vector<double>& pageable) {
    return [g, &pageable](const double* dev, size_t n) { return fetch(g, dev, n, pageable); };
}

// The body of every *_maximize entry point on an sls_gp handle (`who`), under the locking rule of eval_points: the shared maximiser
// (lbfgs_driver.hpp) with one of two searches, and a mapped block for the best start -- one synchronisation, no copies.
// starts: nvar x S column-major, on the host (uploaded here) or already on the device.  The outputs and the return value are
// maximize_finish's; the starts' end variables stay in f.g->lb.x (leading dimension round_up(S, 128)).
template <class Obj>
static long maximize_starts(const char* who, const Obj& f, const double* starts, bool starts_on_host, int S, int n_local,
                            const sls_lbfgs_opts* opts_in, long off, double* x_out, double* val_out, long* idx_out, double* x_stars,
                            double* y_stars) {
    sls_gp* g = f.g;
    sls_ctx* c = g->ctx;
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    MultistartRun r = maximize_begin(who, g, g->lb, opts_in, S, n_local, f.nvar);
    DBuf sd;
    if (starts_on_host) {
        sd.ensure((size_t)f.nvar * S);
        h2d(c, sd.p, starts, (size_t)f.nvar * S);
    }
    const double* starts_dev = starts_on_host ? sd.p : starts;
    LockstepStats ls;
    if (f.wave_acq >= 0 && wave_path_applies(g, S)) {
        // Small problems: one wavefront per start runs the whole search in a single launch (kernels_wave.hip)
        ls.issued_dev = maximize_wave(g, f.wave_acq, f.ucb_h, starts_dev, r);
        ls.rounds = n_local;
    } else {
        lockstep_rounds(c, r.st, g->lb, starts_dev, S, n_local,
                        [&](const double* trial, long ld, int nlive, const int* live, double* val, double* grad) {
                            f.eval(trial, ld, nlive, live, val, grad, ld);
                        },
                        &ls);
    }
    std::vector<double> pageable;
    return maximize_finish(c, r, ls, f.best, staged_fetch(g, pageable), off, x_out, val_out, idx_out, x_stars, y_stars);
}

extern "C" int sls_acq_last_stats(sls_gp* g, long* evals_issued, long* evals_cap, int* rounds, int* live_at_end) {
    if (!g) return SLS_ERR_INVALID;
    CtxCall call_(g->ctx);
    if (evals_issued) *evals_issued = g->stat_issued;
    if (evals_cap) *evals_cap = g->stat_cap;
    if (rounds) *rounds = g->stat_rounds;
    if (live_at_end) *live_at_end = g->stat_live_end;
    return SLS_OK;
}

extern "C" int sls_acq_maximize(sls_gp* g, int acq_type, double ucb_h, const double* starts, int S, int n_local,
                                const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                                long* idx_out, double* x_stars, double* y_stars) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && starts, "sls_acq_maximize: NULL argument");
    maximize_starts("sls_acq_maximize", acq_objective(g, nullptr, acq_type, ucb_h), starts, true, S, n_local, opts, start_index_offset,
                    x_out, val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}

static void check_pair(sls_gp* g, sls_gp* gs) {
    SLS_REQUIRE(g && gs, "NULL handle");
    SLS_REQUIRE(g->ctx == gs->ctx && g->D == gs->D, "the two regressors must share the context and the dimensionality");
    refuse_laplace(g, "sls_acq_*_pair");
    refuse_laplace(gs, "sls_acq_*_pair");
}

extern "C" int sls_acq_maximize_pair(sls_gp* g, sls_gp* gs, int acq_type, double ucb_h, const double* starts, int S, int n_local,
                                     const sls_lbfgs_opts* opts, double* x_out, double* val_out, long* idx_out) {
    SLS_TRY
    CtxCall call_(g);
    check_pair(g, gs);
    SLS_REQUIRE(starts, "sls_acq_maximize_pair: starts is NULL");
    maximize_starts("sls_acq_maximize_pair", acq_objective(g, gs, acq_type, ucb_h), starts, true, S, n_local, opts, 0, x_out, val_out,
                    idx_out, nullptr, nullptr);
    SLS_CATCH
}

extern "C" int sls_acq_eval_pair(sls_gp* g, sls_gp* gs, int acq_type, double ucb_h, const double* Xs, int M, double* val,
                                 double* grad) {
    SLS_TRY
    CtxCall call_(g);
    check_pair(g, gs);
    SLS_REQUIRE(Xs && M >= 0, "sls_acq_eval_pair: bad argument");
    const auto f = acq_objective(g, gs, acq_type, ucb_h);
    if (M == 0) return SLS_OK;
    eval_points(f, Xs, M, val, grad);
    SLS_CATCH
}

extern "C" int sls_acq_maximize_dev(sls_gp* g, int acq_type, double ucb_h, const double* starts_dev, int S, int n_local,
                                    const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out,
                                    long* idx_out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && starts_dev, "sls_acq_maximize_dev: NULL argument");
    maximize_starts("sls_acq_maximize_dev", acq_objective(g, nullptr, acq_type, ucb_h), starts_dev, false, S, n_local, opts,
                    start_index_offset, x_out, val_out, idx_out, nullptr, nullptr);
    SLS_CATCH
}

// ---- max-value entropy search (include/sls_hip.h) ------------------------------------------------------------------
// The MES objective of a call: the y* samples validated and uploaded once into ys (the caller's, alive for the call); mu, sigma and
// their gradients of g in the handle's pair blocks, then the MES combiner on the samples
static auto mes_objective(const char* who, sls_gp* g, const double* y_star, int K, DBuf& ys) {
    SLS_REQUIRE(y_star != nullptr, "%s: y_star is NULL", who);
    SLS_REQUIRE(K >= 1 && K <= SLS_MES_MAX_SAMPLES, "%s: K = %d (1 .. %d)", who, K, SLS_MES_MAX_SAMPLES);
    for (int k = 0; k < K; ++k) SLS_REQUIRE(std::isfinite(y_star[k]), "%s: y_star[%d] is not finite", who, k);
    ys.ensure((size_t)K);
    h2d(g->ctx, ys.p, y_star, (size_t)K);
    const double* ysd = ys.p;
    return objective(g, g->D, sum_best(g), [=](const double* xr, long ldr, int n, const int*, double* val, double* grad, long ldo) {
        eval_pair_blocks(g, nullptr, xr, ldr, n, grad != nullptr, ldo);
        ProfScope ps(g->ctx, "mes");
        launch_mes_combine(g->ctx->stream, n, g->D, ldo, g->pair_mu.p, g->pair_sg.p, g->pair_dmu.p, g->pair_dsg.p, ysd, K, val, grad);
    });
}

// The scalar terms on their own (test hooks): n inputs through `launch(in, m, out)` in chunks, out[k] (device) for the outputs
// the caller named in host[k] (nullptr for the others), k < nout
template <class Launch>
static int scalar_terms(const char* who, sls_ctx* ctx, const double* in, long n, int nout, double* const* host, Launch&& launch) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SLS_REQUIRE(n >= 0, "%s: n = %ld", who, n);
    if (n == 0 || std::all_of(host, host + nout, [](const double* h) { return h == nullptr; })) return SLS_OK;
    SLS_REQUIRE(in != nullptr, "%s: the input array is NULL", who);
    SLS_HIP(hipSetDevice(ctx->device));
    const long chunk = std::min(n, 1L << 22);
    DBuf buf;
    buf.ensure((size_t)(1 + nout) * chunk);
    double* dev[3];
    for (int k = 0; k < nout; ++k) dev[k] = host[k] ? buf.p + (k + 1) * chunk : nullptr;
    for (long i0 = 0; i0 < n; i0 += chunk) {
        const long m = std::min(chunk, n - i0);
        h2d(ctx, buf.p, in + i0, (size_t)m);
        launch(buf.p, m, dev);
        for (int k = 0; k < nout; ++k)
            if (host[k]) d2h(ctx, host[k] + i0, dev[k], (size_t)m);
        sync(ctx);   // buf is refilled by the next chunk
    }
    SLS_CATCH
}
extern "C" int sls_mes_terms(sls_ctx* ctx, const double* t, long n, double* g, double* dg) {
    double* const host[2] = {g, dg};
    return scalar_terms("sls_mes_terms", ctx, t, n, 2, host,
                        [&](const double* in, long m, double* const* out) { launch_mes_terms(ctx->stream, in, m, out[0], out[1]); });
}
extern "C" int sls_logei_terms(sls_ctx* ctx, const double* u, long n, double* log_h, double* b1, double* b2) {
    double* const host[3] = {log_h, b1, b2};
    return scalar_terms("sls_logei_terms", ctx, u, n, 3, host, [&](const double* in, long m, double* const* out) {
        launch_logei_terms(ctx->stream, in, m, out[0], out[1], out[2]);
    });
}
extern "C" int sls_qlognei_terms(sls_ctx* ctx, const double* a, long n, double* L, double* R) {
    double* const host[2] = {L, R};
    return scalar_terms("sls_qlognei_terms", ctx, a, n, 2, host,
                        [&](const double* in, long m, double* const* out) { launch_qlognei_terms(ctx->stream, in, m, out[0], out[1]); });
}

extern "C" int sls_mes_eval(sls_gp* g, const double* y_star, int K, const double* Xs, int M, double* val, double* grad) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_mes_eval: gp is NULL");
    SLS_REQUIRE(M >= 0, "sls_mes_eval: M = %d", M);
    DBuf ys;
    const auto f = mes_objective("sls_mes_eval", g, y_star, K, ys);
    if (M == 0) {
        sync(g->ctx);
        return SLS_OK;
    }
    SLS_REQUIRE(Xs != nullptr, "sls_mes_eval: Xs is NULL");
    SLS_REQUIRE(val != nullptr, "sls_mes_eval: val is NULL");
    eval_points(f, Xs, M, val, grad);
    SLS_CATCH
}

extern "C" int sls_mes_maximize(sls_gp* g, const double* y_star, int K, const double* starts, int S, int n_local,
                                const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                                double* x_stars, double* y_stars) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_mes_maximize: gp is NULL");
    SLS_REQUIRE(starts != nullptr, "sls_mes_maximize: starts is NULL");
    DBuf ys;
    maximize_starts("sls_mes_maximize", mes_objective("sls_mes_maximize", g, y_star, K, ys), starts, true, S, n_local, opts,
                    start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}

// ---- joint entropy search (include/sls_hip.h) ------------------------------------------------------------------------------
// The snapshot of the conditioned optima and the blocks of a candidate chunk (grown on demand, kept with the object so that the rounds
// of a maximisation allocate nothing).
// The part every criterion on K fixed points shares (joint entropy search, the knowledge gradient): the snapshot of the points and
// the chunk pass around a criterion's combiner.
struct PointSet {
    sls_gp* gp = nullptr;
    sls_ctx* ctx = nullptr;
    long generation = 0;
    int D = 0, K = 0, Kp = 0, Np = 0;
    // W [i + k*Np] (Np x Kp, 0 for k >= K and i >= N), xs [d + k*D] (raw, clamped), mu*, sigma* (K each)
    DBuf W, xs, mu_star, sg_star;
    // per chunk, candidate-major with the chunk's leading dimension: cov / cx / H (Sp x Kp), A_mu, A_sigma, csum (Sp), Go (Sp x D)
    DBuf cov, cx, H, a_mu, a_sg, csum, Go;
};
struct sls_jes : PointSet {
    DBuf v, dd, inv_v, f_star;   // K doubles each
};

// alpha (+ gradient, + the covariances) at S candidate-major points xr[n + d*ldr]; val[n], grad[n + d*ldo] (may be nullptr),
// cov_out[n + k*ldc] (may be nullptr).  eval_candidates reuses K*, C* and P per chunk, and this pass needs the chunk's K* and C* after
// it: it drives the tiled evaluation ONE chunk at a time.  A candidate's bits do not depend on the chunk it falls into.
// combine(sc, Sp, ldk, mu, sigma, s0, val, a_mu, a_sg, H) is the criterion's combiner on the chunk that starts at candidate s0 (a_mu,
// a_sg, H nullptr without grad); `scope` is the profiling name of the combiner and the finish.
template <class Combine>
static void pointset_eval_device(PointSet* j, const char* scope, Combine&& combine, const double* xr, long ldr, int S, double* val,
                                 double* grad, long ldo, double* cov_out, long ldc) {
    sls_gp* g = j->gp;
    sls_ctx* c = g->ctx;
    const int D = g->D, Np = g->Np, N = g->N, K = j->K, Kp = j->Kp;
    const KernelSpec ks{g->kernel, g->a};
    // mu, sigma and their gradients always (sigma as the gradient evaluations form it, whether or not grad is asked for)
    g->pair_mu.ensure(ldo); g->pair_sg.ensure(ldo);
    g->pair_dmu.ensure((size_t)ldo * D); g->pair_dsg.ensure((size_t)ldo * D);
    const int chunk_max = std::min(round_up(S, 128), c->cand_chunk);
    const size_t blk = (size_t)chunk_max * Kp;
    j->cov.ensure(blk);
    if (grad) {
        j->cx.ensure(blk); j->H.ensure(blk);
        j->a_mu.ensure(chunk_max); j->a_sg.ensure(chunk_max); j->csum.ensure(chunk_max);
        j->Go.ensure((size_t)chunk_max * D);
    }
    for (int s0 = 0; s0 < S; s0 += chunk_max) {
        const int sc = std::min(chunk_max, S - s0), Sp = round_up(sc, 128);
        const long ldk = Sp;
        EvalOut eo;
        eo.ldo = ldo;
        eo.mu = g->pair_mu.p + s0; eo.sigma = g->pair_sg.p + s0; eo.dmu = g->pair_dmu.p + s0; eo.dsigma = g->pair_dsg.p + s0;
        eval_candidates(g, xr + s0, ldr, sc, eo);   // one chunk: K* (g->Ks), C*, X~* (g->XsT) of these sc candidates stay behind it
        const double* Cs = (g->kernel == SLS_KERNEL_ARD_MATERN52) ? g->Cs.p : g->Ks.p;
        {
            ProfScope ps(c, "jes_cov");
            launch_jes_cross(c->stream, xr + s0, 1, ldr, sc, Sp, j->xs.p, D, K, Kp, g->inv_ell.p, ks, j->cov.p, grad ? j->cx.p : nullptr, ldk);
            // c = k(x, x*) - K* W: accumulated onto the prior term on the tile GEMM, k = the training points in increasing order
            launch_gemm_plain(c->stream, g->Ks.p, ldk, false, j->W.p, Np, true, j->cov.p, ldk, Sp / 128, Kp / 128, Np, -1.0, 1.0);
        }
        if (cov_out)
            SLS_HIP(hipMemcpy2DAsync(cov_out + s0, (size_t)ldc * 8, j->cov.p, (size_t)ldk * 8, (size_t)sc * 8, K, hipMemcpyDeviceToDevice,
                                     c->stream));
        {
            ProfScope ps(c, scope);
            if (grad && Kp > K) SLS_HIP(hipMemsetAsync(j->H.p + (size_t)K * ldk, 0, (size_t)(Kp - K) * ldk * 8, c->stream));
            combine(sc, Sp, ldk, eo.mu, eo.sigma, s0, val + s0, grad ? j->a_mu.p : nullptr, grad ? j->a_sg.p : nullptr,
                    grad ? j->H.p : nullptr);
        }
        if (grad) {
            {
                // U[m + i*ldk] = -sum_k H[m + k*ldk] W[i + k*Np] into P's block: one weight vector W h(x) per candidate
                ProfScope ps(c, "jes_agg");
                launch_gemm_plain(c->stream, j->H.p, ldk, false, j->W.p, Np, false, g->P.p, ldk, Sp / 128, Np / 128, Kp, -1.0, 0.0);
            }
            {
                ProfScope ps(c, "jes_grad");
                launch_jes_weight(c->stream, Sp, Np, ldk, Cs, g->P.p, j->csum.p);
                launch_jes_optima_grad(c->stream, xr + s0, 1, ldr, sc, j->xs.p, D, K, g->inv_ell.p, j->H.p, j->cx.p, ldk, j->Go.p);
            }
            {
                ProfScope ps(c, "jes_grad_gemm");
                if (g->gram_direct)
                    launch_grad_direct(c->stream, g->P.p, nullptr, ldk, Sp, xr + s0, 1, ldr, sc, g->X.p, D, g->inv_ell.p, N, nullptr, g->Gs.p,
                                       nullptr);
                else
                    launch_grad_gemm(c->stream, g->P.p, nullptr, ldk, Sp, g->XT.p, nullptr, Np, Np, D <= 64 ? -g->Dcols : g->Dcols, g->Gs.p,
                                     nullptr, grad_split_scratch(g->Gpart, D, Sp), 1);
            }
        }
        ProfScope ps(c, scope);
        launch_jes_finish(c->stream, sc, D, ldo, ldk, eo.sigma, eo.dmu, eo.dsigma, j->a_mu.p, j->a_sg.p, g->Gs.p, j->Go.p,
                          g->gram_direct ? nullptr : g->XsT.p, j->csum.p, g->inv_ell.p, val + s0, grad ? grad + s0 : nullptr);
    }
}

// The JES objective; cov_out (device, may be nullptr): the covariances of every candidate with the optima, [n + k*ldc]
static auto jes_objective(sls_jes* j, double noise_var, double* cov_out, long ldc) {
    return objective(j->gp, j->D, sum_best(j->gp), [=](const double* xr, long ldr, int S, const int*, double* val, double* grad, long ldo) {
        pointset_eval_device(
            j, "jes",
            [&](int sc, int Sp, long ldk, const double* mu, const double* sigma, int, double* v, double* a_mu, double* a_sg, double* H) {
                launch_jes_combine(j->ctx->stream, sc, Sp, ldk, mu, sigma, j->cov.p, j->f_star.p, j->dd.p, j->inv_v.p, j->K, noise_var, v,
                                   a_mu, a_sg, H);
            },
            xr, ldr, S, val, grad, ldo, cov_out, ldc);
    });
}

// the object is what its handle still stands for
static void pointset_check(const char* who, const char* made_by, PointSet* j) {
    SLS_REQUIRE(j->gp->generation == j->generation,
                "%s: the GP handle was refitted, grown or switched in sigma mode since %s (generation %ld, now %ld): create a new object", who,
                made_by, j->generation, j->gp->generation);
}
static void jes_check(const char* who, sls_jes* j) { pointset_check(who, "sls_jes_create", j); }
static void jes_check_noise(const char* who, double noise_var) {
    SLS_REQUIRE(std::isfinite(noise_var) && noise_var > 0.0, "%s: noise_var = %g (finite, > 0)", who, noise_var);
}

// x (D x K on the host) checked finite and clamped into [0,1]^D, as starts are
static std::vector<double> pointset_clamped(const char* who, const char* name, const char* noun, const double* x, int D, int K) {
    std::vector<double> xh((size_t)D * K);
    for (size_t i = 0; i < xh.size(); ++i) {
        SLS_REQUIRE(std::isfinite(x[i]), "%s: %s[%d] of %s %d is not finite", who, name, (int)(i % D), noun, (int)(i / D));
        xh[i] = std::min(1.0, std::max(0.0, x[i]));
    }
    return xh;
}
// The snapshot of K points of a fitted handle (its state lock held): W = K_y^-1 k(X, x_k), mu(x_k), sigma(x_k).  xh stays alive until the
// caller's sync.
static void pointset_snapshot(PointSet* j, sls_gp* g, const std::vector<double>& xh, int K, const char* scope) {
    sls_ctx* c = g->ctx;
    const int D = g->D, N = g->N, Np = g->Np, Kp = round_up(K, 128);
    j->gp = g; j->ctx = c; j->generation = g->generation;
    j->D = D; j->K = K; j->Kp = Kp; j->Np = Np;
    j->W.ensure((size_t)Np * Kp);
    j->xs.ensure((size_t)D * K);
    j->mu_star.ensure(Kp); j->sg_star.ensure(Kp);
    h2d(c, j->xs.p, xh.data(), xh.size());
    {
        ProfScope ps(c, scope);
        // K(X, X*) [i + k*Np] from the raw differences (rows i >= N and columns k >= K exactly 0), then W = K_y^-1 K(X, X*) on the factor
        launch_jes_cross(c->stream, g->X.p, D, 1, N, Np, j->xs.p, D, K, Kp, g->inv_ell.p, KernelSpec{g->kernel, g->a}, j->W.p, nullptr, Np);
        launch_potrs(c->stream, g->L.p, g->Linv.p, Np, j->W.p, Kp);
    }
    // mu, sigma through the tiled evaluation, exactly as sls_gp_predict's tiled route forms them (mean and deviation, no gradient)
    EvalOut eo;
    eo.ldo = Kp;
    eo.mu = j->mu_star.p; eo.sigma = j->sg_star.p;
    eval_candidates(g, j->xs.p, 0, K, eo, true);
}

extern "C" int sls_jes_create(sls_gp* g, const double* x_star, const double* f_star, int K, double star_noise, sls_jes** out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_jes_create: gp is NULL");
    refuse_laplace(g, "sls_jes_create");
    SLS_REQUIRE(out != nullptr, "sls_jes_create: out is NULL");
    *out = nullptr;
    SLS_REQUIRE(K >= 1 && K <= SLS_JES_MAX_OPTIMA, "sls_jes_create: K = %d (1 .. %d)", K, SLS_JES_MAX_OPTIMA);
    SLS_REQUIRE(x_star != nullptr, "sls_jes_create: x_star is NULL");
    SLS_REQUIRE(f_star != nullptr, "sls_jes_create: f_star is NULL");
    SLS_REQUIRE(std::isfinite(star_noise) && star_noise >= 0.0, "sls_jes_create: star_noise = %g (finite, >= 0)", star_noise);
    for (int k = 0; k < K; ++k) SLS_REQUIRE(std::isfinite(f_star[k]), "sls_jes_create: f_star[%d] is not finite", k);
    const std::vector<double> xh = pointset_clamped("sls_jes_create", "x_star", "optimum", x_star, g->D, K);
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    sls_ctx* c = g->ctx;
    std::unique_ptr<sls_jes> j(new sls_jes);
    j->v.ensure(K); j->dd.ensure(K); j->inv_v.ensure(K); j->f_star.ensure(K);
    h2d(c, j->f_star.p, f_star, (size_t)K);
    pointset_snapshot(j.get(), g, xh, K, "jes_setup");
    {
        ProfScope ps(c, "jes_setup");
        launch_jes_optima(c->stream, K, j->mu_star.p, j->sg_star.p, j->f_star.p, star_noise, j->v.p, j->dd.p, j->inv_v.p);
    }
    sync(c);   // the staging vectors go out of scope; nothing but the error state comes back
    slsk::ctx_retain(c);
    *out = j.release();
    SLS_CATCH
}

extern "C" int sls_jes_destroy(sls_jes* j) {
    if (!j) return SLS_OK;
    slsk::note_entry();
    destroy_handle(j);
    return SLS_OK;
}

extern "C" int sls_jes_optima(sls_jes* j, double* mu_star, double* var_star) {
    SLS_TRY
    SLS_REQUIRE(j != nullptr, "sls_jes_optima: j is NULL");
    CtxCall call_(j);
    jes_check("sls_jes_optima", j);
    if (mu_star) d2h(j->ctx, mu_star, j->mu_star.p, (size_t)j->K);
    if (var_star) d2h(j->ctx, var_star, j->v.p, (size_t)j->K);
    sync(j->ctx);
    SLS_CATCH
}

extern "C" int sls_jes_terms(sls_ctx* ctx, const double* t, long n, double* tau, double* dtau) {
    double* const host[2] = {tau, dtau};
    return scalar_terms("sls_jes_terms", ctx, t, n, 2, host,
                        [&](const double* in, long m, double* const* out) { launch_jes_terms(ctx->stream, in, m, out[0], out[1]); });
}

extern "C" int sls_jes_eval(sls_jes* j, double noise_var, const double* Xs, int M, double* val, double* grad, double* cov) {
    SLS_TRY
    SLS_REQUIRE(j != nullptr, "sls_jes_eval: j is NULL");
    CtxCall call_(j);
    SLS_REQUIRE(M >= 0, "sls_jes_eval: M = %d", M);
    jes_check_noise("sls_jes_eval", noise_var);
    jes_check("sls_jes_eval", j);
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Xs != nullptr, "sls_jes_eval: Xs is NULL");
    SLS_REQUIRE(val != nullptr, "sls_jes_eval: val is NULL");
    const int Mp = round_up(M, 128);
    DBuf covd;
    if (cov) covd.ensure((size_t)Mp * j->K);
    eval_points(jes_objective(j, noise_var, covd.p, Mp), Xs, M, val, grad, ExtraBlock{&covd, j->K, cov});
    SLS_CATCH
}

extern "C" int sls_jes_maximize(sls_jes* j, double noise_var, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                                long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars,
                                double* y_stars) {
    SLS_TRY
    SLS_REQUIRE(j != nullptr, "sls_jes_maximize: j is NULL");
    CtxCall call_(j);
    SLS_REQUIRE(starts != nullptr, "sls_jes_maximize: starts is NULL");
    jes_check_noise("sls_jes_maximize", noise_var);
    jes_check("sls_jes_maximize", j);
    maximize_starts("sls_jes_maximize", jes_objective(j, noise_var, nullptr, 0), starts, true, S, n_local, opts, start_index_offset, x_out,
                    val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}

// ---- knowledge gradient on a discrete set (include/sls_hip.h) ---------------------------------------------------------------------
// The snapshot of the K fixed points: the point set (W, x_k, a_k = mu(x_k)) plus a_max and its index.
struct sls_kg : PointSet {
    double a_max = 0.0;
    int arg_max = 0;
};

// The KG objective: joint entropy search's chunk pass around launch_kg_combine; slope_out (device, may be nullptr): the slopes b_k of
// every candidate, [n + k*lds]
static auto kg_objective(sls_kg* k, double noise_var, int include_self, double* slope_out, long lds) {
    return objective(k->gp, k->D, sum_best(k->gp), [=](const double* xr, long ldr, int S, const int*, double* val, double* grad, long ldo) {
        pointset_eval_device(
            k, "kg",
            [&](int sc, int Sp, long ldk, const double* mu, const double* sigma, int s0, double* v, double* a_mu, double* a_sg, double* H) {
                launch_kg_combine(k->ctx->stream, sc, Sp, ldk, mu, sigma, k->cov.p, k->mu_star.p, k->a_max, k->K, noise_var, include_self, v,
                                  a_mu, a_sg, H, slope_out ? slope_out + s0 : nullptr, lds);
            },
            xr, ldr, S, val, grad, ldo, nullptr, 0);
    });
}
static void kg_check_noise(const char* who, double noise_var) {
    SLS_REQUIRE(std::isfinite(noise_var) && noise_var >= 0.0, "%s: noise_var = %g (finite, >= 0)", who, noise_var);
}

extern "C" int sls_kg_create(sls_gp* g, const double* x_ref, int K, sls_kg** out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_kg_create: gp is NULL");
    refuse_laplace(g, "sls_kg_create");
    SLS_REQUIRE(out != nullptr, "sls_kg_create: out is NULL");
    *out = nullptr;
    SLS_REQUIRE(K >= 1 && K <= SLS_KG_MAX_POINTS, "sls_kg_create: K = %d (1 .. %d)", K, SLS_KG_MAX_POINTS);
    SLS_REQUIRE(x_ref != nullptr, "sls_kg_create: x_ref is NULL");
    const std::vector<double> xh = pointset_clamped("sls_kg_create", "x_ref", "point", x_ref, g->D, K);
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    sls_ctx* c = g->ctx;
    std::unique_ptr<sls_kg> k(new sls_kg);
    pointset_snapshot(k.get(), g, xh, K, "kg_setup");
    std::vector<double> a(K);
    d2h(c, a.data(), k->mu_star.p, (size_t)K);
    sync(c);
    k->a_max = a[0];
    for (int i = 1; i < K; ++i)
        if (a[i] > k->a_max) { k->a_max = a[i]; k->arg_max = i; }   // the lowest index wins ties
    slsk::ctx_retain(c);
    *out = k.release();
    SLS_CATCH
}

extern "C" int sls_kg_destroy(sls_kg* k) {
    if (!k) return SLS_OK;
    slsk::note_entry();
    destroy_handle(k);
    return SLS_OK;
}

extern "C" int sls_kg_points(sls_kg* k, double* mu_ref, double* mu_max, int* arg_max) {
    SLS_TRY
    SLS_REQUIRE(k != nullptr, "sls_kg_points: k is NULL");
    CtxCall call_(k);
    pointset_check("sls_kg_points", "sls_kg_create", k);
    if (mu_ref) d2h(k->ctx, mu_ref, k->mu_star.p, (size_t)k->K);
    if (mu_max) *mu_max = k->a_max;
    if (arg_max) *arg_max = k->arg_max;
    sync(k->ctx);
    SLS_CATCH
}

extern "C" int sls_kg_eval(sls_kg* k, double noise_var, int include_self, const double* Xs, int M, double* val, double* grad,
                           double* slope) {
    SLS_TRY
    SLS_REQUIRE(k != nullptr, "sls_kg_eval: k is NULL");
    CtxCall call_(k);
    SLS_REQUIRE(M >= 0, "sls_kg_eval: M = %d", M);
    kg_check_noise("sls_kg_eval", noise_var);
    pointset_check("sls_kg_eval", "sls_kg_create", k);
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Xs != nullptr, "sls_kg_eval: Xs is NULL");
    SLS_REQUIRE(val != nullptr, "sls_kg_eval: val is NULL");
    const int Mp = round_up(M, 128);
    DBuf sld;
    if (slope) sld.ensure((size_t)Mp * k->K);
    eval_points(kg_objective(k, noise_var, include_self != 0, sld.p, Mp), Xs, M, val, grad, ExtraBlock{&sld, k->K, slope});
    SLS_CATCH
}

extern "C" int sls_kg_maximize(sls_kg* k, double noise_var, int include_self, const double* starts, int S, int n_local,
                               const sls_lbfgs_opts* opts, long start_index_offset, double* x_out, double* val_out, long* idx_out,
                               double* x_stars, double* y_stars) {
    SLS_TRY
    SLS_REQUIRE(k != nullptr, "sls_kg_maximize: k is NULL");
    CtxCall call_(k);
    SLS_REQUIRE(starts != nullptr, "sls_kg_maximize: starts is NULL");
    kg_check_noise("sls_kg_maximize", noise_var);
    pointset_check("sls_kg_maximize", "sls_kg_create", k);
    maximize_starts("sls_kg_maximize", kg_objective(k, noise_var, include_self != 0, nullptr, 0), starts, true, S, n_local, opts,
                    start_index_offset, x_out, val_out, idx_out, x_stars, y_stars);
    SLS_CATCH
}

// The combiner alone on caller-supplied lines (a test hook): M candidates at a time in blocks of at most 4096.
extern "C" int sls_kg_lines(sls_ctx* ctx, const double* a, const double* B, const double* a_self, const double* b_self, int K, int M,
                            double* val, double* beta, double* prob, double* self_out) {
    SLS_TRY
    CtxCall call_(ctx);
    SLS_REQUIRE(ctx != nullptr, "sls_kg_lines: ctx is NULL");
    SLS_REQUIRE(K >= 1 && K <= SLS_KG_MAX_POINTS, "sls_kg_lines: K = %d (1 .. %d)", K, SLS_KG_MAX_POINTS);
    SLS_REQUIRE(M >= 0, "sls_kg_lines: M = %d", M);
    SLS_REQUIRE((a_self == nullptr) == (b_self == nullptr), "sls_kg_lines: a_self and b_self go together");
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(a != nullptr && B != nullptr, "sls_kg_lines: a or B is NULL");
    SLS_REQUIRE(val != nullptr, "sls_kg_lines: val is NULL");
    SLS_REQUIRE(self_out == nullptr || a_self != nullptr, "sls_kg_lines: self_out without a self line");
    for (int k = 0; k < K; ++k) SLS_REQUIRE(std::isfinite(a[k]), "sls_kg_lines: a[%d] is not finite", k);
    for (size_t i = 0; i < (size_t)M * K; ++i) SLS_REQUIRE(std::isfinite(B[i]), "sls_kg_lines: B[%zu] is not finite", i);
    for (int m = 0; a_self && m < M; ++m)
        SLS_REQUIRE(std::isfinite(a_self[m]) && std::isfinite(b_self[m]), "sls_kg_lines: the self line of candidate %d is not finite", m);
    SLS_HIP(hipSetDevice(ctx->device));
    const double a_max = *std::max_element(a, a + K);
    const size_t MK = (size_t)M * K;
    DBuf buf;
    buf.ensure((size_t)K + 3 * MK + 5 * (size_t)M);
    double *ad = buf.p, *Bd = ad + K, *betad = Bd + MK, *probd = betad + MK, *asd = probd + MK, *bsd = asd + M, *vald = bsd + M,
           *spi = vald + M, *sbeta = spi + M;
    h2d(ctx, ad, a, (size_t)K);
    h2d(ctx, Bd, B, MK);
    if (a_self) {
        h2d(ctx, asd, a_self, (size_t)M);
        h2d(ctx, bsd, b_self, (size_t)M);
    }
    {
        ProfScope ps(ctx, "kg");
        launch_kg_lines(ctx->stream, M, M, ad, a_max, Bd, K, a_self ? asd : nullptr, a_self ? bsd : nullptr, vald, beta ? betad : nullptr,
                        prob ? probd : nullptr, self_out ? spi : nullptr, self_out ? sbeta : nullptr);
    }
    d2h(ctx, val, vald, (size_t)M);
    if (beta) d2h(ctx, beta, betad, MK);
    if (prob) d2h(ctx, prob, probd, MK);
    if (self_out) {
        d2h(ctx, self_out, sbeta, (size_t)M);
        d2h(ctx, self_out + M, spi, (size_t)M);
    }
    sync(ctx);
    SLS_CATCH
}

// ---- maximisation over affine subspaces (include/sls_hip.h) --------------------------------------------------------------
// Any objective in the D variables of a handle as one in the d variables z of x = c + A z (sub_eval, sub_maps.hpp, over the handle's
// blocks sub_x / sub_gx).  Never the one-launch search: its kernel knows no maps.
template <class Obj>
static auto sub_objective(const Obj& f, const SubMaps& m) {
    sls_gp* g = f.g;
    return objective(g, m.d, f.best, [=](const double* z, long ld, int n, const int* live, double* val, double* grad_z, long) {
        sub_eval(g->ctx, m, g->sub_x, g->sub_gx, z, ld, n, live, grad_z,
                 [&](const double* x, double* gx) { f.eval(x, ld, n, nullptr, val, gx, ld); });
    });
}

// The body of sls_acq_eval_sub and sls_mes_eval_sub (M >= 1): Z is d x M on the host; results to the caller's arrays, X_out from the
// expanded points.
template <class Obj>
static void eval_sub_points(const char* who, const Obj& f, const sls_submaps* maps, const double* Z, int M, double* val, double* grad_z,
                            double* X_out) {
    sls_gp* g = f.g;
    SubMapsDev up;
    upload_sub_maps(who, g->ctx, maps, g->D, M, up);
    eval_points(sub_objective(f, up.m), Z, M, val, grad_z, ExtraBlock{&g->sub_x, g->D, X_out, true});
}

// The body of sls_acq_maximize_sub and sls_mes_maximize_sub: the shared maximiser in the d variables -- the step kernels see z in
// [0,1]^d and nothing else --, then one more expand launch for the points of the end variables.
template <class Obj>
static void maximize_sub(const char* who, const Obj& f, const sls_submaps* maps, const double* starts_z, int S, int n_local,
                         const sls_lbfgs_opts* opts_in, long off, double* z_out, double* x_out, double* val_out, long* idx_out,
                         double* z_stars, double* x_stars, double* y_stars) {
    sls_gp* g = f.g;
    sls_ctx* c = g->ctx;
    SLS_REQUIRE(S >= 1, "%s: need S >= 1 (S = %d)", who, S);
    SubMapsDev up;
    upload_sub_maps(who, c, maps, g->D, S, up);
    const long winner = maximize_starts(who, sub_objective(f, up.m), starts_z, true, S, n_local, opts_in, off, z_out, val_out, idx_out,
                                        z_stars, y_stars);
    if (!x_out && !x_stars) return;
    const int D = g->D;
    const long ld = round_up(S, 128);
    g->sub_x.ensure((size_t)D * ld);
    sub_expand(c, up.m, S, nullptr, g->lb.x.p, ld, g->sub_x.p, ld);
    std::vector<double> pageable;
    const double* xs = fetch(g, g->sub_x.p, (size_t)D * ld, pageable);
    if (x_out)
        for (int rr = 0; rr < D; ++rr) x_out[rr] = xs[(size_t)winner + (size_t)rr * ld];
    cm_to_host(xs, ld, D, S, x_stars);
}

extern "C" int sls_acq_eval_sub(sls_gp* g, int acq_type, double ucb_h, const sls_submaps* maps, const double* Z, int M, double* val,
                                double* grad_z, double* X_out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && M >= 0, "sls_acq_eval_sub: bad argument");
    const auto f = acq_objective(g, nullptr, acq_type, ucb_h);
    if (M == 0) return SLS_OK;
    SLS_REQUIRE(Z != nullptr, "sls_acq_eval_sub: Z is NULL");
    eval_sub_points("sls_acq_eval_sub", f, maps, Z, M, val, grad_z, X_out);
    SLS_CATCH
}

extern "C" int sls_acq_maximize_sub(sls_gp* g, int acq_type, double ucb_h, const sls_submaps* maps, const double* starts_z, int S,
                                    int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* z_out, double* x_out,
                                    double* val_out, long* idx_out, double* z_stars, double* x_stars, double* y_stars) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && starts_z, "sls_acq_maximize_sub: NULL argument");
    maximize_sub("sls_acq_maximize_sub", acq_objective(g, nullptr, acq_type, ucb_h), maps, starts_z, S, n_local, opts, start_index_offset,
                 z_out, x_out, val_out, idx_out, z_stars, x_stars, y_stars);
    SLS_CATCH
}

extern "C" int sls_mes_eval_sub(sls_gp* g, const double* y_star, int K, const sls_submaps* maps, const double* Z, int M, double* val,
                                double* grad_z, double* X_out) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_mes_eval_sub: gp is NULL");
    SLS_REQUIRE(M >= 0, "sls_mes_eval_sub: M = %d", M);
    DBuf ys;
    const auto f = mes_objective("sls_mes_eval_sub", g, y_star, K, ys);
    if (M == 0) {
        sync(g->ctx);
        return SLS_OK;
    }
    SLS_REQUIRE(Z != nullptr, "sls_mes_eval_sub: Z is NULL");
    SLS_REQUIRE(val != nullptr, "sls_mes_eval_sub: val is NULL");
    eval_sub_points("sls_mes_eval_sub", f, maps, Z, M, val, grad_z, X_out);
    SLS_CATCH
}

extern "C" int sls_mes_maximize_sub(sls_gp* g, const double* y_star, int K, const sls_submaps* maps, const double* starts_z, int S,
                                    int n_local, const sls_lbfgs_opts* opts, long start_index_offset, double* z_out, double* x_out,
                                    double* val_out, long* idx_out, double* z_stars, double* x_stars, double* y_stars) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_mes_maximize_sub: gp is NULL");
    SLS_REQUIRE(starts_z != nullptr, "sls_mes_maximize_sub: starts_z is NULL");
    DBuf ys;
    maximize_sub("sls_mes_maximize_sub", mes_objective("sls_mes_maximize_sub", g, y_star, K, ys), maps, starts_z, S, n_local, opts,
                 start_index_offset, z_out, x_out, val_out, idx_out, z_stars, x_stars, y_stars);
    SLS_CATCH
}

// ---- expected utility of the best option of a query pair (include/sls_hip.h) -----------------------------------------
// pairs per pass: half the candidate chunk (two cross-covariance blocks per pair), so the workspace stays at what a single-point
// acquisition uses at the same chunk setting
static int eubo_pairs_per_pass(const sls_ctx* c) { return std::max(128, c->cand_chunk / 2 / 128 * 128); }

static void ensure_eubo_ws(sls_gp* g, int chunk) {
    ensure_eval_ws(g, chunk);   // option x: the handle's own blocks
    if (chunk <= g->eubo_chunk && g->eubo_np == g->Np) return;
    const size_t Np = g->Np, C = std::max(chunk, g->eubo_np == g->Np ? g->eubo_chunk : 0);
    const size_t nbt = Np / 128;
    g->eubo_Ks.ensure(C * Np);
    if (g->kernel == SLS_KERNEL_ARD_MATERN52) g->eubo_Cs.ensure(C * Np);
    g->eubo_Kd.ensure(C * Np);
    g->eubo_parts.ensure(6 * nbt * C);   // mu, ca: one per row tile; kw (not used), cw: one per half row tile
    g->eubo_Gs.ensure(C * g->Dcols);
    g->eubo_Gm.ensure(C * g->Dcols);
    g->eubo_XsT.ensure(C * g->Dcols);
    g->eubo_ns.ensure(C);
    g->eubo_chunk = (int)C;
    g->eubo_np = g->Np;
}

// EUBO (+ its 2D gradient, grad may be NULL) at S pairs, candidate-major raw coordinates xr[n + r*ldr]: rows 0..D-1 the option x,
// rows D..2D-1 the option x'.  val / grad candidate-major with leading dimension ldo (grad: 2D rows).  Always the tiled kernels;
// the gradient products are formed whether or not grad is asked for (the guard looks at them).
static void eval_pairs(sls_gp* g, const double* xr, long ldr, int S, double* val, double* grad, long ldo) {
    sls_ctx* c = g->ctx;
    const int Np = g->Np, N = g->N, D = g->D;
    const int chunk_max = std::min(round_up(S, 128), eubo_pairs_per_pass(c));
    ensure_eubo_ws(g, chunk_max);
    const int nbt = Np / 128;
    const bool matern = g->kernel == SLS_KERNEL_ARD_MATERN52;
    const bool solve = g->sigma_mode == 1;
    if (solve) g->Vs.ensure((size_t)chunk_max * Np);
    KernelSpec ks{g->kernel, g->a};
    for (int s0 = 0; s0 < S; s0 += chunk_max) {
        const int sc = std::min(chunk_max, S - s0);
        const int Sp = round_up(sc, 128);
        const long ldk = Sp;
        double* Ks[2] = {g->Ks.p, g->eubo_Ks.p};
        double* Cs[2] = {matern ? g->Cs.p : g->Ks.p, matern ? g->eubo_Cs.p : g->eubo_Ks.p};
        double* XsT[2] = {g->XsT.p, g->eubo_XsT.p};
        double* ns[2] = {g->ns.p, g->eubo_ns.p};
        double* Gs[2] = {g->Gs.p, g->eubo_Gs.p};
        double* Gm[2] = {g->Gm.p, g->eubo_Gm.p};
        double* mu_part[2] = {g->parts.p, g->eubo_parts.p};
        double *ca_part[2], *kw_part[2], *cw_part[2];
        for (int o = 0; o < 2; ++o) {
            ca_part[o] = mu_part[o] + (size_t)nbt * ldk;
            kw_part[o] = ca_part[o] + (size_t)nbt * ldk;
            cw_part[o] = kw_part[o] + (size_t)2 * nbt * ldk;
        }
        double* kw_solve = solve ? cw_part[0] + (size_t)2 * nbt * ldk : nullptr;   // the handle's parts block has 10 nbt rows
        for (int o = 0; o < 2; ++o) {
            ProfScope ps(c, "cross_gram");
            launch_prep_cands(c->stream, xr + (size_t)o * D * ldr + s0, ldr, D, sc, g->inv_ell.p, XsT[o], ldk, Sp, g->Dcols, ns[o]);
            if (g->gram_direct)
                launch_cross_gram_direct(c->stream, xr + (size_t)o * D * ldr + s0, 1, ldr, sc, Sp, g->X.p, D, g->inv_ell.p, Np, N, ks,
                                         g->alpha.p, Ks[o], Cs[o], ldk, mu_part[o], ca_part[o]);
            else
                launch_cross_gram(c->stream, XsT[o], ldk, ns[o], Sp, g->XT.p, Np, g->nx.p, Np, N, g->Dp, ks, g->alpha.p, Ks[o], Cs[o], ldk,
                                  mu_part[o], ca_part[o]);
        }
        {
            ProfScope ps(c, "eubo");
            launch_pair_diff(c->stream, Ks[0], Ks[1], ldk, Np, g->eubo_Kd.p);
        }
        if (solve) {
            // w = K_y^-1 d as L^-T (L^-1 d): V = Kd L^-T once, then the tile kernel with (L^-1)^T in the place of K^-1 (eval_candidates'
            // solve_grad branch); d^T K_y^-1 d = |L^-1 d|^2 from the triangular contraction
            {
                ProfScope ps(c, "acq_gemm");
                launch_gemm_plain(c->stream, g->eubo_Kd.p, ldk, false, g->Linv.p, Np, false, g->Vs.p, ldk, Sp / 128, Np / 128, Np, 1.0, 0.0);
            }
            ProfScope ps(c, "var_gemm");
            launch_var_gemm(c->stream, g->eubo_Kd.p, ldk, Sp, g->Linv.p, Np, kw_solve, kw_solve + (size_t)2 * nbt * ldk);
        }
        int split_first = 0x7fffffff;
        for (int o = 0; o < 2; ++o) {
            {
                // P = C*_o .* W and the c_o . w sums; Cs is never the first operand here, so the tile kernel also forms d . w
                ProfScope ps(c, "acq_gemm");
                split_first = launch_acq_gemm(c->stream, solve ? g->Vs.p : g->eubo_Kd.p, Cs[o], ldk, Sp, solve ? g->U.p : g->Kinv.p, Np,
                                              g->P.p, kw_part[o], cw_part[o], c->d_info + 32);
            }
            ProfScope ps(c, "grad_gemm");
            if (g->gram_direct) {   // as in eval_candidates
                launch_grad_direct(c->stream, g->P.p, Cs[o], ldk, Sp, xr + (size_t)o * D * ldr + s0, 1, ldr, sc, g->X.p, D, g->inv_ell.p, N,
                                   g->alpha.p, Gs[o], Gm[o]);
                SLS_HIP(hipMemsetAsync(ca_part[o], 0, (size_t)nbt * ldk * 8, c->stream));
                SLS_HIP(hipMemsetAsync(cw_part[o], 0, (size_t)2 * nbt * ldk * 8, c->stream));
                continue;
            }
            launch_grad_gemm(c->stream, g->P.p, Cs[o], ldk, Sp, g->XT.p, g->XaT.p, Np, Np, D <= 64 ? -g->Dcols : g->Dcols, Gs[o], Gm[o],
                             grad_split_scratch(g->Gpart, D, Sp));
        }
        {
            ProfScope ps(c, "eubo");
            EuboFinalizeArgs f;
            f.S = sc; f.D = D; f.nbt = nbt; f.ntm = Sp / 128; f.split_first = split_first; f.kernel = g->kernel; f.ldk = ldk;
            for (int o = 0; o < 2; ++o) {
                f.mu_part[o] = mu_part[o]; f.ca_part[o] = ca_part[o]; f.cw_part[o] = cw_part[o];
                f.Gs[o] = Gs[o]; f.Gm[o] = Gm[o]; f.XsT[o] = XsT[o];
            }
            f.kw_part = kw_part[0]; f.kw_solve_part = kw_solve; f.inv_ell = g->inv_ell.p; f.a = g->a;
            if (g->gram_direct) {   // the pair's own prior covariance from the raw coordinate differences as well
                for (int o = 0; o < 2; ++o) f.xr[o] = xr + (size_t)o * D * ldr + s0;
                f.ldr = ldr;
            }
            f.ldo = ldo;
            f.val = val ? val + s0 : nullptr;
            f.grad = grad ? grad + s0 : nullptr;
            launch_eubo_finalize(c->stream, f);
        }
    }
}

// The pair objective over [0,1]^(2D): every block sized by the number of variables is sized for 2D (the optimiser's workspace, the
// downloads, and the mapped block of the best start, which sls_eubo_maximize ensures); the handle's own sizes stay as they are
static auto eubo_objective(sls_gp* g) {
    return objective(g, 2 * g->D, BestBlock{g->eubo_best.dev, g->eubo_best.host, false},
                     [=](const double* xr, long ldr, int n, const int*, double* val, double* grad, long ldo) {
                         eval_pairs(g, xr, ldr, n, val, grad, ldo);   // the block of x' is xr + D ldr
                     });
}

extern "C" int sls_eubo_eval(sls_gp* g, const double* pairs, int M, double* val, double* grad) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_eubo_eval: gp is NULL");
    refuse_laplace(g, "sls_eubo_eval");
    SLS_REQUIRE(pairs != nullptr, "sls_eubo_eval: pairs is NULL");
    SLS_REQUIRE(M >= 0, "sls_eubo_eval: M = %d", M);
    if (M == 0) return SLS_OK;
    eval_points(eubo_objective(g), pairs, M, val, grad);
    SLS_CATCH
}

extern "C" int sls_eubo_maximize(sls_gp* g, const double* starts, int S, int n_local, const sls_lbfgs_opts* opts,
                                 long start_index_offset, double* x_out, double* val_out, long* idx_out, double* x_stars,
                                 double* y_stars) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g != nullptr, "sls_eubo_maximize: gp is NULL");
    refuse_laplace(g, "sls_eubo_maximize");
    SLS_REQUIRE(starts != nullptr, "sls_eubo_maximize: starts is NULL");
    g->eubo_best.ensure(g->ctx, (size_t)(8 + 2 * g->D) * sizeof(double), true);
    maximize_starts("sls_eubo_maximize", eubo_objective(g), starts, true, S, n_local, opts, start_index_offset, x_out, val_out, idx_out,
                    x_stars, y_stars);
    SLS_CATCH
}

// ---- free functions ----------------------------------------------------------------------------------------------
extern "C" int sls_gram(sls_ctx* c, const double* X, int D, int N, const double* theta, double b, int kernel, double* K_out) {
    SLS_TRY
    CtxCall call_(c);
    SLS_REQUIRE(c && X && K_out && D >= 1 && N >= 1, "sls_gram: bad argument");
    check_theta(theta, D);
    SLS_HIP(hipSetDevice(c->device));
    const int Np = round_up(N, 128), Dp = round_up(D, 16);
    DBuf Xd, il, XT, nx, K;
    Xd.ensure((size_t)D * N); il.ensure(Dp); XT.ensure((size_t)Np * Dp); nx.ensure(Np); K.ensure((size_t)Np * Np);
    std::vector<double> ilh(Dp, 0.0);
    for (int d = 0; d < D; ++d) ilh[d] = 1.0 / theta[1 + d];
    h2d(c, Xd.p, X, (size_t)D * N);
    h2d(c, il.p, ilh.data(), Dp);
    launch_prep_points(c->stream, Xd.p, D, N, il.p, XT.p, Np, Np, Dp, nx.p);
    // the entries themselves are the result here: the expansion serves them only while it is as good as the direct form (kernels.hpp)
    if (gram_direct_form(theta + 1, D, gram_entry_bound(D))) launch_gram_sym_direct(c->stream, Xd.p, D, il.p, Np, N, KernelSpec{kernel, theta[0]}, b, K.p, false);
    else launch_gram_sym(c->stream, XT.p, Np, Dp, nx.p, Np, N, KernelSpec{kernel, theta[0]}, b, K.p, false);
    d2h_matrix(c, K_out, K.p, N, Np);
    sync(c);
    SLS_CATCH
}

extern "C" int sls_gram_cross(sls_ctx* c, const double* X, int D, int N, const double* Xs, int M, const double* theta, int kernel,
                              double* Ks_out) {
    SLS_TRY
    CtxCall call_(c);
    SLS_REQUIRE(c && X && Xs && Ks_out && D >= 1 && N >= 1 && M >= 1, "sls_gram_cross: bad argument");
    check_theta(theta, D);
    SLS_HIP(hipSetDevice(c->device));
    const int Np = round_up(N, 128), Mp = round_up(M, 128), Dp = round_up(D, 16);
    DBuf Xd, Xsd, il, XT, XsT, nx, ns, Ks, Cs;
    Xd.ensure((size_t)D * N); Xsd.ensure((size_t)D * M); il.ensure(Dp);
    XT.ensure((size_t)Np * Dp); XsT.ensure((size_t)Mp * Dp); nx.ensure(Np); ns.ensure(Mp);
    Ks.ensure((size_t)Mp * Np);
    const bool matern = kernel == SLS_KERNEL_ARD_MATERN52;
    if (matern) Cs.ensure((size_t)Mp * Np);
    std::vector<double> ilh(Dp, 0.0);
    for (int d = 0; d < D; ++d) ilh[d] = 1.0 / theta[1 + d];
    h2d(c, Xd.p, X, (size_t)D * N);
    h2d(c, Xsd.p, Xs, (size_t)D * M);
    h2d(c, il.p, ilh.data(), Dp);
    launch_prep_points(c->stream, Xd.p, D, N, il.p, XT.p, Np, Np, Dp, nx.p);
    launch_prep_points(c->stream, Xsd.p, D, M, il.p, XsT.p, Mp, Mp, Dp, ns.p);
    if (gram_direct_form(theta + 1, D, gram_entry_bound(D)))
        launch_cross_gram_direct(c->stream, Xsd.p, D, 1, M, Mp, Xd.p, D, il.p, Np, N, KernelSpec{kernel, theta[0]}, nullptr, Ks.p,
                                 matern ? Cs.p : Ks.p, Mp, nullptr, nullptr);
    else
        launch_cross_gram(c->stream, XsT.p, Mp, ns.p, Mp, XT.p, Np, nx.p, Np, N, Dp, KernelSpec{kernel, theta[0]}, nullptr, Ks.p,
                          matern ? Cs.p : Ks.p, Mp, nullptr, nullptr);
    // device image is candidate-major [m + i*Mp]; the API returns N x M column-major (column m = k(xs_m, X))
    std::vector<double> t((size_t)Mp * Np);
    d2h(c, t.data(), Ks.p, (size_t)Mp * Np);
    sync(c);
    for (int m = 0; m < M; ++m)
        for (int i = 0; i < N; ++i) Ks_out[i + (size_t)m * N] = t[(size_t)m + (size_t)i * Mp];
    SLS_CATCH
}

static void upload_padded_spd(sls_ctx* c, DBuf& A, const double* src, int N, int Np) {
    A.ensure((size_t)Np * Np);
    launch_fill(c->stream, A.p, (long)Np * Np, 0.0);
    h2d_matrix(c, A.p, src, N, Np);
    if (Np > N) {
        std::vector<double> ones(Np - N, 1.0);
        SLS_HIP(hipMemcpy2DAsync(A.p + (size_t)N * (Np + 1), (size_t)(Np + 1) * 8, ones.data(), 8, 8, Np - N,
                                 hipMemcpyHostToDevice, c->stream));
        sync(c);
    }
}

extern "C" int sls_potrf(sls_ctx* c, double* A, int N) {
    SLS_TRY
    CtxCall call_(c);
    SLS_REQUIRE(c && A && N >= 1, "sls_potrf: bad argument");
    SLS_HIP(hipSetDevice(c->device));
    const int Np = round_up(N, 128);
    DBuf Ad, Li;
    Li.ensure((size_t)Np * Np);
    int info2[2] = {0, 0};
    std::vector<double> out((size_t)N * N);
    for (int attempt = 0;; ++attempt) {
        upload_padded_spd(c, Ad, A, N, Np);
        SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
        c->potrf_tick_rearm();
        launch_potrf(c->stream, Ad.p, Np, Li.p, c->d_info, 0, c->potrf_df_sync(Np));
        launch_zero_upper(c->stream, Ad.p, Np);
        SLS_HIP(hipMemcpyAsync(info2, c->d_info, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        d2h_matrix(c, out.data(), Ad.p, N, Np);
        sync(c);
        if (!potrf_gave_up(c, info2[1], attempt)) break;
    }
    std::copy(out.begin(), out.end(), A);
    const int info = info2[0];
    if (info != 0) {
        set_error("sls_potrf: matrix is not positive definite (pivot %d)", info - 1);
        return SLS_ERR_NOT_SPD;
    }
    SLS_CATCH
}

extern "C" int sls_potrs(sls_ctx* c, const double* L, int N, double* B, int nrhs) {
    SLS_TRY
    CtxCall call_(c);
    SLS_REQUIRE(c && L && B && N >= 1 && nrhs >= 1, "sls_potrs: bad argument");
    SLS_HIP(hipSetDevice(c->device));
    const int Np = round_up(N, 128), Rp = round_up(nrhs, 128);
    DBuf Ld, Li, Bd;
    upload_padded_spd(c, Ld, L, N, Np);
    launch_zero_upper(c->stream, Ld.p, Np);
    Li.ensure((size_t)Np * Np);
    launch_diag_inverse(c->stream, Ld.p, Np, Li.p);
    Bd.ensure((size_t)Np * Rp);
    launch_fill(c->stream, Bd.p, (long)Np * Rp, 0.0);
    SLS_HIP(hipMemcpy2DAsync(Bd.p, (size_t)Np * 8, B, (size_t)N * 8, (size_t)N * 8, nrhs, hipMemcpyHostToDevice, c->stream));
    launch_potrs(c->stream, Ld.p, Li.p, Np, Bd.p, Rp);
    SLS_HIP(hipMemcpy2DAsync(B, (size_t)N * 8, Bd.p, (size_t)Np * 8, (size_t)N * 8, nrhs, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    SLS_CATCH
}

extern "C" int sls_potri(sls_ctx* c, const double* L, int N, double* Ainv) {
    SLS_TRY
    CtxCall call_(c);
    SLS_REQUIRE(c && L && Ainv && N >= 1, "sls_potri: bad argument");
    SLS_HIP(hipSetDevice(c->device));
    const int Np = round_up(N, 128);
    DBuf Ld, Li, Ki, Ui;
    upload_padded_spd(c, Ld, L, N, Np);
    launch_zero_upper(c->stream, Ld.p, Np);
    Li.ensure((size_t)Np * Np);
    Ki.ensure((size_t)Np * Np);
    Ui.ensure((size_t)Np * Np);
    launch_fill(c->stream, Li.p, (long)Np * Np, 0.0);
    launch_diag_inverse(c->stream, Ld.p, Np, Li.p);
    launch_trtri(c->stream, Ld.p, Np, Li.p, Ki.p, Ui.p);
    launch_lauum(c->stream, Ui.p, Np, Ki.p);
    d2h_matrix(c, Ainv, Ki.p, N, Np);
    sync(c);
    SLS_CATCH
}

// Leave-one-out predictions of the fitted handle at its own hyper-parameters and data (kernels_loo.hip): closed forms in
// diag(K_y^-1) and alpha, both part of the fitted state.  Explicit-inverse mode: the diagonal of Kinv; Cholesky-solve mode:
// d_i = sum_k (L^-1)_ki^2 from the factor's inverse, the matrix that mode predicts with.
extern "C" int sls_gp_loo(sls_gp* g, double* loo_mu, double* loo_var, double* loo_logp) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g, "sls_gp_loo: NULL handle");
    refuse_laplace(g, "sls_gp_loo");
    std::shared_lock<std::shared_mutex> state_(g->state_mtx);
    sls_ctx* c = g->ctx;
    const int N = g->N, Np = g->Np;
    DBuf ws;   // pooled: five vectors of the terms, d, and the sum
    ws.ensure((size_t)6 * Np + 8);
    double* v = ws.p;
    double* dvec = v + (size_t)5 * Np;
    {
        ProfScope ps(c, "loo_terms");
        if (g->sigma_mode == 1) {
            launch_loo_diag_linv(c->stream, g->Linv.p, Np, N, dvec);
            launch_loo_terms(c->stream, dvec, 1, g->alpha.p, g->y.p, Np, N, v, v + Np, v + 2 * (size_t)Np, v + 3 * (size_t)Np,
                             v + 4 * (size_t)Np, dvec + Np);
        } else {
            launch_loo_terms(c->stream, g->Kinv.p, (long)Np + 1, g->alpha.p, g->y.p, Np, N, v, v + Np, v + 2 * (size_t)Np,
                             v + 3 * (size_t)Np, v + 4 * (size_t)Np, dvec + Np);
        }
    }
    if (loo_mu) d2h(c, loo_mu, v, N);
    if (loo_var) d2h(c, loo_var, v + Np, N);
    if (loo_logp) d2h(c, loo_logp, v + 2 * (size_t)Np, N);
    sync(c);
    SLS_CATCH
}

// Grow the fitted state by one observation in O(N^2): Schur-complement update of K^-1, one new row of L and L^-1,
// alpha, mu at the data points, arg max and log-determinant.  Replaces the full refit of the dummy regressor in
// FindNextPoints (src/acquisition-function.cpp:280-293).  When N is a multiple of 128 the padded buffers are full and
// the handle is rebuilt from scratch on the device instead (same results).
extern "C" int sls_gp_append_point(sls_gp* g, const double* x, double y_new) {
    SLS_TRY
    CtxCall call_(g);
    SLS_REQUIRE(g && x, "sls_gp_append_point: NULL argument");
    refuse_laplace(g, "sls_gp_append_point");
    std::unique_lock<std::shared_mutex> state_(g->state_mtx);   // ends with gp_fetch_summary's synchronisation: the state is complete
    sls_ctx* c = g->ctx;
    const int D = g->D, N = g->N, Np = g->Np;
    if (g->host_stale) {   // the device copies are authoritative after sls_gp_refit_dev
        d2h(c, g->Xh.data(), g->X.p, (size_t)D * N);
        d2h(c, g->yh.data(), g->y.p, (size_t)N);
        sync(c);
        g->host_stale = false;
    }
    g->Xh.insert(g->Xh.end(), x, x + D);
    g->yh.push_back(y_new);
    if (N % 128 == 0) {
        gp_setup(g);   // buffers full: re-size with one more 128-block and refit on the device
        return SLS_OK;
    }
    // candidate-major upload of the single point, cross covariances k = k(X, x) through the regular evaluation kernels
    upload_candidates(g, x, D, 1, 128);
    ensure_eval_ws(g, 128);
    g->outv.ensure(4 * (size_t)Np + 8);
    double* kvec = g->outv.p;            // k (Np, strided copy of Ks row 0)
    double* uvec = kvec + Np;
    double* lvec = uvec + Np;
    double* tmp = lvec + Np;
    double* scal = tmp + Np;
    KernelSpec ks{g->kernel, g->a};
    launch_prep_cands(c->stream, g->raw.p, 128, D, 1, g->inv_ell.p, g->XsT.p, 128, 128, g->Dcols, g->ns.p);
    double* Cs = (g->kernel == SLS_KERNEL_ARD_MATERN52) ? g->Cs.p : g->Ks.p;
    if (g->gram_direct)
        launch_cross_gram_direct(c->stream, g->raw.p, 1, 128, 1, 128, g->X.p, D, g->inv_ell.p, Np, N, ks, nullptr, g->Ks.p, Cs, 128, nullptr,
                                 nullptr);
    else
        launch_cross_gram(c->stream, g->XsT.p, 128, g->ns.p, 128, g->XT.p, Np, g->nx.p, Np, N, g->Dp, ks, nullptr, g->Ks.p, Cs, 128,
                          nullptr, nullptr);
    // Ks[n + i*128], n = 0 -> stride-128 gather into a dense vector (padding rows i >= N are 0)
    SLS_HIP(hipMemcpy2DAsync(kvec, 8, g->Ks.p, 128 * 8, 8, Np, hipMemcpyDeviceToDevice, c->stream));
    launch_gemv_n(c->stream, g->Kinv.p, Np, kvec, uvec, g->gemv_part.p);     // u = K^-1 k   (padding: identity block x 0 = 0)
    launch_gemv_n(c->stream, g->Linv.p, Np, kvec, lvec, g->gemv_part.p, true);     // l = L^-1 k
    launch_append_dots(c->stream, kvec, uvec, lvec, g->y.p, N, scal);
    const double kappa = g->a + g->b;
    launch_append_update(c->stream, g->Kinv.p, g->L.p, g->Linv.p, g->alpha.p, Np, N, uvec, lvec, scal, kappa, y_new);
    // new training point joins X, y, the scaled copies and the hoisted quantities
    SLS_HIP(hipMemcpyAsync(g->y.p + N, &g->yh[N], 8, hipMemcpyHostToDevice, c->stream));
    g->X.ensure((size_t)D * (N + 1));   // may reallocate: refill from the host copy
    SLS_HIP(hipMemcpyAsync(g->X.p, g->Xh.data(), (size_t)D * (N + 1) * 8, hipMemcpyHostToDevice, c->stream));
    g->N = N + 1;
    g->generation = ++g_gp_generation;
    launch_prep_points(c->stream, g->X.p, D, N + 1, g->inv_ell.p, g->XT.p, Np, Np, g->Dcols, g->nx.p);
    launch_scale_rows(c->stream, g->XT.p, g->alpha.p, g->XaT.p, Np, Np, g->Dcols);
    if (g->sigma_mode == 1) launch_transpose_full(c->stream, g->Linv.p, g->U.p, Np);   // the rank-1 growth does not maintain U
    SLS_HIP(hipMemsetAsync(c->d_info, 0, 64, c->stream));
    launch_fit_summary(c->stream, g->y.p, g->alpha.p, g->b, N + 1, g->mu_data.p, g->L.p, Np, c->d_info, g->scal.p, g->d_idx, g->sum.dev);
    gp_fetch_summary(g);
    SLS_REQUIRE(std::isfinite(g->logdet), "sls_gp_append_point: the extended K_y is not positive definite");
    SLS_CATCH
}

