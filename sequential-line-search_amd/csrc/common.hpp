// Shared host-side plumbing of libsls_hip: context, error handling, device buffers, per-kernel event timing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/sls_hip.h"
#include "kernels.hpp"

namespace slsk {

void set_error(const char* fmt, ...);
// true: the persistent factorisation gave up (a bounded device-side wait expired, e.g. another stream kept CUs busy so
// that its workgroups were not all resident).  The context falls back to the multi-launch schedule for good and the
// caller repeats the factorisation once; a second failure throws HipFail{SLS_ERR_HIP}.
bool potrf_gave_up(sls_ctx* c, int abort_flag, int attempt);
// what a fitted handle was created from (capi_multi.hip: replicas of an existing handle)
int gp_export_inputs(sls_gp* g, int* D, int* N, int* kernel, int* sigma_mode, int* device, double* b, std::vector<double>* X,
                     std::vector<double>* y, std::vector<double>* theta);

// The fitted state of a GP handle as the posterior entry points (capi_post.hip) read it: device pointers in the layout of
// kernels.hpp, and the handle's state lock (shared while reading).
struct GpView {
    sls_ctx* ctx;
    int D, N, Np, Dp, Dcols, kernel;
    double a, b;
    const double *XT, *nx, *inv_ell, *alpha, *Linv;
    const double *y, *L;   // the data's targets (N, padded to Np) and the Cholesky factor of K_y (Np x Np)
    const double* X;       // the raw design matrix (D x N): what the direct-difference Gram forms read
    bool gram_direct;      // the fit is beyond the guard of the norm expansion (gram_direct_form, kernels.hpp)
    long generation;       // sls_gp_generation
    bool laplace;          // the handle carries a Laplace posterior (sls_gp_set_laplace); then, Np x Np each:
    const double *lap_T, *lap_LBinv;   // T = I - B^-1 (symmetric, product form) and L_B^-1 (zero above the diagonal)
    std::shared_mutex* state;
};
GpView gp_view(sls_gp* g);
// does the handle carry a Laplace posterior (sls_gp_set_laplace)?  Takes the context's lock.
bool gp_has_laplace(sls_gp* g);
// what sls_acq_last_stats reports for the handle: the one place every maximiser stores it (lbfgs_driver.hpp)
void gp_set_acq_stats(sls_gp* g, long issued, long cap, int rounds, int live_end);
// sls_lbfgs_opts as the caller's struct_size declares it, over the library's defaults (capi.hip)
sls_lbfgs_opts read_lbfgs_opts(const sls_lbfgs_opts* in);

struct HipFail {
    int code;
};

#define SLS_HIP(x)                                                                                 \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            slsk::set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            throw slsk::HipFail{SLS_ERR_HIP};                                                      \
        }                                                                                          \
    } while (0)

#define SLS_REQUIRE(cond, ...)                 \
    do {                                       \
        if (!(cond)) {                         \
            slsk::set_error(__VA_ARGS__);      \
            throw slsk::HipFail{SLS_ERR_INVALID}; \
        }                                      \
    } while (0)

// Every C-ABI entry point that can fail: SLS_TRY ... SLS_CATCH around its body turn HipFail / exceptions into the return code.
#define SLS_TRY slsk::note_entry(); try {
#define SLS_CATCH                                   \
    }                                               \
    catch (const slsk::HipFail& f) { return f.code; } \
    catch (const std::exception& e) {               \
        slsk::set_error("exception: %s", e.what()); \
        return SLS_ERR_INVALID;                     \
    }                                               \
    return SLS_OK;

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Per-device cache of freed device blocks, keyed by exact size: hipMalloc / hipFree cost 50-300 us each and a GP handle owns
// ~30 buffers, which made CREATING a handle at N = 2048 take longer than FITTING it (BASELINE config C2).  A regressor that
// is rebuilt with the same shapes (every step of the reference's optimisers) gets its blocks back without touching the
// driver.  At most SLS_POOL_MB (default 16384) MB stay cached per device; beyond that blocks go back to the driver.
void note_entry();                           // every C-ABI entry point: device work may be queued from here on
void* pool_alloc(size_t bytes);              // throws HipFail on failure
void pool_free(void* p, size_t bytes, bool in_flight = false);   // in_flight: work queued in THIS entry may still use the block
void pool_trim(int device);                  // return every cached block of `device` to the driver

// Owning device buffer of doubles (or raw bytes).
struct DBuf {
    double* p = nullptr;
    size_t n = 0;  // doubles
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { release(); }
    void release(bool in_flight = false) {
        if (p) pool_free(p, n * sizeof(double), in_flight);
        p = nullptr;
        n = 0;
    }
    void ensure(size_t doubles) {
        if (doubles <= n && p) return;
        release(true);   // a regrow in the middle of an entry point: kernels queued a moment ago may still read the old block
        p = static_cast<double*>(pool_alloc(doubles * sizeof(double)));
        n = doubles;
    }
};
// launch_grad_gemm's `part` for a launch of Sp candidates (kernels.hpp): b grown to the split form's scratch, or nullptr where the
// launch does not split (D > 64, or SLS_GRAD_SPLIT_TILES says so)
inline double* grad_split_scratch(DBuf& b, int D, int Sp) {
    if (D > 64 || !grad_gemm_wants_split(Sp)) return nullptr;
    b.ensure((size_t)8 * Sp * 64);
    return b.p;
}

// Owning page-locked host block from a context's pool (sls_ctx::host_take / host_give), device-mapped on request.  The block
// remembers the context it was taken from, so release() and the destructor need no argument.  The pool is not thread safe and this
// type takes NO lock: every ensure / release / destruction runs with that context's lock held (CtxCall; destroy_handle for the
// members of a handle) or where nobody else can reach the context any more (ctx_destroy_now, before host_free is walked).
struct HostBuf {
    double* host = nullptr;
    double* dev = nullptr;   // mapped blocks: the same memory as the device sees it
    size_t bytes = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    void release();
    // At least `need` bytes: a block that is large enough stays; otherwise the old one goes back and `take` bytes (default: need)
    // are taken.  The object is empty while it takes, so a throwing host_take leaves no dangling pointer.  true: the block is new.
    bool ensure(sls_ctx* c, size_t need, bool mapped_, size_t take = 0);

   private:
    sls_ctx* ctx = nullptr;
    bool mapped = false;
};

struct ProfEntry {
    double ms = 0;
    long launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace slsk

struct sls_ctx {
    // One stream, one info word, one profiling table per context: every entry point that touches the device takes this
    // lock, so a context (and all handles created from it) may be used from several host threads, one call at a time.
    std::recursive_mutex mtx;
    // handles (sls_gp, sls_nll, sls_comm) created from this context and still alive.  sls_ctx_destroy with live handles only marks
    // the context: the last handle to go frees it (garbage-collected bindings destroy context and handles in no particular order,
    // and a handle's destructor takes this lock).
    int live_handles = 0;
    bool destroy_requested = false;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int cand_chunk = 16384;
    bool prof_on = false;
    std::map<std::string, slsk::ProfEntry> prof;
    std::vector<hipEvent_t> event_pool;
    // scratch
    slsk::DBuf scratch;   // generic host<->device staging
    int* d_info = nullptr;  // device int[4]: potrf info etc.
    bool potrf_persistent_ok = true;     // cleared when a single-launch factorisation gave up (bounded wait expired)
    int potrf_rearm = 0;                 // fits left on the multi-launch schedule before the single-launch form is tried again
    int potrf_rearm_next = 16;           // ... and how many it will be after the next give-up (16, 64, 256, ... 4096)
    void potrf_tick_rearm();             // once per fit, BEFORE the factorisation is enqueued
    long potrf_fallbacks = 0;            // how often a single-launch factorisation gave up (sls_prof_get("potrf_fallbacks"))
    slsk::DBuf potrf_df;                 // flag tables of the dataflow form (grown on demand)
    int* potrf_df_sync(int Np);          // nullptr: single-launch form switched off for this context (no side effects)
    bool potrf_df_available(int Np) const;   // the same question without allocating the flag tables
    bool potrf_single_pending = false;   // a single-launch factorisation was handed its flag tables since the last verdict
    // streams + device-mapped page-locked blocks lent to concurrent small evaluations (capi.hip: eval_in_slot), created on demand,
    // kept for the life of the context
    struct EvalSlot {
        hipStream_t stream = nullptr;
        slsk::HostBuf block;   // query points in, results out
        bool busy = false;
    };
    std::mutex slot_mtx;
    std::condition_variable slot_cv;
    std::vector<std::unique_ptr<EvalSlot>> slots;
    static constexpr int MAX_SLOTS = 16;   // concurrent small evaluations per context; further callers wait for a free slot

    // page-locked host blocks (result blocks the small-problem kernels write directly, staging for uploads) handed out to the
    // handles of this context and taken back when a handle dies: hipHostMalloc + hipHostFree cost ~260 us per block (round 4, C3:
    // two blocks per SubmitFeedbackData were 0.5 ms of its 4 ms)
    struct HostBlock {
        void* p;
        size_t bytes;
        bool mapped;
    };
    std::vector<HostBlock> host_free;
    void* host_take(size_t bytes, bool mapped, size_t* got);
    void host_give(void* p, size_t bytes, bool mapped);

    hipEvent_t get_event();
    void prof_begin(const char* name, hipEvent_t& e0);
    void prof_end(const char* name, hipEvent_t e0);
    void prof_collect();
};

namespace slsk {
inline void HostBuf::release() {
    if (host) ctx->host_give(host, bytes, mapped);
    host = dev = nullptr;
    bytes = 0;
}
inline bool HostBuf::ensure(sls_ctx* c, size_t need, bool mapped_, size_t take) {
    if (host && need <= bytes) return false;
    release();
    ctx = c;
    mapped = mapped_;
    host = static_cast<double*>(c->host_take(std::max(need, take), mapped, &bytes));
    if (mapped) SLS_HIP(hipHostGetDevicePointer((void**)&dev, host, 0));
    return true;
}
void ctx_retain(sls_ctx* c);     // a handle was created (caller holds c->mtx)
void ctx_release(sls_ctx* c);    // a handle is gone (caller does NOT hold c->mtx: this may free the context)
// The context's lock for the length of an entry point.  A NULL context / handle takes nothing: the entry point's own SLS_REQUIRE
// reports it.  From a handle (anything with a ctx member): also the handle's device, whatever the caller's current device is.
struct CtxCall {
    std::unique_lock<std::recursive_mutex> lock;
    explicit CtxCall(sls_ctx* c) {
        if (c) lock = std::unique_lock<std::recursive_mutex>(c->mtx);
    }
    template <class H>
    explicit CtxCall(H* h) : CtxCall(h ? h->ctx : nullptr) {
        if (h) (void)hipSetDevice(h->ctx->device);
    }
};
// Entry points that only read a fitted GP handle (capi_post.hip, capi_path.hip): the context's lock, the handle's device, the
// handle's state lock (shared), and the view re-read under the locks -- a refit or an appended point may have changed it.
// expect_generation >= 0: the handle must still be what an object derived from it (sls_path) was made from.
struct GpReadCall {
    GpView g;
    CtxCall ctx_lock;
    std::shared_lock<std::shared_mutex> state_lock;
    explicit GpReadCall(sls_gp* gp, long expect_generation = -1, const char* who = "") : g(gp_view(gp)), ctx_lock(g.ctx) {
        (void)hipSetDevice(g.ctx->device);
        state_lock = std::shared_lock<std::shared_mutex>(*g.state);
        g = gp_view(gp);
        if (expect_generation >= 0)
            SLS_REQUIRE(g.generation == expect_generation,
                        "%s: the GP handle was refitted or grown since sls_path_create (generation %ld, now %ld): create a new object",
                        who, expect_generation, g.generation);
    }
};
// The tail of every handle's destroy: under the context's lock and on its device, drain the stream (and `drain`, a lock that work
// off the context's stream holds shared), delete, and give the context's reference back outside the lock.
template <class H>
void destroy_handle(H* h, std::shared_mutex* drain = nullptr) {
    sls_ctx* c = h->ctx;
    {
        CtxCall call(h);
        (void)hipStreamSynchronize(c->stream);
        if (drain) { std::unique_lock<std::shared_mutex> wait_(*drain); }   // released before the delete (it may be a member)
        delete h;
    }
    ctx_release(c);
}
// RAII kernel-timing scope: records HIP events on the context's stream when profiling is enabled.
struct ProfScope {
    sls_ctx* c;
    const char* name;
    hipEvent_t e0 = nullptr;
    ProfScope(sls_ctx* c_, const char* n) : c(c_), name(n) {
        if (c->prof_on) c->prof_begin(name, e0);
    }
    void rename(const char* n) { name = n; }   // the launch behind the scope turned out to be something else (fused form declined)
    ~ProfScope() {
        if (c->prof_on) c->prof_end(name, e0);
    }
};

// n doubles between host and device, asynchronous on the context's stream
inline void h2d(sls_ctx* c, double* dst, const double* src, size_t n) {
    SLS_HIP(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
}
inline void d2h(sls_ctx* c, double* dst, const double* src, size_t n) {
    SLS_HIP(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
}
// The two host-side transposes of the entry points.  The caller's points are rows x M column-major (X[r + m*rows]); the kernels
// read candidate-major blocks t[m + r*ld].  host_to_cm pads the columns M .. Mp with the centre of the box.
inline std::vector<double> host_to_cm(const double* X, int rows, int M, int Mp) {
    std::vector<double> t((size_t)Mp * rows, 0.5);
    for (int m = 0; m < M; ++m)
        for (int r = 0; r < rows; ++r) t[(size_t)m + (size_t)r * Mp] = X[r + (size_t)m * rows];
    return t;
}
// candidate-major src[m + r*ld] into the caller's array (NULL: not asked for): rows = 1: a vector of M; else rows x M column-major
template <class T>
void cm_to_host(const T* src, long ld, int rows, int M, T* host) {
    if (!host) return;
    for (int m = 0; m < M; ++m)
        for (int r = 0; r < rows; ++r) host[r + (size_t)m * rows] = src[(size_t)m + (size_t)r * ld];
}
}  // namespace slsk
