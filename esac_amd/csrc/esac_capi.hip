// esac_capi.hip -- C ABI (include/esac_hip.h) over the HIP kernels.
// Host side of the drop-in boundary: argument validation with the reference's
// failure convention (everything that would have thrown c10::Error / cv::Exception
// through pybind11 becomes a negative status + message), workspace ownership,
// kernel launches on the caller's stream, optional per-phase hipEvent timers
// (the StopWatch prints of esac.cpp:124,149,161,179).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <sched.h>
#include <time.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/esac_hip.h"
#include "esac_kernels.hpp"
#include "eval_math.hpp"
#include "gt_math.hpp"
#include "pose_math.hpp"

using namespace esac;

// RCCL's handful of types, declared here (see rccl() below: the library is bound by dlopen, its headers are not needed)
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
}

static_assert(ESAC_RES_SCORE == ESAC_RES_SCORE_K && ESAC_RES_HYP == ESAC_RES_HYP_K && ESAC_RES_EXPERT == ESAC_RES_EXPERT_K &&
                  ESAC_RES_RVEC == ESAC_RES_RVEC_K && ESAC_RES_POSE == ESAC_RES_POSE_K &&
                  ESAC_RES_REF_STEPS == ESAC_RES_REF_STEPS_K && ESAC_RES_INLIERS == ESAC_RES_INLIERS_K &&
                  ESAC_RES_PROB == ESAC_RES_PROB_K && ESAC_RES_ENTROPY == ESAC_RES_ENTROPY_K &&
                  ESAC_RES_CONTENDERS == ESAC_RES_CONTENDERS_K && ESAC_RES_LM_ITERS == ESAC_RES_LM_ITERS_K &&
                  ESAC_MAX_REF_STEPS == ESAC_MAX_REF_STEPS_K && ESAC_BWD_MAX_SLOTS == ESAC_BWD_SLOTS_K &&
                  ESAC_FLAG_EXACT_SCORES == ESAC_FLAG_EXACT_SCORES_K && ESAC_FLAG_EXACT_SAMPLING == ESAC_FLAG_EXACT_SAMPLING_K &&
                  ESAC_FLAG_SCORES_BY_INDEX == ESAC_FLAG_SCORES_BY_INDEX_K && ESAC_FLAG_STRICT_REFERENCE == ESAC_FLAG_STRICT_REFERENCE_K &&
                  ESAC_FLAG_STRICT_TRAINING == ESAC_FLAG_STRICT_TRAINING_K &&
                  ESAC_REFINE_TEAM_MAX == ESAC_REFINE_TEAM_MAX_K &&
                  ESAC_REFINE_TEAM_DEFAULT == ESAC_REFINE_TEAM_DEFAULT_K &&
                  (ESAC_FLAG_AUTO_EXACT & (ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING | ESAC_FLAG_SCORES_BY_INDEX)) == 0,
              "result layout drifted between include/esac_hip.h and esac_kernels.hpp");

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_OK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(-100 - (int)_e, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Makes the context's GPU current for the duration of one entry point and restores the caller's device afterwards
// (torch and every other runtime user read the same thread-local "current device").
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur;
        if (cur != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct esac_hip_ctx {
    int device = 0;
    int capN = 0, capP = 0, capB = 0;  // capN / capP count elements over ALL frames of a batch
    KArgs ws{};  // only the workspace pointers are kept here
    int lastN = 0, lastH = 0, lastW = 0;
    int lastB = 1;  // frames of the most recent launch set (esac_hip_read: B x the single-frame size reads the per-frame forward buffers of all of them)
    bool timing = false;
    int timing_period = 1;       // record the phase events / device-side stamps on every timing_period-th forward call
    long long timing_calls = 0;  // forward calls since timing was enabled
    bool keep_errs = false;  // esac_hip_set_debug: store the winner's error image
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    double* h_pin = nullptr;  // pinned, device-visible host buffer: result record [32] + epoch word
    double* d_pin = nullptr;  // its device address
    double epoch = 0;         // bumped by every entry point: hand-off word of the pinned record
    double sample_epoch = 0;  // epoch of the most recent SAMPLING launch: what the device-side status word is tagged with
    int wait_mode = ESAC_WAIT_SPIN;
    int coop_max = 0;         // cooperative refinement workgroups this device holds at once (refine_coop_capacity)
    bool coop_stall = false;  // ESAC_DEBUG_COOP_STALL
    int team = ESAC_REFINE_TEAM_DEFAULT;  // members of the refinement team on small grids (esac_hip_set_refine_team; 0: one workgroup)
    bool team_spread = false;             // ESAC_DEBUG_TEAM_SPREAD: the members are consecutive workgroups (one per XCD)
    bool team_auto = true;                // the default team size is chosen per grid (ESAC_REFINE_TEAM_AUTO=0: exactly the default, A/B)
    bool team_auto_env_off = false;
    unsigned long long refine_tag = 0;    // tag of the most recent shared (cooperative / team) refinement launch, 0: none yet
    unsigned long long checked_tag = 0;   // the failed launch esac_hip_check has already counted as a strike
    bool refine_was_team = false;         // the most recent forward's refinement launch was a team's
    long long team_fallbacks = 0;         // blocking calls whose team timed out and were refined again by one workgroup
    int team_strikes = 0;                 // consecutive forward calls whose team timed out; at ESAC_TEAM_STRIKES the context stops asking
    bool team_latched_off = false;        // ... for teams (a caller that keeps the GPU's CUs busy on another stream would otherwise pay the
    long long solo_since_latch = 0;       // time-out on every frame); re-armed after ESAC_TEAM_REARM_CALLS calls or by esac_hip_set_refine_team
    bool fold_select = true;              // the team kernel may run the selection in its prologue (ESAC_FOLD_SELECT=0: measurement scripts)
    int last_nsel = 0;                    // slots the most recent blocking esac_hip_backward refined (0: none yet; reported, decides nothing)
    bool slot_teams = true;               // training path: slots may be refined by teams (off after a time-out until
                                          // esac_hip_set_refine_team re-arms it; ESAC_SLOT_TEAMS=0)
    long long slot_team_calls = 0, slot_team_fallbacks = 0;
    bool last_bwd_teams = false;          // the most recent esac_hip_backward refined its slots by teams
    BwdArgs bws{};  // training-path workspace (pointers only), sized for bN hypotheses, bP cells, bslots slots, brows slot-table rows
    int bP = 0, bcap = 0;  // bcap: slots per frame the single calls have needed so far (where the next one starts)
    long long bN = 0, bslots = 0, brows = 0;  // over all frames of a batch
    int bB = 0;                               // frames of the per-frame records
    bool b_lists = false;
    // batched training calls (esac_hip_backward_batch)
    int bcap_batch = 0;                       // slots per frame the batches have needed so far
    long long bwd_budget = 2048LL << 20;      // bytes of slot workspace a batch may use (ESAC_BWD_BATCH_BUDGET_MB): beyond it, chunks of frames
    int last_bwd_frames = 1;                  // frames whose training-path buffers the workspace holds (the last launch set)
    int last_bwd_batch_cap = 0;               // slots per frame of the last launch set when it was a batch's (0: a single call)
    double* h_gt = nullptr;                   // pinned staging of the per-frame ground truth [ESAC_MAX_BATCH,22]
    double* d_gt = nullptr;                   // ... and its device copy
    // esac_hip_backward_batch_dev: nothing of the call is staged on the host
    double* d_gt_dev = nullptr;               // [ESAC_MAX_BATCH,22] written by k_bwd_gt_prepare in stream order
    int* d_frame_status = nullptr;            // [ESAC_MAX_BATCH] per-frame outcome of the most recent such call (BwdArgs::frame_status)
    int last_dev_batch = 0;                   // its B while it is the most recent call on the context (esac_hip_check reads that many words)
    // esac_hip_set_bwd_pose_records: what the NEXT training call writes its forward-format records to (one-shot: take_pose_arm)
    double* pose_rec = nullptr;               // DEVICE [pose_rec_frames, ESAC_RES_DOUBLES], null: not armed
    int pose_rec_frames = 0;
    // per-frame cameras of a batch (esac_hip_forward_batch_cams / esac_hip_backward_batch_cams)
    FrameCam* h_cams = nullptr;               // pinned staging [ESAC_MAX_BATCH]: the caller's array is free when the call returns
    FrameCam* d_cams = nullptr;               // ... and the table the kernels read (KArgs::cams)
    hipEvent_t cams_ev = nullptr;             // recorded behind the most recent upload: the staging is rewritten only after it
    bool cams_queued = false;
    float4* sc4 = nullptr;  // packed copy of the maps for the sampler (ensure_pack_ws)
    long long sc4_cells = 0;
    // tile-stationary score workspace (ensure_tiled_ws)
    int tN = 0, tChunks = 0;
    long long tPart = 0;
    bool rt32_stale = false;  // esac_hip_write_hyps ran: the fp32 [R|t] rows are rebuilt by the next esac_hip_score
    double host_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // esac_hip_host_turn: where the host's time of the most recent blocking forward went
    double host_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... summed over the blocking forward calls since the last reset (esac_hip_host_turn_mean)
    double host_last_return = 0;                    // CLOCK_MONOTONIC at which the previous blocking forward returned
    long long host_n = 0;
    // speculative forward (forward_impl): the straggler chain of the sampler runs on this stream beside the launch stream
    hipStream_t side = nullptr;
    hipStream_t side2 = nullptr;          // ... and the selection among the settled hypotheses + the join on this one, beside the speculative refinement
    hipEvent_t spec_ev = nullptr;         // recorded on the caller's stream at the entry of a speculative call: both streams wait for it
    bool spec_off = false, spec_env_off = false;  // ESAC_DEBUG_NO_SPECULATION / ESAC_SPECULATE=0
    bool spec_second_best = false;        // ESAC_DEBUG_SPEC_SECOND_BEST
    bool spec_lose_chain = false;         // ESAC_DEBUG_SPEC_LOSE_CHAIN
    long long spec_calls = 0;             // forward calls that took the speculative route
    double last_spec_epoch = 0;           // epoch of the most recent speculative call (0: the most recent forward was not)
    ncclComm_t comm = nullptr;  // esac_hip_comm_init: this context's rank in an RCCL communicator (the multi-GPU score exchange)
    int comm_ranks = 0, comm_rank = 0;
};

static inline double now_ns() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e9 + (double)ts.tv_nsec;
}

extern "C" int esac_hip_abi_version(void) { return ESAC_HIP_ABI_VERSION; }
extern "C" const char* esac_hip_last_error(void) { return g_err; }
extern "C" int esac_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

constexpr int ESAC_SLOT_TEAMS_MAX = 32;  // training path: slots refined by teams when the call selects at most this many
constexpr int ESAC_TEAM_STRIKES = 2;
constexpr long long ESAC_TEAM_REARM_CALLS = 1000;

// RCCL, bound at the first esac_hip_comm_* call (see "the one collective of the multi-GPU path" below).  The handful of
// types and entry points this file needs are declared HERE (the stable NCCL 2.x C API: a 128-byte unique id, an opaque
// communicator, ncclResult_t 0 = success, ncclSum = 0, ncclDouble = 8), not taken from <rccl/rccl.h>: a single-GPU build of the
// library needs neither RCCL's headers at compile time nor its shared object at run time.
static_assert(sizeof(ncclUniqueId) == ESAC_COMM_ID_BYTES, "unique id size");
constexpr ncclResult_t ncclSuccess = 0;
constexpr int NCCL_SUM = 0, NCCL_DOUBLE = 8;  // ncclRedOp_t ncclSum, ncclDataType_t ncclFloat64
struct Rccl {
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*all_reduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    ncclResult_t (*comm_count)(const ncclComm_t, int*) = nullptr;      // what the communicator itself reports (esac_hip_comm_info)
    ncclResult_t (*comm_user_rank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*comm_cu_device)(const ncclComm_t, int*) = nullptr;
    bool ok = false;
};
static const Rccl& rccl() {
    static const Rccl bound = [] {
        Rccl r;
        void* h = nullptr;
        // the copy the process already holds first (torch ships its own librccl.so under another path: two copies of RCCL in
        // one process would each bring up their own transports), then the loader's search path, then ROCm's
        for (const char* name : {"librccl.so.1", "librccl.so"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD))) break;
        if (!h)
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
                if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return r;
        r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(dlsym(h, "ncclAllReduce"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(h, "ncclGetErrorString"));
        r.comm_count = reinterpret_cast<decltype(r.comm_count)>(dlsym(h, "ncclCommCount"));
        r.comm_user_rank = reinterpret_cast<decltype(r.comm_user_rank)>(dlsym(h, "ncclCommUserRank"));
        r.comm_cu_device = reinterpret_cast<decltype(r.comm_cu_device)>(dlsym(h, "ncclCommCuDevice"));
        r.ok = r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.all_reduce && r.error_string;
        return r;
    }();
    return bound;
}
static void drop_comm(esac_hip_ctx* c) {
    if (c->comm) (void)rccl().comm_destroy(c->comm);  // a communicator exists only if RCCL was bound
    c->comm = nullptr;
    c->comm_ranks = 0;
}

static void free_ws(esac_hip_ctx* c) {
    void* ptrs[] = {c->ws.hyps,       c->ws.hyps_R,      c->ws.rt32,         c->ws.sample_xy, c->ws.tries,      c->ws.samp_resume, c->ws.samp_round, c->ws.best_try, c->ws.samp_cand, c->ws.samp_entries, c->ws.samp_count, c->ws.samp_pending, c->ws.fast_scores,
                    c->ws.scores,     c->ws.exact_flag,   c->ws.n_contenders, c->ws.sel_partials, c->ws.sel_arrived, c->ws.stats,
                    c->ws.errs,       c->ws.inlier_map,   c->ws.inlier_counts, c->ws.result, c->ws.corr_list, c->ws.cycles, c->ws.tstamps, c->ws.span_acc,
                    c->ws.status,     c->ws.coop_partials, c->ws.coop_counter, c->ws.refine_info, c->ws.order,        c->ws.rt_sorted,  c->ws.chunks,     c->ws.n_chunks,  c->ws.partials, c->ws.bucket_fill,
                    c->ws.spec_flag,  c->ws.spec_state,  c->ws.spec_cnt};
    c->tN = c->tChunks = 0;
    c->tPart = 0;
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    c->ws = KArgs{};
    c->capN = c->capP = c->capB = 0;
}

extern "C" int esac_hip_create(esac_hip_ctx** out, int device) {
    if (!out) return fail(-1, "esac_hip_create: null ctx pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(-2, "esac_hip_create: no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(-3, "esac_hip_create: device %d out of range [0,%d)", device, n);
    DeviceGuard guard(device);
    esac_hip_ctx* c = new esac_hip_ctx();
    c->device = device;
    for (auto& ev : c->ev) HIP_OK(hipEventCreate(&ev));
    HIP_OK(hipHostMalloc((void**)&c->h_pin, (size_t)ESAC_PIN_DOUBLES * ESAC_MAX_BATCH * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->h_pin, 0, (size_t)ESAC_PIN_DOUBLES * ESAC_MAX_BATCH * sizeof(double));
    HIP_OK(hipHostGetDevicePointer((void**)&c->d_pin, c->h_pin, 0));
    c->coop_max = refine_coop_capacity();  // CUs x resident workgroups of the cooperative refinement kernel on THIS device
    if (const char* e = getenv("ESAC_REFINE_TEAM")) {  // start value of esac_hip_set_refine_team (measurement scripts)
        const int g = atoi(e);
        c->team = g < 2 ? 0 : (g > ESAC_REFINE_TEAM_MAX ? ESAC_REFINE_TEAM_MAX : g);
    }
    if (const char* e = getenv("ESAC_FOLD_SELECT")) c->fold_select = atoi(e) != 0;
    if (const char* e = getenv("ESAC_REFINE_TEAM_AUTO")) c->team_auto_env_off = atoi(e) == 0;
    if (c->team_auto_env_off || getenv("ESAC_REFINE_TEAM")) c->team_auto = false;  // (an explicit start value is an explicit size)
    if (const char* e = getenv("ESAC_SLOT_TEAMS")) c->slot_teams = atoi(e) != 0;
    if (const char* e = getenv("ESAC_SPECULATE")) c->spec_off = c->spec_env_off = atoi(e) == 0;
    if (const char* e = getenv("ESAC_BWD_BATCH_BUDGET_MB")) {
        const long long mb = atoll(e);
        if (mb > 0) c->bwd_budget = mb << 20;
    }
    *out = c;
    return 0;
}

static void free_bws(esac_hip_ctx* c) {
    void* ptrs[] = {c->bws.sel,   c->bws.n_sel, c->bws.probs,    c->bws.losses,     c->bws.ref_hyps, c->bws.sgrad, c->bws.dloss,
                    c->bws.maps,  c->bws.map_info, c->bws.corr_lists, c->bws.grad1, c->bws.grad2,   c->bws.out, c->bws.team_gran, c->bws.arrived,
                    c->bws.sel_max};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    c->bws = BwdArgs{};
    c->bN = c->bslots = c->brows = 0;
    c->bP = c->bB = 0;
    c->b_lists = false;
}

extern "C" int esac_hip_destroy(esac_hip_ctx* c) {
    if (!c) return 0;
    DeviceGuard guard(c->device);
    free_ws(c);
    free_bws(c);
    if (c->d_gt) (void)hipFree(c->d_gt);
    if (c->d_gt_dev) (void)hipFree(c->d_gt_dev);
    if (c->d_frame_status) (void)hipFree(c->d_frame_status);
    if (c->d_cams) (void)hipFree(c->d_cams);
    if (c->h_cams) (void)hipHostFree(c->h_cams);
    if (c->cams_ev) (void)hipEventDestroy(c->cams_ev);
    if (c->h_gt) (void)hipHostFree(c->h_gt);
    if (c->sc4) (void)hipFree(c->sc4);
    drop_comm(c);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->side2) (void)hipStreamDestroy(c->side2);
    if (c->spec_ev) (void)hipEventDestroy(c->spec_ev);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete c;
    return 0;
}

template <typename T>
static int alloc(T** p, size_t n) {
    HIP_OK(hipMalloc((void**)p, n * sizeof(T)));
    return 0;
}

static int ensure_ws(esac_hip_ctx* c, int N1, int P1, int B = 1) {
    const long long N = (long long)N1 * B, P = (long long)P1 * B;
    if (N <= c->capN && P <= c->capP && B <= c->capB) return 0;
    if (N > 0x7fffffffLL || P > 0x7fffffffLL) return fail(-4, "batch too large");
    HIP_OK(hipDeviceSynchronize());
    const int nN = N > c->capN ? (int)N : c->capN, nP = P > c->capP ? (int)P : c->capP;
    const int nB = B > c->capB ? B : c->capB;
    // hypotheses handed in through esac_hip_write_hyps (and the status word) survive a growing workspace
    double* old_hyps = c->ws.hyps;
    const size_t old_n = (size_t)c->capN;
    unsigned long long old_status = 0;
    if (c->ws.status) HIP_OK(hipMemcpy(&old_status, c->ws.status, sizeof(old_status), hipMemcpyDeviceToHost));
    c->ws.hyps = nullptr;
    free_ws(c);
    int rc = 0;
    rc |= alloc(&c->ws.hyps, (size_t)nN * 6);
    rc |= alloc(&c->ws.hyps_R, (size_t)nN * 9);
    rc |= alloc(&c->ws.rt32, (size_t)nN * 12);
    rc |= alloc(&c->ws.status, (size_t)1);
    // the exchange buffer of shared refinements: partial sums of cooperating workgroups [2][256][32] doubles, or the granules
    // of up to ESAC_TEAM_BATCH_MAX teams (16 bytes each)
    static_assert((size_t)ESAC_TEAM_BATCH_MAX * ESAC_TEAM_GRANULES * 2 >= (size_t)2 * ESAC_REFINE_COOP_MAX * 32, "exchange buffer");
    rc |= alloc(&c->ws.coop_partials, (size_t)ESAC_TEAM_BATCH_MAX * ESAC_TEAM_GRANULES * 2);
    rc |= alloc(&c->ws.coop_counter, (size_t)2);
    rc |= alloc(&c->ws.refine_info, (size_t)8);
    rc |= alloc(&c->ws.sample_xy, (size_t)nN * 8);
    rc |= alloc(&c->ws.tries, (size_t)nN);
    rc |= alloc(&c->ws.samp_resume, (size_t)nN);
    rc |= alloc(&c->ws.samp_round, (size_t)nN);
    rc |= alloc(&c->ws.best_try, (size_t)nN);
    rc |= alloc(&c->ws.samp_cand, (size_t)nN * ESAC_SAMPLE_LIST_PER_HYP * ESAC_CAND_DOUBLES);
    rc |= alloc(&c->ws.samp_entries, (size_t)nN * 2 * ESAC_SAMPLE_LIST_PER_HYP);  // (hypothesis, try) pairs
    rc |= alloc(&c->ws.samp_count, (size_t)4 + 2 * 1024);  // list counters + 1024 x 2 per-expert counters (esac_kernels.hip: expert_stats)
    rc |= alloc(&c->ws.samp_pending, (size_t)nN);
    rc |= alloc(&c->ws.fast_scores, (size_t)nN);
    rc |= alloc(&c->ws.scores, (size_t)nN);
    rc |= alloc(&c->ws.exact_flag, (size_t)nN);
    rc |= alloc(&c->ws.n_contenders, (size_t)4 * nB);
    rc |= alloc(&c->ws.sel_partials, (size_t)nN * ESAC_SELECT_SPLIT);
    rc |= alloc(&c->ws.sel_arrived, (size_t)nN);
    rc |= alloc(&c->ws.stats, (size_t)4 * nB);
    rc |= alloc(&c->ws.errs, (size_t)nP);
    rc |= alloc(&c->ws.inlier_map, (size_t)nP * 2);  // two buffers, see esac_refine.hip
    {
        char* cl = nullptr;
        rc |= alloc(&cl, ((size_t)nP + (size_t)2048 * nB) * 16);  // sum over frames of corr_entries(P) < P + 2048 each
        c->ws.corr_list = cl;
    }
    rc |= alloc(&c->ws.inlier_counts, (size_t)(ESAC_MAX_REF_STEPS + 1) * nB);
    rc |= alloc(&c->ws.result, (size_t)ESAC_RES_DOUBLES * nB);
    rc |= alloc(&c->ws.cycles, (size_t)32);
    rc |= alloc(&c->ws.tstamps, (size_t)nN * 2);
    rc |= alloc(&c->ws.span_acc, (size_t)2);
    rc |= alloc(&c->ws.spec_flag, (size_t)nN);
    rc |= alloc(&c->ws.spec_state, (size_t)8);
    rc |= alloc(&c->ws.spec_cnt, (size_t)ESAC_SPEC_CNT_INTS);
    if (rc) {
        if (old_hyps) (void)hipFree(old_hyps);
        return rc;
    }
    HIP_OK(hipMemset(c->ws.span_acc, 0, 2 * sizeof(long long)));
    HIP_OK(hipMemset(c->ws.spec_flag, 0, (size_t)nN));
    HIP_OK(hipMemset(c->ws.spec_state, 0, 8 * sizeof(double)));
    HIP_OK(hipMemset(c->ws.spec_cnt, 0, ESAC_SPEC_CNT_INTS * sizeof(int)));
    HIP_OK(hipMemset(c->ws.coop_counter, 0, 2 * sizeof(unsigned long long)));  // [1]: tag of the last failed shared refinement (esac_hip_check)
    HIP_OK(hipMemset(c->ws.coop_partials, 0, (size_t)ESAC_TEAM_BATCH_MAX * ESAC_TEAM_GRANULES * 2 * sizeof(double)));  // (also the teams' granules)
    HIP_OK(hipMemset(c->ws.refine_info, 0, 8 * sizeof(int)));
    HIP_OK(hipMemset(c->ws.samp_count, 0, (4 + 2 * 1024) * sizeof(int)));       // the screened chain leaves them at zero (esac_kernels.hip)
    HIP_OK(hipMemset(c->ws.hyps, 0, (size_t)nN * 6 * sizeof(double)));
    HIP_OK(hipMemcpy(c->ws.status, &old_status, sizeof(old_status), hipMemcpyHostToDevice));
    if (old_hyps) {
        if (old_n) HIP_OK(hipMemcpy(c->ws.hyps, old_hyps, old_n * 6 * sizeof(double), hipMemcpyDeviceToDevice));
        (void)hipFree(old_hyps);
    }
    HIP_OK(hipMemset(c->ws.result, 0, (size_t)ESAC_RES_DOUBLES * nB * sizeof(double)));
    HIP_OK(hipMemset(c->ws.n_contenders, 0, (size_t)4 * nB * sizeof(int)));
    HIP_OK(hipMemset(c->ws.sel_arrived, 0, (size_t)nN * sizeof(int)));  // k_select_rescore leaves it zero after every call
    c->capN = nN;
    c->capP = nP;
    c->capB = nB;
    return 0;
}

// Which shape the fp32 score runs in.  Per-hypothesis stream (k_score_fast): every hypothesis re-reads its expert's map,
// fine while a map is L2-resident and hypotheses are few.  Tile-stationary (esac_score_tiled.hip): each map tile is read
// once per chunk of <= 256 hypotheses -- pays when a map no longer fits the caches next to the other experts' maps
// (full-resolution 480x640 maps: 3.7 MB each) and enough hypotheses share it.  ESAC_FLAG_SCORE_TILED / _STREAM override.
static bool want_tiled(const esac_hip_params* p, const float* d_sc, int B) {
    const long long P = (long long)p->H * p->W;
    const bool legal = B == 1 && (p->W & 3) == 0 && (reinterpret_cast<uintptr_t>(d_sc) & 15) == 0 &&
                       p->E <= ESAC_TILED_MAX_EXPERTS && P >= 4;
    const long long partial_bytes = (long long)tiled_sub_tiles((int)P) * p->N * 4;
    if (!legal || partial_bytes > (4LL << 30) || (p->flags & ESAC_FLAG_SCORE_STREAM)) return false;
    // the tile kernel folds k = |beta| log2(e) into the pose rows and multiplies by 2^(-+k tau) after the exp2: beyond
    // k tau ~ 126 that constant under- / overflows (scores NaN or saturated); the stream keeps the subtraction in the
    // exponent and is right for any parameters
    if (!(fabsf(p->inlier_beta) * 1.4426950408889634f * fabsf(p->inlier_thresh) <= 100.0f)) return false;
    if (p->flags & ESAC_FLAG_SCORE_TILED) return true;
    return P >= 32768 && p->N >= 64;
}

// Packed (x,y,z,0) copy of the maps for the sampler: worth one extra pass over the maps when they are far beyond the L2s
// (every random 4-byte gather would otherwise fetch its own cache line, three per cell) and hypotheses of several experts
// will need many tries.  Single frames only.
static bool want_pack(const esac_hip_params* p, int B) {
    if (B != 1) return false;
    if (p->flags & ESAC_FLAG_PACK_MAPS) return true;
    return p->E > 1 && (long long)p->E * p->H * p->W * 12 >= (32LL << 20) && p->N >= 256;
}
static int ensure_pack_ws(esac_hip_ctx* c, long long cells) {
    if (cells <= c->sc4_cells) return 0;
    HIP_OK(hipDeviceSynchronize());
    if (c->sc4) (void)hipFree(c->sc4);
    c->sc4 = nullptr;
    c->sc4_cells = 0;
    HIP_OK(hipMalloc((void**)&c->sc4, (size_t)cells * sizeof(float4)));
    c->sc4_cells = cells;
    return 0;
}

static int ensure_tiled_ws(esac_hip_ctx* c, int N, int P, int E) {
    const int n_sub = tiled_sub_tiles(P);
    const int chunks = N / ESAC_TILED_HC + (E < N ? E : N) + 1;
    const long long part = (long long)n_sub * N;
    if (N <= c->tN && chunks <= c->tChunks && part <= c->tPart) return 0;
    HIP_OK(hipDeviceSynchronize());
    void* ptrs[] = {c->ws.order, c->ws.rt_sorted, c->ws.chunks, c->ws.n_chunks, c->ws.partials, c->ws.bucket_fill};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    c->ws.order = nullptr; c->ws.rt_sorted = nullptr; c->ws.chunks = nullptr; c->ws.n_chunks = nullptr; c->ws.partials = nullptr;
    c->ws.bucket_fill = nullptr;
    const int nN = N > c->tN ? N : c->tN, nC = chunks > c->tChunks ? chunks : c->tChunks;
    const long long nP = part > c->tPart ? part : c->tPart;
    c->tN = c->tChunks = 0;
    c->tPart = 0;
    int rc = 0;
    rc |= alloc(&c->ws.order, (size_t)nN);
    rc |= alloc(&c->ws.rt_sorted, (size_t)nN * 12);
    rc |= alloc(&c->ws.chunks, (size_t)nC * 4);
    rc |= alloc(&c->ws.n_chunks, (size_t)4);
    rc |= alloc(&c->ws.partials, (size_t)nP);
    rc |= alloc(&c->ws.bucket_fill, (size_t)ESAC_TILED_MAX_EXPERTS);
    if (rc) return rc;
    c->tN = nN; c->tChunks = nC; c->tPart = nP;
    return 0;
}

// One camera's checks (cam_frame >= 0: a record of a per-frame table, the error names the frame)
static int check_cam(const esac_hip_params* p, int shift_x, int shift_y, float focal, int cam_frame) {
    char where[32] = "";
    if (cam_frame >= 0) snprintf(where, sizeof(where), " in frame %d", cam_frame);
    {   // pixel centres col*sub + sub/2 - shift (esac_util.h:64-66) are formed in int32 on the device
        const int64_t lim = 0x7fffffffLL, half = p->sub_sampling / 2;
        const int64_t xs[4] = {half - shift_x, (int64_t)(p->W - 1) * p->sub_sampling + half - shift_x,
                               half - shift_y, (int64_t)(p->H - 1) * p->sub_sampling + half - shift_y};
        for (int64_t v : xs)
            if (v > lim || v < -lim) return fail(-4, "pixel positions overflow int32 (subSampling=%d, shift=(%d,%d))%s", p->sub_sampling, shift_x, shift_y, where);
    }
    if (!(focal > 0)) return fail(-4, "focal length must be positive%s", where);
    return 0;
}
static esac_hip_params with_cam(const esac_hip_params& p, const esac_hip_frame_cam& cam) {
    esac_hip_params q = p;
    q.shift_x = cam.shift_x; q.shift_y = cam.shift_y;
    q.focal = cam.focal; q.ppx = cam.ppx; q.ppy = cam.ppy;
    return q;
}

// Validation: what the reference leaves to accessor<>() / OpenCV asserts.
// training: the call is one of esac_hip_backward* (the only entry points that honour ESAC_FLAG_STRICT_TRAINING)
static int make_args(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, KArgs* out,
                     int B = 1, long long sc_frame_stride = 0, int cam_frame = -1, bool training = false) {
    if (!c) return fail(-1, "null context");
    if (!p) return fail(-1, "null params");
    if (!d_sc || !d_assign) return fail(-1, "null scene-coordinate or assignment pointer");
    if (p->E <= 0 || p->N <= 0) return fail(-4, "E=%d, N=%d must be positive", p->E, p->N);
    if (p->H < 3 || p->W < 3 || (int64_t)(p->H - 1) * (p->W - 1) < 4)
        return fail(-4, "grid %dx%d too small: 4 distinct cells must exist in [0,W-2]x[0,H-2] (esac_util.h:164-176)", p->H, p->W);
    if ((int64_t)p->H * p->W > (int64_t)1 << 28 || p->H > 65535 || p->W > 65535)
        return fail(-4, "grid %dx%d too large (at most 65535 rows / columns, 2^28 cells)", p->H, p->W);
    if (p->sub_sampling <= 0) return fail(-4, "subSampling=%d must be positive", p->sub_sampling);
    if ((p->flags & ESAC_FLAG_STRICT_REFERENCE) && (p->flags & (ESAC_FLAG_SCORE_TILED | ESAC_FLAG_SCORE_STREAM | ESAC_FLAG_AUTO_EXACT)))
        return fail(-4, "ESAC_FLAG_STRICT_REFERENCE cannot be combined with ESAC_FLAG_SCORE_TILED, ESAC_FLAG_SCORE_STREAM or ESAC_FLAG_AUTO_EXACT "
                        "(flags=%d): strict mode scores every hypothesis in reference arithmetic", p->flags);
    if (p->flags & ESAC_FLAG_STRICT_TRAINING) {
        if (p->flags & ESAC_FLAG_STRICT_REFERENCE)
            return fail(-4, "ESAC_FLAG_STRICT_TRAINING cannot be combined with ESAC_FLAG_STRICT_REFERENCE (flags=%d): one is the training "
                            "path's strict mode, the other the forward path's", p->flags);
        if (!training)
            return fail(-4, "ESAC_FLAG_STRICT_TRAINING is a flag of esac_hip_backward, esac_hip_backward_batch and esac_hip_backward_batch_cams "
                            "(flags=%d): the forward path's strict mode is ESAC_FLAG_STRICT_REFERENCE", p->flags);
    }
    if (int rc_cam = check_cam(p, p->shift_x, p->shift_y, p->focal, cam_frame)) return rc_cam;
    const int P = p->H * p->W;
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "batch size %d outside [1,%d]", B, ESAC_MAX_BATCH);
    int rc = ensure_ws(c, p->N, P, B);
    if (rc) return rc;
    const bool tiled = want_tiled(p, d_sc, B);
    if (tiled && (rc = ensure_tiled_ws(c, p->N, P, p->E))) return rc;
    const bool pack = want_pack(p, B);
    if (pack && (rc = ensure_pack_ws(c, (long long)p->E * P))) return rc;
    KArgs a = c->ws;
    a.sc4 = pack ? c->sc4 : nullptr;
    if (tiled) {
        a.n_sub = tiled_sub_tiles(P);
        a.n_chunks_max = p->N / ESAC_TILED_HC + (p->E < p->N ? p->E : p->N) + 1;
    } else {
        a.partials = nullptr;  // launch_score: per-hypothesis stream
    }
    a.frames = B;
    a.sc_frame_stride = sc_frame_stride;
    a.cams = nullptr;  // (the _cams entry points set it after stage_cams)
    a.sc = d_sc;
    a.assign = d_assign;
    a.E = p->E; a.H = p->H; a.W = p->W; a.N = p->N;
    a.shift_x = p->shift_x; a.shift_y = p->shift_y; a.sub = p->sub_sampling;
    a.focal = p->focal; a.ppx = p->ppx; a.ppy = p->ppy;
    a.tau = p->inlier_thresh; a.alpha = p->inlier_alpha; a.beta = p->inlier_beta; a.max_reproj = p->max_reproj;
    a.seed = p->seed; a.call = p->call;
    a.max_tries = p->max_tries > 0 ? p->max_tries : ESAC_MAX_SAMPLING_TRIES;
    a.max_ref_steps = p->max_ref_steps >= 0 ? (p->max_ref_steps < ESAC_MAX_REF_STEPS ? p->max_ref_steps : ESAC_MAX_REF_STEPS)
                                            : ESAC_MAX_REF_STEPS;
    a.hyp_offset = p->hyp_offset;
    a.hyp_index = p->d_hyp_index;
    a.expert_base = p->expert_base;
    a.coop_max = c->coop_max;
    a.coop_extra = c->coop_stall ? 1 : 0;
    a.team = c->team;  // (the forward entry points fold the time-out latch in: forward_team)
    a.team_auto = c->team_auto ? 1 : 0;
    a.team_stride = c->team_spread ? 1 : 8;
    a.solo = 0;
    a.spec_mode = 0;
    a.spec_gate = 0;
    a.spec_debug = 0;
    a.spec_flag = nullptr;  // (forward_impl hands the flags to the kernels of a speculative call only)
    a.samp_cap = (int)(((long long)c->capN * ESAC_SAMPLE_LIST_PER_HYP) > 0x7fffffffLL ? 0x7fffffff : (long long)c->capN * ESAC_SAMPLE_LIST_PER_HYP);
    a.flags = p->flags;
    if (a.flags & ESAC_FLAG_STRICT_REFERENCE) a.flags |= ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;  // (implied)
    // the training path's strict mode: the strict bit the samplers, k_rescore_strict and trial_rejected read, and the two exact routes
    if (a.flags & ESAC_FLAG_STRICT_TRAINING) a.flags |= ESAC_FLAG_STRICT_REFERENCE | ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;
    c->epoch += 1.0;  // every call gets its own epoch: result hand-off word and the tag of the status word
    a.epoch = c->epoch;
    a.sample_epoch = c->sample_epoch;  // launches that sample call mark_sampling() and overwrite this
    // (device-side span stamps only on sampled calls in timing mode: forward_impl clears tstamps otherwise)
    if (!c->keep_errs) a.errs = nullptr;
    // band of the fp32 maximum that is re-scored exactly: the stream's rounding (<= 2e-5 * alpha measured) plus two
    // cells' weight -- an ill-conditioned projection (scene point next to the camera centre) can put a cell on the other
    // side of tau under fp32, which moves a score by alpha / (H*W); on small grids that exceeds alpha * 1e-3
    a.margin = p->rescore_margin > 0 ? p->rescore_margin : fabsf(p->inlier_alpha) * (ESAC_DEFAULT_MARGIN + 2.0f / (float)P);
    c->lastN = p->N; c->lastH = p->H; c->lastW = p->W;
    c->lastB = B;
    c->last_dev_batch = 0;  // (esac_hip_backward_batch_dev sets it again once its launches are queued)
    *out = a;
    return 0;
}

// Per-frame cameras of a batch: every record checked like a single call's camera (p: the call's parameters, already validated by
// make_args with record 0), then staged in pinned memory of the context's own and uploaded on `s` -- once per call; chunks and
// re-runs offset the device pointer.  The staging is rewritten only after the previous upload has left it (an asynchronous
// forward batch may still have its copy queued); the device table is rewritten in stream order behind its last readers.
static int stage_cams(esac_hip_ctx* c, const esac_hip_params* p, const esac_hip_frame_cam* h_cams, int B, hipStream_t s) {
    static_assert(sizeof(esac_hip_frame_cam) == sizeof(FrameCam) && offsetof(esac_hip_frame_cam, focal) == offsetof(FrameCam, focal) &&
                  offsetof(esac_hip_frame_cam, ppy) == offsetof(FrameCam, ppy), "esac_hip_frame_cam is the device record");
    for (int b = 0; b < B; b++)
        if (int rc = check_cam(p, h_cams[b].shift_x, h_cams[b].shift_y, h_cams[b].focal, b)) return rc;
    if (!c->h_cams) {
        HIP_OK(hipHostMalloc((void**)&c->h_cams, (size_t)ESAC_MAX_BATCH * sizeof(FrameCam), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&c->d_cams, (size_t)ESAC_MAX_BATCH * sizeof(FrameCam)));
        HIP_OK(hipEventCreateWithFlags(&c->cams_ev, hipEventDisableTiming));
    }
    if (c->cams_queued) {
        HIP_OK(hipEventSynchronize(c->cams_ev));
        c->cams_queued = false;
    }
    memcpy(c->h_cams, h_cams, (size_t)B * sizeof(FrameCam));
    HIP_OK(hipMemcpyAsync(c->d_cams, c->h_cams, (size_t)B * sizeof(FrameCam), hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(c->cams_ev, s));
    c->cams_queued = true;
    return 0;
}

// The forward path's team request: off while the context is latched (two team time-outs in a row, see forward_impl).  The latch is
// the FORWARD path's: the training path's slot teams have a switch of their own (esac_hip_ctx::slot_teams).
static void forward_team(const esac_hip_ctx* c, KArgs& a) {
    if (c->team_latched_off) a.team = 0;
    if (a.flags & ESAC_FLAG_REFINE_SOLO) {
        a.team = 0;
        a.solo = 1;
    }
}

static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-200 - (int)e, "launch of %s failed: %s", what, hipGetErrorString(e));
    return 0;
}

// A launch that (re)samples the hypotheses: the status word (out-of-range hypAssignment) is tagged with ITS epoch, and
// every later stage / check on this context compares against that -- not against the epoch of whatever call came last.
// (The sampler forms the fp32 [R|t] rows of its hypotheses itself: nothing of esac_hip_write_hyps is left to rebuild.)
static void mark_sampling(esac_hip_ctx* c, KArgs& a) {
    c->rt32_stale = false;
    c->sample_epoch = a.epoch;
    a.sample_epoch = a.epoch;
}

// hypotheses that came from esac_hip_write_hyps: the first stage that reads their fp32 [R|t] rows and rotation matrices forms them
static void ensure_rt32(esac_hip_ctx* c, const KArgs& a, hipStream_t s) {
    if (c->rt32_stale) launch_hyps_to_rt32(a, s);
    c->rt32_stale = false;
}
// stage entry points: validate, make the context's GPU current, launch one phase on the caller's stream
template <typename Launch>
static int run_stage(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream,
                     const char* what, Launch launch) {
    if (!c) return fail(-1, "null context");
    DeviceGuard guard(c->device);
    KArgs a;
    int rc = make_args(c, d_sc, d_assign, p, &a);
    if (rc) return rc;
    launch(c, a, (hipStream_t)stream);
    return check_launch(what);
}
extern "C" int esac_hip_sample(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_sample", [](esac_hip_ctx* cc, const KArgs& a0, hipStream_t s) {
        KArgs a = a0;
        mark_sampling(cc, a);
        launch_sample(a, s);
    });
}
extern "C" int esac_hip_score(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_score_fast", [](esac_hip_ctx* cc, const KArgs& a, hipStream_t s) {
        ensure_rt32(cc, a, s);
        launch_score(a, s);
    });
}
extern "C" int esac_hip_select(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_select_rescore", [](esac_hip_ctx* cc, const KArgs& a, hipStream_t s) {
        ensure_rt32(cc, a, s);
        launch_select_rescore(a, s);
    });
}
extern "C" int esac_hip_refine(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_refine", [](esac_hip_ctx* cc, const KArgs& a0, hipStream_t s) {
        KArgs a = a0;
        forward_team(cc, a);
        cc->refine_tag = launch_refine(a, s);
    });
}
extern "C" int esac_hip_score_exact(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_rescore(all)", [](esac_hip_ctx* cc, const KArgs& a, hipStream_t s) {
        ensure_rt32(cc, a, s);
        launch_rescore_all(a, s);
        launch_stats_exact(a, s);  // softmax statistics of the exact scores (the record's probability / entropy)
    });
}

// Blocking calls: the last kernel stores the record and the call's epoch word into pinned host memory (one ESAC_PIN_DOUBLES slot
// per frame: record, epoch word, status word, check word) and the host polls.  A slot has landed when its epoch word is this
// call's AND its check word fits the other 34 words (the kernel stores them without a fence: esac_kernels.hpp, pin_mix).
static int wait_record(esac_hip_ctx* c, hipStream_t s, int B, double want, const char* who) {
    auto all_landed = [&]() {
        for (int b = 0; b < B; b++) {
            const volatile unsigned long long* w = reinterpret_cast<const volatile unsigned long long*>(c->h_pin + (size_t)b * ESAC_PIN_DOUBLES);
            if (*(const volatile double*)(c->h_pin + (size_t)b * ESAC_PIN_DOUBLES + 32) != want) return false;
            unsigned long long h = 0;
            for (int k = 0; k < 34; k++) h ^= pin_mix(w[k], k);
            if (h != w[34]) return false;
        }
        return true;
    };
    bool landed = false;
    if (c->wait_mode == ESAC_WAIT_BLOCK) {
        HIP_OK(hipStreamSynchronize(s));
        landed = all_landed();
    } else {
        const bool yield = c->wait_mode == ESAC_WAIT_YIELD;
        for (long spins = 0; spins < 200000000L; spins++) {
            if (all_landed()) {
                landed = true;
                break;
            }
            if (yield) sched_yield();
            if ((spins & (yield ? 63 : 1023)) == (yield ? 63 : 1023) && hipStreamQuery(s) == hipSuccess) {  // stream idle: kernels are done (or failed)
                landed = all_landed();
                break;
            }
        }
    }
    if (!landed) {
        HIP_OK(hipStreamSynchronize(s));
        if (!all_landed()) return fail(-9, "%s did not deliver a result record", who);
    }
    return 0;
}

// ---- the steps of a forward call (forward_impl strings them together)
static double pin_status(const esac_hip_ctx* c, int b) { return c->h_pin[(size_t)b * ESAC_PIN_DOUBLES + ESAC_PIN_STATUS]; }
// ESAC_FLAG_AUTO_EXACT: the guaranteed routes where they are free (include/esac_hip.h)
static void apply_auto_exact(KArgs& a, int B) {
    if ((a.flags & ESAC_FLAG_AUTO_EXACT) && B == 1 && a.E == 1 && (long long)a.N * a.H * a.W <= ESAC_AUTO_EXACT_MAX_WORK)
        a.flags |= ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING;
}
// KArgs::fold_select of the serial route (a team that refines <= 256 hypotheses of one frame runs their selection in its prologue)
static int serial_fold(const esac_hip_ctx* c, const KArgs& a) {
    return !c->fold_select ? 0 : refine_folds_select(a) ? 1 : refine_folds_exact_stats(a) ? 2 : 0;
}
// Stage k of the serial route (0: sample, 1: score, 2: select, 3: refine); returns the name check_launch reports it under.
// ESAC_FLAG_EXACT_SCORES: every hypothesis scored in the reference's arithmetic (esac_util.h:235-260), softmax
// statistics from those scores -- the score vector, probability and entropy are then the reference's own values
static inline const char* enqueue_serial_stage(esac_hip_ctx* c, const KArgs& a, int k, hipStream_t s) {
    const bool exact = (a.flags & ESAC_FLAG_EXACT_SCORES) != 0;
    switch (k) {
        case 0: launch_sample(a, s); return "k_sample";
        case 1: if (exact) launch_rescore_all(a, s); else launch_score(a, s); return exact ? "k_rescore(all)" : "k_score_fast";
        case 2: if (exact) { if (a.fold_select != 2) launch_stats_exact(a, s); } else if (!a.fold_select) launch_select_rescore(a, s); return exact ? "k_stats_exact" : "k_select_rescore";
        default: c->refine_tag = launch_refine(a, s); return "k_refine";
    }
}
// a team timed out: twice in a row and the context stops asking for teams (every call would pay the time-out first) until re-armed
static void note_team_timeout(esac_hip_ctx* c) {
    c->team_fallbacks++;
    if (++c->team_strikes >= ESAC_TEAM_STRIKES && !c->team_latched_off) {
        c->team_latched_off = true;
        c->solo_since_latch = 0;
    }
}
// A forward call up to its first launch (p carries record 0 of a per-frame camera table in its inline fields); *tm: the call is timed
static int prepare_forward(esac_hip_ctx* c, const float* d_sc, long long sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p,
                           int B, hipStream_t s, const esac_hip_frame_cam* h_cams, double t_entry, KArgs* out, bool* tm) {
    KArgs& a = *out;
    int rc = make_args(c, d_sc, d_assign, p, &a, B, sc_frame_stride, h_cams ? 0 : -1);
    if (rc) return rc;
    if (h_cams && B > 1) {  // (one frame: record 0 is the whole table)
        if ((rc = stage_cams(c, p, h_cams, B, s))) return rc;
        a.cams = c->d_cams;
    }
    if (c->team_latched_off && ++c->solo_since_latch > ESAC_TEAM_REARM_CALLS) {  // (blocking or not: every forward call counts)
        c->team_latched_off = false;               // try a team again; one more time-out latches at once
        c->team_strikes = ESAC_TEAM_STRIKES - 1;
    }
    forward_team(c, a);
    c->host_ns[6] = t_entry;
    c->host_ns[0] = now_ns() - t_entry;
    apply_auto_exact(a, B);
    // events and stamps cost GPU time themselves (an empty event pair reads ~5 us): sample every timing_period-th call
    *tm = c->timing && (c->timing_calls++ % c->timing_period) == 0;
    // device-side span stamps: only the per-hypothesis stream (k_score_fast) writes them, and k_select_rescore reduces them --
    // a call whose selection runs in the refinement kernel's prologue keeps ITS launch sequence under timing (the phase
    // events then bracket what an untimed call runs) and takes no stamps
    if (!*tm || a.partials || (a.flags & ESAC_FLAG_EXACT_SCORES)) a.tstamps = nullptr;
    if (a.tstamps) {
        KArgs probe = a;
        probe.tstamps = nullptr;
        if (c->fold_select && refine_folds_select(probe)) a.tstamps = nullptr;
    }
    return 0;
}

// Several experts: the sampler's straggler chain (wrong-expert hypotheses, which practically never win) runs BESIDE the scoring,
// selection and refinement of what the first pass settled (KArgs::spec_mode; k_spec_join makes the outputs the serial order's)
// (not where the selection runs in the refinement kernel's prologue -- a single frame of <= 256 hypotheses on a team: that
// route re-scores its contenders member by member, another summation order than k_select_rescore's and k_spec_join's)
static bool speculation_eligible(const esac_hip_ctx* c, const KArgs& a, int B, hipStream_t s) {
    if (c->spec_off || B != 1 || (a.flags & ESAC_FLAG_EXACT_SCORES) || !sample_can_split(a) || a.partials || (long long)a.H * a.W >= 32768 ||
        (c->fold_select && refine_folds_select(a)))
        return false;
    if (s == nullptr) return true;
    // a stream that is being captured into a graph takes no launches on other streams beside it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool plain = hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return plain;
}
static int ensure_spec_streams(esac_hip_ctx* c) {
    if (!c->side) HIP_OK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    if (!c->side2) HIP_OK(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
    if (!c->spec_ev) HIP_OK(hipEventCreateWithFlags(&c->spec_ev, hipEventDisableTiming));
    return 0;
}
static int enqueue_speculative(esac_hip_ctx* c, KArgs& a, hipStream_t s, bool tm, double t_entry) {
    c->spec_calls++;
    c->last_spec_epoch = a.epoch;
    a.tstamps = nullptr;
    a.fold_select = 0;
    a.spec_flag = c->ws.spec_flag;
    KArgs chain;
    int chain_waves = 0;
    // The caller's stream may hold any amount of work ahead of this call (the expert networks that produce d_sc), and the
    // context's own streams are ordered against it by nothing else: they wait for THIS event before anything of this call
    // runs on them, so that their bounded waits for the hand-off words below start counting when the caller's stream has
    // reached the call -- not when the host enqueued it.  (Recorded here, in front of the first pass: on an idle stream it
    // is satisfied long before the two streams get their first launch, and their wait for it sits beside the first pass and
    // the score kernel, off the critical path.)
    HIP_OK(hipEventRecord(c->spec_ev, s));
    launch_sample_split(a, s, &chain, &chain_waves);
    if (int rc = check_launch("k_sample (first pass)")) return rc;
    c->host_ns[1] = now_ns() - t_entry;
    if (tm) HIP_OK(hipEventRecord(c->ev[1], s));
    // WITHIN the call the streams hand over through WORDS in device memory (spec_state[3]: "the chain may start", [4]: "the
    // chain is done"), not through events: an event between two streams costs the waiting side 8-13 us on this platform even
    // when it is long satisfied (profiles/r06_ab_speculation.txt).  Whoever waits is enqueued BEHIND the launch it waits for
    // (host order below), so that even two streams that share a hardware queue cannot wait for each other; every wait is
    // bounded in wall time -- and begins behind spec_ev, i.e. when the caller's stream has reached this call.
    KArgs as = a;  // the settled hypotheses: score, selection, refinement of their winner -- no record leaves the workspace
    as.spec_mode = 1;
    as.result_user = nullptr;
    as.result_pin = nullptr;
    launch_score(as, s);
    if (int rc = check_launch("k_score_fast (settled)")) return rc;
    c->host_ns[2] = now_ns() - t_entry;
    if (tm) HIP_OK(hipEventRecord(c->ev[2], s));
    // The chain starts when the speculative refinement has its CUs, not when the first pass is done: its thousands of
    // single-wavefront workgroups fill every SIMD of the chip, and whatever the launch stream starts while it is in full
    // swing finds no CU to run on until it has drained (measured: started behind the first pass, the selection took 27 us
    // instead of 10; started behind the score kernel, the refinement's team waited 34 us for its CUs).
    // The SELECTION among the settled hypotheses is not on the critical path either (round 6, second half).  The refinement starts
    // from the fp32 argmax of the settled hypotheses (spec_mode 2: spec_pick_fast) right behind the score kernel; the selection
    // kernel (band, exact re-scores) and the join behind it run on a second stream of the context's own, the join resident and
    // waiting when the refinement and the chain finish ("the refinement is done": spec_state[6]); the gated second refinement
    // on the caller's stream waits for the join's verdict ("the join is done": spec_state[7]).  Every waiter is enqueued
    // behind what it waits for.  (With selection and join on the caller's stream, in front of and behind the refinement:
    // cfg3 0.1404 ms against 0.1288, cfg4 0.1915 against 0.184, same box -- profiles/r06_ab_select_beside.txt.)
    if (tm) HIP_OK(hipEventRecord(c->ev[3], s));
    KArgs ar = as;
    ar.spec_mode = 2;
    ar.spec_debug = c->spec_second_best ? 1 : 0;
    c->refine_tag = launch_refine(ar, s);  // (its first workgroup opens the chain: spec_open_chain)
    c->refine_was_team = refine_team_members(ar) > 0;
    if (int rc = check_launch("k_refine (speculative)")) return rc;
    // (host order: the selection first -- the join waits behind it; a launch call is 3-4 us of host time, and the chain's five
    // in front of it would hold the selection back by 20 us.  The JOIN is enqueued behind the chain it waits for.)
    HIP_OK(hipStreamWaitEvent(c->side2, c->spec_ev, 0));
    launch_spec_wait(a, 3, c->side2);
    launch_select_rescore(as, c->side2);
    if (int rc = check_launch("k_select_rescore (settled)")) return rc;
    HIP_OK(hipStreamWaitEvent(c->side, c->spec_ev, 0));
    launch_spec_wait(a, 3, c->side);
    launch_sample_stragglers(chain, chain_waves, c->side);
    if (!c->spec_lose_chain) launch_score_stragglers(a, c->side);  // behind the chain on the side stream; its last workgroup writes "the chain is done"
    if (int rc = check_launch("straggler chain")) return rc;
    launch_spec_join(a, c->side2);
    if (int rc = check_launch("k_spec_join")) return rc;
    // The second refinement is enqueued NOW and returns at once unless the join marked the speculation as failed
    // (KArgs::spec_gate): a failed speculation then costs the refinement, not a host round trip on top of it (and an
    // asynchronous call could not look at the join's verdict anyway); a speculation that held has delivered its record
    // before the gate opens
    KArgs ag = a;
    ag.spec_gate = 1;
    (void)launch_refine(ag, s);  // (esac_hip_check follows the speculative launch's tag: a team time-out there is the common case of the two)
    if (int rc = check_launch("k_refine (gated)")) return rc;
    c->host_ns[3] = now_ns() - t_entry;
    return 0;
}
// Blocking call, after its record has landed.  The members of a team did not all become resident in time (a shared or partitioned
// GPU, or the caller's own kernels on another stream holding the CUs): the same refinement(s) in ONE workgroup each -- the
// hypotheses, scores and selection of this call are still in the workspace.  Then the slots to the caller's records, and the
// status words as error codes.
static int collect_records(esac_hip_ctx* c, KArgs& a, int B, hipStream_t s, double* h_result_out) {
    bool team_failed = false, bad_assign = false, timed_out = false;
    for (int b = 0; b < B; b++) team_failed |= pin_status(c, b) == ESAC_PIN_TEAM_TIMEOUT;
    const bool was_team = refine_team_members(a) > 0;
    if (team_failed && was_team) {
        note_team_timeout(c);
        a.epoch = c->epoch += 1.0;
        a.team = 0; a.solo = 1;
        if (a.fold_select) {  // the selection was that kernel's too
            a.fold_select = 0;
            enqueue_serial_stage(c, a, 2, s);
        }
        enqueue_serial_stage(c, a, 3, s);
        if (int rc = check_launch("k_refine (one workgroup, after a team time-out)")) return rc;
        if (int rc = wait_record(c, s, B, c->epoch, "esac_hip_forward: the refinement kernel")) return rc;
    } else if (was_team) {
        c->team_strikes = 0;
    }
    __sync_synchronize();
    for (int b = 0; b < B; b++) {
        memcpy(h_result_out + (size_t)b * ESAC_RES_DOUBLES, (const void*)(c->h_pin + (size_t)b * ESAC_PIN_DOUBLES),
               ESAC_RES_DOUBLES * sizeof(double));
        bad_assign |= pin_status(c, b) == ESAC_PIN_BAD_ASSIGN;
        timed_out |= pin_status(c, b) == ESAC_PIN_TEAM_TIMEOUT;
    }
    if (timed_out) return fail(-12, "esac_hip_forward: the cooperating refinement workgroups could not synchronise (not all of them became resident)");
    if (bad_assign)
        return fail(-10, "hypAssignment holds a value outside [0,%d) (device-resident tensor; such hypotheses were scored against expert 0)", a.E);
    return 0;
}

static int forward_impl(esac_hip_ctx* c, const float* d_sc, long long sc_frame_stride, const int64_t* d_assign,
                        const esac_hip_params* p, int B, void* stream, double* d_scores_out, double* d_result_out,
                        double* h_result_out, const esac_hip_frame_cam* h_cams = nullptr) {
    if (!c) return fail(-1, "null context");
    const double t_entry = now_ns();
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    esac_hip_params p0;
    if (h_cams && p) {  // the inline fields carry record 0 (device_common.hpp:frame_view)
        p0 = with_cam(*p, h_cams[0]);
        p = &p0;
    }
    KArgs a;
    bool tm = false;
    int rc = prepare_forward(c, d_sc, sc_frame_stride, d_assign, p, B, s, h_cams, t_entry, &a, &tm);
    if (rc) return rc;
    a.scores_user = d_scores_out; a.result_user = d_result_out;
    a.result_pin = h_result_out ? c->d_pin : nullptr;
    c->last_spec_epoch = 0;
    const bool spec = speculation_eligible(c, a, B, s);
    if (spec && (rc = ensure_spec_streams(c))) return rc;
    if (tm) HIP_OK(hipEventRecord(c->ev[0], s));
    mark_sampling(c, a);
    if (spec) {
        if ((rc = enqueue_speculative(c, a, s, tm, t_entry))) return rc;
    } else {
        constexpr int stamp[4] = {1, 2, 0, 3};  // the host_ns slot stamped behind stage k (the selection has none)
        for (int k = 0; k < 4; k++) {
            if (k == 2) a.fold_select = serial_fold(c, a);
            const char* what = enqueue_serial_stage(c, a, k, s);
            if (k == 3) c->refine_was_team = refine_team_members(a) > 0;
            if ((rc = check_launch(what))) return rc;
            if (stamp[k]) c->host_ns[stamp[k]] = now_ns() - t_entry;
            if (tm && k < 3) HIP_OK(hipEventRecord(c->ev[k + 1], s));
        }
    }
    if (tm) {
        HIP_OK(hipEventRecord(c->ev[4], s));
        // an EMPTY interval: what two adjacent hipEventRecord calls measure with nothing in between,
        // i.e. the part of every bracketed phase that is not kernel time
        HIP_OK(hipEventRecord(c->ev[5], s));
        HIP_OK(hipEventRecord(c->ev[6], s));
        c->ev_valid = true;
    }
    if (h_result_out) {
        if ((rc = wait_record(c, s, B, c->epoch, "esac_hip_forward: the refinement kernel"))) return rc;
        if (spec && pin_status(c, 0) == ESAC_PIN_NO_CHAIN) {
            // the context's own stream never reported the straggler chain as done within 20 ms (it shares a hardware queue with
            // the caller's stream and something else is holding that queue, or its launch failed): no more speculation on this
            // context, and this call again -- the serial route
            c->spec_off = c->spec_env_off = true;
            HIP_OK(hipStreamSynchronize(c->side));
            if (c->side2) HIP_OK(hipStreamSynchronize(c->side2));
            HIP_OK(hipStreamSynchronize(s));
            // (p, no h_cams: a speculative call is ONE frame, whose camera table is record 0 -- in p's inline fields already, and checked)
            return forward_impl(c, d_sc, sc_frame_stride, d_assign, p, B, stream, d_scores_out, d_result_out, h_result_out);
        }
        c->host_ns[4] = now_ns() - t_entry;
        if ((rc = collect_records(c, a, B, s, h_result_out))) return rc;
    }
    c->host_ns[5] = now_ns() - t_entry;
    if (h_result_out) {  // running sums (seven additions: the caller's timed loop is not touched by reading them later)
        for (int k = 0; k < 6; k++) c->host_sum[k] += c->host_ns[k];
        if (c->host_last_return > 0) c->host_sum[6] += t_entry - c->host_last_return;  // the caller's time between two calls
        c->host_last_return = t_entry + c->host_ns[5];
        c->host_n++;
    }
    return 0;
}

extern "C" int esac_hip_host_turn_mean(esac_hip_ctx* c, double out_ns[8], int reset) {
    if (!c || !out_ns) return fail(-1, "esac_hip_host_turn_mean: null argument");
    const double n = c->host_n > 0 ? (double)c->host_n : 1.0;
    for (int k = 0; k < 6; k++) out_ns[k] = c->host_sum[k] / n;
    out_ns[6] = c->host_n > 1 ? c->host_sum[6] / (double)(c->host_n - 1) : 0.0;
    out_ns[7] = (double)c->host_n;
    if (reset) {
        for (double& v : c->host_sum) v = 0;
        c->host_n = 0;
        c->host_last_return = 0;
    }
    return 0;
}

extern "C" int esac_hip_host_turn(esac_hip_ctx* c, double out_ns[8]) {
    if (!c || !out_ns) return fail(-1, "esac_hip_host_turn: null argument");
    for (int k = 0; k < 8; k++) out_ns[k] = c->host_ns[k];
    return 0;
}

// Mean GPU time of each stage of the forward chain for THIS input: the chain runs once, then every stage is launched
// `reps` times back to back between one pair of hipEvents on `stream` (stages are idempotent given their inputs).
// A host-side loop around single launches cannot do this for ~5 us kernels: it is bound by the caller's launch rate.
extern "C" int esac_hip_time_stages(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p,
                                    void* stream, int reps, float out_ms[4]) {
    if (!c || !out_ms || reps < 1) return fail(-1, "esac_hip_time_stages: bad argument");
    DeviceGuard guard(c->device);
    KArgs a;
    int rc = make_args(c, d_sc, d_assign, p, &a);
    if (rc) return rc;
    a.tstamps = nullptr;
    forward_team(c, a);
    hipStream_t s = (hipStream_t)stream;
    mark_sampling(c, a);
    apply_auto_exact(a, 1);
    // the serial route of esac_hip_forward; where the refinement kernel runs the selection, stage 2 is part of stage 3 (reads 0)
    a.fold_select = serial_fold(c, a);
    for (int k = 0; k < 4; k++) enqueue_serial_stage(c, a, k, s);
    if ((rc = check_launch("forward chain"))) return rc;
    hipEvent_t ev[8];
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    for (int k = 0; k < 4; k++) {
        enqueue_serial_stage(c, a, k, s);  // one untimed launch: the timed ones then start from the same (warm) state
        HIP_OK(hipEventRecord(ev[2 * k], s));
        for (int r = 0; r < reps; r++) enqueue_serial_stage(c, a, k, s);
        HIP_OK(hipEventRecord(ev[2 * k + 1], s));
    }
    if ((rc = check_launch("stage timing"))) return rc;
    HIP_OK(hipEventSynchronize(ev[7]));
    for (int k = 0; k < 4; k++) {
        HIP_OK(hipEventElapsedTime(&out_ms[k], ev[2 * k], ev[2 * k + 1]));
        out_ms[k] /= (float)reps;
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return 0;
}

// Multi-GPU exchange (esac_amd/distributed.py): winner among the per-rank records of the all-reduced buffer.
extern "C" int esac_hip_pick_record(esac_hip_ctx* c, const double* d_records, int world, void* stream, double* h_record_out, double* d_zero,
                                    int n_zero) {
    if (!c || !d_records || !h_record_out || world < 1 || n_zero < 0 || (n_zero > 0 && !d_zero))
        return fail(-1, "esac_hip_pick_record: bad argument");
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    c->epoch += 1.0;
    const double want = c->epoch;
    launch_pick_record(d_records, world, c->d_pin, want, d_zero, n_zero, s);
    int rc = check_launch("k_pick_record");
    if (rc) return rc;
    volatile double* word = c->h_pin + 32;
    bool landed = false;
    for (long spins = 0; spins < 200000000L; spins++) {
        if (*word == want) {
            landed = true;
            break;
        }
        if ((spins & 1023) == 1023 && hipStreamQuery(s) == hipSuccess) {
            landed = *word == want;
            break;
        }
    }
    if (!landed) {
        HIP_OK(hipStreamSynchronize(s));
        if (*word != want) return fail(-9, "esac_hip_pick_record: the kernel did not deliver a record");
    }
    __sync_synchronize();
    memcpy(h_record_out, (const void*)c->h_pin, ESAC_RES_DOUBLES * sizeof(double));
    if (pin_status(c, 0) == ESAC_PIN_TEAM_TIMEOUT)
        return fail(-12, "esac_hip_pick_record: the refinement team of at least one rank timed out (its record carries ESAC_RES_VALID = 3); "
                         "every rank sees the same records: run the frame again with ESAC_FLAG_REFINE_SOLO");
    if (pin_status(c, 0) == ESAC_PIN_NONE) return fail(-11, "esac_hip_pick_record: no rank produced a hypothesis");
    return 0;
}

// ---- the one collective of the multi-GPU path, straight on RCCL (esac_amd/distributed.py bootstraps the id over the caller's
// process group; the per-frame data path then never enters torch.distributed, whose enqueue of a collective costs the host
// 20-27 us a call: bench.py sharded_world1).  RCCL is bound at the first esac_hip_comm_* call, not at link time: a single-GPU
// process never maps the 570 MB library, and one that already holds a copy (torch ships its own librccl.so.1) gets that copy.
#define RCCL_BOUND() \
    if (!rccl().ok) return fail(-14, "RCCL is not available in this process (librccl.so.1 could not be loaded)")
#define NCCL_OK(expr)                                                                                       \
    do {                                                                                                    \
        ncclResult_t _r = (expr);                                                                           \
        if (_r != ncclSuccess) return fail(-300 - (int)_r, "%s: %s", #expr, rccl().error_string(_r));       \
    } while (0)
extern "C" int esac_hip_comm_unique_id(void* out, size_t bytes) {
    if (!out || bytes < sizeof(ncclUniqueId)) return fail(-1, "esac_hip_comm_unique_id: need %zu bytes", sizeof(ncclUniqueId));
    RCCL_BOUND();
    ncclUniqueId id;
    NCCL_OK(rccl().get_unique_id(&id));
    memcpy(out, &id, sizeof(id));
    return 0;
}
extern "C" int esac_hip_comm_init(esac_hip_ctx* c, int nranks, int rank, const void* unique_id, size_t bytes) {
    if (!c || !unique_id || bytes < sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(-1, "esac_hip_comm_init: bad argument");
    RCCL_BOUND();
    DeviceGuard guard(c->device);
    drop_comm(c);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    NCCL_OK(rccl().comm_init_rank(&c->comm, nranks, id, rank));
    c->comm_ranks = nranks;
    c->comm_rank = rank;
    return 0;
}
extern "C" int esac_hip_comm_destroy(esac_hip_ctx* c) {
    if (!c) return fail(-1, "null context");
    DeviceGuard guard(c->device);
    drop_comm(c);
    return 0;
}
extern "C" int esac_hip_allreduce_sum(esac_hip_ctx* c, double* d_buf, size_t count, void* stream) {
    if (!c || !d_buf) return fail(-1, "esac_hip_allreduce_sum: null argument");
    if (!c->comm) return fail(-13, "esac_hip_allreduce_sum: no communicator (esac_hip_comm_init)");
    DeviceGuard guard(c->device);
    NCCL_OK(rccl().all_reduce(d_buf, d_buf, count, NCCL_DOUBLE, NCCL_SUM, c->comm, (hipStream_t)stream));
    return 0;
}
// What the communicator ITSELF reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), beside what the context was told
// and the GPU it is bound to: the proof a multi-GPU bench line carries of how many ranks RCCL saw (bench.py: ranks_seen).
extern "C" int esac_hip_comm_info(esac_hip_ctx* c, int32_t out[4]) {
    if (!c || !out) return fail(-1, "esac_hip_comm_info: null argument");
    if (!c->comm) return fail(-13, "esac_hip_comm_info: no communicator (esac_hip_comm_init)");
    int count = c->comm_ranks, rank = c->comm_rank, dev = -1;
    if (rccl().comm_count) NCCL_OK(rccl().comm_count(c->comm, &count));
    if (rccl().comm_user_rank) NCCL_OK(rccl().comm_user_rank(c->comm, &rank));
    if (rccl().comm_cu_device) NCCL_OK(rccl().comm_cu_device(c->comm, &dev));
    out[0] = count;
    out[1] = rank;
    out[2] = dev;
    out[3] = c->device;
    return 0;
}

extern "C" int esac_hip_forward(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p,
                                void* stream, double* d_scores_out, double* d_result_out, double* h_result_out) {
    return forward_impl(c, d_sc, 0, d_assign, p, 1, stream, d_scores_out, d_result_out, h_result_out);
}

extern "C" int esac_hip_forward_batch(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride,
                                      const int64_t* d_assign, const esac_hip_params* p, void* stream,
                                      double* d_scores_out, double* d_result_out, double* h_result_out) {
    return esac_hip_forward_batch_cams(c, B, d_sc, sc_frame_stride, d_assign, p, nullptr, stream, d_scores_out, d_result_out, h_result_out);
}

extern "C" int esac_hip_forward_batch_cams(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride,
                                           const int64_t* d_assign, const esac_hip_params* p, const esac_hip_frame_cam* h_cams,
                                           void* stream, double* d_scores_out, double* d_result_out, double* h_result_out) {
    if (h_cams && (B < 1 || B > ESAC_MAX_BATCH)) return fail(-4, "batch size %d outside [1,%d]", B, ESAC_MAX_BATCH);  // (before h_cams[0] is read)
    return forward_impl(c, d_sc, (long long)sc_frame_stride, d_assign, p, B, stream, d_scores_out, d_result_out, h_result_out, h_cams);
}

// ---------------------------------------------------------------- training path
// `cap` = slots (hypotheses with p >= PROB_THRESH) per frame the slab workspace must hold, for B frames (a batch: every buffer
// frame-major, device_common.hpp:bwd_frame_view); it only ever grows
static int ensure_bws(esac_hip_ctx* c, int N, int P, int cap, int B = 1) {
    const bool lists = P > ESAC_REFINE_LDS_CAP;
    const long long NB = (long long)N * B, slots = (long long)cap * B, rows = (long long)bwd_rows(N) * B;
    if (NB <= c->bN && P <= c->bP && slots <= c->bslots && rows <= c->brows && B <= c->bB && (!lists || c->b_lists)) return 0;
    HIP_OK(hipDeviceSynchronize());
    const long long nN = NB > c->bN ? NB : c->bN, nslots = slots > c->bslots ? slots : c->bslots, nrows = rows > c->brows ? rows : c->brows;
    const int nP = P > c->bP ? P : c->bP, nB = B > c->bB ? B : c->bB;
    const bool nlists = lists || c->b_lists;
    free_bws(c);
    int rc = 0;
    rc |= alloc(&c->bws.sel, (size_t)nN);
    rc |= alloc(&c->bws.n_sel, (size_t)4 * nB);
    rc |= alloc(&c->bws.probs, (size_t)nN);
    rc |= alloc(&c->bws.losses, (size_t)nN);
    rc |= alloc(&c->bws.ref_hyps, (size_t)nN * 6);
    rc |= alloc(&c->bws.sgrad, (size_t)nN);
    rc |= alloc(&c->bws.dloss, (size_t)nrows * 6);  // small per-slot tables: worst case min(N, 1000) rows per frame
    rc |= alloc(&c->bws.maps, (size_t)nslots * 2 * nP);
    rc |= alloc(&c->bws.map_info, (size_t)nrows * 4);
    if (nlists) {
        char* cl = nullptr;
        rc |= alloc(&cl, (size_t)nslots * ((size_t)nP + 2048) * 16);  // corr_entries(P) < P + 2048 per slot
        c->bws.corr_lists = cl;
    }
    rc |= alloc(&c->bws.grad1, (size_t)nslots * nP * 3);
    rc |= alloc(&c->bws.grad2, (size_t)nslots * nP * 3);
    rc |= alloc(&c->bws.out, (size_t)4 * nB);
    rc |= alloc(&c->bws.arrived, (size_t)1);
    rc |= alloc(&c->bws.sel_max, (size_t)1);
    rc |= alloc(&c->bws.team_gran, (size_t)nslots * 2 * ESAC_REFINE_TEAM_MAX * 32 * 2);  // 16-byte granules: [slot][parity][member][value]
    if (rc) {
        free_bws(c);
        return rc;
    }
    HIP_OK(hipMemset(c->bws.n_sel, 0, (size_t)4 * nB * sizeof(int)));
    HIP_OK(hipMemset(c->bws.arrived, 0, sizeof(int)));
    HIP_OK(hipMemset(c->bws.sel_max, 0, sizeof(int)));
    HIP_OK(hipMemset(c->bws.team_gran, 0, (size_t)nslots * 2 * ESAC_REFINE_TEAM_MAX * 32 * 2 * sizeof(double)));
    c->bN = nN; c->bP = nP; c->bslots = nslots; c->brows = nrows; c->bB = nB; c->b_lists = nlists;
    return 0;
}

// Bytes of slot workspace one slot is CHARGED against the context's budget (ESAC_BWD_BATCH_BUDGET_MB): two inlier maps, the two
// 3P-double slabs, and the correspondence list at its true size corr_entries(P).  The batched calls size their chunks by this
// and nothing else.  It is less than ensure_bws allocates per slot: that rounds the list up to its bound P + 2048 entries and
// adds the slot's team granules (2 * ESAC_REFINE_TEAM_MAX * 32 granules of 16 bytes), and the per-frame tables (selection,
// probabilities, losses, poses, dloss, map_info: a few dozen bytes per hypothesis) are not charged at all.  The chunk sizes
// that tests and callers see under a given budget follow from this value, so it stays what it is.
static long long bwd_slot_bytes(int P) {
    return 2LL * P + 2LL * 3 * P * (long long)sizeof(double) + (P > ESAC_REFINE_LDS_CAP ? corr_entries(P) * 16 : 0);
}

// The slot count a rerun after an overflow is sized by: the selection's true count in whole 32s, at most the worst case
static int grown_cap(int needed, int worst) { return needed + 31 > worst ? worst : (needed + 31) / 32 * 32; }

// The loss's view of a ground-truth camera pose (gt_math.hpp: the text k_bwd_gt_prepare runs on the device), on the host.
// false: singular.
static bool gt_host(const float* h_gt_pose, double gt[16], double gt_pose[6]) { return gt_from_pose(h_gt_pose, gt, gt_pose); }

// The checks of the two batched entry points, before either touches the device.  Both report under `who` (the asynchronous call
// under the blocking call's name too: its callers match these messages); what they differ in is the result pointer -- `out` is
// host memory of the blocking call (async == false) and device memory of the asynchronous one, each with its own message and
// its own place in the order.
static int check_batch_call(const char* who, const esac_hip_ctx* c, const esac_hip_params* p, int B, bool tensors, bool async, const void* out,
                            int64_t sc_frame_stride, int64_t grad_frame_stride) {
    if (!c) return fail(-1, "null context");
    if (!p) return fail(-1, "null params");
    if (!tensors) return fail(-1, "%s: null coordinate, gradient, assignment or ground-truth pointer", who);
    if (async && !out) return fail(-1, "esac_hip_backward_batch_dev: d_out (device double[B,4]) is required");
    if (p->flags & ESAC_FLAG_STRICT_REFERENCE)
        return fail(-4, "%s: the training path has no strict mode (ESAC_FLAG_STRICT_REFERENCE is a forward flag)", who);
    if (!async && !out) return fail(-4, "%s: the batched call is blocking only: h_out (host double[B,4]) is required", who);
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "%s: batch size %d outside [1,%d]", who, B, ESAC_MAX_BATCH);
    if (p->d_hyp_index || p->hyp_offset)
        return fail(-4, "%s: sharded calls are not supported (the expectation needs every hypothesis)", who);
    if (p->E > 65535) return fail(-4, "%s: at most 65535 experts (one grid row per expert in the accumulation kernel)", who);
    if (p->E <= 0 || p->H <= 0 || p->W <= 0 || p->N <= 0) return fail(-4, "E=%d, H=%d, W=%d, N=%d must be positive", p->E, p->H, p->W, p->N);
    const long long slab = (long long)p->E * 3 * p->H * p->W;
    if (sc_frame_stride < 0) return fail(-4, "%s: negative coordinate frame stride", who);
    if (B > 1 && grad_frame_stride < slab)
        return fail(-4, "%s: gradient frame stride %lld < E*3*H*W = %lld (frames would share gradients)", who,
                    (long long)grad_frame_stride, slab);
    return 0;
}

// Hypotheses and their reference-arithmetic scores of every frame of `a` (per_frame_shape: each frame of a batch summed as a
// single call sums it)
static int enqueue_bwd_sampling(esac_hip_ctx* c, KArgs& a, hipStream_t s, bool per_frame_shape) {
    a.tstamps = nullptr;
    mark_sampling(c, a);
    launch_sample(a, s);                                        // esac.cpp:276; frame b of a batch: call p->call + b
    if (int rc = check_launch("k_sample")) return rc;
    launch_rescore_all(a, s, per_frame_shape);                  // esac.cpp:295-316, reference arithmetic for every hypothesis
    return check_launch("k_rescore(all)");
}

// The KArgs of a batch's chunk [b0, b0 + nb): camera record b0 in the inline fields, the call counter, the tensors and the camera
// table offset by the chunk's first frame (validated, workspaces grown, a fresh epoch: make_args)
static int chunk_args(esac_hip_ctx* c, const float* d_sc, int64_t sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p,
                      const esac_hip_frame_cam* h_cams, int b0, int nb, KArgs* a) {
    esac_hip_params pc = h_cams ? with_cam(*p, h_cams[b0]) : *p;
    pc.call = p->call + (uint64_t)b0;
    if (int rc = make_args(c, d_sc + (size_t)b0 * sc_frame_stride, d_assign + (size_t)b0 * p->N, &pc, a, nb, sc_frame_stride, -1, true)) return rc;
    if (h_cams) a->cams = c->d_cams + b0;
    return 0;
}

// What a training call works on and towards, beyond the context's workspace.  The per-frame pointers are those of the call's
// frame 0: fill_bwd offsets them by a chunk's first frame.
struct BwdCall {
    float* out_grad;              // accumulated into
    long long grad_frame_stride;  // 0: a single call
    double w_rot, w_trans, cut;
    const double* gt = nullptr;        // single call: gt[16] and gt_pose[6] on the host, passed inline; or
    const double* gt_pose = nullptr;
    const double* gt_frames = nullptr; // batch: [B, ESAC_GT_DOUBLES] on the device
    bool batch = false;                // the batch-wide overflow word (BwdArgs::sel_max)
    int* frame_status = nullptr;       // asynchronous batch only: [B] per-frame outcomes and
    double* rec_dev = nullptr;         // [B,4] the caller's device records
    double* pose_rec = nullptr;        // [B,ESAC_RES_DOUBLES] the caller's device records of the winners' refined poses (an armed call)
};

// esac_hip_set_bwd_pose_records armed the context for the NEXT training call: every training entry point takes the arming when
// it is entered, whatever becomes of the call (one-shot, consumed by a rejected call too).
struct PoseArm {
    double* rec = nullptr;
    int frames = 0;
};
static PoseArm take_pose_arm(esac_hip_ctx* c) {
    PoseArm arm;
    if (!c) return arm;
    arm.rec = c->pose_rec;
    arm.frames = c->pose_rec_frames;
    c->pose_rec = nullptr;
    c->pose_rec_frames = 0;
    return arm;
}
// ... and checks it against the call's frames before anything is launched
static int check_pose_arm(const char* who, const PoseArm& arm, int B) {
    if (arm.rec && arm.frames < B)
        return fail(-4, "%s: esac_hip_set_bwd_pose_records armed %d frame(s), the call has %d", who, arm.frames, B);
    return 0;
}

// a.bwd of one selection .. accumulation pass over `frames` frames from frame b0 of the call, `cap` slots each, in the context's
// slot workspace (which ensure_bws has sized).  Every field a route does not use is null / 0 here, in this one place.
// want_teams: refine the slots by teams where this call can (single blocking calls; a.bwd.team_max_slots != 0 says it will).
static void fill_bwd(esac_hip_ctx* c, KArgs& a, const BwdCall& call, int b0, int frames, int cap, bool want_teams) {
    c->last_bwd_frames = frames;
    c->last_bwd_batch_cap = call.batch ? cap : 0;
    a.frames = frames;  // (a rerun after an overflow may take fewer frames: their samples stay where they are)
    a.bwd = c->bws;
    a.bwd.cap = cap;
    a.bwd.team = 0;  // (the slot-team launch sets these two)
    a.bwd.team_tag = 0;
    a.bwd.team_max_slots = want_teams && refine_slots_can_team(a) ? ESAC_SLOT_TEAMS_MAX : 0;  // 0: one workgroup per slot
    a.bwd.out_grad = call.out_grad + (size_t)b0 * call.grad_frame_stride;
    a.bwd.grad_frame_stride = call.grad_frame_stride;
    a.bwd.w_rot = call.w_rot;
    a.bwd.w_trans = call.w_trans;
    a.bwd.cut = call.cut;
    for (int i = 0; i < 16; i++) a.bwd.gt[i] = call.gt ? call.gt[i] : 0.0;
    for (int i = 0; i < 6; i++) a.bwd.gt_pose[i] = call.gt_pose ? call.gt_pose[i] : 0.0;
    a.bwd.gt_frames = call.gt_frames ? call.gt_frames + (size_t)b0 * ESAC_GT_DOUBLES : nullptr;
    if (!call.batch) a.bwd.sel_max = nullptr;
    a.bwd.frame_status = call.frame_status ? call.frame_status + b0 : nullptr;
    a.bwd.rec_dev = call.rec_dev ? call.rec_dev + (size_t)b0 * 4 : nullptr;
    a.bwd.pose_rec = call.pose_rec ? call.pose_rec + (size_t)b0 * ESAC_RES_DOUBLES : nullptr;
}

// Selection .. accumulation of a.bwd's frames on `s`: enqueues and returns; a caller that wants the outcome waits for it.
// Slot refinement (esac.cpp:328-347): by teams of 8 (esac_refine_team.hip) when THIS call's selection holds few enough slots
// that every team has an XCD's CUs to itself (<= 32), one workgroup per slot otherwise.  The count is only known on the
// device, so both launches are issued and each returns at once when the other one's case applies (team_max_slots): the
// route is a function of the call's own inputs, not of what an earlier call on the context selected.
// result_pin: the last workgroup of the accumulation hands the call's records (a frame's four values + "a slot team timed out")
// to the pinned slots, one per frame: no copies, no stream-completion round trip.  NULL: nobody polls.
static int enqueue_bwd_chain(esac_hip_ctx* c, KArgs& a, hipStream_t s, double* result_pin) {
    int rc;
    if (a.bwd.sel_max) HIP_OK(hipMemsetAsync(a.bwd.sel_max, 0, sizeof(int), s));
    launch_bwd_select(a, s);                                    // esac.cpp:319-331
    if ((rc = check_launch("k_bwd_select"))) return rc;
    if (a.bwd.team_max_slots) {
        launch_refine_slots_team(a, s);                         // a team per slot, when n_sel <= team_max_slots
        c->slot_team_calls++;
    }
    launch_refine_slots(a, s);                                  // one workgroup per slot otherwise
    if ((rc = check_launch("k_refine(slots)"))) return rc;
    if (a.bwd.pose_rec) {                                       // an armed call: the winner's refined pose as a forward record
        launch_bwd_pose_record(a, s);
        if ((rc = check_launch("k_bwd_pose_record"))) return rc;
    }
    launch_bwd_loss(a, s);                                      // esac.cpp:354-362 + dLoss + softmax derivative (+ rec_dev)
    if ((rc = check_launch("k_bwd_loss"))) return rc;
    launch_bwd_paths(a, s);                                     // esac.cpp:375-463 (path I) and :470-488 (path II), side by side
    if ((rc = check_launch("k_bwd_paths"))) return rc;
    KArgs acc = a;
    acc.result_pin = result_pin;
    launch_bwd_accumulate(acc, s);                              // esac.cpp:491-508
    return check_launch("k_bwd_accumulate");
}

// Arms the next training call on the context (include/esac_hip.h): a pointer and a count, nothing is launched or waited for.
extern "C" int esac_hip_set_bwd_pose_records(esac_hip_ctx* c, double* d_records, int frames) {
    if (!c) return fail(-1, "null context");
    if (d_records && frames < 1) return fail(-4, "esac_hip_set_bwd_pose_records: frames = %d (at least 1 with a record buffer)", frames);
    c->pose_rec = d_records;
    c->pose_rec_frames = d_records ? frames : 0;
    return 0;
}

extern "C" int esac_hip_backward(esac_hip_ctx* c, const float* d_sc, float* d_out_gradients, const int64_t* d_assign,
                                 const float* h_gt_pose, float w_loss_rot, float w_loss_trans, float loss_cut,
                                 const esac_hip_params* p, void* stream, double* h_out) {
    const PoseArm arm = take_pose_arm(c);
    if (!d_out_gradients || !h_gt_pose) return fail(-1, "esac_hip_backward: null gradient tensor or ground-truth pose");
    if (!c) return fail(-1, "null context");
    if (p && (p->flags & ESAC_FLAG_STRICT_REFERENCE))
        return fail(-4, "esac_hip_backward: the training path has no strict mode (ESAC_FLAG_STRICT_REFERENCE is a forward flag)");
    DeviceGuard guard(c->device);
    KArgs a;
    int rc = make_args(c, d_sc, d_assign, p, &a, 1, 0, -1, true);
    if (rc) return rc;
    if (p->E > 65535) return fail(-4, "esac_hip_backward: at most 65535 experts (one grid row per expert in the accumulation kernel)");
    if (p->d_hyp_index || p->hyp_offset)
        return fail(-4, "esac_hip_backward: sharded calls are not supported (the expectation needs every hypothesis)");
    if ((rc = check_pose_arm("esac_hip_backward", arm, 1))) return rc;
    const int P = p->H * p->W;
    // Slot workspace (two 3P-double slabs + two inlier maps per slot).  How many hypotheses reach PROB_THRESH is only
    // known on the device: a blocking call starts from what earlier calls needed (at least 64 slots) and, when the
    // selection overflows it, grows the workspace and runs selection..accumulation again -- the accumulation kernel
    // adds nothing on overflow, so the caller's tensor is untouched by the aborted pass.  An asynchronous call
    // (h_out == NULL) cannot look at the count and reserves the worst case min(N, 1000).
    const int worst = p->N < ESAC_BWD_MAX_SLOTS ? p->N : ESAC_BWD_MAX_SLOTS;
    int cap = worst;
    if (h_out) {
        cap = c->bcap > 64 ? c->bcap : 64;
        if (cap > worst) cap = worst;
    }
    double gt[16], gt_pose[6];
    if (!gt_host(h_gt_pose, gt, gt_pose)) return fail(-4, "esac_hip_backward: the ground-truth pose is singular");
    BwdCall call = {d_out_gradients, 0, w_loss_rot, w_loss_trans, loss_cut};
    call.gt = gt;
    call.gt_pose = gt_pose;
    call.pose_rec = arm.rec;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = enqueue_bwd_sampling(c, a, s, false))) return rc;
    // A blocking call can refine again with one workgroup per slot should a slot team time out; an asynchronous one cannot and
    // does not use teams.
    bool use_teams = h_out && c->slot_teams;
    for (int attempt = 0;; attempt++) {
        if ((rc = ensure_bws(c, p->N, P, cap))) return rc;
        if (cap > c->bcap) c->bcap = cap;
        fill_bwd(c, a, call, 0, 1, cap, use_teams);
        const bool teams = a.bwd.team_max_slots != 0;
        if ((rc = enqueue_bwd_chain(c, a, s, h_out ? c->d_pin : nullptr))) return rc;
        if (!h_out) return 0;
        if ((rc = wait_record(c, s, 1, a.epoch, "esac_hip_backward: the accumulation kernel"))) return rc;
        __sync_synchronize();
        for (int k = 0; k < 4; k++) h_out[k] = c->h_pin[k];
        const bool team_failed = c->h_pin[4] == 1.0;
        if (teams && team_failed) {  // a team timed out: nothing was accumulated; one workgroup per slot from here on
            c->slot_team_fallbacks++;
            c->slot_teams = false;
            use_teams = false;
            attempt--;
            c->epoch += 1.0;
            a.epoch = c->epoch;
            continue;
        }
        c->last_nsel = (int)h_out[1];
        c->last_bwd_teams = teams && c->last_nsel <= ESAC_SLOT_TEAMS_MAX;
        const int needed = (int)h_out[1];
        if (needed <= cap || attempt >= 1) break;  // one retry suffices: the second pass is sized by the true count
        cap = grown_cap(needed, worst);
        c->epoch += 1.0;
        a.epoch = c->epoch;
    }
    if (h_out[3] != 0.0)
        return fail(-10, "hypAssignment holds a value outside [0,%d) (device-resident tensor; such hypotheses were scored against expert 0)", p->E);
    return 0;
}

// B independent frames of the training path in one set of launches per chunk (include/esac_hip.h).  Frame b is the b-th of B
// consecutive esac_hip_backward calls (call p->call + b); its slots are refined with one workgroup each.  The slot workspace of
// B x cap slots is bounded by the context's budget: beyond it the frames go in chunks of consecutive frames, each with its own
// launch set (the frames are independent, so the chunking changes no result).  An overflow of the slot workspace in ANY frame
// of a chunk stops the accumulation of every frame of it (one batch-wide word, BwdArgs::sel_max); the host grows `cap` to the
// largest frame's count and runs selection .. accumulation of the chunk again, so nothing is added twice.
extern "C" int esac_hip_backward_batch(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                       int64_t grad_frame_stride, const int64_t* d_assign, const float* h_gt_poses, float w_loss_rot,
                                       float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out) {
    return esac_hip_backward_batch_cams(c, B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, h_gt_poses, nullptr,
                                        w_loss_rot, w_loss_trans, loss_cut, p, stream, h_out);
}

// ... with a camera per frame (h_cams: host, B records; NULL: the five fields of p for every frame).  Record b0 of a chunk goes
// into the chunk's inline fields, the table pointer is offset by the chunk's first frame like gt_frames and the call counter.
extern "C" int esac_hip_backward_batch_cams(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                            int64_t grad_frame_stride, const int64_t* d_assign, const float* h_gt_poses,
                                            const esac_hip_frame_cam* h_cams, float w_loss_rot, float w_loss_trans, float loss_cut,
                                            const esac_hip_params* p, void* stream, double* h_out) {
    const PoseArm arm = take_pose_arm(c);
    int rc = check_batch_call("esac_hip_backward_batch", c, p, B, d_sc && d_out_gradients && d_assign && h_gt_poses, false, h_out,
                              sc_frame_stride, grad_frame_stride);
    if (rc) return rc;
    if ((rc = check_pose_arm("esac_hip_backward_batch", arm, B))) return rc;
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (!c->h_gt) {
        HIP_OK(hipHostMalloc((void**)&c->h_gt, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&c->d_gt, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double)));
    }
    HIP_OK(hipStreamSynchronize(s));  // (the staging buffer is free: a batch that failed half-way may have left its copy queued)
    for (int b = 0; b < B; b++) {
        double* g = c->h_gt + (size_t)b * ESAC_GT_DOUBLES;
        if (!gt_host(h_gt_poses + (size_t)b * 16, g, g + 16))
            return fail(-4, "esac_hip_backward_batch: the ground-truth pose of frame %d is singular", b);
    }
    // validation of the parameters (make_args) before anything is launched: the caller's gradients stay untouched on an error
    KArgs a;
    const esac_hip_params p0 = h_cams ? with_cam(*p, h_cams[0]) : *p;
    if ((rc = make_args(c, d_sc, d_assign, &p0, &a, 1, 0, h_cams ? 0 : -1, true))) return rc;
    if (h_cams && (rc = stage_cams(c, &p0, h_cams, B, s))) return rc;  // (checks every record before the first launch)
    HIP_OK(hipMemcpyAsync(c->d_gt, c->h_gt, (size_t)B * ESAC_GT_DOUBLES * sizeof(double), hipMemcpyHostToDevice, s));
    BwdCall call = {d_out_gradients, grad_frame_stride, w_loss_rot, w_loss_trans, loss_cut};
    call.gt_frames = c->d_gt;
    call.batch = true;
    call.pose_rec = arm.rec;
    const int N = p->N, P = p->H * p->W, worst = bwd_rows(N);
    int cap = c->bcap_batch > 64 ? c->bcap_batch : 64;
    if (cap > worst) cap = worst;
    auto chunk_frames = [&](int cap_, int left) {
        const long long f = c->bwd_budget / ((long long)cap_ * bwd_slot_bytes(P));
        return (int)(f < 1 ? 1 : (f > left ? left : f));
    };
    bool any_bad = false;
    for (int b0 = 0; b0 < B;) {
        int nb = chunk_frames(cap, B - b0);
        if ((rc = chunk_args(c, d_sc, sc_frame_stride, d_assign, p, h_cams, b0, nb, &a))) return rc;
        if ((rc = enqueue_bwd_sampling(c, a, s, true))) return rc;
        for (int attempt = 0;; attempt++) {
            if ((rc = ensure_bws(c, N, P, cap, nb))) return rc;
            if (cap > c->bcap_batch) c->bcap_batch = cap;
            fill_bwd(c, a, call, b0, nb, cap, false);
            if ((rc = enqueue_bwd_chain(c, a, s, c->d_pin))) return rc;  // one pinned slot per frame of the chunk
            if ((rc = wait_record(c, s, nb, a.epoch, "esac_hip_backward_batch: the accumulation kernel"))) return rc;
            __sync_synchronize();
            int needed = 0;
            for (int b = 0; b < nb; b++) {
                const int n = (int)c->h_pin[(size_t)b * ESAC_PIN_DOUBLES + 1];
                needed = n > needed ? n : needed;
            }
            if (needed <= cap || attempt >= 1) {  // one retry suffices: the second pass is sized by the largest true count
                for (int b = 0; b < nb; b++)
                    for (int k = 0; k < 4; k++) h_out[(size_t)(b0 + b) * 4 + k] = c->h_pin[(size_t)b * ESAC_PIN_DOUBLES + k];
                break;
            }
            cap = grown_cap(needed, worst);
            const int fit = chunk_frames(cap, nb);
            nb = fit < nb ? fit : nb;
            c->epoch += 1.0;
            a.epoch = c->epoch;
        }
        for (int b = 0; b < nb; b++) any_bad |= h_out[(size_t)(b0 + b) * 4 + 3] != 0.0;
        b0 += nb;
    }
    if (any_bad)
        return fail(-10, "hypAssignment holds a value outside [0,%d) in at least one frame (h_out[b*4+3] = 1 names them; such "
                         "hypotheses were scored against expert 0)", p->E);
    return 0;
}

// The asynchronous batch (include/esac_hip.h): ground truth, records and per-frame outcomes stay on the device, the host enqueues
// and returns.  Nothing in here waits for the stream -- the one wait is stage_cams' on the PREVIOUS call's table copy -- and
// nothing is run twice: every frame owns the worst-case min(N, 1000) slots, so no selection can overflow, and the frames go in
// chunks of consecutive frames sized by that worst case, one launch set after the other on the stream (which serialises their
// use of the workspace).  A workspace that has to grow is grown before the first launch (ensure_ws / ensure_bws: one device
// synchronisation, on the first call of a shape only).
extern "C" int esac_hip_backward_batch_dev(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                           int64_t grad_frame_stride, const int64_t* d_assign, const float* d_gt_poses,
                                           const esac_hip_frame_cam* h_cams, float w_loss_rot, float w_loss_trans, float loss_cut,
                                           const esac_hip_params* p, void* stream, double* d_out) {
    const PoseArm arm = take_pose_arm(c);
    int rc = check_batch_call("esac_hip_backward_batch", c, p, B, d_sc && d_out_gradients && d_assign && d_gt_poses, true, d_out,
                              sc_frame_stride, grad_frame_stride);
    if (rc) return rc;
    if ((rc = check_pose_arm("esac_hip_backward_batch_dev", arm, B))) return rc;
    // the chunking is known before anything is launched: cap is the worst case, so the first chunk is the largest
    const int N = p->N, P = p->H * p->W, cap = bwd_rows(N);
    const long long fit = c->bwd_budget / ((long long)cap * bwd_slot_bytes(P));
    if (fit < 1)
        return fail(-4, "esac_hip_backward_batch_dev: one frame's worst case (%d slots, %lld MiB) exceeds the slot-workspace budget of "
                        "%lld MiB (ESAC_BWD_BATCH_BUDGET_MB); the blocking esac_hip_backward_batch sizes the workspace by the "
                        "selection's true count", cap, ((long long)cap * bwd_slot_bytes(P)) >> 20, c->bwd_budget >> 20);
    const int chunk = (int)(fit > B ? B : fit);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (!c->d_gt_dev) {
        HIP_OK(hipMalloc((void**)&c->d_gt_dev, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double)));
        HIP_OK(hipMalloc((void**)&c->d_frame_status, (size_t)ESAC_MAX_BATCH * sizeof(int)));
    }
    // validation of the parameters and of every camera record, and the workspaces of the largest chunk, before anything is
    // launched: the caller's gradients stay untouched on an error
    KArgs a;
    const esac_hip_params p0 = h_cams ? with_cam(*p, h_cams[0]) : *p;
    if ((rc = make_args(c, d_sc, d_assign, &p0, &a, chunk, sc_frame_stride, h_cams ? 0 : -1, true))) return rc;
    if ((rc = ensure_bws(c, N, P, cap, chunk))) return rc;
    if (h_cams && (rc = stage_cams(c, &p0, h_cams, B, s))) return rc;  // (checks every record before the first launch)
    launch_bwd_gt_prepare(d_gt_poses, B, c->d_gt_dev, c->d_frame_status, s);
    if ((rc = check_launch("k_bwd_gt_prepare"))) return rc;
    BwdCall call = {d_out_gradients, grad_frame_stride, w_loss_rot, w_loss_trans, loss_cut};
    call.gt_frames = c->d_gt_dev;
    call.batch = true;
    call.frame_status = c->d_frame_status;
    call.rec_dev = d_out;
    call.pose_rec = arm.rec;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        if ((rc = chunk_args(c, d_sc, sc_frame_stride, d_assign, p, h_cams, b0, nb, &a))) return rc;
        if ((rc = enqueue_bwd_sampling(c, a, s, true))) return rc;
        fill_bwd(c, a, call, b0, nb, cap, false);  // (the slot workspace was sized for the largest chunk above)
        if ((rc = enqueue_bwd_chain(c, a, s, nullptr))) return rc;  // k_bwd_loss writes frame b's record into d_out[b*4..]
    }
    c->last_dev_batch = B;
    return 0;
}

// Asynchronous calls (no host result) cannot report an out-of-range hypAssignment themselves: this waits for the
// device and returns -10 when the most recent call on the context flagged one, 0 otherwise.
extern "C" int esac_hip_check(esac_hip_ctx* c) {
    if (!c) return fail(-1, "null context");
    DeviceGuard guard(c->device);
    if (!c->ws.status) return 0;
    HIP_OK(hipDeviceSynchronize());
    unsigned long long st = 0, coop[2] = {0, 0};
    HIP_OK(hipMemcpy(&st, c->ws.status, sizeof(st), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(coop, c->ws.coop_counter, sizeof(coop), hipMemcpyDeviceToHost));
    if (c->refine_tag != 0 && coop[1] == c->refine_tag) {  // the failure word carries the tag of the launch that failed: only the most recent one counts
        // asynchronous calls learn of a team time-out here (or from the pick of the multi-GPU exchange, whose caller then asks here):
        // the same two-strikes latch as the blocking call's, so that a GPU whose CUs are held by someone else does not cost every
        // frame the 1 ms wait
        if (c->refine_was_team && c->checked_tag != c->refine_tag) {
            c->checked_tag = c->refine_tag;
            note_team_timeout(c);
        }
        return fail(-12, "the cooperating refinement workgroups of the most recent call could not synchronise (not all of them became resident)");
    }
    if (c->last_dev_batch > 0) {  // esac_hip_backward_batch_dev was the most recent call: its per-frame outcomes
        static thread_local int words[ESAC_MAX_BATCH];
        const int B = c->last_dev_batch;
        HIP_OK(hipMemcpy(words, c->d_frame_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++)
            if (words[b] == 2) return fail(-4, "esac_hip_backward_batch_dev: the ground-truth pose of frame %d is singular", b);
        for (int b = 0; b < B; b++)
            if (words[b] == 1)
                return fail(-10, "hypAssignment holds a value outside [0,E) in frame %d of the most recent batch (d_out[b*4+3] = 1 names "
                                 "every such frame; such hypotheses were scored against expert 0)", b);
    }
    if (st != 0 && (double)st == c->sample_epoch) return fail(-10, "hypAssignment held a value outside [0,E) in the most recent sampling call");
    return 0;
}

// Multi-GPU: this rank's share of a load-balanced split of the hypotheses, built on the device (one launch, no host
// round trip); see include/esac_hip.h.
extern "C" int esac_hip_shard_balanced(esac_hip_ctx* c, const int64_t* d_assign, int N, int E, int world, int rank, int expert_base,
                                       void* stream, int32_t* d_index_out, int64_t* d_assign_out, int32_t* d_info_out) {
    if (!c || !d_assign || !d_index_out || !d_assign_out) return fail(-1, "esac_hip_shard_balanced: null argument");
    if (N <= 0 || E <= 0 || E > ESAC_TILED_MAX_EXPERTS) return fail(-4, "esac_hip_shard_balanced: N=%d, E=%d (1 <= E <= %d)", N, E, ESAC_TILED_MAX_EXPERTS);
    if (world < 1 || rank < 0 || rank >= world) return fail(-4, "esac_hip_shard_balanced: rank %d of %d", rank, world);
    DeviceGuard guard(c->device);
    launch_shard_balanced(d_assign, N, E, world, rank, expert_base, d_index_out, d_assign_out, d_info_out, (hipStream_t)stream);
    return check_launch("k_shard_balanced");
}

// The test loop's figures of a batch, on the device (esac_eval.hip; include/esac_hip.h): one launch on the caller's stream, no
// workspace, no state of the context beyond its device.
static_assert(ESAC_EVAL_ROT_DEG == ESAC_EVAL_ROT_DEG_K && ESAC_EVAL_TRANS_CM == ESAC_EVAL_TRANS_CM_K && ESAC_EVAL_POSE_OK == ESAC_EVAL_POSE_OK_K &&
                  ESAC_EVAL_CLASS_OK == ESAC_EVAL_CLASS_OK_K && ESAC_EVAL_QUAT == ESAC_EVAL_QUAT_K && ESAC_EVAL_INV_T == ESAC_EVAL_INV_T_K &&
                  ESAC_EVAL_EXPERT == ESAC_EVAL_EXPERT_K && ESAC_EVAL_HYP == ESAC_EVAL_HYP_K && ESAC_EVAL_STATUS == ESAC_EVAL_STATUS_K &&
                  ESAC_EVAL_DOUBLES == ESAC_EVAL_DOUBLES_K && ESAC_RES_DOUBLES == ESAC_EVAL_REC_DOUBLES && ESAC_RES_HYP == ESAC_EVAL_REC_HYP &&
                  ESAC_RES_EXPERT == ESAC_EVAL_REC_EXPERT && ESAC_RES_POSE == ESAC_EVAL_REC_POSE && ESAC_RES_VALID == ESAC_EVAL_REC_VALID,
              "eval row / record layout drifted between include/esac_hip.h and eval_math.hpp");
extern "C" int esac_hip_eval_batch(esac_hip_ctx* c, int B, const double* d_records, const float* d_gt_poses, const int64_t* d_gt_experts,
                                   float rot_thresh_deg, float trans_thresh_cm, void* stream, double* d_out) {
    if (!c) return fail(-1, "null context");
    if (B < 1 || B > ESAC_MAX_BATCH) return fail(-4, "esac_hip_eval_batch: batch size %d outside [1,%d]", B, ESAC_MAX_BATCH);
    if (!d_records || !d_gt_poses || !d_out)
        return fail(-4, "esac_hip_eval_batch: null %s pointer", !d_records ? "d_records" : !d_gt_poses ? "d_gt_poses" : "d_out");
    if (!(rot_thresh_deg >= 0.0f) || !(rot_thresh_deg <= FLT_MAX) || !(trans_thresh_cm >= 0.0f) || !(trans_thresh_cm <= FLT_MAX))
        return fail(-4, "esac_hip_eval_batch: the thresholds must be finite and not negative (rotation %g deg, translation %g cm)",
                    (double)rot_thresh_deg, (double)trans_thresh_cm);
    DeviceGuard guard(c->device);
    launch_eval_batch(B, d_records, d_gt_poses, d_gt_experts, (double)rot_thresh_deg, (double)trans_thresh_cm, d_out, (hipStream_t)stream);
    return check_launch("k_eval_batch");
}

extern "C" int esac_hip_set_wait(esac_hip_ctx* c, int mode) {
    if (!c) return fail(-1, "null context");
    if (mode != ESAC_WAIT_SPIN && mode != ESAC_WAIT_YIELD && mode != ESAC_WAIT_BLOCK) return fail(-4, "esac_hip_set_wait: unknown mode %d", mode);
    c->wait_mode = mode;
    return 0;
}

extern "C" int esac_hip_read(esac_hip_ctx* c, int which, void* h_dst, size_t bytes) {
    if (!c || !h_dst) return fail(-1, "esac_hip_read: null argument");
    DeviceGuard guard(c->device);
    const size_t N = (size_t)c->lastN, P = (size_t)c->lastH * c->lastW;
    const void* src = nullptr;
    size_t want = 0;
    switch (which) {
        case ESAC_BUF_HYPS: src = c->ws.hyps; want = N * 6 * sizeof(double); break;
        case ESAC_BUF_SAMPLE_XY: src = c->ws.sample_xy; want = N * 8 * sizeof(int32_t); break;
        case ESAC_BUF_TRIES: src = c->ws.tries; want = N * sizeof(int32_t); break;
        case ESAC_BUF_SCORES: src = c->ws.scores; want = N * sizeof(double); break;
        case ESAC_BUF_RESULT: src = c->ws.result; want = ESAC_RES_DOUBLES * sizeof(double); break;
        case ESAC_BUF_INLIER_MAP: {
            // the refinement kernel alternates between two map buffers; result[31] names the one that
            // holds the last ACCEPTED inlier set (-1: no re-fit was accepted -> all zeros)
            if (bytes != P) return fail(-7, "esac_hip_read: inlier map holds %zu bytes, caller asked for %zu", P, bytes);
            HIP_OK(hipDeviceSynchronize());
            double which_buf = -1;
            HIP_OK(hipMemcpy(&which_buf, c->ws.result + 31, sizeof(double), hipMemcpyDeviceToHost));
            if (which_buf < 0) {
                memset(h_dst, 0, P);
                return 0;
            }
            HIP_OK(hipMemcpy(h_dst, c->ws.inlier_map + (which_buf > 0.5 ? P : 0), P, hipMemcpyDeviceToHost));
            return 0;
        }
        case ESAC_BUF_INLIER_COUNTS: src = c->ws.inlier_counts; want = (ESAC_MAX_REF_STEPS + 1) * sizeof(int32_t); break;
        case ESAC_BUF_WINNER_ERRS:
            if (!c->keep_errs) return fail(-6, "esac_hip_read: the error image is only kept after esac_hip_set_debug(ctx, ESAC_DEBUG_ERROR_IMAGE)");
            src = c->ws.errs; want = P * sizeof(float); break;
        case ESAC_BUF_EXACT_FLAGS: src = c->ws.exact_flag; want = N; break;
        case ESAC_BUF_SPEC_FLAGS: src = c->ws.spec_flag; want = N; break;
        case ESAC_BUF_CYCLES: src = c->ws.cycles; want = 32 * sizeof(long long); break;
        case ESAC_BUF_BWD_TEAM_INFO: {
            if (bytes != 4 * sizeof(int32_t)) return fail(-7, "esac_hip_read: the slot-team info holds 16 bytes, caller asked for %zu", bytes);
            const int32_t info[4] = {c->last_bwd_teams ? 1 : 0, (int32_t)c->slot_team_calls, (int32_t)c->slot_team_fallbacks, (int32_t)c->last_nsel};
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
        case ESAC_BUF_SPEC_INFO: {
            if (bytes != 4 * sizeof(int32_t)) return fail(-7, "esac_hip_read: the speculation info holds 16 bytes, caller asked for %zu", bytes);
            double st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c->ws.spec_state) {
                HIP_OK(hipDeviceSynchronize());
                HIP_OK(hipMemcpy(st, c->ws.spec_state, sizeof(st), hipMemcpyDeviceToHost));
            }
            const int32_t info[4] = {(int32_t)c->spec_calls, (int32_t)st[2], c->last_spec_epoch != 0 ? 1 : 0,
                                     c->last_spec_epoch != 0 && st[0] == c->last_spec_epoch ? 1 : 0};
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
        case ESAC_BUF_REFINE_INFO: {
            if (bytes != 8 * sizeof(int32_t)) return fail(-7, "esac_hip_read: the refinement info holds 32 bytes, caller asked for %zu", bytes);
            if (!c->ws.refine_info) return fail(-6, "esac_hip_read: buffer %d is empty (no call has run yet)", which);
            HIP_OK(hipDeviceSynchronize());
            int32_t info[8];
            HIP_OK(hipMemcpy(info, c->ws.refine_info, sizeof(info), hipMemcpyDeviceToHost));
            info[6] = (int32_t)((c->team_fallbacks & 0x3fffffff) | (c->team_latched_off ? 0x40000000 : 0));
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
        case ESAC_BUF_BWD_PROBS: src = c->bws.probs; want = N * sizeof(double); break;
        case ESAC_BUF_BWD_LOSSES: src = c->bws.losses; want = N * sizeof(double); break;
        case ESAC_BUF_BWD_REF_HYPS: src = c->bws.ref_hyps; want = N * 6 * sizeof(double); break;
        case ESAC_BUF_BWD_SCORE_GRADS: src = c->bws.sgrad; want = N * sizeof(double); break;
        case ESAC_BUF_BWD_SLOTS: src = c->bws.sel; want = N * sizeof(int32_t); break;
        case ESAC_BUF_BWD_SLOT_INFO: src = c->bws.map_info; want = (size_t)(c->lastN < ESAC_BWD_MAX_SLOTS ? c->lastN : ESAC_BWD_MAX_SLOTS) * 4 * sizeof(int32_t); break;
        case ESAC_BUF_BWD_DLOSS: src = c->bws.dloss; want = (size_t)(c->lastN < ESAC_BWD_MAX_SLOTS ? c->lastN : ESAC_BWD_MAX_SLOTS) * 6 * sizeof(double); break;
        case ESAC_BUF_BWD_PATH1:
        case ESAC_BUF_BWD_PATH2: {
            // [slots,3,P] doubles; the caller asks for the first k slots (k = bytes / (3 P 8))
            const size_t slab = 3 * P * sizeof(double);
            // slots the slab workspace holds (>= the slots of the last call); after a batch, frame 0's slabs: its per-frame cap
            const size_t cap = c->last_bwd_batch_cap > 0 ? (size_t)c->last_bwd_batch_cap : (size_t)c->bslots;
            src = which == ESAC_BUF_BWD_PATH1 ? c->bws.grad1 : c->bws.grad2;
            if (!src || slab == 0) return fail(-6, "esac_hip_read: buffer %d is empty (no backward call has run yet)", which);
            if (bytes == 0 || bytes % slab || bytes / slab > cap)
                return fail(-7, "esac_hip_read: buffer %d is read in whole slabs of %zu bytes, at most %zu", which, slab, cap);
            want = bytes;
            break;
        }
        case ESAC_BUF_BWD_MAPS: {
            // [slots,2,P] bytes: both map buffers of each slot, read in whole slots like the slabs (k = bytes / (2 P))
            const size_t pair = 2 * P;
            const size_t cap = c->last_bwd_batch_cap > 0 ? (size_t)c->last_bwd_batch_cap : (size_t)c->bslots;
            src = c->bws.maps;
            if (!src || pair == 0) return fail(-6, "esac_hip_read: buffer %d is empty (no backward call has run yet)", which);
            if (bytes == 0 || bytes % pair || bytes / pair > cap)
                return fail(-7, "esac_hip_read: buffer %d is read in whole slots of %zu bytes, at most %zu", which, pair, cap);
            want = bytes;
            break;
        }
        default: return fail(-5, "esac_hip_read: unknown buffer id %d", which);
    }
    // after a batched training call the per-frame buffers above hold its (last chunk's) frames frame-major: B x the size reads them all
    const bool per_frame = which == ESAC_BUF_BWD_PROBS || which == ESAC_BUF_BWD_LOSSES || which == ESAC_BUF_BWD_REF_HYPS ||
                           which == ESAC_BUF_BWD_SCORE_GRADS || which == ESAC_BUF_BWD_SLOTS || which == ESAC_BUF_BWD_SLOT_INFO ||
                           which == ESAC_BUF_BWD_DLOSS;
    if (per_frame && c->last_bwd_frames > 1 && want > 0 && bytes == want * (size_t)c->last_bwd_frames) want = bytes;
    // ... and after a batched call the sampler's and the refinement's per-frame buffers hold its frames frame-major
    const bool fwd_per_frame = which == ESAC_BUF_HYPS || which == ESAC_BUF_SAMPLE_XY || which == ESAC_BUF_TRIES || which == ESAC_BUF_SCORES ||
                               which == ESAC_BUF_INLIER_COUNTS;
    if (fwd_per_frame && c->lastB > 1 && want > 0 && bytes == want * (size_t)c->lastB) want = bytes;
    if (!src || want == 0) return fail(-6, "esac_hip_read: buffer %d is empty (no call has run yet)", which);
    if (bytes != want) return fail(-7, "esac_hip_read: buffer %d holds %zu bytes, caller asked for %zu", which, want, bytes);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h_dst, src, want, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int esac_hip_write_hyps(esac_hip_ctx* c, const double* h_hyps, int N) {
    if (!c || !h_hyps || N <= 0) return fail(-1, "esac_hip_write_hyps: bad argument");
    DeviceGuard guard(c->device);
    int rc = ensure_ws(c, N, c->capP > 0 ? c->capP : 1);
    if (rc) return rc;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(c->ws.hyps, h_hyps, (size_t)N * 6 * sizeof(double), hipMemcpyHostToDevice));
    // the fp32 [R | t] rows of the streaming score are relative to each expert map's origin (device_common.hpp:
    // map_centre): they are rebuilt by the next esac_hip_score, which knows the maps
    c->rt32_stale = true;
    c->lastN = N;
    return 0;
}

extern "C" int esac_hip_set_refine_team(esac_hip_ctx* c, int members) {
    if (!c) return fail(-1, "null context");
    if (members < ESAC_REFINE_TEAM_AUTO || members > ESAC_REFINE_TEAM_MAX)
        return fail(-4, "esac_hip_set_refine_team: %d members (0..%d, or ESAC_REFINE_TEAM_AUTO)", members, ESAC_REFINE_TEAM_MAX);
    // ESAC_REFINE_TEAM_AUTO: back to the default policy (the size chosen per grid); a number: exactly that many
    c->team_auto = members == ESAC_REFINE_TEAM_AUTO && !c->team_auto_env_off;
    c->team = members == ESAC_REFINE_TEAM_AUTO ? ESAC_REFINE_TEAM_DEFAULT : members < 2 ? 0 : members;
    c->team_latched_off = false;  // an explicit request re-arms the forward teams and the training path's slot teams
    c->team_strikes = 0;
    c->slot_teams = true;
    return 0;
}

extern "C" int esac_hip_set_debug(esac_hip_ctx* c, int flags) {
    if (!c) return fail(-1, "null context");
    c->keep_errs = (flags & ESAC_DEBUG_ERROR_IMAGE) != 0;
    c->coop_stall = (flags & ESAC_DEBUG_COOP_STALL) != 0;
    c->team_spread = (flags & ESAC_DEBUG_TEAM_SPREAD) != 0;
    c->spec_off = c->spec_env_off || (flags & ESAC_DEBUG_NO_SPECULATION) != 0;
    c->spec_second_best = (flags & ESAC_DEBUG_SPEC_SECOND_BEST) != 0;
    c->spec_lose_chain = (flags & ESAC_DEBUG_SPEC_LOSE_CHAIN) != 0;
    return 0;
}

extern "C" int esac_hip_set_timing(esac_hip_ctx* c, int enabled) {
    if (!c) return fail(-1, "null context");
    c->timing = enabled != 0;
    c->timing_period = enabled > 1 ? enabled : 1;
    c->timing_calls = 0;
    c->ev_valid = false;
    if (c->ws.span_acc) {
        DeviceGuard guard(c->device);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemset(c->ws.span_acc, 0, 2 * sizeof(long long)));
    }
    return 0;
}

extern "C" int esac_hip_phase_ms(esac_hip_ctx* c, float out[6]) {
    if (!c || !out) return fail(-1, "esac_hip_phase_ms: null argument");
    if (!c->timing || !c->ev_valid) return fail(-8, "esac_hip_phase_ms: timing is off or no forward has run");
    DeviceGuard guard(c->device);
    HIP_OK(hipEventSynchronize(c->ev[4]));
    for (int i = 0; i < 4; i++) HIP_OK(hipEventElapsedTime(&out[i], c->ev[i], c->ev[i + 1]));
    HIP_OK(hipEventElapsedTime(&out[4], c->ev[0], c->ev[4]));
    HIP_OK(hipEventSynchronize(c->ev[6]));
    HIP_OK(hipEventElapsedTime(&out[5], c->ev[5], c->ev[6]));
    return 0;
}

extern "C" int esac_hip_score_span_ms(esac_hip_ctx* c, float* mean_ms, int* launches) {
    if (!c || !mean_ms) return fail(-1, "esac_hip_score_span_ms: null argument");
    if (!c->ws.span_acc) return fail(-8, "esac_hip_score_span_ms: no forward has run");
    DeviceGuard guard(c->device);
    HIP_OK(hipDeviceSynchronize());
    // mean device-side span of the score kernel since timing was enabled (100 MHz wall clock -> ms)
    long long acc[2] = {0, 0};
    HIP_OK(hipMemcpy(acc, c->ws.span_acc, sizeof(acc), hipMemcpyDeviceToHost));
    *mean_ms = acc[1] > 0 ? (float)((double)acc[0] / (double)acc[1] * 1e-5) : 0.0f;
    if (launches) *launches = (int)acc[1];
    return 0;
}
