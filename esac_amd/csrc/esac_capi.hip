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
#include "call_policy.hpp"
#include "batch_plan.hpp"
#include "esac_kernels.hpp"
#include "front_route_policy.hpp"
#include "eval_math.hpp"
#include "gt_math.hpp"
#include "pose_math.hpp"
#include "verify_math.hpp"
#include "verify_policy.hpp"

using namespace esac;

// RCCL's handful of types, declared here (see rccl() below: the library is bound by dlopen, its headers are not needed)
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
}

static_assert(ESAC_RES_SCORE == ESAC_RES_SCORE_K && ESAC_RES_HYP == ESAC_RES_HYP_K && ESAC_RES_EXPERT == ESAC_RES_EXPERT_K && ESAC_RES_RVEC == ESAC_RES_RVEC_K && ESAC_RES_POSE == ESAC_RES_POSE_K &&
                  ESAC_RES_REF_STEPS == ESAC_RES_REF_STEPS_K && ESAC_RES_INLIERS == ESAC_RES_INLIERS_K && ESAC_RES_PROB == ESAC_RES_PROB_K && ESAC_RES_ENTROPY == ESAC_RES_ENTROPY_K &&
                  ESAC_RES_CONTENDERS == ESAC_RES_CONTENDERS_K && ESAC_RES_LM_ITERS == ESAC_RES_LM_ITERS_K && ESAC_MAX_REF_STEPS == ESAC_MAX_REF_STEPS_K && ESAC_BWD_MAX_SLOTS == ESAC_BWD_SLOTS_K &&
                  ESAC_FLAG_EXACT_SCORES == ESAC_FLAG_EXACT_SCORES_K && ESAC_FLAG_EXACT_SAMPLING == ESAC_FLAG_EXACT_SAMPLING_K &&
                  ESAC_FLAG_SCORES_BY_INDEX == ESAC_FLAG_SCORES_BY_INDEX_K && ESAC_FLAG_STRICT_REFERENCE == ESAC_FLAG_STRICT_REFERENCE_K && ESAC_FLAG_STRICT_TRAINING == ESAC_FLAG_STRICT_TRAINING_K &&
                  ESAC_REFINE_TEAM_MAX == ESAC_REFINE_TEAM_MAX_K && ESAC_REFINE_TEAM_DEFAULT == ESAC_REFINE_TEAM_DEFAULT_K &&
                  (ESAC_FLAG_AUTO_EXACT & (ESAC_FLAG_EXACT_SCORES | ESAC_FLAG_EXACT_SAMPLING | ESAC_FLAG_SCORES_BY_INDEX)) == 0,
              "result layout drifted between include/esac_hip.h and esac_kernels.hpp");
static_assert(POLICY_TILED_HC == ESAC_TILED_HC && POLICY_TILED_MAX_EXPERTS == ESAC_TILED_MAX_EXPERTS && POLICY_LDS_CAP == ESAC_REFINE_LDS_CAP &&
                  POLICY_SAMPLE_LIST_PER_HYP == ESAC_SAMPLE_LIST_PER_HYP, "call_policy.hpp drifted from esac_kernels.hpp");

#define HIP_OK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(-100 - (int)_e, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// Makes the context's GPU current for the duration of one entry point and restores the caller's device afterwards
// (torch and every other runtime user read the same thread-local "current device").
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() = default;  // (a call that learns its context's device behind its checks enters then: begin_bwd_batch)
    explicit DeviceGuard(int dev) { enter(dev); }
    void enter(int dev) {
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

// Owner of one workspace's device buffers: every buffer is allocated, remembered and (when asked) zero-filled at ONE site.
// A failed get leaves its status in `err` (and the message in the error channel); the gets after it do nothing.
struct DevBufs {
    void* ptrs[48];
    int n = 0, err = 0;
    template <typename T>
    void get(T** p, size_t count, bool zero = false) {
        if (err) return;
        err = [&]() -> int {
            HIP_OK(hipMalloc((void**)p, count * sizeof(T)));
            ptrs[n++] = *p;
            if (zero) HIP_OK(hipMemset(*p, 0, count * sizeof(T)));
            return 0;
        }();
    }
    void release(const void* keep = nullptr) {  // frees everything it handed out (but `keep`, then the caller's) and clears the list
        for (int i = 0; i < n; i++)
            if (ptrs[i] != keep) (void)hipFree(ptrs[i]);
        n = err = 0;
    }
};

// The pinned, device-visible host slots the blocking calls' last kernels deliver to: one per frame, ESAC_PIN_DOUBLES doubles
// (result record [32] + epoch word + status word + check word + pad)
struct PinView {
    double *h = nullptr, *d = nullptr;  // host address, and the device's of the same memory
    const volatile double* record(int b) const { return h + (size_t)b * ESAC_PIN_DOUBLES; }
    double word(int b, int k) const { return record(b)[k]; }
    double status(int b) const { return word(b, ESAC_PIN_STATUS); }
    void copy_out(int b, double* dst, int n = ESAC_RES_DOUBLES) const { memcpy(dst, (const void*)record(b), n * sizeof(double)); }
};

// esac_hip_set_bwd_pose_records armed the context for the NEXT training call: every training entry point takes the arming when
// it is entered, whatever becomes of the call (one-shot, consumed by a rejected call too).
struct PoseArm {
    double* rec = nullptr;  // DEVICE [frames, ESAC_RES_DOUBLES], null: not armed
    int frames = 0;
};
// The most recent call on the context, as esac_hip_read and esac_hip_check need it.  make_args assigns the record as a whole (the
// training-path fields of what the slot workspace still holds carried over); the writers behind it are named at their fields.
struct LastCall {
    int N = 0, H = 0, W = 0, B = 1;  // B: frames of the most recent launch set (B x the single-frame size reads the forward buffers of all)
    size_t map1 = 0;        // where frame 0's SECOND inlier-map buffer starts in its slot: the cells of the grid frame 0's refinement ran on
                            // (k_refine alternates maps + cur * P with ITS P) -- H * W, or frame 0's own h * w after a ragged batch (prepare_forward)
    int bwd_frames = 1;     // frames whose training-path buffers the workspace holds (fill_bwd: the last launch set)
    int batch_cap = 0;      // slots per frame of that launch set when it was a batch's (fill_bwd; 0: a single call)
    size_t slot_cells = 0;  // a ragged training batch was the most recent call: the cells of its (last chunk's) frame 0, whose slots lie
                            // that far apart (chunk_args; esac_hip_read of the slabs and the slot maps); 0 otherwise
    int dev_batch = 0;      // B of the asynchronous training batch while it is the most recent call (esac_hip_check reads that many words)
};
// A frame table on its way to the device (stage_cams): pinned staging of the context's own, the table the kernels read, and the
// event behind the most recent upload -- the staging is rewritten only after it
struct CamTable {
    esac_hip_frame_cam* h_cams = nullptr;  // pinned staging [ESAC_MAX_BATCH]: the caller's array is free when the call returns
    FrameCam* d_cams = nullptr;            // ... and the table the kernels read (KArgs::cams)
    hipEvent_t cams_ev = nullptr;
    bool cams_queued = false;
    void release() {
        if (d_cams) (void)hipFree(d_cams);
        if (h_cams) (void)hipHostFree(h_cams);
        if (cams_ev) (void)hipEventDestroy(cams_ev);
    }
};
struct esac_hip_ctx {
    int device = 0;
    int capN = 0, capP = 0, capB = 0;  // capN / capP count elements over ALL frames of a batch
    KArgs ws{};  // only the workspace pointers are kept here
    DevBufs fwd_bufs;    // the forward workspace (ensure_ws)
    DevBufs tiled_bufs;  // the tile-stationary score workspace (ensure_tiled_ws); dies with the forward workspace
    LastCall last;  // what esac_hip_read and esac_hip_check know of the most recent call
    bool keep_errs = false;  // esac_hip_set_debug: store the winner's error image
    PinView pin;
    double epoch = 0;         // bumped by every entry point: hand-off word of the pinned record
    double sample_epoch = 0;  // epoch of the most recent SAMPLING launch: what the device-side status word is tagged with
    int wait_mode = ESAC_WAIT_SPIN;
    int coop_max = 0;         // cooperative refinement workgroups this device holds at once (refine_coop_capacity)
    bool coop_stall = false;  // ESAC_DEBUG_COOP_STALL
    struct {  // team policy
        int members = ESAC_REFINE_TEAM_DEFAULT;  // members of the refinement team on small grids (esac_hip_set_refine_team; 0: one workgroup)
        bool spread = false;                  // ESAC_DEBUG_TEAM_SPREAD: the members are consecutive workgroups (one per XCD)
        bool auto_size = true, auto_env_off = false;  // the default team size is chosen per grid (ESAC_REFINE_TEAM_AUTO=0: exactly the default, A/B)
        unsigned long long refine_tag = 0;    // tag of the most recent shared (cooperative / team) refinement launch, 0: none yet
        unsigned long long checked_tag = 0;   // the failed launch esac_hip_check has already counted as a strike
        bool was_team = false;                // the most recent forward's refinement launch was a team's
        TeamLatch latch;                      // the forward path's time-out latch (call_policy.hpp)
        bool fold_select = true;              // the team kernel may run the selection in its prologue (ESAC_FOLD_SELECT=0: measurement scripts)
        bool route = true;                    // a single frame's team may run the route kernel (esac_hip_set_refine_route; ESAC_REFINE_ROUTE=0)
        int last_nsel = 0;                    // slots the most recent blocking esac_hip_backward refined (0: none yet; reported, decides nothing)
        bool slot_teams = true;               // training path: slots may be refined by teams (off after a time-out until
                                              // esac_hip_set_refine_team re-arms it; ESAC_SLOT_TEAMS=0)
        long long slot_calls = 0, slot_fallbacks = 0;
        bool last_bwd_teams = false;          // the most recent esac_hip_backward refined its slots by teams
    } team;
    struct {  // training sizing
        BwdArgs ws{};  // training-path workspace (pointers only), sized for N hypotheses, P cells, `slots` slots, `rows` slot-table rows
        DevBufs bufs;  // ... and its owner (ensure_bws)
        int P = 0, cap = 0;  // cap: slots per frame the single calls have needed so far (where the next one starts)
        long long N = 0, slots = 0, rows = 0;  // over all frames of a batch
        int B = 0;                             // frames of the per-frame records
        bool lists = false;
        // batched training calls (esac_hip_backward_batch)
        int cap_batch = 0;                     // slots per frame the batches have needed so far
        long long budget = 2048LL << 20;       // bytes of slot workspace a batch may use (ESAC_BWD_BATCH_BUDGET_MB): beyond it, chunks of frames
    } train;
    struct : CamTable {  // per-call staging; the table: per-frame cameras of a batch (esac_hip_forward_batch_cams / esac_hip_backward_batch_cams)
        double* h_gt = nullptr;                // pinned staging of the per-frame ground truth [ESAC_MAX_BATCH,22]
        double* d_gt = nullptr;                // ... and its device copy
        // esac_hip_backward_batch_dev: nothing of the call is staged on the host
        double* d_gt_dev = nullptr;            // [ESAC_MAX_BATCH,22] written by k_bwd_gt_prepare in stream order
        int* d_frame_status = nullptr;         // [ESAC_MAX_BATCH] per-frame outcome of the most recent such call (BwdArgs::frame_status)
        // esac_hip_set_bwd_pose_records: what the NEXT training call writes its forward-format records to (one-shot: take_pose_arm)
        PoseArm pose_arm;
    } stage;
    CamTable verify_cams;  // esac_hip_verify_batch's own table: a forward or training batch in flight keeps the one it reads
    float4* sc4 = nullptr;  // packed copy of the maps for the sampler (ensure_pack_ws), of sc4_cells cells
    long long sc4_cells = 0, tPart = 0;  // tN, tChunks, tPart: what the tile-stationary score workspace holds (ensure_tiled_ws)
    int tN = 0, tChunks = 0;
    bool rt32_stale = false;  // esac_hip_write_hyps ran, or the front route sampled: the fp32 [R|t] rows are rebuilt by the next esac_hip_score
    struct {  // the front route (front_route_policy.hpp): k_sample_route + k_rescore_route in front of a single frame's team
        bool on = true;      // esac_hip_set_front_route; ESAC_FRONT_ROUTE=0
        bool taken = false;  // the most recent forward call ran them (esac_hip_front_route_taken)
    } front;
    struct {  // host timing (and the phase events of esac_hip_set_timing)
        bool on = false;
        int period = 1;       // record the phase events / device-side stamps on every period-th forward call
        long long calls = 0;  // forward calls since timing was enabled
        hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        bool ev_valid = false;
        double host_ns[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // esac_hip_host_turn: where the host's time of the most recent blocking forward went
        double host_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // ... summed over the blocking forward calls since the last reset (esac_hip_host_turn_mean)
        double last_return = 0;                         // CLOCK_MONOTONIC at which the previous blocking forward returned
        long long host_n = 0;
    } timing;
    struct {  // speculation (forward_impl): the straggler chain of the sampler runs on `side` beside the launch stream
        hipStream_t side = nullptr, side2 = nullptr;  // ... and the selection among the settled hypotheses + the join on this one, beside the speculative refinement
        hipEvent_t ev = nullptr;          // recorded on the caller's stream at the entry of a speculative call: both streams wait for it
        bool off = false, env_off = false;  // ESAC_DEBUG_NO_SPECULATION / ESAC_SPECULATE=0
        bool second_best = false, lose_chain = false;  // ESAC_DEBUG_SPEC_SECOND_BEST, ESAC_DEBUG_SPEC_LOSE_CHAIN
        long long calls = 0;              // forward calls that took the speculative route
        double last_epoch = 0;            // epoch of the most recent speculative call (0: the most recent forward was not)
    } spec;
    struct {  // communicator (esac_hip_comm_init): this context's rank in an RCCL communicator (the multi-GPU score exchange)
        ncclComm_t handle = nullptr;
        int ranks = 0, rank = 0;
    } comm;
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
    if (c->comm.handle) (void)rccl().comm_destroy(c->comm.handle);  // a communicator exists only if RCCL was bound
    c->comm.handle = nullptr;
    c->comm.ranks = 0;
}

static void free_tiled_ws(esac_hip_ctx* c) {
    c->tiled_bufs.release();
    c->ws.order = nullptr; c->ws.rt_sorted = nullptr; c->ws.chunks = nullptr; c->ws.n_chunks = nullptr; c->ws.partials = nullptr; c->ws.bucket_fill = nullptr;
    c->tN = c->tChunks = 0; c->tPart = 0;
}
static void free_ws(esac_hip_ctx* c, const void* keep = nullptr) {
    free_tiled_ws(c);
    c->fwd_bufs.release(keep);
    c->ws = KArgs{};
    c->capN = c->capP = c->capB = 0;
}

extern "C" int esac_hip_create(esac_hip_ctx** out, int device) {
    if (!out) return fail(-1, "esac_hip_create: null ctx pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(-2, "esac_hip_create: no HIP device available (%s); this library has no CPU fallback", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(-3, "esac_hip_create: device %d out of range [0,%d)", device, n);
    DeviceGuard guard(device);
    esac_hip_ctx* c = new esac_hip_ctx();
    c->device = device;
    for (auto& ev : c->timing.ev) HIP_OK(hipEventCreate(&ev));
    HIP_OK(hipHostMalloc((void**)&c->pin.h, (size_t)ESAC_PIN_DOUBLES * ESAC_MAX_BATCH * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->pin.h, 0, (size_t)ESAC_PIN_DOUBLES * ESAC_MAX_BATCH * sizeof(double));
    HIP_OK(hipHostGetDevicePointer((void**)&c->pin.d, c->pin.h, 0));
    c->coop_max = refine_coop_capacity();  // CUs x resident workgroups of the cooperative refinement kernel on THIS device
    if (const char* e = getenv("ESAC_REFINE_TEAM")) {  // start value of esac_hip_set_refine_team (measurement scripts)
        const int g = atoi(e);
        c->team.members = g < 2 ? 0 : (g > ESAC_REFINE_TEAM_MAX ? ESAC_REFINE_TEAM_MAX : g);
    }
    if (const char* e = getenv("ESAC_FOLD_SELECT")) c->team.fold_select = atoi(e) != 0;
    if (const char* e = getenv("ESAC_REFINE_ROUTE")) c->team.route = atoi(e) != 0;
    if (const char* e = getenv("ESAC_FRONT_ROUTE")) c->front.on = atoi(e) != 0;
    if (const char* e = getenv("ESAC_REFINE_TEAM_AUTO")) c->team.auto_env_off = atoi(e) == 0;
    if (c->team.auto_env_off || getenv("ESAC_REFINE_TEAM")) c->team.auto_size = false;  // (an explicit start value is an explicit size)
    if (const char* e = getenv("ESAC_SLOT_TEAMS")) c->team.slot_teams = atoi(e) != 0;
    if (const char* e = getenv("ESAC_SPECULATE")) c->spec.off = c->spec.env_off = atoi(e) == 0;
    if (const char* e = getenv("ESAC_BWD_BATCH_BUDGET_MB")) {
        const long long mb = atoll(e);
        if (mb > 0) c->train.budget = mb << 20;
    }
    *out = c;
    return 0;
}
static void free_bws(esac_hip_ctx* c) {
    c->train.bufs.release();
    c->train.ws = BwdArgs{};
    c->train.N = c->train.slots = c->train.rows = 0; c->train.P = c->train.B = 0; c->train.lists = false;
}

extern "C" int esac_hip_destroy(esac_hip_ctx* c) {
    if (!c) return 0;
    DeviceGuard guard(c->device);
    free_ws(c);
    free_bws(c);
    if (c->stage.d_gt) (void)hipFree(c->stage.d_gt);
    if (c->stage.d_gt_dev) (void)hipFree(c->stage.d_gt_dev);
    if (c->stage.d_frame_status) (void)hipFree(c->stage.d_frame_status);
    c->stage.release();
    c->verify_cams.release();
    if (c->stage.h_gt) (void)hipHostFree(c->stage.h_gt);
    if (c->sc4) (void)hipFree(c->sc4);
    drop_comm(c);
    if (c->spec.side) (void)hipStreamDestroy(c->spec.side);
    if (c->spec.side2) (void)hipStreamDestroy(c->spec.side2);
    if (c->spec.ev) (void)hipEventDestroy(c->spec.ev);
    if (c->pin.h) (void)hipHostFree(c->pin.h);
    for (auto& ev : c->timing.ev)
        if (ev) (void)hipEventDestroy(ev);
    delete c;
    return 0;
}

static int ensure_ws(esac_hip_ctx* c, int N1, int P1, int B = 1) {
    const long long N = (long long)N1 * B, P = (long long)P1 * B;
    if (N <= c->capN && P <= c->capP && B <= c->capB) return 0;
    if (N > 0x7fffffffLL || P > 0x7fffffffLL) return fail(-4, "batch too large");
    HIP_OK(hipDeviceSynchronize());
    const int nN = N > c->capN ? (int)N : c->capN, nP = P > c->capP ? (int)P : c->capP, nB = B > c->capB ? B : c->capB;
    // hypotheses handed in through esac_hip_write_hyps (and the status word) survive a growing workspace
    double* old_hyps = c->ws.hyps;
    const size_t old_n = (size_t)c->capN;
    unsigned long long old_status = 0;
    if (c->ws.status) HIP_OK(hipMemcpy(&old_status, c->ws.status, sizeof(old_status), hipMemcpyDeviceToHost));
    free_ws(c, old_hyps);  // (old_hyps stays allocated while the new buffers are: their addresses are what they always were)
    DevBufs& m = c->fwd_bufs;
    KArgs& w = c->ws;
    const bool Z = true;  // get(.., Z): zero-filled
    m.get(&w.hyps, (size_t)nN * 6, Z);  m.get(&w.hyps_R, (size_t)nN * 9);
    m.get(&w.rt32, (size_t)nN * 12);  m.get(&w.status, (size_t)1);
    // the exchange buffer of shared refinements: partial sums of cooperating workgroups [2][256][32] doubles, or the granules
    // of up to ESAC_TEAM_BATCH_MAX teams (16 bytes each)
    static_assert((size_t)ESAC_TEAM_BATCH_MAX * ESAC_TEAM_GRANULES * 2 >= (size_t)2 * ESAC_REFINE_COOP_MAX * 32, "exchange buffer");
    m.get(&w.coop_partials, (size_t)ESAC_TEAM_BATCH_MAX * ESAC_TEAM_GRANULES * 2, Z);  // (also the teams' granules)
    m.get(&w.coop_counter, (size_t)2, Z);  // [1]: tag of the last failed shared refinement (esac_hip_check)
    m.get(&w.refine_info, (size_t)8, Z);  m.get(&w.sample_xy, (size_t)nN * 8);
    m.get(&w.tries, (size_t)nN);  m.get(&w.samp_resume, (size_t)nN);
    m.get(&w.samp_round, (size_t)nN);  m.get(&w.best_try, (size_t)nN);
    m.get(&w.samp_cand, (size_t)nN * ESAC_SAMPLE_LIST_PER_HYP * ESAC_CAND_DOUBLES);
    m.get(&w.samp_entries, (size_t)nN * 2 * ESAC_SAMPLE_LIST_PER_HYP);  // (hypothesis, try) pairs
    // list counters + 1024 x 2 per-expert counters (esac_kernels.hip: expert_stats); the screened chain leaves them at zero
    m.get(&w.samp_count, (size_t)4 + 2 * 1024, Z);  m.get(&w.samp_pending, (size_t)nN);
    m.get(&w.fast_scores, (size_t)nN);  m.get(&w.scores, (size_t)nN);
    m.get(&w.exact_flag, (size_t)nN);  m.get(&w.n_contenders, (size_t)4 * nB, Z);
    m.get(&w.sel_partials, (size_t)nN * ESAC_SELECT_SPLIT);
    m.get(&w.sel_arrived, (size_t)nN, Z);  // k_select_rescore leaves it zero after every call
    m.get(&w.stats, (size_t)4 * nB);  m.get(&w.errs, (size_t)nP);
    m.get(&w.inlier_map, (size_t)nP * 2);  // two buffers, see esac_refine.hip
    m.get((char**)&w.corr_list, ((size_t)nP + (size_t)2048 * nB) * 16);  // sum over frames of corr_entries(P) < P + 2048 each
    m.get(&w.inlier_counts, (size_t)(ESAC_MAX_REF_STEPS + 1) * nB);  m.get(&w.result, (size_t)ESAC_RES_DOUBLES * nB, Z);
    m.get(&w.cycles, (size_t)32);  m.get(&w.tstamps, (size_t)nN * 2);
    m.get(&w.span_acc, (size_t)2, Z);  m.get(&w.spec_flag, (size_t)nN, Z);
    m.get(&w.spec_state, (size_t)8, Z);  m.get(&w.spec_cnt, (size_t)ESAC_SPEC_CNT_INTS, Z);
    int rc = m.err;
    if (!rc) rc = [&]() -> int {
        HIP_OK(hipMemcpy(w.status, &old_status, sizeof(old_status), hipMemcpyHostToDevice));
        if (old_hyps && old_n) HIP_OK(hipMemcpy(w.hyps, old_hyps, old_n * 6 * sizeof(double), hipMemcpyDeviceToDevice));
        return 0;
    }();
    if (old_hyps) (void)hipFree(old_hyps);
    if (rc) {  // everything this call allocated is released, the capacities read zero
        free_ws(c);
        return rc;
    }
    c->capN = nN; c->capP = nP; c->capB = nB;
    return 0;
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
    const int chunks = tiled_chunks(N, E);
    const long long part = (long long)n_sub * N;
    if (N <= c->tN && chunks <= c->tChunks && part <= c->tPart) return 0;
    HIP_OK(hipDeviceSynchronize());
    const int nN = N > c->tN ? N : c->tN, nC = chunks > c->tChunks ? chunks : c->tChunks;
    const long long nP = part > c->tPart ? part : c->tPart;
    free_tiled_ws(c);
    DevBufs& m = c->tiled_bufs;
    m.get(&c->ws.order, (size_t)nN);  m.get(&c->ws.rt_sorted, (size_t)nN * 12);
    m.get(&c->ws.chunks, (size_t)nC * 4);  m.get(&c->ws.n_chunks, (size_t)4);
    m.get(&c->ws.partials, (size_t)nP);  m.get(&c->ws.bucket_fill, (size_t)ESAC_TILED_MAX_EXPERTS);
    if (const int rc = m.err) {  // everything this call allocated is released, the capacities read zero
        free_tiled_ws(c);
        return rc;
    }
    c->tN = nN; c->tChunks = nC; c->tPart = nP;
    return 0;
}

// A call's argument block: checked (call_policy.hpp: check_args), the workspaces grown, pointers copied, the derived scalars
// filled in (call_scalars), a fresh epoch
static int make_args(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, KArgs* out,
                     int B = 1, long long sc_frame_stride = 0, int cam_frame = -1, bool training = false) {
    int rc = check_args(c != nullptr, d_sc && d_assign, p, B, cam_frame, training);
    if (rc) return rc;
    const int P = p->H * p->W;
    if ((rc = ensure_ws(c, p->N, P, B))) return rc;
    const bool tiled = want_tiled(p, d_sc, B, tiled_sub_tiles(P));
    if (tiled && (rc = ensure_tiled_ws(c, p->N, P, p->E))) return rc;
    const bool pack = want_pack(p, B);
    if (pack && (rc = ensure_pack_ws(c, (long long)p->E * P))) return rc;
    KArgs a = c->ws;
    a.sc4 = pack ? c->sc4 : nullptr;
    if (tiled) {
        a.n_sub = tiled_sub_tiles(P);
        a.n_chunks_max = tiled_chunks(p->N, p->E);
    } else {
        a.partials = nullptr;  // launch_score: per-hypothesis stream
    }
    a.frames = B; a.sc_frame_stride = sc_frame_stride;
    a.cams = nullptr;  // (the batch routes set both from their plan, behind stage_cams)
    a.shapes = 0;
    a.sc = d_sc; a.assign = d_assign;
    a.E = p->E; a.H = p->H; a.W = p->W; a.N = p->N;
    a.shift_x = p->shift_x; a.shift_y = p->shift_y; a.sub = p->sub_sampling;
    a.focal = p->focal; a.ppx = p->ppx; a.ppy = p->ppy;
    a.tau = p->inlier_thresh; a.alpha = p->inlier_alpha; a.beta = p->inlier_beta; a.max_reproj = p->max_reproj;
    a.seed = p->seed; a.call = p->call;
    const CallScalars v = call_scalars(p, c->capN);
    a.max_tries = v.max_tries; a.max_ref_steps = v.max_ref_steps; a.samp_cap = v.samp_cap; a.flags = v.flags; a.margin = v.margin;
    a.hyp_offset = p->hyp_offset; a.hyp_index = p->d_hyp_index; a.expert_base = p->expert_base;
    a.coop_max = c->coop_max; a.coop_extra = c->coop_stall ? 1 : 0;
    a.team = c->team.members;  // (the forward entry points fold the time-out latch in: forward_team)
    a.team_auto = c->team.auto_size ? 1 : 0; a.team_stride = c->team.spread ? 1 : 8;
    a.route = c->team.route ? 1 : 0;
    a.solo = 0; a.spec_mode = 0; a.spec_gate = 0; a.spec_debug = 0;
    a.spec_flag = nullptr;  // (forward_impl hands the flags to the kernels of a speculative call only)
    a.epoch = c->epoch += 1.0;  // every call gets its own epoch: result hand-off word and the tag of the status word
    a.sample_epoch = c->sample_epoch;  // launches that sample call mark_sampling() and overwrite this
    // (device-side span stamps only on sampled calls in timing mode: forward_impl clears tstamps otherwise)
    if (!c->keep_errs) a.errs = nullptr;
    c->last = LastCall{p->N, p->H, p->W, B, (size_t)P, c->last.bwd_frames, c->last.batch_cap, 0, 0};
    *out = a;
    return 0;
}

// The table of a planned batch call (batch_plan.hpp: every record is checked), staged in pinned memory of the context's own and
// uploaded on `s` -- once per call; chunks and re-runs offset the device pointer.  The staging is rewritten only after the previous
// upload has left it (an asynchronous batch may still have its copy queued); the device table in stream order behind its last readers.
static int stage_cams(CamTable& t, const BatchPlan& plan, const esac_hip_frame_cam* h_cams, int B, hipStream_t s) {
    static_assert(sizeof(esac_hip_frame_cam) == sizeof(FrameCam) && offsetof(esac_hip_frame_cam, focal) == offsetof(FrameCam, focal) &&
                  offsetof(esac_hip_frame_cam, ppy) == offsetof(FrameCam, ppy), "esac_hip_frame_cam is the device record");
    static_assert(offsetof(esac_hip_frame_cam, reserved) == offsetof(FrameCam, h) && offsetof(FrameCam, w) == offsetof(FrameCam, h) + 4 &&
                  offsetof(FrameCam, margin) == offsetof(FrameCam, h) + 8, "reserved[0..2] = the frame's h, w and margin");
    if (!t.h_cams) {
        HIP_OK(hipHostMalloc((void**)&t.h_cams, (size_t)ESAC_MAX_BATCH * sizeof(FrameCam), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&t.d_cams, (size_t)ESAC_MAX_BATCH * sizeof(FrameCam)));
        HIP_OK(hipEventCreateWithFlags(&t.cams_ev, hipEventDisableTiming));
    }
    if (t.cams_queued) {
        HIP_OK(hipEventSynchronize(t.cams_ev));
        t.cams_queued = false;
    }
    plan_records(plan, h_cams, B, t.h_cams);
    HIP_OK(hipMemcpyAsync(t.d_cams, t.h_cams, (size_t)B * sizeof(FrameCam), hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(t.cams_ev, s));
    t.cams_queued = true;
    return 0;
}
static int stage_cams(esac_hip_ctx* c, const BatchPlan& plan, const esac_hip_frame_cam* h_cams, int B, hipStream_t s) {
    return stage_cams(c->stage, plan, h_cams, B, s);
}

static void forward_team(const esac_hip_ctx* c, KArgs& a) { forward_team(c->team.latch, a.flags, &a.team, &a.solo); }

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
    c->sample_epoch = a.sample_epoch = a.epoch;
}

// hypotheses that came from esac_hip_write_hyps: the first stage that reads their fp32 [R|t] rows and rotation matrices forms them
static void ensure_rt32(esac_hip_ctx* c, const KArgs& a, hipStream_t s) {
    if (c->rt32_stale) launch_hyps_to_rt32(a, s);
    c->rt32_stale = false;
}
// stage entry points: validate, make the context's GPU current, launch one phase on the caller's stream
template <typename Launch>
static int run_stage(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream, const char* what, Launch launch) {
    if (!c) return fail(-1, "null context");
    DeviceGuard guard(c->device);
    KArgs a;
    if (int rc = make_args(c, d_sc, d_assign, p, &a)) return rc;
    launch(c, a, (hipStream_t)stream);
    return check_launch(what);
}
extern "C" int esac_hip_sample(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_sample", [](esac_hip_ctx* cc, KArgs a, hipStream_t s) { mark_sampling(cc, a); launch_sample(a, s); });
}
extern "C" int esac_hip_score(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_score_fast", [](esac_hip_ctx* cc, const KArgs& a, hipStream_t s) { ensure_rt32(cc, a, s); launch_score(a, s); });
}
extern "C" int esac_hip_select(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_select_rescore", [](esac_hip_ctx* cc, const KArgs& a, hipStream_t s) { ensure_rt32(cc, a, s); launch_select_rescore(a, s); });
}
extern "C" int esac_hip_refine(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream) {
    return run_stage(c, d_sc, d_assign, p, stream, "k_refine", [](esac_hip_ctx* cc, KArgs a, hipStream_t s) { forward_team(cc, a); cc->team.refine_tag = launch_refine(a, s); });
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
            const volatile unsigned long long* w = reinterpret_cast<const volatile unsigned long long*>(c->pin.record(b));
            if (c->pin.word(b, 32) != want) return false;
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
            if ((landed = all_landed())) break;
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
// ESAC_FLAG_AUTO_EXACT: the guaranteed routes where they are free (include/esac_hip.h)
static void apply_auto_exact(KArgs& a, int B) { a.flags = auto_exact_flags(a.flags, B, a.E, a.N, a.H, a.W); }
// KArgs::fold_select of the serial route (a team that refines <= 256 hypotheses of one frame runs their selection in its prologue)
static int serial_fold(const esac_hip_ctx* c, const KArgs& a) {
    return !c->team.fold_select ? 0 : refine_folds_select(a) ? 1 : refine_folds_exact_stats(a) ? 2 : 0;
}
// The serial route's first two stages on the route kernels?  (a: the call's arguments as its first launch will see them;
// table: the caller handed a camera table in -- also where a single frame's record 0 went inline)
static bool front_route_eligible(const esac_hip_ctx* c, const KArgs& a, bool table) {
    static_assert(FRONT_FLAG_EXACT_SCORES == ESAC_FLAG_EXACT_SCORES, "mirror of include/esac_hip.h");
    const FrontRouteQuery q{c->front.on, true, a.frames, a.N, a.E, a.H, a.W, a.flags, a.max_tries, a.first_try, a.hyp_offset, table || a.cams != nullptr,
                            a.shapes, a.sc4 != nullptr, a.hyp_index != nullptr, a.spec_flag != nullptr, a.tstamps != nullptr, a.errs != nullptr};
    return front_takes_route(q);
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
        default: c->team.refine_tag = launch_refine(a, s); return "k_refine";
    }
}
// A forward call up to its first launch (p: the plan's block where there is a table -- record 0 inline); *tm: the call is timed
static int prepare_forward(esac_hip_ctx* c, const float* d_sc, long long sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p,
                           int B, hipStream_t s, const esac_hip_frame_cam* h_cams, const BatchPlan& plan, double t_entry, KArgs* out, bool* tm) {
    KArgs& a = *out;
    int rc = make_args(c, d_sc, d_assign, p, &a, B, sc_frame_stride, h_cams ? 0 : -1);
    if (rc) return rc;
    if (plan.stage) {
        // a ragged table: p's H x W is the capacity -- make_args has sized the workspaces, and every host decision below reads
        // a.H * a.W as that (team size and cells per lane, LDS or global list, the selection's split, the sampler's plan); the
        // kernels take the frame's own grid and margin from the table (device_common.hpp:frame_view)
        if ((rc = stage_cams(c, plan, h_cams, B, s))) return rc;
        a.cams = c->stage.d_cams;
        a.shapes = plan.shapes;
        // esac_hip_read(ESAC_BUF_INLIER_MAP): the one-workgroup refinement alternates its two map buffers P cells apart with the
        // P of the frame's OWN grid (the team kernel only ever writes buffer 0)
        if (plan.cells0) c->last.map1 = plan.cells0;
    }
    c->team.latch.forward_call();
    forward_team(c, a);
    c->timing.host_ns[6] = t_entry;
    c->timing.host_ns[0] = now_ns() - t_entry;
    apply_auto_exact(a, B);
    // events and stamps cost GPU time themselves (an empty event pair reads ~5 us): sample every timing_period-th call
    *tm = c->timing.on && (c->timing.calls++ % c->timing.period) == 0;
    // device-side span stamps: only the per-hypothesis stream (k_score_fast) writes them, and k_select_rescore reduces them --
    // a call whose selection runs in the refinement kernel's prologue keeps ITS launch sequence under timing (the phase
    // events then bracket what an untimed call runs) and takes no stamps
    if (!*tm || a.partials || (a.flags & ESAC_FLAG_EXACT_SCORES)) a.tstamps = nullptr;
    if (a.tstamps) {
        KArgs probe = a;
        probe.tstamps = nullptr;
        if (c->team.fold_select && refine_folds_select(probe)) a.tstamps = nullptr;
    }
    return 0;
}

// Several experts: the sampler's straggler chain (wrong-expert hypotheses, which practically never win) runs BESIDE the scoring,
// selection and refinement of what the first pass settled (KArgs::spec_mode; k_spec_join makes the outputs the serial order's)
// (not where the selection runs in the refinement kernel's prologue -- a single frame of <= 256 hypotheses on a team: that
// route re-scores its contenders member by member, another summation order than k_select_rescore's and k_spec_join's)
static bool speculation_eligible(const esac_hip_ctx* c, const KArgs& a, int B, hipStream_t s) {
    if (c->spec.off || B != 1 || (a.flags & ESAC_FLAG_EXACT_SCORES) || !sample_can_split(a) || a.partials || (long long)a.H * a.W >= 32768 || (c->team.fold_select && refine_folds_select(a)))
        return false;
    if (s == nullptr) return true;
    // a stream that is being captured into a graph takes no launches on other streams beside it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool plain = hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    return plain;
}
static int ensure_spec_streams(esac_hip_ctx* c) {
    if (!c->spec.side) HIP_OK(hipStreamCreateWithFlags(&c->spec.side, hipStreamNonBlocking));
    if (!c->spec.side2) HIP_OK(hipStreamCreateWithFlags(&c->spec.side2, hipStreamNonBlocking));
    if (!c->spec.ev) HIP_OK(hipEventCreateWithFlags(&c->spec.ev, hipEventDisableTiming));
    return 0;
}
static int enqueue_speculative(esac_hip_ctx* c, KArgs& a, hipStream_t s, bool tm, double t_entry) {
    c->spec.calls++;
    c->spec.last_epoch = a.epoch;
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
    HIP_OK(hipEventRecord(c->spec.ev, s));
    launch_sample_split(a, s, &chain, &chain_waves);
    if (int rc = check_launch("k_sample (first pass)")) return rc;
    c->timing.host_ns[1] = now_ns() - t_entry;
    if (tm) HIP_OK(hipEventRecord(c->timing.ev[1], s));
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
    c->timing.host_ns[2] = now_ns() - t_entry;
    if (tm) HIP_OK(hipEventRecord(c->timing.ev[2], s));
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
    if (tm) HIP_OK(hipEventRecord(c->timing.ev[3], s));
    KArgs ar = as;
    ar.spec_mode = 2;
    ar.spec_debug = c->spec.second_best ? 1 : 0;
    c->team.refine_tag = launch_refine(ar, s);  // (its first workgroup opens the chain: spec_open_chain)
    c->team.was_team = refine_team_members(ar) > 0;
    if (int rc = check_launch("k_refine (speculative)")) return rc;
    // (host order: the selection first -- the join waits behind it; a launch call is 3-4 us of host time, and the chain's five
    // in front of it would hold the selection back by 20 us.  The JOIN is enqueued behind the chain it waits for.)
    HIP_OK(hipStreamWaitEvent(c->spec.side2, c->spec.ev, 0));
    launch_spec_wait(a, 3, c->spec.side2);
    launch_select_rescore(as, c->spec.side2);
    if (int rc = check_launch("k_select_rescore (settled)")) return rc;
    HIP_OK(hipStreamWaitEvent(c->spec.side, c->spec.ev, 0));
    launch_spec_wait(a, 3, c->spec.side);
    launch_sample_stragglers(chain, chain_waves, c->spec.side);
    if (!c->spec.lose_chain) launch_score_stragglers(a, c->spec.side);  // behind the chain on the side stream; its last workgroup writes "the chain is done"
    if (int rc = check_launch("straggler chain")) return rc;
    launch_spec_join(a, c->spec.side2);
    if (int rc = check_launch("k_spec_join")) return rc;
    // The second refinement is enqueued NOW and returns at once unless the join marked the speculation as failed
    // (KArgs::spec_gate): a failed speculation then costs the refinement, not a host round trip on top of it (and an
    // asynchronous call could not look at the join's verdict anyway); a speculation that held has delivered its record
    // before the gate opens
    KArgs ag = a;
    ag.spec_gate = 1;
    (void)launch_refine(ag, s);  // (esac_hip_check follows the speculative launch's tag: a team time-out there is the common case of the two)
    if (int rc = check_launch("k_refine (gated)")) return rc;
    c->timing.host_ns[3] = now_ns() - t_entry;
    return 0;
}
// Blocking call, after its record has landed.  The members of a team did not all become resident in time (a shared or partitioned
// GPU, or the caller's own kernels on another stream holding the CUs): the same refinement(s) in ONE workgroup each -- the
// hypotheses, scores and selection of this call are still in the workspace.  Then the slots to the caller's records, and the
// status words as error codes.
static int collect_records(esac_hip_ctx* c, KArgs& a, int B, hipStream_t s, double* h_result_out) {
    bool team_failed = false, bad_assign = false, timed_out = false;
    for (int b = 0; b < B; b++) team_failed |= c->pin.status(b) == ESAC_PIN_TEAM_TIMEOUT;
    const bool was_team = refine_team_members(a) > 0;
    if (team_failed && was_team) {
        c->team.latch.timed_out();
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
        c->team.latch.strikes = 0;
    }
    __sync_synchronize();
    for (int b = 0; b < B; b++) {
        c->pin.copy_out(b, h_result_out + (size_t)b * ESAC_RES_DOUBLES);
        bad_assign |= c->pin.status(b) == ESAC_PIN_BAD_ASSIGN;
        timed_out |= c->pin.status(b) == ESAC_PIN_TEAM_TIMEOUT;
    }
    if (timed_out) return fail(-12, "esac_hip_forward: the cooperating refinement workgroups could not synchronise (not all of them became resident)");
    if (bad_assign)
        return fail(-10, "hypAssignment holds a value outside [0,%d) (device-resident tensor; such hypotheses were scored against expert 0)", a.E);
    return 0;
}

static int forward_impl(esac_hip_ctx* c, const float* d_sc, long long sc_frame_stride, const int64_t* d_assign,
                        const esac_hip_params* p, int B, void* stream, double* d_scores_out, double* d_result_out, double* h_result_out, const esac_hip_frame_cam* h_cams = nullptr,
                        bool shapes = false) {
    BatchPlan plan;  // (without a table: a null check, and the call goes on with the caller's block)
    int rc = plan_batch(BATCH_FORWARD, "esac_hip_forward_batch_shapes", c != nullptr, d_sc && d_assign, true, p, B, h_cams, shapes, sc_frame_stride, 0, &plan);
    if (rc) return rc;
    if (h_cams) p = &plan.p;
    if (!c) return fail(-1, "null context");
    const double t_entry = now_ns();
    DeviceGuard guard(c->device);
    const hipStream_t s = (hipStream_t)stream;
    KArgs a;
    bool tm = false;
    if ((rc = prepare_forward(c, d_sc, sc_frame_stride, d_assign, p, B, s, h_cams, plan, t_entry, &a, &tm))) return rc;
    a.scores_user = d_scores_out; a.result_user = d_result_out;
    a.result_pin = h_result_out ? c->pin.d : nullptr;
    c->spec.last_epoch = 0;
    c->front.taken = false;
    const bool spec = speculation_eligible(c, a, B, s);
    if (spec && (rc = ensure_spec_streams(c))) return rc;
    if (tm) HIP_OK(hipEventRecord(c->timing.ev[0], s));
    mark_sampling(c, a);
    if (spec) {
        if ((rc = enqueue_speculative(c, a, s, tm, t_entry))) return rc;
    } else {
        constexpr int stamp[4] = {1, 2, 0, 3};  // the host_ns slot stamped behind stage k (the selection has none)
        // the front route: the sampler and the exact score with this call's modes compiled in.  Its sampler stores no fp32
        // rows -- no kernel of this call reads them, and the next stage that does rebuilds them (ensure_rt32)
        const bool front = c->front.taken = front_route_eligible(c, a, h_cams != nullptr);
        if (front) c->rt32_stale = true;
        for (int k = 0; k < 4; k++) {
            if (k == 2) a.fold_select = serial_fold(c, a);
            const char* what;
            if (front && k == 0)      launch_sample_route(a, s), what = "k_sample_route";
            else if (front && k == 1) launch_rescore_route(a, s), what = "k_rescore_route";
            else                      what = enqueue_serial_stage(c, a, k, s);
            if (k == 3) c->team.was_team = refine_team_members(a) > 0;
            if ((rc = check_launch(what))) return rc;
            if (stamp[k]) c->timing.host_ns[stamp[k]] = now_ns() - t_entry;
            if (tm && k < 3) HIP_OK(hipEventRecord(c->timing.ev[k + 1], s));
        }
    }
    if (tm) {
        HIP_OK(hipEventRecord(c->timing.ev[4], s));
        // an EMPTY interval: what two adjacent hipEventRecord calls measure with nothing in between,
        // i.e. the part of every bracketed phase that is not kernel time
        HIP_OK(hipEventRecord(c->timing.ev[5], s));
        HIP_OK(hipEventRecord(c->timing.ev[6], s));
        c->timing.ev_valid = true;
    }
    if (h_result_out) {
        if ((rc = wait_record(c, s, B, c->epoch, "esac_hip_forward: the refinement kernel"))) return rc;
        if (spec && c->pin.status(0) == ESAC_PIN_NO_CHAIN) {
            // the context's own stream never reported the straggler chain as done within 20 ms (it shares a hardware queue with
            // the caller's stream and something else is holding that queue, or its launch failed): no more speculation on this
            // context, and this call again -- the serial route
            c->spec.off = c->spec.env_off = true;
            HIP_OK(hipStreamSynchronize(c->spec.side));
            if (c->spec.side2) HIP_OK(hipStreamSynchronize(c->spec.side2));
            HIP_OK(hipStreamSynchronize(s));
            // (p, no h_cams: a speculative call is ONE frame, whose camera table is record 0 -- in p's inline fields already, and checked)
            return forward_impl(c, d_sc, sc_frame_stride, d_assign, p, B, stream, d_scores_out, d_result_out, h_result_out);
        }
        c->timing.host_ns[4] = now_ns() - t_entry;
        if ((rc = collect_records(c, a, B, s, h_result_out))) return rc;
    }
    c->timing.host_ns[5] = now_ns() - t_entry;
    if (h_result_out) {  // running sums (seven additions: the caller's timed loop is not touched by reading them later)
        for (int k = 0; k < 6; k++) c->timing.host_sum[k] += c->timing.host_ns[k];
        if (c->timing.last_return > 0) c->timing.host_sum[6] += t_entry - c->timing.last_return;  // the caller's time between two calls
        c->timing.last_return = t_entry + c->timing.host_ns[5];
        c->timing.host_n++;
    }
    return 0;
}

extern "C" int esac_hip_host_turn_mean(esac_hip_ctx* c, double out_ns[8], int reset) {
    if (!c || !out_ns) return fail(-1, "esac_hip_host_turn_mean: null argument");
    const double n = c->timing.host_n > 0 ? (double)c->timing.host_n : 1.0;
    for (int k = 0; k < 6; k++) out_ns[k] = c->timing.host_sum[k] / n;
    out_ns[6] = c->timing.host_n > 1 ? c->timing.host_sum[6] / (double)(c->timing.host_n - 1) : 0.0;
    out_ns[7] = (double)c->timing.host_n;
    if (reset) {
        for (double& v : c->timing.host_sum) v = 0;
        c->timing.host_n = 0;
        c->timing.last_return = 0;
    }
    return 0;
}
extern "C" int esac_hip_host_turn(esac_hip_ctx* c, double out_ns[8]) {
    if (!c || !out_ns) return fail(-1, "esac_hip_host_turn: null argument");
    for (int k = 0; k < 8; k++) out_ns[k] = c->timing.host_ns[k];
    return 0;
}

// Mean GPU time of each stage of the forward chain for THIS input: the chain runs once, then every stage is launched
// `reps` times back to back between one pair of hipEvents on `stream` (stages are idempotent given their inputs).
// A host-side loop around single launches cannot do this for ~5 us kernels: it is bound by the caller's launch rate.
extern "C" int esac_hip_time_stages(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream, int reps, float out_ms[4]) {
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
extern "C" int esac_hip_pick_record(esac_hip_ctx* c, const double* d_records, int world, void* stream, double* h_record_out, double* d_zero, int n_zero) {
    if (!c || !d_records || !h_record_out || world < 1 || n_zero < 0 || (n_zero > 0 && !d_zero))
        return fail(-1, "esac_hip_pick_record: bad argument");
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    c->epoch += 1.0;
    const double want = c->epoch;
    launch_pick_record(d_records, world, c->pin.d, want, d_zero, n_zero, s);
    if (int rc = check_launch("k_pick_record")) return rc;
    // (not wait_record: k_pick_record hands over with fences and NO check word -- the epoch word alone says the record is there)
    const volatile double* word = c->pin.record(0) + 32;
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
    c->pin.copy_out(0, h_record_out);
    if (c->pin.status(0) == ESAC_PIN_TEAM_TIMEOUT)
        return fail(-12, "esac_hip_pick_record: the refinement team of at least one rank timed out (its record carries ESAC_RES_VALID = 3); "
                         "every rank sees the same records: run the frame again with ESAC_FLAG_REFINE_SOLO");
    if (c->pin.status(0) == ESAC_PIN_NONE) return fail(-11, "esac_hip_pick_record: no rank produced a hypothesis");
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
    NCCL_OK(rccl().comm_init_rank(&c->comm.handle, nranks, id, rank));
    c->comm.ranks = nranks;
    c->comm.rank = rank;
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
    if (!c->comm.handle) return fail(-13, "esac_hip_allreduce_sum: no communicator (esac_hip_comm_init)");
    DeviceGuard guard(c->device);
    NCCL_OK(rccl().all_reduce(d_buf, d_buf, count, NCCL_DOUBLE, NCCL_SUM, c->comm.handle, (hipStream_t)stream));
    return 0;
}
// What the communicator ITSELF reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), beside what the context was told
// and the GPU it is bound to: the proof a multi-GPU bench line carries of how many ranks RCCL saw (bench.py: ranks_seen).
extern "C" int esac_hip_comm_info(esac_hip_ctx* c, int32_t out[4]) {
    if (!c || !out) return fail(-1, "esac_hip_comm_info: null argument");
    if (!c->comm.handle) return fail(-13, "esac_hip_comm_info: no communicator (esac_hip_comm_init)");
    int count = c->comm.ranks, rank = c->comm.rank, dev = -1;
    if (rccl().comm_count) NCCL_OK(rccl().comm_count(c->comm.handle, &count));
    if (rccl().comm_user_rank) NCCL_OK(rccl().comm_user_rank(c->comm.handle, &rank));
    if (rccl().comm_cu_device) NCCL_OK(rccl().comm_cu_device(c->comm.handle, &dev));
    out[0] = count;
    out[1] = rank;
    out[2] = dev;
    out[3] = c->device;
    return 0;
}

extern "C" int esac_hip_forward(esac_hip_ctx* c, const float* d_sc, const int64_t* d_assign, const esac_hip_params* p, void* stream, double* d_scores_out, double* d_result_out, double* h_result_out) {
    return forward_impl(c, d_sc, 0, d_assign, p, 1, stream, d_scores_out, d_result_out, h_result_out);
}
extern "C" int esac_hip_forward_batch(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p, void* stream,
                                      double* d_scores_out, double* d_result_out, double* h_result_out) {
    return esac_hip_forward_batch_cams(c, B, d_sc, sc_frame_stride, d_assign, p, nullptr, stream, d_scores_out, d_result_out, h_result_out);
}
extern "C" int esac_hip_forward_batch_cams(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p, const esac_hip_frame_cam* h_cams,
                                           void* stream, double* d_scores_out, double* d_result_out, double* h_result_out) {
    return forward_impl(c, d_sc, (long long)sc_frame_stride, d_assign, p, B, stream, d_scores_out, d_result_out, h_result_out, h_cams);
}
// Frames that differ in image size: esac_hip_forward_batch_cams with frame b's grid in h_cams[b].reserved[0..1]; p->H * p->W is
// the capacity in cells (include/esac_hip.h).  reserved[2] is the library's (the frame's margin goes there on the way to the device).
extern "C" int esac_hip_forward_batch_shapes(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, const int64_t* d_assign, const esac_hip_params* p, const esac_hip_frame_cam* h_cams,
                                             void* stream, double* d_scores_out, double* d_result_out, double* h_result_out) {
    return forward_impl(c, d_sc, (long long)sc_frame_stride, d_assign, p, B, stream, d_scores_out, d_result_out, h_result_out, h_cams, true);
}

// ---------------------------------------------------------------- training path
// `cap` = slots (hypotheses with p >= PROB_THRESH) per frame the slab workspace must hold, for B frames (a batch: every buffer
// frame-major, device_common.hpp:bwd_frame_strides); it only ever grows
static int ensure_bws(esac_hip_ctx* c, int N, int P, int cap, int B = 1) {
    const bool lists = P > ESAC_REFINE_LDS_CAP;
    const long long NB = (long long)N * B, slots = (long long)cap * B, rows = (long long)bwd_rows(N) * B;
    if (NB <= c->train.N && P <= c->train.P && slots <= c->train.slots && rows <= c->train.rows && B <= c->train.B && (!lists || c->train.lists)) return 0;
    HIP_OK(hipDeviceSynchronize());
    const long long nN = NB > c->train.N ? NB : c->train.N, nslots = slots > c->train.slots ? slots : c->train.slots, nrows = rows > c->train.rows ? rows : c->train.rows;
    const int nP = P > c->train.P ? P : c->train.P, nB = B > c->train.B ? B : c->train.B;
    const bool nlists = lists || c->train.lists;
    free_bws(c);
    DevBufs& m = c->train.bufs;
    BwdArgs& w = c->train.ws;
    const bool Z = true;  // zero-filled
    m.get(&w.sel, (size_t)nN);  m.get(&w.n_sel, (size_t)4 * nB, Z);
    m.get(&w.probs, (size_t)nN);  m.get(&w.losses, (size_t)nN);
    m.get(&w.ref_hyps, (size_t)nN * 6);  m.get(&w.sgrad, (size_t)nN);
    m.get(&w.dloss, (size_t)nrows * 6);  // small per-slot tables: worst case min(N, 1000) rows per frame
    m.get(&w.maps, (size_t)nslots * 2 * nP);  m.get(&w.map_info, (size_t)nrows * 4);
    if (nlists) m.get((char**)&w.corr_lists, (size_t)nslots * ((size_t)nP + 2048) * 16);  // corr_entries(P) < P + 2048 per slot
    m.get(&w.grad1, (size_t)nslots * nP * 3);  m.get(&w.grad2, (size_t)nslots * nP * 3);
    m.get(&w.out, (size_t)4 * nB);  m.get(&w.arrived, (size_t)1, Z);
    m.get(&w.sel_max, (size_t)1, Z);
    m.get(&w.team_gran, (size_t)nslots * 2 * ESAC_REFINE_TEAM_MAX * 32 * 2, Z);  // 16-byte granules: [slot][parity][member][value]
    if (const int rc = m.err) {  // everything this call allocated is released, the capacities read zero
        free_bws(c);
        return rc;
    }
    c->train.N = nN; c->train.P = nP; c->train.slots = nslots; c->train.rows = nrows; c->train.B = nB; c->train.lists = nlists;
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

// A batched training call as its extern "C" signature carries it (gt_poses, out: host memory of the blocking entry points, device
// memory of the asynchronous ones).  shapes: h_cams carries every frame's grid and p's H x W is the capacity (a ragged batch).
struct BwdBatchIn {
    int B; const float* d_sc; int64_t sc_frame_stride; float* d_out_gradients; int64_t grad_frame_stride; const int64_t* d_assign;
    const float* gt_poses; const esac_hip_frame_cam* h_cams; float w_loss_rot, w_loss_trans, loss_cut;
    const esac_hip_params* p; void* stream; double* out; bool shapes;
};

// The KArgs of a batch's chunk [b0, b0 + nb): camera record b0 in the inline fields, the call counter, the tensors and the camera
// table offset by the chunk's first frame (validated, workspaces grown, a fresh epoch: make_args).  KArgs::shapes is the plan's,
// decided over the WHOLE table, so that every chunk of a ragged batch takes the same refinement kernel
static int chunk_args(esac_hip_ctx* c, const BwdBatchIn& in, const BatchPlan& plan, int b0, int nb, KArgs* a) {
    esac_hip_params pc = in.h_cams ? with_cam(plan.p, in.h_cams[b0]) : plan.p;
    pc.call = plan.p.call + (uint64_t)b0;
    if (int rc = make_args(c, in.d_sc + (size_t)b0 * in.sc_frame_stride, in.d_assign + (size_t)b0 * pc.N, &pc, a, nb, in.sc_frame_stride, -1, true)) return rc;
    if (in.h_cams) a->cams = c->stage.d_cams + b0;
    a->shapes = plan.shapes;
    // esac_hip_read of the slabs / slot maps: frame 0 of this chunk keeps its slots at its OWN h*w (device_common.hpp:bwd_frame_strides)
    if (plan.shapes) c->last.slot_cells = (size_t)in.h_cams[b0].reserved[0] * (size_t)in.h_cams[b0].reserved[1];
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

static PoseArm take_pose_arm(esac_hip_ctx* c) {
    const PoseArm arm = c ? c->stage.pose_arm : PoseArm{};
    if (c) c->stage.pose_arm = PoseArm{};
    return arm;
}
// ... and checks it against the call's frames before anything is launched
static int check_pose_arm(const char* who, const PoseArm& arm, int B) { return check_pose_arm(who, arm.rec != nullptr, arm.frames, B); }

// a.bwd of one selection .. accumulation pass over `frames` frames from frame b0 of the call, `cap` slots each, in the context's
// slot workspace (which ensure_bws has sized).  Every field a route does not use is null / 0 here, in this one place.
// want_teams: refine the slots by teams where this call can (single blocking calls; a.bwd.team_max_slots != 0 says it will).
static void fill_bwd(esac_hip_ctx* c, KArgs& a, const BwdCall& call, int b0, int frames, int cap, bool want_teams) {
    c->last.bwd_frames = frames;
    c->last.batch_cap = call.batch ? cap : 0;
    a.frames = frames;  // (a rerun after an overflow may take fewer frames: their samples stay where they are)
    a.bwd = c->train.ws;
    a.bwd.cap = cap;
    a.bwd.team = 0; a.bwd.team_tag = 0;  // (the slot-team launch sets these two)
    a.bwd.team_max_slots = want_teams && refine_slots_can_team(a) ? ESAC_SLOT_TEAMS_MAX : 0;  // 0: one workgroup per slot
    a.bwd.out_grad = call.out_grad + (size_t)b0 * call.grad_frame_stride;
    a.bwd.grad_frame_stride = call.grad_frame_stride;
    a.bwd.w_rot = call.w_rot; a.bwd.w_trans = call.w_trans; a.bwd.cut = call.cut;
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
        c->team.slot_calls++;
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
    c->stage.pose_arm = PoseArm{d_records, d_records ? frames : 0};
    return 0;
}

extern "C" int esac_hip_backward(esac_hip_ctx* c, const float* d_sc, float* d_out_gradients, const int64_t* d_assign, const float* h_gt_pose,
                                 float w_loss_rot, float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out) {
    const PoseArm arm = take_pose_arm(c);
    int rc = check_backward_entry(d_out_gradients && h_gt_pose, c != nullptr, p);
    if (rc) return rc;
    DeviceGuard guard(c->device);
    KArgs a;
    if ((rc = make_args(c, d_sc, d_assign, p, &a, 1, 0, -1, true))) return rc;
    if ((rc = check_backward_call(p))) return rc;
    if ((rc = check_pose_arm("esac_hip_backward", arm, 1))) return rc;
    const int P = p->H * p->W;
    // Slot workspace (two 3P-double slabs + two inlier maps per slot), start_cap slots of it (call_policy.hpp).  When the
    // selection of a blocking call overflows it, the call grows the workspace and runs selection..accumulation again -- the
    // accumulation kernel adds nothing on overflow, so the caller's tensor is untouched by the aborted pass.
    const int worst = p->N < ESAC_BWD_MAX_SLOTS ? p->N : ESAC_BWD_MAX_SLOTS;
    int cap = start_cap(h_out != nullptr, c->train.cap, worst);
    double gt[16], gt_pose[6];
    if (!gt_from_pose(h_gt_pose, gt, gt_pose))  // (gt_math.hpp: the text k_bwd_gt_prepare runs on the device; false: singular)
        return fail(-4, "esac_hip_backward: the ground-truth pose is singular");
    BwdCall call = {d_out_gradients, 0, w_loss_rot, w_loss_trans, loss_cut};
    call.gt = gt; call.gt_pose = gt_pose; call.pose_rec = arm.rec;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = enqueue_bwd_sampling(c, a, s, false))) return rc;
    // A blocking call can refine again with one workgroup per slot should a slot team time out; an asynchronous one cannot and
    // does not use teams.
    bool use_teams = h_out && c->team.slot_teams;
    for (int attempt = 0;; attempt++) {
        if ((rc = ensure_bws(c, p->N, P, cap))) return rc;
        if (cap > c->train.cap) c->train.cap = cap;
        fill_bwd(c, a, call, 0, 1, cap, use_teams);
        const bool teams = a.bwd.team_max_slots != 0;
        if ((rc = enqueue_bwd_chain(c, a, s, h_out ? c->pin.d : nullptr))) return rc;
        if (!h_out) return 0;
        if ((rc = wait_record(c, s, 1, a.epoch, "esac_hip_backward: the accumulation kernel"))) return rc;
        __sync_synchronize();
        c->pin.copy_out(0, h_out, 4);
        const bool team_failed = c->pin.word(0, 4) == 1.0;
        if (teams && team_failed) {  // a team timed out: nothing was accumulated; one workgroup per slot from here on
            c->team.slot_fallbacks++;
            c->team.slot_teams = use_teams = false;
            attempt--;
            a.epoch = c->epoch += 1.0;
            continue;
        }
        c->team.last_nsel = (int)h_out[1];
        c->team.last_bwd_teams = teams && c->team.last_nsel <= ESAC_SLOT_TEAMS_MAX;
        const int needed = (int)h_out[1];
        if (needed <= cap || attempt >= 1) break;  // one retry suffices: the second pass is sized by the true count
        cap = grown_cap(needed, worst);
        a.epoch = c->epoch += 1.0;
    }
    if (h_out[3] != 0.0)
        return fail(-10, "hypAssignment holds a value outside [0,%d) (device-resident tensor; such hypotheses were scored against expert 0)", p->E);
    return 0;
}

// Where both batched training routes start: the pose arm taken, the call planned (batch_plan.hpp: every check before anything is
// allocated or launched -- the caller's gradients stay untouched on an error), the context's GPU current, the parameters through
// make_args once, the table on its way to the device, and what every chunk of the call shares.  Nothing in here waits for the
// stream; the one wait is stage_cams' on the PREVIOUS call's table copy.
struct BwdBatchStart {
    DeviceGuard guard;
    BatchPlan plan;   // plan.p is the call's parameter block from here on.  A ragged batch: its H x W is the capacity -- the workspaces,
                      // the chunks (a chunk of small frames could hold more of them; the charge is the safe side and keeps the chunking
                      // a function of the parameters alone) and every launch are sized by it
    hipStream_t s;
    KArgs a;
    BwdCall call;     // (gt_frames, and the asynchronous route's frame_status and rec_dev, are the body's to set)
    int N, P, worst;  // worst: the slots a frame can need, min(N, 1000)
    long long slot_bytes;
};
static int begin_bwd_batch(esac_hip_ctx* c, const BwdBatchIn& in, BatchRoute route, BwdBatchStart* st) {
    const PoseArm arm = take_pose_arm(c);
    const bool async = route == BATCH_TRAIN_ASYNC;
    int rc = plan_batch(route, async ? "esac_hip_backward_batch_dev_shapes" : "esac_hip_backward_batch_shapes", c != nullptr,
                        in.d_sc && in.d_out_gradients && in.d_assign && in.gt_poses, in.out != nullptr, in.p, in.B, in.h_cams, in.shapes,
                        in.sc_frame_stride, in.grad_frame_stride, &st->plan);
    if (rc) return rc;
    if ((rc = check_pose_arm(async ? "esac_hip_backward_batch_dev" : "esac_hip_backward_batch", arm, in.B))) return rc;
    st->guard.enter(c->device);
    st->s = (hipStream_t)in.stream;
    if ((rc = make_args(c, in.d_sc, in.d_assign, &st->plan.p, &st->a, 1, 0, in.h_cams ? 0 : -1, true))) return rc;
    if (st->plan.stage && (rc = stage_cams(c, st->plan, in.h_cams, in.B, st->s))) return rc;
    st->call = BwdCall{in.d_out_gradients, in.grad_frame_stride, in.w_loss_rot, in.w_loss_trans, in.loss_cut};
    st->call.batch = true; st->call.pose_rec = arm.rec;
    st->N = st->plan.p.N; st->P = st->plan.p.H * st->plan.p.W; st->worst = bwd_rows(st->N);
    st->slot_bytes = bwd_slot_bytes(st->P, corr_entries(st->P));
    return 0;
}

// B independent frames of the training path in one set of launches per chunk (include/esac_hip.h).  Frame b is the b-th of B
// consecutive esac_hip_backward calls (call p->call + b); its slots are refined with one workgroup each.  The slot workspace of
// B x cap slots is bounded by the context's budget: beyond it the frames go in chunks of consecutive frames, each with its own
// launch set (the frames are independent, so the chunking changes no result).  An overflow of the slot workspace in ANY frame
// of a chunk stops the accumulation of every frame of it (one batch-wide word, BwdArgs::sel_max); the host grows `cap` to the
// largest frame's count and runs selection .. accumulation of the chunk again, so nothing is added twice.  A camera per frame
// (in.h_cams: host, B records; NULL: p's five fields for every frame): chunk_args puts record b0 of a chunk into its inline fields.
static int backward_batch_impl(esac_hip_ctx* c, const BwdBatchIn& in) {
    BwdBatchStart st;
    int rc = begin_bwd_batch(c, in, BATCH_TRAIN_BLOCKING, &st);
    if (rc) return rc;
    const hipStream_t s = st.s;
    KArgs& a = st.a;
    double* const h_out = in.out;
    if (!c->stage.h_gt) {
        HIP_OK(hipHostMalloc((void**)&c->stage.h_gt, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double), hipHostMallocDefault));
        HIP_OK(hipMalloc((void**)&c->stage.d_gt, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double)));
    }
    HIP_OK(hipStreamSynchronize(s));  // (the staging buffer is free: a batch that failed half-way may have left its copy queued)
    const int B = in.B;
    for (int b = 0; b < B; b++) {
        double* g = c->stage.h_gt + (size_t)b * ESAC_GT_DOUBLES;
        if (!gt_from_pose(in.gt_poses + (size_t)b * 16, g, g + 16))
            return fail(-4, "esac_hip_backward_batch: the ground-truth pose of frame %d is singular", b);
    }
    HIP_OK(hipMemcpyAsync(c->stage.d_gt, c->stage.h_gt, (size_t)B * ESAC_GT_DOUBLES * sizeof(double), hipMemcpyHostToDevice, s));
    st.call.gt_frames = c->stage.d_gt;
    int cap = start_cap(true, c->train.cap_batch, st.worst);
    bool any_bad = false;
    for (int b0 = 0; b0 < B;) {
        int nb = chunk_frames(c->train.budget, cap, st.slot_bytes, B - b0);
        if ((rc = chunk_args(c, in, st.plan, b0, nb, &a))) return rc;
        if ((rc = enqueue_bwd_sampling(c, a, s, true))) return rc;
        for (int attempt = 0;; attempt++) {
            if ((rc = ensure_bws(c, st.N, st.P, cap, nb))) return rc;
            if (cap > c->train.cap_batch) c->train.cap_batch = cap;
            fill_bwd(c, a, st.call, b0, nb, cap, false);
            if ((rc = enqueue_bwd_chain(c, a, s, c->pin.d))) return rc;  // one pinned slot per frame of the chunk
            if ((rc = wait_record(c, s, nb, a.epoch, "esac_hip_backward_batch: the accumulation kernel"))) return rc;
            __sync_synchronize();
            int needed = 0;
            for (int b = 0; b < nb; b++) needed = (int)c->pin.word(b, 1) > needed ? (int)c->pin.word(b, 1) : needed;
            if (needed <= cap || attempt >= 1) {  // one retry suffices: the second pass is sized by the largest true count
                for (int b = 0; b < nb; b++) c->pin.copy_out(b, h_out + (size_t)(b0 + b) * 4, 4);
                break;
            }
            cap = grown_cap(needed, st.worst);
            const int fit = chunk_frames(c->train.budget, cap, st.slot_bytes, nb);
            nb = fit < nb ? fit : nb;
            a.epoch = c->epoch += 1.0;
        }
        for (int b = 0; b < nb; b++) any_bad |= h_out[(size_t)(b0 + b) * 4 + 3] != 0.0;
        b0 += nb;
    }
    if (any_bad)
        return fail(-10, "hypAssignment holds a value outside [0,%d) in at least one frame (h_out[b*4+3] = 1 names them; such "
                         "hypotheses were scored against expert 0)", st.plan.p.E);
    return 0;
}
extern "C" int esac_hip_backward_batch(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                       int64_t grad_frame_stride, const int64_t* d_assign, const float* h_gt_poses, float w_loss_rot,
                                       float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out) {
    return backward_batch_impl(c, BwdBatchIn{B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, h_gt_poses, nullptr, w_loss_rot, w_loss_trans, loss_cut, p, stream, h_out, false});
}
extern "C" int esac_hip_backward_batch_cams(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                            int64_t grad_frame_stride, const int64_t* d_assign, const float* h_gt_poses, const esac_hip_frame_cam* h_cams,
                                            float w_loss_rot, float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out) {
    return backward_batch_impl(c, BwdBatchIn{B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, h_gt_poses, h_cams, w_loss_rot, w_loss_trans, loss_cut, p, stream, h_out, false});
}
// Frames that differ in image size (include/esac_hip.h): frame b's grid in h_cams[b].reserved[0..1], its maps and its gradients
// dense at the head of their slots; p->H * p->W is the capacity in cells.
extern "C" int esac_hip_backward_batch_shapes(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                              int64_t grad_frame_stride, const int64_t* d_assign, const float* h_gt_poses, const esac_hip_frame_cam* h_cams,
                                              float w_loss_rot, float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* h_out) {
    return backward_batch_impl(c, BwdBatchIn{B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, h_gt_poses, h_cams, w_loss_rot, w_loss_trans, loss_cut, p, stream, h_out, true});
}

// The asynchronous batch (include/esac_hip.h): ground truth, records and per-frame outcomes stay on the device, the host enqueues
// and returns.  Nothing in here or in begin_bwd_batch waits for the stream, and nothing is run twice: every frame owns the worst-case
// min(N, 1000) slots, so no selection can overflow, and the frames go in chunks of consecutive frames sized by that worst case, one
// launch set after the other on the stream (which serialises their use of the workspace).  A workspace that has to grow is grown
// before the first launch (ensure_ws / ensure_bws: one device synchronisation, on the first call of a shape only).
static int backward_batch_dev_impl(esac_hip_ctx* c, const BwdBatchIn& in) {
    BwdBatchStart st;
    int rc = begin_bwd_batch(c, in, BATCH_TRAIN_ASYNC, &st);
    if (rc) return rc;
    // the chunking is known before anything is launched: cap is the worst case, so the first chunk is the largest
    const int B = in.B, cap = st.worst;
    if ((rc = check_async_budget(c->train.budget, cap, st.slot_bytes))) return rc;
    const int chunk = chunk_frames(c->train.budget, cap, st.slot_bytes, B);
    if (!c->stage.d_gt_dev) {
        HIP_OK(hipMalloc((void**)&c->stage.d_gt_dev, (size_t)ESAC_MAX_BATCH * ESAC_GT_DOUBLES * sizeof(double)));
        HIP_OK(hipMalloc((void**)&c->stage.d_frame_status, (size_t)ESAC_MAX_BATCH * sizeof(int)));
    }
    if ((rc = ensure_ws(c, st.N, st.P, chunk))) return rc;  // the workspaces of the largest chunk
    if ((rc = ensure_bws(c, st.N, st.P, cap, chunk))) return rc;
    launch_bwd_gt_prepare(in.gt_poses, B, c->stage.d_gt_dev, c->stage.d_frame_status, st.s);
    if ((rc = check_launch("k_bwd_gt_prepare"))) return rc;
    st.call.gt_frames = c->stage.d_gt_dev; st.call.frame_status = c->stage.d_frame_status; st.call.rec_dev = in.out;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        if ((rc = chunk_args(c, in, st.plan, b0, nb, &st.a))) return rc;
        if ((rc = enqueue_bwd_sampling(c, st.a, st.s, true))) return rc;
        fill_bwd(c, st.a, st.call, b0, nb, cap, false);  // (the slot workspace was sized for the largest chunk above)
        if ((rc = enqueue_bwd_chain(c, st.a, st.s, nullptr))) return rc;  // k_bwd_loss writes frame b's record into d_out[b*4..]
    }
    c->last.dev_batch = B;
    return 0;
}
extern "C" int esac_hip_backward_batch_dev(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                           int64_t grad_frame_stride, const int64_t* d_assign, const float* d_gt_poses, const esac_hip_frame_cam* h_cams,
                                           float w_loss_rot, float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* d_out) {
    return backward_batch_dev_impl(c, BwdBatchIn{B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, d_gt_poses, h_cams, w_loss_rot, w_loss_trans, loss_cut, p, stream, d_out, false});
}
// ... of frames that differ in image size (esac_hip_backward_batch_shapes without a host inside the call)
extern "C" int esac_hip_backward_batch_dev_shapes(esac_hip_ctx* c, int B, const float* d_sc, int64_t sc_frame_stride, float* d_out_gradients,
                                                  int64_t grad_frame_stride, const int64_t* d_assign, const float* d_gt_poses, const esac_hip_frame_cam* h_cams,
                                                  float w_loss_rot, float w_loss_trans, float loss_cut, const esac_hip_params* p, void* stream, double* d_out) {
    return backward_batch_dev_impl(c, BwdBatchIn{B, d_sc, sc_frame_stride, d_out_gradients, grad_frame_stride, d_assign, d_gt_poses, h_cams, w_loss_rot, w_loss_trans, loss_cut, p, stream, d_out, true});
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
    if (c->team.refine_tag != 0 && coop[1] == c->team.refine_tag) {  // the failure word carries the tag of the launch that failed: only the most recent one counts
        // asynchronous calls learn of a team time-out here (or from the pick of the multi-GPU exchange, whose caller then asks here):
        // the same two-strikes latch as the blocking call's, so that a GPU whose CUs are held by someone else does not cost every
        // frame the 1 ms wait
        if (c->team.was_team && c->team.checked_tag != c->team.refine_tag) {
            c->team.checked_tag = c->team.refine_tag;
            c->team.latch.timed_out();
        }
        return fail(-12, "the cooperating refinement workgroups of the most recent call could not synchronise (not all of them became resident)");
    }
    if (c->last.dev_batch > 0) {  // esac_hip_backward_batch_dev was the most recent call: its per-frame outcomes
        static thread_local int words[ESAC_MAX_BATCH];
        const int B = c->last.dev_batch;
        HIP_OK(hipMemcpy(words, c->stage.d_frame_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
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
    if (int rc = check_shard_balanced(c && d_assign && d_index_out && d_assign_out, N, E, world, rank)) return rc;
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
    if (int rc = check_eval_batch(c != nullptr, B, d_records != nullptr, d_gt_poses != nullptr, d_out != nullptr, rot_thresh_deg, trans_thresh_cm)) return rc;
    DeviceGuard guard(c->device);
    launch_eval_batch(B, d_records, d_gt_poses, d_gt_experts, (double)rot_thresh_deg, (double)trans_thresh_cm, d_out, (hipStream_t)stream);
    return check_launch("k_eval_batch");
}

// K given poses per frame against the maps (esac_verify.hip; include/esac_hip.h): one launch on the caller's stream, no workspace
// of the context's but a frame table of its own -- the hypothesis, score and result buffers of a forward or training call, and
// the table such a call in flight reads, stay as they are.
static_assert(ESAC_VERIFY_SCORE == ESAC_VERIFY_SCORE_K && ESAC_VERIFY_N == ESAC_VERIFY_N_K && ESAC_VERIFY_SSE == ESAC_VERIFY_SSE_K &&
                  ESAC_VERIFY_SIGMA2 == ESAC_VERIFY_SIGMA2_K && ESAC_VERIFY_STATUS == ESAC_VERIFY_STATUS_K && ESAC_VERIFY_A == ESAC_VERIFY_A_K &&
                  ESAC_VERIFY_C == ESAC_VERIFY_C_K && ESAC_VERIFY_DOUBLES == ESAC_VERIFY_DOUBLES_K && ESAC_VERIFY_OK == ESAC_VERIFY_OK_K &&
                  ESAC_VERIFY_FEW == ESAC_VERIFY_FEW_K && ESAC_VERIFY_PINV == ESAC_VERIFY_PINV_K && ESAC_VERIFY_BAD_POSE == ESAC_VERIFY_BAD_POSE_K &&
                  ESAC_VERIFY_BAD_EXPERT == ESAC_VERIFY_BAD_EXPERT_K && ESAC_VERIFY_POSE_RT == ESAC_VERIFY_POSE_RT_K &&
                  ESAC_VERIFY_POSE_4X4 == ESAC_VERIFY_POSE_4X4_K && ESAC_VERIFY_MAX_POSES == VERIFY_MAX_POSES,
              "verify row layout drifted between include/esac_hip.h, verify_math.hpp and verify_policy.hpp");
extern "C" int esac_hip_verify_batch(esac_hip_ctx* c, int B, int K, const float* d_sc, int64_t sc_frame_stride, const void* d_poses,
                                     int pose_format, const int32_t* d_experts, const esac_hip_params* p, const esac_hip_frame_cam* cams,
                                     int ragged, void* stream, double* d_out) {
    BatchPlan plan;
    if (int rc = plan_verify(c != nullptr, B, K, d_sc != nullptr, sc_frame_stride, d_poses != nullptr, pose_format, d_experts != nullptr, p, cams,
                             ragged != 0, d_out != nullptr, &plan)) return rc;
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    const esac_hip_params& q = plan.p;
    KArgs a{};  // (no workspace pointer is set: the kernel reads the maps, the camera and the score parameters)
    a.sc = d_sc; a.frames = B; a.sc_frame_stride = sc_frame_stride;
    a.E = q.E; a.H = q.H; a.W = q.W; a.N = K;
    a.shift_x = q.shift_x; a.shift_y = q.shift_y; a.sub = q.sub_sampling;
    a.focal = q.focal; a.ppx = q.ppx; a.ppy = q.ppy;
    a.tau = q.inlier_thresh; a.alpha = q.inlier_alpha; a.beta = q.inlier_beta; a.max_reproj = q.max_reproj;
    a.flags = q.flags;
    if (plan.stage) {
        if (int rc = stage_cams(c->verify_cams, plan, cams, B, s)) return rc;
        a.cams = c->verify_cams.d_cams;
        a.shapes = plan.shapes;
    }
    launch_verify_batch(a, VerifyArgs{d_poses, d_experts, d_out, K, pose_format}, s);
    return check_launch("k_verify_batch");
}

extern "C" int esac_hip_set_wait(esac_hip_ctx* c, int mode) {
    if (int rc = check_wait(c != nullptr, mode)) return rc;
    c->wait_mode = mode;
    return 0;
}

extern "C" int esac_hip_read(esac_hip_ctx* c, int which, void* h_dst, size_t bytes) {
    if (!c || !h_dst) return fail(-1, "esac_hip_read: null argument");
    DeviceGuard guard(c->device);
    const size_t P = (size_t)c->last.H * c->last.W;
    const void* src = nullptr;
    switch (which) {
#define ESAC_READ_SRC(id, member, elem, count, frames) case id: src = c->member; break;
        ESAC_READ_TABLE(ESAC_READ_SRC)
#undef ESAC_READ_SRC
        case ESAC_BUF_REFINE_INFO: src = c->ws.refine_info; break;
        case ESAC_BUF_BWD_PATH1: src = c->train.ws.grad1; break;
        case ESAC_BUF_BWD_PATH2: src = c->train.ws.grad2; break;
        case ESAC_BUF_BWD_MAPS: src = c->train.ws.maps; break;
    }
    // slots the slab workspace holds (>= the slots of the last call); after a batch, frame 0's slabs: its per-frame cap
    // (after a ragged training batch the slabs and slot maps of frame 0 are read in units of that frame's own cells: its slots lie there)
    const bool slot_read = which == ESAC_BUF_BWD_PATH1 || which == ESAC_BUF_BWD_PATH2 || which == ESAC_BUF_BWD_MAPS;
    const LastCall& last = c->last;
    const ReadDims dims = {(size_t)last.N, slot_read && last.slot_cells ? last.slot_cells : P, (size_t)bwd_rows(last.N), last.B, last.bwd_frames,
                           last.batch_cap > 0 ? (size_t)last.batch_cap : (size_t)c->train.slots, c->keep_errs};
    size_t want = 0;
    if (int rc = read_size(which, bytes, src != nullptr, dims, &want)) return rc;
    switch (which) {
        case ESAC_BUF_INLIER_MAP: {
            // the refinement kernel alternates between two map buffers; result[31] names the one that
            // holds the last ACCEPTED inlier set (-1: no re-fit was accepted -> all zeros)
            HIP_OK(hipDeviceSynchronize());
            double which_buf = -1;
            HIP_OK(hipMemcpy(&which_buf, c->ws.result + 31, sizeof(double), hipMemcpyDeviceToHost));
            if (which_buf < 0) {
                memset(h_dst, 0, P);
                return 0;
            }
            // (after a ragged batch the P bytes are frame 0's slot view: its map is the first h_0 * w_0 of them; last.map1 + P <= 2 P)
            HIP_OK(hipMemcpy(h_dst, c->ws.inlier_map + (which_buf > 0.5 ? c->last.map1 : 0), P, hipMemcpyDeviceToHost));
            return 0;
        }
        case ESAC_BUF_BWD_TEAM_INFO: {
            const int32_t info[4] = {c->team.last_bwd_teams ? 1 : 0, (int32_t)c->team.slot_calls, (int32_t)c->team.slot_fallbacks, (int32_t)c->team.last_nsel};
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
        case ESAC_BUF_SPEC_INFO: {
            double st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c->ws.spec_state) {
                HIP_OK(hipDeviceSynchronize());
                HIP_OK(hipMemcpy(st, c->ws.spec_state, sizeof(st), hipMemcpyDeviceToHost));
            }
            const int32_t info[4] = {(int32_t)c->spec.calls, (int32_t)st[2], c->spec.last_epoch != 0 ? 1 : 0, c->spec.last_epoch != 0 && st[0] == c->spec.last_epoch ? 1 : 0};
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
        case ESAC_BUF_REFINE_INFO: {
            HIP_OK(hipDeviceSynchronize());
            int32_t info[8];
            HIP_OK(hipMemcpy(info, c->ws.refine_info, sizeof(info), hipMemcpyDeviceToHost));
            info[6] = (int32_t)((c->team.latch.fallbacks & 0x3fffffff) | (c->team.latch.off ? 0x40000000 : 0));
            memcpy(h_dst, info, sizeof(info));
            return 0;
        }
    }
    // the table's buffers, the slabs and the maps: `want` bytes from the head of the buffer
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h_dst, src, want, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int esac_hip_write_hyps(esac_hip_ctx* c, const double* h_hyps, int N) {
    if (!c || !h_hyps || N <= 0) return fail(-1, "esac_hip_write_hyps: bad argument");
    DeviceGuard guard(c->device);
    if (int rc = ensure_ws(c, N, c->capP > 0 ? c->capP : 1)) return rc;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(c->ws.hyps, h_hyps, (size_t)N * 6 * sizeof(double), hipMemcpyHostToDevice));
    // the fp32 [R | t] rows of the streaming score are relative to each expert map's origin (device_common.hpp:
    // map_centre): they are rebuilt by the next esac_hip_score, which knows the maps
    c->rt32_stale = true;
    c->last.N = N;
    return 0;
}

extern "C" int esac_hip_set_refine_team(esac_hip_ctx* c, int members) {
    if (int rc = check_refine_team(c != nullptr, members)) return rc;
    c->team.auto_size = members == ESAC_REFINE_TEAM_AUTO && !c->team.auto_env_off;
    c->team.members = requested_team(members);
    c->team.latch.requested();  // an explicit request re-arms the forward teams and the training path's slot teams
    c->team.slot_teams = true;
    return 0;
}
extern "C" int esac_hip_set_refine_route(esac_hip_ctx* c, int on) {
    if (!c) return fail(-1, "null context");
    c->team.route = on != 0;
    return 0;
}
extern "C" int esac_hip_set_front_route(esac_hip_ctx* c, int on) {
    if (!c) return fail(-1, "null context");
    c->front.on = on != 0;
    return 0;
}
extern "C" int esac_hip_front_route_taken(esac_hip_ctx* c) {
    if (!c) return fail(-1, "null context");
    return c->front.taken ? 1 : 0;
}
extern "C" int esac_hip_read_rotations(esac_hip_ctx* c, double* h_dst, int N) {
    if (!c || !h_dst || N <= 0) return fail(-1, "esac_hip_read_rotations: bad argument");
    if (N > c->last.N || !c->ws.hyps_R) return fail(-2, "esac_hip_read_rotations: the workspace holds %d hypotheses", c->last.N);
    DeviceGuard guard(c->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h_dst, c->ws.hyps_R, (size_t)N * 9 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int esac_hip_set_debug(esac_hip_ctx* c, int flags) {
    if (!c) return fail(-1, "null context");
    c->keep_errs = (flags & ESAC_DEBUG_ERROR_IMAGE) != 0;
    c->coop_stall = (flags & ESAC_DEBUG_COOP_STALL) != 0;
    c->team.spread = (flags & ESAC_DEBUG_TEAM_SPREAD) != 0;
    c->spec.off = c->spec.env_off || (flags & ESAC_DEBUG_NO_SPECULATION) != 0;
    c->spec.second_best = (flags & ESAC_DEBUG_SPEC_SECOND_BEST) != 0;
    c->spec.lose_chain = (flags & ESAC_DEBUG_SPEC_LOSE_CHAIN) != 0;
    return 0;
}
extern "C" int esac_hip_set_timing(esac_hip_ctx* c, int enabled) {
    if (!c) return fail(-1, "null context");
    c->timing.on = enabled != 0;
    c->timing.period = enabled > 1 ? enabled : 1;
    c->timing.calls = 0;
    c->timing.ev_valid = false;
    if (c->ws.span_acc) {
        DeviceGuard guard(c->device);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemset(c->ws.span_acc, 0, 2 * sizeof(long long)));
    }
    return 0;
}
extern "C" int esac_hip_phase_ms(esac_hip_ctx* c, float out[6]) {
    if (!c || !out) return fail(-1, "esac_hip_phase_ms: null argument");
    if (!c->timing.on || !c->timing.ev_valid) return fail(-8, "esac_hip_phase_ms: timing is off or no forward has run");
    DeviceGuard guard(c->device);
    HIP_OK(hipEventSynchronize(c->timing.ev[4]));
    for (int i = 0; i < 4; i++) HIP_OK(hipEventElapsedTime(&out[i], c->timing.ev[i], c->timing.ev[i + 1]));
    HIP_OK(hipEventElapsedTime(&out[4], c->timing.ev[0], c->timing.ev[4]));
    HIP_OK(hipEventSynchronize(c->timing.ev[6]));
    HIP_OK(hipEventElapsedTime(&out[5], c->timing.ev[5], c->timing.ev[6]));
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
