// call_policy_probe.cpp -- TEST-ONLY: the C ABI host's decisions (esac_amd/csrc/call_policy.hpp, plain C++) behind one C entry
// point, so that the CPU suite can hold them against a recording of what esac_capi.hip answered before the header existed
// (tests/test_call_policy_host.py).  A row is a kind, a vector of doubles in and a status, a message and a vector of doubles out.
// Built by tests/native/build.py (build_call_policy_probe); with -DCALL_POLICY_PROBE_MAIN the same source is a stand-alone program
// that reads rows from standard input and compares (the sanitizer build).  Not part of the product library.
#include <stdlib.h>
#include <string.h>

#include "../../esac_amd/csrc/call_policy.hpp"
using namespace esac;

// a[0..16]: E, H, W, N, shift_x, shift_y, focal, subSampling, flags, max_tries, max_ref_steps, rescore_margin, alpha, beta, tau,
// hyp_offset, "has a hypothesis index"
static esac_hip_params mk(const double* a) {
    esac_hip_params p;
    memset(&p, 0, sizeof(p));
    p.E = (int)a[0]; p.H = (int)a[1]; p.W = (int)a[2]; p.N = (int)a[3]; p.shift_x = (int)a[4]; p.shift_y = (int)a[5]; p.focal = (float)a[6];
    p.sub_sampling = (int)a[7]; p.flags = (int)a[8]; p.max_tries = (int)a[9]; p.max_ref_steps = (int)a[10]; p.rescore_margin = (float)a[11];
    p.inlier_alpha = (float)a[12]; p.inlier_beta = (float)a[13]; p.inlier_thresh = (float)a[14]; p.hyp_offset = (int)a[15];
    p.d_hyp_index = a[16] != 0 ? (const int32_t*)64 : nullptr;
    return p;
}

extern "C" const char* row_error() { return g_err; }
extern "C" int run_row(const char* kind, const double* a, int na, double* out, int* n_out) {
    g_err[0] = 0;
    *n_out = 0;
    const double* b = a + 17;  // what follows the parameters, in the kinds that take them
    if (!strcmp(kind, "args")) {  // ctx, tensors, params given, B, cam_frame, training, offset of d_sc, hypotheses held, n_sub
        const esac_hip_params p = mk(a);
        if (int rc = check_args(b[0] != 0, b[1] != 0, b[2] != 0 ? &p : nullptr, (int)b[3], (int)b[4], b[5] != 0)) return rc;
        const bool tiled = want_tiled(&p, (const void*)(256 + (long)b[6]), (int)b[3], (int)b[8]);
        const CallScalars v = call_scalars(&p, (long long)b[7]);
        const double vals[10] = {(double)tiled, (double)want_pack(&p, (int)b[3]), (double)v.max_tries, (double)v.max_ref_steps, (double)v.samp_cap,
                                 (double)v.flags, (double)v.margin, (double)auto_exact_flags(v.flags, (int)b[3], p.E, p.N, p.H, p.W),
                                 tiled ? b[8] : 0.0, tiled ? (double)tiled_chunks(p.N, p.E) : 0.0};
        memcpy(out, vals, sizeof(vals));
        *n_out = 10;
        return 0;
    }
    if (!strcmp(kind, "batch")) {  // ctx, params given, tensors, asynchronous, out, B, coordinate stride, gradient stride
        const esac_hip_params p = mk(a);
        return check_batch_call("esac_hip_backward_batch", b[0] != 0, b[1] != 0 ? &p : nullptr, (int)b[5], b[2] != 0, b[3] != 0, b[4] != 0,
                                (int64_t)b[6], (int64_t)b[7]);
    }
    if (!strcmp(kind, "pose_arm")) return check_pose_arm("esac_hip_backward_batch_dev", a[0] != 0, (int)a[1], (int)a[2]);
    if (!strcmp(kind, "backward")) {  // gradient + ground truth, ctx, params given, coordinates, armed frames (< 0: armed with none)
        const esac_hip_params p = mk(a);
        if (int rc = check_backward_entry(b[0] != 0, b[1] != 0, b[2] != 0 ? &p : nullptr)) return rc;
        if (int rc = check_args(true, b[3] != 0, b[2] != 0 ? &p : nullptr, 1, -1, true)) return rc;
        if (int rc = check_backward_call(&p)) return rc;
        return check_pose_arm("esac_hip_backward", b[4] != 0, b[4] > 0 ? (int)b[4] : 0, 1);
    }
    if (!strcmp(kind, "eval")) return check_eval_batch(a[0] != 0, (int)a[1], a[2] != 0, a[3] != 0, a[4] != 0, (float)a[5], (float)a[6]);
    if (!strcmp(kind, "shard")) return check_shard_balanced(a[0] != 0, (int)a[1], (int)a[2], (int)a[3], (int)a[4]);
    if (!strcmp(kind, "set_team")) {  // ctx, members: on a latched context with two strikes
        TeamLatch latch;
        latch.timed_out();
        latch.timed_out();
        if (int rc = check_refine_team(a[0] != 0, (int)a[1])) return rc;
        latch.requested();
        out[0] = requested_team((int)a[1]); out[1] = latch.off; out[2] = latch.strikes;
        *n_out = 3;
        return 0;
    }
    if (!strcmp(kind, "set_wait")) return check_wait(a[0] != 0, (int)a[1]);
    *n_out = 1;
    if (!strcmp(kind, "slot_bytes")) { out[0] = (double)bwd_slot_bytes((int)a[0], (long long)a[1]); return 0; }  // P, corr_entries(P)
    if (!strcmp(kind, "grown_cap")) { out[0] = grown_cap((int)a[0], (int)a[1]); return 0; }
    if (!strcmp(kind, "chunk")) {  // budget, cap, P, left, corr_entries(P)
        out[0] = chunk_frames((long long)a[0], (int)a[1], bwd_slot_bytes((int)a[2], (long long)a[4]), (int)a[3]);
        return 0;
    }
    if (!strcmp(kind, "start_cap")) { out[0] = start_cap(a[0] != 0, (int)a[1], (int)a[2]); return 0; }
    *n_out = 0;
    if (!strcmp(kind, "async")) {  // budget, B, corr_entries(P), bwd_rows(N): the asynchronous batch up to its first HIP call
        const esac_hip_params p = mk(a);
        if (int rc = check_batch_call("esac_hip_backward_batch", true, &p, (int)b[1], true, true, true, 0, 1LL << 40)) return rc;
        return check_async_budget((long long)b[0], (int)b[3], bwd_slot_bytes(p.H * p.W, (long long)b[2]));
    }
    if (!strcmp(kind, "latch")) {  // pairs (op, value); 1: a time-out, 2: a forward call with flags `value`, 3: `value` members are
        TeamLatch latch;           // requested, 4: a team held, 5: `value` forward calls.  Five values out per pair.
        int members = ESAC_REFINE_TEAM_DEFAULT, n = 0;
        for (int i = 0; i < na; i += 2) {
            const int op = (int)a[i], v = (int)a[i + 1];
            int team = -7, solo = -7;
            if (op == 1) latch.timed_out();
            if (op == 3) {
                if (int rc = check_refine_team(true, v)) return rc;
                members = requested_team(v);
                latch.requested();
            }
            if (op == 4) latch.strikes = 0;
            for (int r = 0; r < (op == 2 ? 1 : op == 5 ? v : 0); r++) {
                latch.forward_call();
                team = members;
                solo = 0;
                forward_team(latch, op == 2 ? v : 0, &team, &solo);
            }
            const double vals[5] = {(double)team, (double)solo, (double)latch.off, (double)latch.strikes, (double)latch.fallbacks};
            memcpy(out + n, vals, sizeof(vals));
            n += 5;
        }
        *n_out = n;
        return 0;
    }
    if (!strcmp(kind, "read")) {  // id, bytes, N, H, W, forward frames, training frames, buffers exist, error image kept, a batch's
        size_t want = 0;          // slots per frame, slots of the workspace, bwd_rows(N)
        const ReadDims d = {(size_t)a[2], (size_t)a[3] * (size_t)a[4], (size_t)a[11], (int)a[5], (int)a[6], a[9] > 0 ? (size_t)a[9] : (size_t)a[10], a[8] != 0};
        return read_size((int)a[0], (size_t)a[1], a[7] != 0, d, &want);
    }
    return fail(-999, "unknown row kind %s", kind);
}

#ifdef CALL_POLICY_PROBE_MAIN
// rows on standard input: kind|status|inputs|values|message, numbers separated by blanks; exit status 1 when a row differs
static int numbers(char* s, double* v) {
    int n = 0;
    for (char* t = strtok(s, " "); t; t = strtok(nullptr, " ")) v[n++] = strtod(t, nullptr);
    return n;
}
int main() {
    static char line[1 << 16];
    static double in[4096], want[4096], got[4096];
    int rows = 0, bad = 0;
    while (fgets(line, sizeof(line), stdin)) {
        line[strcspn(line, "\n")] = 0;
        char* f[5] = {line, nullptr, nullptr, nullptr, nullptr};
        for (int k = 1; k < 5; k++) {
            f[k] = strchr(f[k - 1], '|');
            if (!f[k]) return 2;
            *f[k]++ = 0;
        }
        const int status = atoi(f[1]), na = numbers(f[2], in), nw = numbers(f[3], want);
        int ng = 0;
        const int rc = run_row(f[0], in, na, got, &ng);
        const bool same = rc == status && !strcmp(g_err, f[4]) && ng == nw && !memcmp(got, want, (size_t)nw * sizeof(double));
        if (!same) printf("row %d (%s): status %d, message '%s'\n", rows, f[0], rc, g_err);
        bad += !same;
        rows++;
    }
    printf("%d rows, %d differ\n", rows, bad);
    return bad != 0;
}
#endif
