// sample_plan.hpp -- what the sampler launches for a call, decided ONCE.  Plain C++ (no HIP header): the launchers of
// esac_kernels.hip enqueue a plan (launch_sample: all of it on one stream; launch_sample_split: the first pass on the launch
// stream, the tail handed back for a stream of the context's own), the CPU suite reads it through
// tests/native/sample_plan_probe.cpp.
#pragma once

namespace esac {

constexpr int ESAC_FLAG_EXACT_SAMPLING_K = 16;     // = ESAC_FLAG_EXACT_SAMPLING (include/esac_hip.h; checked in esac_capi.hip)
constexpr int ESAC_FLAG_STRICT_REFERENCE_K = 256;  // the reference's rule wherever the default knowingly differs (include/esac_hip.h)

constexpr int ESAC_LATENCY_MAX = 1024;  // up to this many hypotheses in flight: a workgroup per hypothesis (the latency shapes)
constexpr int ESAC_HANDOVER = 32;  // (64: k_sample<128> 41 us + screened search 29 us at config 3; 32: 30 + 31 us)
constexpr int FIRST_PHASE_TRIES = 32;  // tries per hypothesis before the screened chain takes over
constexpr int ESAC_FIRST_WIDE_MAX = 8192;  // up to this many hypotheses: one pass, 32 lanes per hypothesis (else two passes of 16)
constexpr int ESAC_CHAIN_WAVES = 8192;  // wavefronts of the screened search that work whatever the number of pending hypotheses is
// wavefronts of the screened chain: every one of them works whatever the number of pending hypotheses is (they take the
// 64-try rounds of the hypotheses on the list in order), so the launch is sized for the chip -- 2048 wavefronts are
// resident at two per SIMD -- with some slack for the tail; when (nearly) every hypothesis is pending, as in the
// 50-expert workloads, eight per hypothesis measured best (A/B on one box, config 5a: 4 / 8 / 32 per hypothesis ->
// 2.00 / 1.95 / 2.18 ms)
constexpr int ESAC_CHAIN_PER_HYP = 8;
// (every pending hypothesis needs at least ONE wavefront: wavefront L serves list entry L % count, so a launch smaller
// than the list would leave its tail unscreened -- beyond this many hypotheses the launch grows with them)
constexpr int ESAC_CHAIN_WAVE_CAP = 131072;

enum SampleFirst {
    SAMPLE_FIRST_NONE,  // no first pass: the screened chain takes every hypothesis from try 0
    SAMPLE_256x2,       // k_sample<256,2>: four wavefronts per hypothesis, two lanes per try
    SAMPLE_128x4,       // k_sample<128,4>: two wavefronts per hypothesis, four lanes per try
    SAMPLE_64x2,        // k_sample<64,2>: one wavefront per hypothesis, two lanes per try
    SAMPLE_128x1,       // k_sample<128,1>: two wavefronts per hypothesis, one try per lane, the whole budget
    SAMPLE_FIRST32,     // k_sample_first<32>: two hypotheses per wavefront, 32 tries each
    SAMPLE_FIRST16      // k_sample_first<16>: four hypotheses per wavefront, 16 tries each per pass
};
enum SampleTail {
    SAMPLE_TAIL_NONE,
    SAMPLE_TAIL_EXACT,  // k_sample<64,1>: every remaining try solved in full
    SAMPLE_TAIL_CHAIN   // k_sample_prescreen .. k_sample_screened<true>
};

struct SamplePlan {
    bool pack;           // k_pack_cells in front of everything
    bool strict;         // the kernels with the reference's alignment (k_sample_strict, k_sample_first_strict)
    SampleFirst first;   // the first pass: `passes` launches of grid (grid_x, frames) x block; pass k starts at try
    int grid_x, block;   // first_try + k * pass_tries
    int passes, pass_tries;
    int handover;        // KArgs::handover of the first pass and the tail
    SampleTail tail;
    bool pending_list;   // k_pending_list between the first pass and the tail (behind the first pass, on its stream)
    int tail_first_try;  // KArgs::first_try of k_pending_list and the tail
    int chain_waves;     // wavefronts of the screened chain
    // speculative forward: the call has a FIRST PASS which settles most hypotheses and a straggler chain behind it -- several
    // experts, a single frame, the screened route, at most ESAC_FIRST_WIDE_MAX hypotheses (beyond that the chain takes every
    // hypothesis from try 0: nothing is settled early)
    bool splittable;
};

inline SamplePlan sample_plan(int N, int frames, int E, int max_tries, int flags, int first_try, bool packed) {
    const long long total = (long long)N * frames;
    SamplePlan p{};
    p.pack = packed;
    // entries of the "maybe" list, hypotheses of the pending list (+ the per-expert counters behind them, see expert_stats)
    // are zero between calls: the last kernel of the screened chain clears them (k_sample_screened<true>).  A fill in front
    // of every sampling launch cost the headline call, which never appends to them, 5 us (0.2058 -> 0.2010 ms).
    p.handover = 0x7fffffff;
    // Few hypotheses in flight: latency.  A workgroup per hypothesis (the candidates of a try on two or four lanes at first)
    // settles a hypothesis of the right expert within its first round; with several experts the stragglers are handed to
    // the spread, screened search after `handover` tries (every wavefront of that launch works, rounds handed out in order).  Beyond ~10^3
    // hypotheses (several experts) a workgroup per hypothesis no longer fits the chip in one wave of workgroups: the
    // first 32 tries run four hypotheses per wavefront and the screened chain finishes the rest.
    // ESAC_FLAG_EXACT_SAMPLING: no screen anywhere -- every try is solved and decided by the fp64 route (k_sample walks a
    // straggler's whole budget itself, one try per lane; the throughput shape finishes with k_sample<64> instead of the
    // screened chain)
    // ESAC_FLAG_STRICT_REFERENCE (implies the exact route): the same launches, the kernels with the reference's alignment
    p.strict = (flags & ESAC_FLAG_STRICT_REFERENCE_K) != 0;
    const bool exact = p.strict || (flags & ESAC_FLAG_EXACT_SAMPLING_K) != 0;
    const bool handover = E > 1 && max_tries > 1024 && !exact;
    p.splittable = handover && frames == 1 && N <= ESAC_FIRST_WIDE_MAX && first_try == 0;
    const long long w8 = (E == 1 ? 1LL : (long long)ESAC_CHAIN_PER_HYP) * total;
    const long long wcap = total > ESAC_CHAIN_WAVE_CAP ? total : ESAC_CHAIN_WAVE_CAP;
    p.chain_waves = (int)(w8 < ESAC_CHAIN_WAVES ? ESAC_CHAIN_WAVES : (w8 > wcap ? wcap : w8));
    p.grid_x = N;
    p.passes = 1;
    p.tail_first_try = first_try;
    if (total <= (handover ? ESAC_LATENCY_MAX : 1024)) {
        // up to 256 hypotheses: four wavefronts each, two lanes per try (128 tries per round, one workgroup per CU at this
        // kernel's ~445 registers: the chip is full).  Beyond that the workgroups queue up behind each other (1024
        // hypotheses: four ~12 us rounds back to back, 51 us measured): two wavefronts per hypothesis, four lanes per try
        // (32 tries per round -- 93 % of the hypotheses of a usable map are settled in it) put two hypotheses on a CU at a
        // time.
        // 513 .. 1024 hypotheses that hand their stragglers over (round 6): ONE wavefront per hypothesis, two lanes per try -- the
        // same 32 tries in one round, a chain of two candidates instead of one, and all 1024 wavefronts resident at once instead of
        // 2048 in two waves of workgroups: 29.9 -> 25.4 us at config 3 (four lanes per try at one wavefront, two rounds of 16
        // tries: 29.9 again).  Without a hand-over (one expert, ESAC_FLAG_EXACT_SAMPLING) a straggler walks its whole budget in this
        // kernel, one try per lane: two wavefronts per hypothesis halve that tail (config 3 on the guaranteed routes: 0.56 ms
        // against 0.89 with one)
        p.first = total <= 256 ? SAMPLE_256x2 : (total <= 512 || !handover) ? SAMPLE_128x4 : SAMPLE_64x2;
        p.block = p.first == SAMPLE_256x2 ? 256 : p.first == SAMPLE_128x4 ? 128 : 64;
        if (handover) {
            p.handover = p.tail_first_try = ESAC_HANDOVER;
            p.tail = SAMPLE_TAIL_CHAIN;
        }
        return p;
    }
    if (total <= 4096 && !handover) {
        p.first = SAMPLE_128x1;
        p.block = 128;
        return p;
    }
    // throughput: passes of 16 tries with four hypotheses per wavefront, then the unaccepted rest by the screened chain
    p.block = 64;
    if (total <= ESAC_FIRST_WIDE_MAX) {
        p.first = SAMPLE_FIRST32;
        p.grid_x = (N + 1) / 2;
        p.pass_tries = 32;
    } else if (E > 1 && !exact) {
        // tens of thousands of hypotheses over many experts (config 5: 16384 over 50, Dirichlet gating): nearly all of them
        // sit on wrong experts, where 32 tries in full fp64 are 32 solves for nothing -- the screened chain takes them
        // from try 0 (a hypothesis of the right expert costs it one screened round and a handful of fp64 decisions)
        p.first = SAMPLE_FIRST_NONE;
        p.passes = 0;
    } else {
        p.first = SAMPLE_FIRST16;
        p.grid_x = (N + 3) / 4;
        p.pass_tries = 16;
        for (p.passes = 0; p.passes < FIRST_PHASE_TRIES / 16 && first_try + 16 * p.passes < max_tries;) p.passes++;
    }
    p.tail_first_try = first_try + p.passes * p.pass_tries;
    if (p.tail_first_try < max_tries) {
        p.tail = exact ? SAMPLE_TAIL_EXACT : SAMPLE_TAIL_CHAIN;
        // (the list stays in hypothesis order: expert-major and dealt to the XCDs, the full-resolution workload's
        // gathers hit L2 at 0.59 instead of 0.07 and fetch 4.8 GB instead of 11.1 GB per call -- and the kernel takes
        // the same 1.7 ms: it does not wait for them.  profiles/r04_cfg5b_pending_order.txt, LAB_NOTES.md)
        p.pending_list = !exact;
    }
    return p;
}

}  // namespace esac
