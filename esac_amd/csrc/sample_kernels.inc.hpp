// sample_kernels.inc.hpp -- the two fp64 sampling kernels of esac_kernels.hip, as text that file includes once per triangle
// alignment (pose_math.hpp: AlignTriad, AlignHorn).  Included, not instantiated from one template body: the kernels of the default
// route are then compiled from exactly the tokens they always had and keep their code, registers and names, and the
// ESAC_FLAG_STRICT_REFERENCE kernels are the same loops around the reference's own alignment.
// The including file defines ESAC_K_SAMPLE_FIRST, ESAC_K_SAMPLE (the kernels' names), ESAC_SAMPLE_ALIGN and
// ESAC_SAMPLE_FIRST_ATTR (attributes of the first-pass kernel); no include guard on purpose.
// ESAC_SAMPLE_ROUTE (0 / 1), k_sample only: 1 = the headline call's modes as constants (esac_front_route.hip; what makes a call
// eligible: front_route_policy.hpp) -- one frame, one expert, no table, no packed maps, no index list, from try 0, no hand-over,
// no speculation.  ESAC_SAMPLE_RT32 (0 / 1): k_sample stores the fp32 rows of the streaming score (1 everywhere but on the front
// route).  The loop, the draws and the arithmetic are these tokens either way.

// Throughput shape, first phase (see sample_plan.hpp: FIRST_PHASE_TRIES)
template <int TRIES>
__global__ __launch_bounds__(64) ESAC_SAMPLE_FIRST_ATTR void ESAC_K_SAMPLE_FIRST(KArgs a) {
    constexpr int HPW = 64 / TRIES;  // hypotheses per wavefront
    frame_view(a);
    const int lane = threadIdx.x, grp = lane / TRIES, t = a.first_try + (lane & (TRIES - 1));
    const int h = blockIdx.x * HPW + grp;
    const int hc = h < a.N ? h : a.N - 1;
    const bool mine_pending = h < a.N && (a.first_try == 0 || a.tries[hc] == SAMPLE_PENDING);
    if (!__any(mine_pending)) return;  // all hypotheses of this wavefront are done
    const bool active = mine_pending && t < a.max_tries;
    if (a.first_try == 0 && h < a.N && (lane & (TRIES - 1)) == 0) flag_bad_assignment(a, h);
    const int e = expert_of(a, hc);
    const int P = a.H * a.W;
    const float* __restrict__ map = a.sc + (size_t)e * 3 * P;
    const Philox rng(a.seed, a.call);
    const Cam cam = make_cam(a);
    int cx[4] = {0, 0, 0, 0}, cy[4] = {0, 0, 0, 0};
    double rvec[3] = {0, 0, 0}, T[3] = {0, 0, 0};
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    bool accepted = false;
    if (active) {
        V3 Pt[4];
        float Pf[4][3];
        double mu[4], mv[4], Rp[9], Tp[3];
        gather_sample(a, map, P, rng, (uint32_t)global_hyp(a, hc), (uint32_t)t, cx, cy, Pt, Pf, mu, mv);
        double reproj2 = 0;
        if (p3p_4pt<ESAC_SAMPLE_ALIGN>(Pt, mu, mv, cam, Rp, Tp, &reproj2) && (t == a.max_tries - 1 || !cannot_pass(reproj2, (double)a.tau)))
            accepted = accept_sample(Rp, Tp, Pf, mu, mv, cam, (double)a.tau, rvec, T, R);
    }
    const unsigned long long m = __ballot(accepted);
    const unsigned mine = (unsigned)(m >> (TRIES * grp)) & (TRIES == 32 ? 0xffffffffu : 0xffffu);
    if (mine_pending) {
        if (mine) {
            const int first = __ffs((int)mine) - 1;
            if ((lane & (TRIES - 1)) == first) store_hypothesis(a, h, map, rvec, T, R, cx, cy, a.first_try + first);
        } else if (a.max_tries <= a.first_try + TRIES) {
            if (t == a.max_tries - 1) store_hypothesis(a, h, map, rvec, T, R, cx, cy, -1);  // budget exhausted: last state remains
        } else if ((lane & (TRIES - 1)) == 0) {
            a.tries[h] = SAMPLE_PENDING;  // k_pending_list gathers what the last pass leaves pending
        }
    }
}

// SAMPLE_B lanes per hypothesis, LPT lanes per try in the first rounds (see esac_kernels.hip)
template <int SAMPLE_B, int LPT>
__global__ __launch_bounds__(SAMPLE_B) void ESAC_K_SAMPLE(KArgs a) {
    static_assert(LPT == 1 || LPT == 2 || LPT == 4, "lanes per try");
    constexpr int CPLN = 4 / LPT;  // candidates per lane in the shared rounds
    __shared__ int s_first[2][SAMPLE_B / 64];
    __shared__ double s_pose[CPLN > 1 ? SAMPLE_B * 12 : 1];  // [value][lane]: the best candidate's pose so far, per lane
#if ESAC_SAMPLE_ROUTE
    front_route_modes(a);
#else
    frame_view(a);
#endif
    const int h = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = expert_of(a, h);
    const int P = a.H * a.W;
    const float* __restrict__ map = a.sc + (size_t)e * 3 * P;
    const Philox rng(a.seed, a.call);
    const Cam cam = make_cam(a);
    const uint32_t gh = (uint32_t)global_hyp(a, h);
    const double tau = (double)a.tau;
    if (a.first_try > 0 && a.tries[h] != SAMPLE_PENDING) return;  // phase 2 of the throughput shape: done in phase 1
    if (a.first_try == 0 && threadIdx.x == 0) flag_bad_assignment(a, h);
#if !ESAC_SAMPLE_ROUTE
    if (a.handover != 0x7fffffff && threadIdx.x == 0 && expert_stats_on(a)) atomicAdd(expert_stats(a, e), 1);  // (see expert_stats)
#endif

    int parity = 0;
    for (int base = a.first_try, TRIES = 0; base < a.max_tries; base += TRIES, parity ^= 1) {
        const bool quad = LPT > 1 && base < SAMPLE_B;  // workgroup-uniform: the first SAMPLE_B tries go LPT lanes a try
        TRIES = quad ? SAMPLE_B / LPT : SAMPLE_B;
        const int t = base + (quad ? (int)threadIdx.x / LPT : (int)threadIdx.x);
        const int sub = threadIdx.x & (LPT - 1);  // shared rounds only: this lane evaluates roots sub, sub + LPT, ...
        bool holder = !quad;                      // the lane that carries the try's final state (pose or zero pose)
        const bool active = t < a.max_tries;
        int cx[4] = {0, 0, 0, 0}, cy[4] = {0, 0, 0, 0};
        double rvec[3] = {0, 0, 0}, T[3] = {0, 0, 0};
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        bool accepted = false;
        if (active) {
            V3 Pt[4];
            float Pf[4][3];
            double mu[4], mv[4];
            gather_sample(a, map, P, rng, gh, (uint32_t)t, cx, cy, Pt, Pf, mu, mv);
            double Rp[9], Tp[3], reproj2 = 0;
            bool solved;
            if (LPT > 1 && quad) {
                P3PSetup S;
                const bool ok = p3p_setup(Pt, mu, mv, cam, S);
                // Step k: the lanes evaluate roots k * LPT .. k * LPT + LPT - 1 (this lane: root k * LPT + sub), exchange
                // (valid, error) and continue the reference's sequential scan over the candidates (same `>` rule, same NaN
                // behaviour) -- every lane carries the scan's state, and the lane whose candidate has just become the best
                // keeps its pose: after the last step the winner's lane holds the winner's pose.
                const int lane0 = lane & ~(LPT - 1);
                bool have = false;
                double min_reproj = 0;
                int win = -1;
#pragma nounroll
                for (int k = 0; k < CPLN; k++) {
                    const int root = k * LPT + sub;
                    const double x = root == 0 ? S.x[0] : root == 1 ? S.x[1] : root == 2 ? S.x[2] : S.x[3];
                    double R1[9], T1[3], rp = 0;
                    const bool vk = ok && root < S.n && p3p_candidate<ESAC_SAMPLE_ALIGN>(S, x, Pt, mu[3], mv[3], cam, R1, T1, rp);
#pragma unroll
                    for (int j = 0; j < LPT; j++) {
                        const bool vi = __shfl((int)vk, lane0 + j) != 0;
                        const double ri = __shfl(rp, lane0 + j);
                        if (vi && (!have || min_reproj > ri)) {
                            have = true;
                            min_reproj = ri;
                            win = k * LPT + j;
                        }
                    }
                    if (win == root) {  // (more than one step: the pose waits in LDS, not in 24 registers across the next solve)
#pragma unroll
                        for (int q = 0; q < 9; q++) {
                            if (CPLN > 1) s_pose[q * SAMPLE_B + threadIdx.x] = R1[q];
                            else Rp[q] = R1[q];
                        }
#pragma unroll
                        for (int q = 0; q < 3; q++) {
                            if (CPLN > 1) s_pose[(9 + q) * SAMPLE_B + threadIdx.x] = T1[q];
                            else Tp[q] = T1[q];
                        }
                    }
                }
                solved = have && (win & (LPT - 1)) == sub;
                if (CPLN > 1 && solved) {
#pragma unroll
                    for (int q = 0; q < 9; q++) Rp[q] = s_pose[q * SAMPLE_B + threadIdx.x];
#pragma unroll
                    for (int q = 0; q < 3; q++) Tp[q] = s_pose[(9 + q) * SAMPLE_B + threadIdx.x];
                }
                holder = solved || (!have && sub == 0);
                reproj2 = min_reproj;
            } else {
                solved = p3p_4pt<ESAC_SAMPLE_ALIGN>(Pt, mu, mv, cam, Rp, Tp, &reproj2);
            }
            if (solved && (t == a.max_tries - 1 || !cannot_pass(reproj2, tau)))
                accepted = accept_sample(Rp, Tp, Pf, mu, mv, cam, tau, rvec, T, R);
            // a failed solve leaves the zero pose (safeSolvePnP, esac_util.h:107-111)
        }
        // lowest accepted try of the round = the try the reference's sequential loop stops at
        const unsigned long long m = __ballot(accepted);
        if (lane == 0) {
            const int first_lane = __ffsll((long long)m) - 1;
            s_first[parity][wave] = m ? base + (quad ? wave * (64 / LPT) + first_lane / LPT : wave * 64 + first_lane) : 0x7fffffff;
        }
        __syncthreads();
        int first = s_first[parity][0];
#pragma unroll
        for (int w = 1; w < SAMPLE_B / 64; w++) first = min(first, s_first[parity][w]);
        const bool last_round = base + TRIES >= a.max_tries;
        int writer = -1, tries_val = -1;
        if (first != 0x7fffffff) {
            writer = first;
            tries_val = first;
        } else if (last_round) {
            writer = a.max_tries - 1;  // budget exhausted: state of the last try remains
        }
        if (writer >= 0) {
            if (t == writer && holder) store_hypothesis_rows<ESAC_SAMPLE_RT32>(a, h, map, rvec, T, R, cx, cy, tries_val);
            if (a.spec_flag && threadIdx.x == 0) a.spec_flag[h] = 0;  // settled by this pass
            return;
        }
#if !ESAC_SAMPLE_ROUTE
        if (base + TRIES >= a.handover) {  // a straggler (wrong expert): the spread, screened search takes over from here
            if (threadIdx.x < 64) mark_pending(a, h, e, threadIdx.x == 0);
            return;
        }
#endif
    }
}
