// esac_eval.hip -- esac_hip_eval_batch: the result records of a forward batch and the ground truth, turned on the device into
// the numbers the test loop reports (test_esac.py:209-247): rotation / translation error, the 5 cm / 5 deg flag, "expert chosen ==
// true expert", quaternion + translation of the inverted pose.  One lane per frame; the arithmetic is eval_math.hpp (the text the
// host test compiles).  A few hundred dependent fp64 operations per frame and 128 + 64 + 128 bytes of traffic: the kernel is a
// latency chain of ~10 us whatever B is, enqueued behind the batch that writes the records.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "esac_kernels.hpp"
#include "eval_math.hpp"

namespace esac {

__global__ __launch_bounds__(64) void k_eval_batch(int B, const double* __restrict__ records, const float* __restrict__ gt_poses,
                                                   const int64_t* __restrict__ gt_experts, double rot_thresh_deg,
                                                   double trans_thresh_cm, double* __restrict__ out) {
    const int b = (int)(blockIdx.x * 64u + threadIdx.x);
    if (b >= B) return;
    double row[ESAC_EVAL_DOUBLES_K];
    eval_frame(records + (size_t)b * ESAC_EVAL_REC_DOUBLES, gt_poses + (size_t)b * 16, gt_experts != nullptr,
               gt_experts != nullptr ? (long long)gt_experts[b] : -1, rot_thresh_deg, trans_thresh_cm, row);
    double* dst = out + (size_t)b * ESAC_EVAL_DOUBLES_K;
#pragma unroll
    for (int k = 0; k < ESAC_EVAL_DOUBLES_K; k++) dst[k] = row[k];
}

void launch_eval_batch(int B, const double* records, const float* gt_poses, const int64_t* gt_experts, double rot_thresh_deg,
                       double trans_thresh_cm, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_batch, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, B, records, gt_poses, gt_experts, rot_thresh_deg,
                       trans_thresh_cm, out);
}

}  // namespace esac
