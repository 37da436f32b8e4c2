"""`import esac` -- drop-in module name of the reference extension (code/esac/setup.py:28-38,
esac.cpp:513-516).  The MI355X-native implementation lives in esac_amd/ (HIP kernels + C ABI);
this shim only re-exports the reference's two entry points (and their batched companions) plus the RNG/diagnostic helpers."""
from esac_amd.api import (backward, backward_batch, backward_batch_async, forward, forward_batch, get_rng_state, last_result, set_exact_sampling,  # noqa: F401
                          set_exact_scores, set_limits, set_seed, set_strict_reference, set_strict_training)
from esac_amd.api import eval_batch, forward_batch_async  # noqa: F401  (the batched test loop: device records, on-device pose errors)
from esac_amd.api import verify_batch  # noqa: F401  (score, inliers and covariance of GIVEN poses: a ground truth, the previous frame's, a prediction)
from esac_amd.api import set_pose_records  # noqa: F401  (the next training call hands out its winner's refined pose as a forward record)
from esac_amd.api import pack_frames, unpack_frames  # noqa: F401  (frames that differ in image size: forward_batch(shapes=...) / forward_batch_async(shapes=...))
from esac_amd.api import backward_batch_shapes, backward_batch_shapes_async  # noqa: F401  (... and the training calls over such frames)
