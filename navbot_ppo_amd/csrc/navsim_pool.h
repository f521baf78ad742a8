// What navsim_pool.hip (the sector-LiDAR twins, navsim_set_scan_pool) exports to navsim.hip: the host stubs of its kernels.
// navsim.hip casts a stub to its own pointer type for that kernel's signature -- both translation units compile the same text of
// navsim.hip, so the argument structs have one layout -- and launches it like a kernel of its own.
#pragma once

namespace navsim_pool {

enum Kernel {
    kStep,           // step_pool_mov_kernel<BOXES>            (StepKArgs)
    kSteps,          // steps_pool_mov_kernel<BOXES>           (SeqKArgs)
    kRollout,        // rollout_pool_mov_kernel<BOXES>         (Params, RolloutArgs)
    kRolloutHist,    // rollout_hist_pool_mov_kernel<BOXES>    (Params, RolloutArgs)
    kEvaluate,       // evaluate_pool_mov_kernel<BOXES>        (Params, EvalArgs)
    kEvaluateHist,   // evaluate_hist_pool_mov_kernel<BOXES>   (Params, EvalArgs)
    kReset,          // reset_pool_kernel                      (Params, mask, obs)
    kRaycast,        // raycast_pool_kernel                    (Params, pose, n_poses_per_env, shared_poses, n, raw, ranges)
};

// null: the twin is not built
const void* resolve(int kernel, bool boxes);

}  // namespace navsim_pool
