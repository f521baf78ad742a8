"""ctypes binding of libnavsim.so (C ABI: include/navsim.h).  No CPU fallback: if the shared
library is missing or a call fails, this raises."""
import ctypes as C
import os

import torch   # (before the library is loaded: lib() says why)

_HERE = os.path.dirname(os.path.abspath(__file__))
# NAVSIM_LIB: another build of the same library (tools/build_variant.py A/B timing); never a different implementation
LIB_PATH = os.environ.get("NAVSIM_LIB") or os.path.join(_HERE, "libnavsim.so")

NAVSIM_ABI_VERSION = 6


class NavsimError(RuntimeError):
    pass


class NavsimCfg(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32),
        ("n_beams", C.c_int32),
        ("max_episode_steps", C.c_int32),
        ("auto_reset", C.c_int32),
        ("respawn_on_arrive", C.c_int32),
        ("obs_f16", C.c_int32),
        ("lidar_below_min", C.c_int32),
        ("lidar_noise_sigma", C.c_float),
        ("seed", C.c_uint64),
        ("env_id_base", C.c_uint64),
        ("threshold_arrive", C.c_double),
        ("spawn_x", C.c_double),
        ("spawn_y", C.c_double),
        ("spawn_yaw", C.c_double),
        ("goal_lo", C.c_double),
        ("goal_hi", C.c_double),
    ]


class NavsimInfo(C.Structure):
    """navsim_info (include/navsim.h): what the handle is and which kernel instantiation each entry point launches."""
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "n_envs", "n_beams", "obs_f16", "n_segments", "per_env_map", "tile_boxes", "has_map",
        "forced_epb", "forced_pair_cast", "step_epb", "step_waves", "step_cast", "seq_epb", "seq_waves", "seq_cast",
        "rollout_kind", "rollout_epb", "rollout_waves", "rollout_cast", "step_vgprs", "step_scratch_bytes", "step_lds_bytes",
        "seq_vgprs", "seq_scratch_bytes", "seq_lds_bytes")] + [("reserved", C.c_int32 * 6)]


# every symbol include/navsim.h declares: (name, restype, argtypes)
_vp, _i32, _d = C.c_void_p, C.c_int32, C.c_double
SYMBOLS = [
    ("navsim_version", C.c_int, []),
    ("navsim_last_error", C.c_char_p, []),
    ("navsim_default_cfg", None, [C.POINTER(NavsimCfg)]),
    ("navsim_create", C.c_int, [C.POINTER(NavsimCfg), C.POINTER(_vp)]),
    ("navsim_destroy", None, [_vp]),
    ("navsim_set_shape", C.c_int, [_vp, _i32, _i32]),
    ("navsim_get_info", C.c_int, [_vp, C.POINTER(NavsimInfo)]),
    ("navsim_set_scan_pool", C.c_int, [_vp, _i32]),   # sector LiDAR: k rays min-pooled into each scan column
    ("navsim_set_map", C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    ("navsim_set_movers", C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    ("navsim_set_mover_bank", C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    ("navsim_set_goal_rects", C.c_int, [_vp, _i32, _vp, _i32]),
    ("navsim_set_spawn_sampler", C.c_int, [_vp, _vp, _i32, _vp, _i32, _d, _d, _vp]),
    ("navsim_reset", C.c_int, [_vp, _vp, _vp, _vp]),
    ("navsim_step", C.c_int, [_vp] * 12),
    ("navsim_get_state", C.c_int, [_vp] * 8),
    ("navsim_set_state", C.c_int, [_vp] * 8),
    ("navsim_rtg_scan", C.c_int, [_vp, _vp, _i32, _i32, _d, _vp, _i32, _vp]),
    ("navsim_gae_scan", C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _d, _d, _vp, _vp, _i32, _vp]),
    ("navsim_gae_scan_trunc", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _d, _d, _vp, _vp, _i32, _vp]),
    ("navsim_raycast", C.c_int, [_vp, _vp, _vp, _vp]),
    ("navsim_odometry", C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("navsim_rollout_mlp64", C.c_int, [_vp] * 13 + [C.c_uint64, _vp, _i32, _vp]),
    ("navsim_rollout_resmlp512", C.c_int, [_vp] * 13 + [C.c_uint64, _vp, _i32, _vp]),
    ("navsim_step_seq", C.c_int, [_vp, _vp, _i32] + [_vp] * 9),
    ("navsim_evaluate_mlp64", C.c_int, [_vp, _vp, _vp, _i32, _i32] + [_vp] * 7),
    ("navsim_evaluate_resmlp512", C.c_int, [_vp, _vp, _vp, _i32, _i32] + [_vp] * 7),
    # scan history: the 42-column rows of the last three 10-beam scans
    ("navsim_stack_rows", C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    ("navsim_rollout_mlp64_hist", C.c_int, [_vp] * 13 + [C.c_uint64, _vp, _i32, _vp]),
    ("navsim_evaluate_mlp64_hist", C.c_int, [_vp, _vp, _vp, _i32, _i32] + [_vp] * 7),
    # ... continued across launches: the same two with a history carry in and out
    ("navsim_rollout_mlp64_hist_cont", C.c_int, [_vp] * 13 + [C.c_uint64, _vp, _i32, _vp, _vp, _vp]),
    ("navsim_stack_rows_cont", C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    # include/navppo.h
    ("navppo_last_error", C.c_char_p, []),
    ("navppo_mlp64_workspace_bytes", C.c_size_t, [_i32]),
    ("navppo_mlp64_loss_grad", C.c_int, [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    ("navppo_mlp64_loss_grad_net", C.c_int, [_i32, _vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    ("navppo_adam_step", C.c_int, [_vp, _vp, _vp, _vp, C.c_int64] + [C.c_float] * 5 + [_i32, _vp]),
    ("navppo_mlp64_value", C.c_int, [_vp, _vp, _i32, _i32, C.c_int64, _vp, _vp]),
    ("navppo_episode_sums", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
    ("navppo_mlp64_update_epoch", C.c_int, [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 6),
    ("navppo_mlp64_update_epoch_clipped", C.c_int,
     [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, _vp]),
    ("navppo_adam_step_clipped", C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64] + [C.c_float] * 6 + [_i32, _vp, _vp]),
    ("navppo_mlp64_act", C.c_int, [_vp, _vp, _i32, _i32, _vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    ("navppo_mlp64_bf16x3_prep_bytes", C.c_size_t, [C.c_int64, _i32]),
    ("navppo_mlp64_bf16x3_prepare", C.c_int, [_vp, _i32, _i32, C.c_int64, _vp, _vp]),
    ("navppo_mlp64_bf16x3_loss_grad", C.c_int, [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    ("navppo_mlp64_bf16x3_loss_grad_net", C.c_int, [_i32, _vp, _vp, _i32] + [_vp] * 4 + [C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    ("navppo_mlp64_bf16x3_update_epoch", C.c_int, [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 6),
    ("navppo_mlp64_bf16x3_update_epoch_clipped", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, _vp]),
    ("navppo_resmlp512_workspace_bytes", C.c_size_t, [C.c_int64]),
    ("navppo_resmlp512_loss_grad", C.c_int, [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    ("navppo_resmlp512_update_epoch", C.c_int, [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 6),
    ("navppo_resmlp512_update_epoch_clipped", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, _vp]),
    # the *_clipped prototypes with kl_limit and kl_state_dev in front of stream (navppo_adam_step_kl: kl_dev behind them)
    ("navppo_mlp64_update_epoch_kl", C.c_int,
     [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, C.c_float, _vp, _vp]),
    ("navppo_mlp64_bf16x3_update_epoch_kl", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, C.c_float, _vp, _vp]),
    ("navppo_resmlp512_update_epoch_kl", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp, C.c_float, _vp, _vp]),
    ("navppo_adam_step_kl", C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64] + [C.c_float] * 6 + [_i32, _vp, C.c_float, _vp, _vp, _vp]),
    # the *_clipped prototypes with kl_target, lr_min, lr_max, adapt and lr_state_dev in front of stream (navppo_adam_step_lr: kl_dev behind them)
    ("navppo_mlp64_update_epoch_lr", C.c_int,
     [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 + [_i32, _vp, _vp]),
    ("navppo_mlp64_bf16x3_update_epoch_lr", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 + [_i32, _vp, _vp]),
    ("navppo_resmlp512_update_epoch_lr", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 6 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 + [_i32, _vp, _vp]),
    ("navppo_adam_step_lr", C.c_int,
     [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64] + [C.c_float] * 6 + [_i32, _vp] + [C.c_float] * 3 + [_i32, _vp, _vp, _vp]),
    # the *_lr prototypes without the by-value var and with ent_coef, var_min, var_max and var_state_dev in front of stream
    ("navppo_mlp64_update_epoch_var", C.c_int,
     [_vp, _vp, _i32, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 5 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 +
     [_i32, _vp] + [C.c_float] * 3 + [_vp, _vp]),
    ("navppo_mlp64_bf16x3_update_epoch_var", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 5 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 +
     [_i32, _vp] + [C.c_float] * 3 + [_vp, _vp]),
    ("navppo_resmlp512_update_epoch_var", C.c_int,
     [_vp, _vp, _i32] + [_vp] * 4 + [C.c_int64] + [C.c_float] * 5 + [_i32] + [_vp] * 5 + [C.c_float, _vp] + [C.c_float] * 3 +
     [_i32, _vp] + [C.c_float] * 3 + [_vp, _vp]),
    ("navppo_shuffle_batch", C.c_int, [_vp, _i32, _i32] + [_vp] * 4 + [C.c_int64, C.c_uint64, C.c_uint64] + [_vp] * 7),
    ("navppo_return_moments", C.c_int, [_vp, _vp, _i32, _i32, _d, _vp, _vp, _vp]),
    ("navppo_reward_scale", C.c_int, [_vp, _vp, _i32, _vp, _vp, C.c_int64, _d, _d, _vp]),
    ("navppo_group_sums_ws_bytes", C.c_size_t, [_i32, _i32, _i32]),
    ("navppo_group_sums", C.c_int, [_vp] * 7 + [_i32, _i32, _i32, _vp, _vp, _vp]),
    ("navppo_resmlp512_value", C.c_int, [_vp, _vp, _i32, C.c_int64, _vp, _vp, _vp]),
    ("navppo_resmlp512_act", C.c_int, [_vp, _vp, _i32, _vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
]

_lib = None


def lib():
    """Loads libnavsim.so (built by navbot_ppo_amd/build.py).  Raises if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NavsimError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc, gfx950).  There is no CPU implementation to fall back to.")
        # The HIP runtime of the process must be the one PyTorch ships: every device pointer crossing this ABI is a
        # torch allocation.  Importing torch first makes its bundled libamdhip64 the loaded instance; loading
        # libnavsim.so first would pull in /opt/rocm's copy (same soname), which torch would then be bound to as well
        # -- on the GPU boxes that copy reports "no ROCm-capable device".
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the library does not export the symbol
            fn.restype = res
            fn.argtypes = args
        if L.navsim_version() != NAVSIM_ABI_VERSION:
            raise NavsimError(f"libnavsim ABI {L.navsim_version()} != expected {NAVSIM_ABI_VERSION}")
        _lib = L
    return _lib


def check(rc, what="navsim"):
    if rc != 0:
        msg = lib().navsim_last_error()
        raise NavsimError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def _ptr(t, offset=0):
    """The address of tensor `t` (+ `offset` bytes) as an entry point's void*; None (an argument left out) stays None."""
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def _navppo(entry, *args):
    """Calls the navppo_* entry point `entry` (include/navppo.h) with `args` and the current stream; a failure raises under the name
    of the entry point that was called, with its message."""
    L = lib()
    if getattr(L, entry)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0:
        raise RuntimeError(f"{entry} failed: {L.navppo_last_error().decode()}")
