"""Reward normalisation by a running variance of the discounted return (PPOConfig.norm_reward): the two entry points on the device
(navppo_return_moments, navppo_reward_scale) and their host mirrors."""
import torch

from ._native import _navppo, _ptr

RET_RMS_INIT = (0.0, 1.0, 1e-4)   # (mean, var, count) of a fresh run: Stable-Baselines3's RunningMeanStd(epsilon=1e-4)


def _chk_rewards(what, rew, ended=None):
    from ._native import NavsimError
    if not rew.is_cuda:
        raise NavsimError(f"{what} needs device tensors; there is no CPU path")
    assert rew.dtype == torch.float32 and rew.is_contiguous(), f"{what}: rewards are contiguous float32"
    if ended is not None:
        assert rew.dim() == 2 and ended.dtype == torch.uint8 and ended.shape == rew.shape and ended.is_contiguous() and ended.device == rew.device


def _chk_f64(what, t, shape, device):
    assert t.dtype == torch.float64 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == device, \
        f"{what}: a contiguous float64 tensor of shape {tuple(shape)} on {device}"


def return_moments(rew, ended, gamma, carry=None, out=None):
    """(n, mean, M2) of the T N forward discounted returns of a [T, N] rollout, as a float64 [3] device tensor (navppo_return_moments;
    `out`: where to write it).  carry: float64 [N], the running return in front of row 0 on entry and behind row T - 1 on return
    (None: every column starts at 0).  Asynchronous on the current stream; calls on one device must not overlap in time."""
    _chk_rewards("return_moments", rew, ended)
    T, N = rew.shape
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=rew.device)
    _chk_f64("return_moments: out", out, (3,), rew.device)
    if carry is not None:
        _chk_f64("return_moments: carry", carry, (N,), rew.device)
    with torch.cuda.device(rew.device):
        _navppo("navppo_return_moments", _ptr(rew), _ptr(ended), T, N, float(gamma), _ptr(carry), _ptr(out))
    return out


def reward_scale(rms, moments, rew, clip=10.0, eps=1e-8, out=None):
    """Merges the rows of `moments` ([K, 3] or [3] float64, None = no row: frozen statistics) into rms = (mean, var, count, scale)
    (float64 [4], updated in place) and returns clamp(float32(rew * scale), -clip, clip) with scale = 1 / sqrt(var + eps)
    (navppo_reward_scale).  out: where to write the scaled rewards (may be `rew`).  Asynchronous on the current stream."""
    _chk_rewards("reward_scale", rew)
    _chk_f64("reward_scale: rms", rms, (4,), rew.device)
    K = 0
    if moments is not None:
        K = 1 if moments.dim() == 1 else int(moments.shape[0])
        _chk_f64("reward_scale: moments", moments, (3,) if moments.dim() == 1 else (K, 3), rew.device)
    if out is None:
        out = torch.empty_like(rew)
    assert out.dtype == torch.float32 and out.shape == rew.shape and out.is_contiguous() and out.device == rew.device
    with torch.cuda.device(rew.device):
        _navppo("navppo_reward_scale", _ptr(rms), _ptr(moments), K, _ptr(rew), _ptr(out), rew.numel(), float(eps), float(clip))
    return out


def merge_return_moments(rms, rows):
    """The merge rule of navppo_reward_scale on the host, float64: rms = (mean, var, count[, ...]), rows [K, 3] = (n, mean, M2) per
    batch, merged in order with the formula of RunningMeanStd.update_from_moments; a row with n <= 0 or a non-finite entry is skipped.
    Returns (mean, var, count) as a numpy array."""
    import numpy as np
    mean, var, count = (np.float64(v) for v in list(rms)[:3])
    for bn, bm, bm2 in np.asarray(rows, dtype=np.float64).reshape(-1, 3):
        if not (bn > 0 and np.isfinite(bn) and np.isfinite(bm) and np.isfinite(bm2)):
            continue
        d, tot = bm - mean, count + bn
        mean = mean + d * bn / tot
        var = (var * count + bm2 + d * d * count * bn / tot) / tot
        count = tot
    return np.array([mean, var, count], dtype=np.float64)


def reward_norm_reference(rew, ended, gamma, rms=RET_RMS_INIT, carry=None, clip=10.0, eps=1e-8):
    """Host mirror of navppo_return_moments followed by navppo_reward_scale(K = 1), numpy float64 -- the statement of the rule.
    rew [T, N] float32, ended [T, N] (non-zero = an episode ended on that row), rms = (mean, var, count) before the rollout,
    carry [N] float64 or None.  Returns a namespace: moments (n, mean, M2) of the T N running returns, carry [N] behind the last row,
    rms (mean, var, count, scale) after the merge, out [T, N] float32 = clip(float32(rew * scale), -clip, clip)."""
    import types
    import numpy as np
    rew = np.ascontiguousarray(np.asarray(rew, dtype=np.float32))
    done = np.asarray(ended) != 0
    T, N = rew.shape
    R = np.zeros(N, dtype=np.float64) if carry is None else np.array(carry, dtype=np.float64)
    g = np.float64(gamma)
    rets = np.empty((T, N), dtype=np.float64)
    for t in range(T):
        R = g * R + rew[t].astype(np.float64)
        rets[t] = R
        R = np.where(done[t], 0.0, R)
    mean = rets.mean()
    moments = np.array([float(T * N), mean, ((rets - mean) ** 2).sum()], dtype=np.float64)
    m = merge_return_moments(rms, moments)
    scale = np.float64(1.0) / np.sqrt(m[1] + np.float64(eps))
    out = np.clip((rew.astype(np.float64) * scale).astype(np.float32), np.float32(-clip), np.float32(clip))
    return types.SimpleNamespace(moments=moments, carry=R, rms=np.append(m, scale), out=out)
