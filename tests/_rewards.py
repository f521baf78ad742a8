"""Test helper: synthetic [T, N] rollouts with rewards of this simulator's scale (tests of PPOConfig.norm_reward, CPU and GPU)."""
import numpy as np


def synthetic_rollout(T, N, seed=0, p_end=0.01):
    """(rew [T, N] float32, ended [T, N] uint8): 500 x (a change of distance of up to 0.05 m) per step, and on the rows where an
    episode ends (probability p_end per entry) +120 for an arrival or -100 for a collision."""
    g = np.random.default_rng(seed + 1000 * T + N)
    rew = (500.0 * g.uniform(-0.05, 0.05, (T, N))).astype(np.float32)
    ended = g.random((T, N)) < p_end
    rew[ended] = np.where(g.random(int(ended.sum())) < 0.5, 120.0, -100.0).astype(np.float32)
    return rew, ended.astype(np.uint8)
