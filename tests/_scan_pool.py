"""Helpers of the sector-LiDAR tests (scan_pool): the CPU reference and the per-step loops the persistent forms are compared with.

The reference needs nothing new in the oracle: a pooled env IS the env with 10 k beams -- pose, goal draws, reward, flags, episode
sums and RNG counters -- whose rows are passed through the reference's Pick(., k).  PooledOracle wraps an OracleSim / MoverOracle at
n_beams = 10 k and pools the rows it returns (env.pool_scan_reference), so test_gpu_parity._lockstep drives it unchanged.
The guarded allocations are tests/_guards.py's (run_both)."""
import ctypes as C

import numpy as np
import torch

from _guards import run_both   # noqa: F401  (re-exported: the guard helper of the tails tests)
from _movers import MoverOracle
from navbot_ppo_amd import maps
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, pool_scan_reference
from oracle import navsim_oracle as O

DEV = torch.device("cuda")
ACT_SEED, STEP_BASE, VAR = 0x5EED1234ABCD, 5, 0.3   # as in the scan-history and continued-rollout tests
FIELDS = ("obs", "act", "logp", "reward", "done", "arrive", "ended", "ep_return", "ep_length", "ep_path")


class PooledOracle:
    """The oracle of a pooled env: the dense one (10 k beams; with a tape a MoverOracle) with the rows it returns pooled."""

    def __init__(self, N, k, static, tape=None, phase0=None, **kw):
        self.N, self.k = N, k
        kw = {k_: v for k_, v in kw.items() if k_ != "obs_f16"}
        if tape is None:
            self.cpu = O.OracleSim(N, n_beams=10 * k, **kw)
            self.cpu.set_map(static)
        else:
            self.cpu = MoverOracle(N, static, tape, phase0, n_beams=10 * k, **kw)

    def set_goal_rects(self, which, rects):
        self.cpu.set_goal_rects(which, rects)

    def get_state(self):
        return self.cpu.get_state()

    def set_state(self, **kw):
        self.cpu.set_state(**kw)

    def reset(self, *a, **kw):
        return pool_scan_reference(self.cpu.reset(*a, **kw), self.k)

    def step(self, action):
        out = self.cpu.step(action)
        out["obs"] = pool_scan_reference(out["obs"], self.k)
        return out


def dense_raycast(seg, pose, k, below_min="clamp"):
    """[10] the pooled noise-free scan at `pose` as navsim_raycast returns it: per dense ray the sensor value (inf = no return, below
    range_min 0.12 or -inf), then the minimum of every k consecutive ones"""
    best = O.raycast(seg, *pose, n_beams=10 * k)
    r = np.where(best >= 3.5, np.inf, np.where(best < 0.12, -np.inf if below_min == "gazebo" else 0.12, best)).astype(np.float32)
    return r.reshape(10, k).min(axis=1)


def gpu_sim(N, map_name, k, tape=None, phase0=None, pool_first=False, **kw):
    """a handle on `map_name` with its goal rectangles, scan_pool = k set behind (or, pool_first, in front of) the map and the tape"""
    g = NavSim(N, device=DEV, **kw)
    rr, rs = maps.goal_rects(map_name)
    g.set_goal_rects(0, rr)
    g.set_goal_rects(1, rs)
    if pool_first and k != 1:
        g.set_scan_pool(k)
    g.set_map(maps.by_name(map_name) if isinstance(map_name, str) else map_name)
    if tape is not None:
        g.set_movers(tape, phase0)
    if not pool_first and k != 1:
        g.set_scan_pool(k)
    return g


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(x):
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def buffers(sim, n_steps, place=None, place_stats=None):
    """the [T (+ 1), N, .] buffers of a rollout; place(shape, dtype, align): an allocator (guarded outputs), default zeros;
    place_stats(zeros, align): the same for the three episode statistics, which are written where an episode ends only (in-out)"""
    n = sim.N
    zeros = lambda shape, dt, align: torch.zeros(shape, dtype=dt, device=DEV)
    mk = place or zeros
    z = lambda dt, align, *s: mk((n_steps, n) + s, dt, align)
    st = lambda dt: (place_stats or (lambda t, align: t))(zeros((n_steps, n), dt, 4), 4)
    return dict(obs=mk((n_steps + 1, n, 16), sim.obs_dtype, 16), act=z(torch.float32, 8, 2), logp=z(torch.float32, 4),
                reward=z(torch.float32, 4), done=z(torch.uint8, 1), arrive=z(torch.uint8, 1), ended=z(torch.uint8, 1),
                ep_return=st(torch.float32), ep_length=st(torch.int32), ep_path=st(torch.float32))


def stepping_rollout16(sim, flat, n_steps):
    """navsim_rollout_mlp64's reference from the per-step entry points: navsim_reset, then per step navppo_mlp64_act (obs_dim = 16,
    the same seed / env_id_base / step_base) -> navsim_step"""
    L = lib()
    b = buffers(sim, n_steps)
    sim.reset(b["obs"][0])
    var = torch.tensor(VAR, device=DEV)
    base = torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
    f16 = int(sim.obs_dtype == torch.float16)
    for t in range(n_steps):
        rc = L.navppo_mlp64_act(P(flat), P(b["obs"][t]), 16, f16, None, sim.N, P(var), ACT_SEED, int(sim.cfg.env_id_base), P(base), t,
                                P(b["act"][t]), P(b["logp"][t]), None, _st())
        assert rc == 0, L.navppo_last_error().decode()
        sim.step(b["act"][t], b["obs"][t + 1], b["reward"][t], b["done"][t], b["arrive"][t], b["ended"][t], b["ep_return"][t],
                 b["ep_length"][t], ep_path=b["ep_path"][t])
    torch.cuda.synchronize()
    return b, sim.get_state()


def kernel_rollout16(sim, flat, n_steps, b=None):
    """navsim_rollout_mlp64 through the C ABI from a reset"""
    b = buffers(sim, n_steps) if b is None else b
    sim.reset(b["obs"][0])
    var = torch.tensor(VAR, device=DEV)
    base = torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
    rc = lib().navsim_rollout_mlp64(sim._h, P(flat), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]), P(b["arrive"]),
                                    P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var), ACT_SEED, P(base),
                                    n_steps, _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()
    return b, sim.get_state()


def assert_same_rollout(got, got_state, want, want_state, what):
    """every buffer bit for bit (the episode statistics where an episode ended: elsewhere the entry points leave them alone)"""
    e = want["ended"].bool()
    for f in FIELDS:
        x, y = got[f], want[f]
        if f in ("ep_return", "ep_length", "ep_path"):
            x, y = x[e], y[e]
        assert same(x, y), f"{what}: {f}"
    for k in want_state:
        assert np.array_equal(got_state[k], want_state[k]), f"{what}: state {k}"
