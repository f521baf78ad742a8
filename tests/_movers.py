"""Helpers of the mover tests: the tapes they cast and the CPU reference.

The reference needs nothing new in the oracle: an OracleSim WITHOUT auto-reset on a per-env map that is re-composed around every
call -- static segments + the tape phase the rule prescribes for each env -- and an explicit masked reset, on the map of the reset
phase, for the envs whose episode the step ended.  That is what the GPU's in-step auto-reset has to return."""
import math

import numpy as np

from oracle import navsim_oracle as O


def blade_tape(P, M, pad_to=None, radius=0.75):
    """P phases of M segments: K = min(M, 4) straight "blades" tangent to the circle of `radius` about the spawn pose (0, 0), each cut
    into collinear pieces (M of them in all), turning once per P steps.  A robot that leaves the spawn pose straight ahead meets the
    circle after ~12 steps; the reset scan (0.72 m to the nearest blade) stays clear.  pad_to: pad every phase with NaN segments."""
    K = min(M, 4)
    half = 2.5 if K == 1 else radius * math.tan(math.pi / (2 * K)) * (1.0 if K < 4 else 1.6)
    pieces = [M // K + (1 if b < M % K else 0) for b in range(K)]
    frames = []
    for p in range(P):
        segs = []
        for b in range(K):
            a = 2 * math.pi * (p / P + b / K)
            cx, cy, tx, ty = radius * math.cos(a), radius * math.sin(a), -math.sin(a), math.cos(a)
            cuts = np.linspace(-half, half, pieces[b] + 1)
            segs += [[cx + tx * u, cy + ty * u, cx + tx * v, cy + ty * v] for u, v in zip(cuts[:-1], cuts[1:])]
        if pad_to:
            segs += [[math.nan] * 4] * (pad_to - M)
        frames.append(segs)
    return np.asarray(frames, dtype=np.float64).astype(np.float32)


def compose(static, tape, phases):
    """[N, S + M, 4]: env i's static segments followed by tape[phases[i]]"""
    static = np.asarray(static, np.float32)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(static, (len(phases),) + static.shape), tape[np.asarray(phases)]], axis=1))


class MoverOracle:
    """An OracleSim with movers, by composing its per-env map per call.  Same call surface as the OracleSim the lock-step helper of
    test_gpu_parity drives (reset / step / get_state / set_state)."""

    def __init__(self, N, static, tape, phase0=None, **kw):
        kw.pop("auto_reset", None)   # the resets are explicit here
        self.cpu = O.OracleSim(N, auto_reset=False, **kw)
        self.N, self.static, self.tape = N, np.asarray(static, np.float32), np.asarray(tape, np.float32)
        self.P = self.tape.shape[0]
        self.phase0 = np.zeros(N, np.int64) if phase0 is None else np.asarray(phase0, np.int64)
        self._map(self.phase0 % self.P)

    def _map(self, phases):
        self.cpu.set_map(compose(self.static, self.tape, phases), per_env=True)

    def set_goal_rects(self, which, rects):
        self.cpu.set_goal_rects(which, rects)

    def get_state(self):
        return self.cpu.get_state()

    def set_state(self, **kw):
        self.cpu.set_state(**kw)

    def step_phases(self):
        """the phase each env's NEXT step casts"""
        return (self.cpu.get_state()["ep_step"].astype(np.int64) + 1 + self.phase0) % self.P

    def reset(self, mask=None):
        self._map(self.phase0 % self.P)
        return self.cpu.reset(mask=mask)

    def step(self, action, auto_reset=True):
        self._map(self.step_phases())
        out = self.cpu.step(action)
        ended = out["ended"].astype(bool)
        if auto_reset and ended.any():
            out["obs"][ended] = self.reset(mask=ended.astype(np.uint8))[ended]
        return out
