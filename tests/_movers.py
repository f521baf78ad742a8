"""Helpers of the mover tests: the tapes they cast and the CPU reference.

The reference needs nothing new in the oracle: an OracleSim WITHOUT auto-reset on a per-env map that is re-composed around every
call -- static segments + the tape phase the rule prescribes for each env -- and a masked reset of its own, on the map of the reset
phase, for the envs whose episode the step ended, keyed like the auto-reset of that step (OracleSim.reset(noise_key=...): with the
sensor noise on, an in-step auto-reset re-uses the step's noise draws).  That is what the GPU's in-step auto-reset has to return."""
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

    def __init__(self, N, static, tape, phase0=None, watch=False, **kw):
        kw.pop("auto_reset", None)   # the resets are explicit here
        self.seen = [] if watch else None   # watch: per step, does any env's scan hold a tape segment (tape_in_scan)
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

    def reset(self, mask=None, noise_key=None):
        self._map(self.phase0 % self.P)
        return self.cpu.reset(mask=mask, noise_key=noise_key)

    def step(self, action, auto_reset=True):
        self._map(self.step_phases())
        before = self.cpu.get_state()
        out = self.cpu.step(action)
        ended = out["ended"].astype(bool)
        if self.seen is not None:
            self.seen.append(bool(self.tape_in_scan().any()))
        if auto_reset and ended.any():
            # the in-step auto-reset re-uses the sensor-noise draws of the step that ended the episode (an explicit reset has its own)
            out["obs"][ended] = self.reset(mask=ended.astype(np.uint8), noise_key=(before["rng_ctr"], before["ep_step"]))[ended]
        return out

    def tape_in_scan(self):
        """[N] bool: the scan at the env's pose on the phase it last observed differs from the static map's scan at that pose"""
        st = self.cpu.get_state()
        segs = compose(self.static, self.tape, (st["ep_step"].astype(np.int64) + self.phase0) % self.P)
        return np.array([(O.raycast(segs[i], *st["pose"][i]) != O.raycast(self.static, *st["pose"][i])).any() for i in range(self.N)])


# ---------------------------------------------------------------- helpers of tests/test_gpu_movers_edges.py
LIDAR_X = -0.032      # the sensor sits 32 mm behind the robot's centre (turtlebot3_burger.urdf.xacro:137)
RANGE_MIN = 0.12      # gazebo.xacro:118


def tripwire_rows(M, spawn=(0.0, 0.0), half=0.3):
    """[M, 4]: the four sides of a square of half-width `half` around the spawn pose (front, left, right, back), repeated to M rows.
    From the spawn pose every one of the 10 beams ends on it, 0.3 to 0.35 m away (M >= 3; the back side is never seen from there)."""
    x, y = spawn
    sides = [[x + half, y - half, x + half, y + half], [x - half, y + half, x + half, y + half],
             [x - half, y - half, x + half, y - half], [x - half, y - half, x - half, y + half]]
    return np.asarray([sides[j % 4] for j in range(M)], dtype=np.float32)


def embed_with_tripwires(tape, spawn=(0.0, 0.0)):
    """[P + 2, M, 4]: the tape as rows 1..P, a tripwire_rows() phase in front of it and one behind it.  NaN poison around a tape tells
    nothing -- the mover cull drops a NaN segment by design -- but a kernel that reads the row before tape[0] or the row after
    tape[P - 1] casts a wall 0.3 m from the spawn pose that the plain tape does not hold, and its scans change.  Hand the kernel
    rows 1..P (an interior pointer, 16-byte aligned like the allocation: a row is M * 16 bytes)."""
    tape = np.asarray(tape, np.float32)
    wire = tripwire_rows(tape.shape[1], spawn)[None]
    return np.ascontiguousarray(np.concatenate([wire, tape, wire]))


def below_min_poses(tape, phases, reach=0.07):
    """[N, 3] poses that look nose-first at a tape segment from closer than the sensor's range_min: env i's sensor sits `reach` metres
    from the midpoint of the longest segment of tape[phases[i]] (ties: the middle one of them), on its normal, on the side of the
    origin, looking along the normal -- so the two beams next to straight ahead (+-10 degrees) end on that segment, or on the
    collinear piece next to it, at reach / cos(10 deg) < RANGE_MIN."""
    tape = np.asarray(tape, np.float64)
    poses = []
    for p in np.asarray(phases):
        seg = tape[p][np.isfinite(tape[p]).all(axis=1)]
        ln = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1])
        longest = np.flatnonzero(ln >= ln.max() - 1e-6)
        ax, ay, bx, by = seg[longest[len(longest) // 2]]
        mx, my = (ax + bx) / 2, (ay + by) / 2
        nx, ny = -(by - ay), bx - ax
        nn = math.hypot(nx, ny)
        nx, ny = nx / nn, ny / nn
        if nx * mx + ny * my < 0:      # the normal that points away from the origin: the robot stands on the inner side
            nx, ny = -nx, -ny
        ox, oy = mx - reach * nx, my - reach * ny          # the sensor
        th = math.atan2(ny, nx)
        poses.append([ox - LIDAR_X * math.cos(th), oy - LIDAR_X * math.sin(th), th])
    return np.asarray(poses)


def partial_nan_tape(P, M=8, radius=0.75):
    """(tape, whole): `whole` is blade_tape(P, M - 4) plus four copies of a wall 0.25 m ahead of the spawn pose (x = 0.25, y from -1 to
    1: eight of the ten beams of the reset scan end on it) per phase, two in front of the blades' rows and two behind them; `tape` is
    `whole` with exactly ONE coordinate of each copy set to NaN, one copy per position (ax, ay, bx, by).  A segment with a NaN
    coordinate is absent: `tape` must cast as blade_tape(P, M - 4) does, while `whole` does not."""
    wall = np.tile(np.asarray([0.25, -1.0, 0.25, 1.0], np.float32), (P, 2, 1))
    whole = np.ascontiguousarray(np.concatenate([wall, blade_tape(P, M - 4, radius=radius), wall], axis=1))
    tape = whole.copy()
    for j, row in enumerate((0, 1, M - 2, M - 1)):
        tape[:, row, j] = np.nan
    return tape, whole


def blade_tape_m1(P, radius=0.75, half=2.5):
    """blade_tape(P, 1, radius=radius) without the Python loop over the phases (P = 65536: a 1 MB tape)"""
    a = 2 * np.pi * (np.arange(P, dtype=np.float64) / P)
    cx, cy, tx, ty = radius * np.cos(a), radius * np.sin(a), -np.sin(a), np.cos(a)
    return np.stack([cx - tx * half, cy - ty * half, cx + tx * half, cy + ty * half], 1).astype(np.float32)[:, None, :]
