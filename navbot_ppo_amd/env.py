"""Host-side mirror of the reference environment interface over libnavsim.so.

``Env`` is the N=1 drop-in for ``project_ppo/src/environment_new.py:26`` (same constructor
arguments, ``reset()``/``step(action, past_action)`` return types, and the attributes its callers
read: ``position.x/.y`` (ppo.py:535, main.py:202), ``goal_position.position.x/.y``,
``threshold_arrive``, ``past_distance``, ``use_vision``).  ``VecEnv`` is the batched form the
rollout of ``ppo.py:463-641`` becomes on a GPU: N envs per call, device tensors in and out,
auto-reset inside the step kernel.

PyTorch is used for device memory and streams only; all simulation happens in the HIP kernels.
"""
import ctypes as C
import math
import os
import types

import numpy as np
import torch

from . import maps as _maps
from ._native import NavsimCfg, NavsimError, NavsimInfo, check, lib

__all__ = ["NavSim", "VecEnv", "Env", "NavsimError", "rtg_scan", "gae_scan", "gae_scan_trunc", "truncated_returns_reference",
           "stack_rows", "stack_rows_reference", "HistoryWindow", "HostHistoryWindow", "HIST_DIM", "HIST_CARRY",
           "pool_scan_reference", "check_scan_pool", "MAX_SCAN_POOL"]

HIST_DIM = 42   # columns of a scan-history row (navsim_stack_rows)
HIST_CARRY = 22   # floats per env of a history carry: columns 16..37 of a history row (include/navsim.h)


def _chk_carry(what, t, n_envs, device):
    """a history carry before its pointer crosses the ABI: [N, 22] contiguous float32 on `device`, 16-byte aligned (None passes)"""
    if t is None:
        return
    if (not torch.is_tensor(t) or t.device != device or t.dtype != torch.float32 or tuple(t.shape) != (n_envs, HIST_CARRY)
            or not t.is_contiguous() or t.data_ptr() % 16):
        raise NavsimError(f"{what}: a contiguous, 16-byte aligned float32 tensor [{n_envs}, {HIST_CARRY}] on {device}, got "
                          f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")


MAX_SCAN_POOL = 4   # rays per scan column (navsim_set_scan_pool); more is not built


def check_scan_pool(scan_pool, n_beams=10, per_env_map=False, policy=None):
    """The refusals of ``scan_pool`` (sector LiDAR) that need no device, with the library's reasons: an int in 1..4; above 1 only
    with 10 beams, a shared static map and a policy that is not the 512-wide one.  Returns the int."""
    if isinstance(scan_pool, bool) or not isinstance(scan_pool, (int, np.integer)) or not 1 <= int(scan_pool) <= MAX_SCAN_POOL:
        raise ValueError(f"scan_pool {scan_pool!r}: an int in 1..{MAX_SCAN_POOL} (1 = off; more than {MAX_SCAN_POOL} rays per "
                         "column is not built)")
    k = int(scan_pool)
    if k > 1 and int(n_beams) != 10:
        raise ValueError(f"scan_pool > 1 needs n_beams == 10, not {n_beams}: pooling a 36-beam scan is not built")
    if k > 1 and per_env_map:
        raise ValueError("scan_pool > 1 needs a shared static map: pooling over per-env maps is not built")
    if k > 1 and policy == "resmlp512":
        raise ValueError("scan_pool > 1 with policy='resmlp512' is not built (the pooled kernels carry the mlp64 policies); "
                         "use policy='mlp64x2'")
    return k


def pool_scan_reference(rows_dense, k):
    """The sector-LiDAR rule on the host, numpy -- its statement: rows_dense [..., 10 k + 6] are the rows of an env with 10 k beams
    (scan / 3.5, then the six other columns); column c of the result [..., 16] is the minimum of dense columns k c .. k c + k - 1
    (the reference's pick_laser.Pick(scan, k): -inf wins, ties are ties), columns 10..15 are the dense row's last six.  k = 1
    returns the rows as they are."""
    rows = np.asarray(rows_dense)
    k = check_scan_pool(k)
    if rows.shape[-1] != 10 * k + 6:
        raise ValueError(f"pool_scan_reference: rows of {10 * k + 6} columns for k = {k}, got {rows.shape}")
    scan = rows[..., :10 * k].reshape(rows.shape[:-1] + (10, k)).min(axis=-1)
    return np.concatenate([scan, rows[..., 10 * k:]], axis=-1)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class NavSim:
    """One libnavsim handle (= one GPU's shard of envs) with torch tensors as buffers."""

    def __init__(self, n_envs, n_beams=10, max_episode_steps=0, auto_reset=False, respawn_on_arrive=False,
                 seed=0, env_id_base=0, threshold_arrive=0.2, spawn=(0.0, 0.0, 0.0), goal_box=(-3.6, 3.6),
                 obs_f16=False, device=None, lidar_below_min="clamp", lidar_noise_sigma=0.0, envs_per_workgroup=None,
                 pair_cast=None, scan_pool=1):
        """envs_per_workgroup / pair_cast: kernel-shape overrides of THIS handle (navsim_set_shape; tests and A/B timing --
        results never depend on them).  None = the dev tools' NAVSIM_EPB / NAVSIM_PAIR_CAST environment variables if set
        (read here, per handle; libnavsim itself reads nothing from the environment), else the built-in rule.
        scan_pool: sector LiDAR (set_scan_pool); 1 = off."""
        scan_pool = check_scan_pool(scan_pool, n_beams)
        if not torch.cuda.is_available():
            raise NavsimError("navbot_ppo_amd needs a HIP device (MI355X); there is no CPU path")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise NavsimError(f"navbot_ppo_amd needs a HIP device, got device={device!r}; there is no CPU path")
        if self.device.index is None:   # "cuda" names the current device: tensors report "cuda:N", and _chk compares devices
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.B, self.D = int(n_envs), int(n_beams), int(n_beams) + 6
        self.obs_dtype = torch.float16 if obs_f16 else torch.float32
        self.cfg = NavsimCfg(self.N, self.B, int(max_episode_steps), int(bool(auto_reset)), int(bool(respawn_on_arrive)),
                             int(bool(obs_f16)), {"clamp": 0, "gazebo": 1}[lidar_below_min], float(lidar_noise_sigma),
                             int(seed), int(env_id_base), float(threshold_arrive),
                             float(spawn[0]), float(spawn[1]), float(spawn[2]), float(goal_box[0]), float(goal_box[1]))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().navsim_create(C.byref(self.cfg), C.byref(self._h)), "navsim_create")
        self._seg = None  # keeps the map tensor alive: the handle only borrows the pointer
        self._mov_tape = self._mov_phase0 = None   # the same for the mover tape (set_movers)
        self._mov_bank = None   # set_mover_bank's host arrays (periods, rectangles), for set_mover_assignment
        self.movers_period = self.movers_segments = 0
        self.movers_tapes, self.movers_tape_id = 0, None   # set_mover_bank: tapes in the bank, the envs' tape ids (None = all 0)
        self.generation = 0  # bumped whenever device pointers / scalars a captured hipGraph would have frozen change
        def knob(name):   # a dev tool's environment variable; anything that is not an integer is ignored, as the library used to
            try:
                return int(os.environ[name])
            except (KeyError, ValueError):
                return None
        if envs_per_workgroup is None and knob("NAVSIM_EPB") is not None:
            envs_per_workgroup = knob("NAVSIM_EPB")
        if pair_cast is None and knob("NAVSIM_PAIR_CAST") is not None:
            pair_cast = knob("NAVSIM_PAIR_CAST") != 0
        if envs_per_workgroup is not None or pair_cast is not None:
            self.set_shape(envs_per_workgroup or 0, pair_cast)
        self.scan_pool = 1
        if scan_pool != 1:   # (off: not one call more than before)
            self.set_scan_pool(scan_pool)

    def set_scan_pool(self, k):
        """Sector LiDAR (navsim_set_scan_pool): the simulator casts 10 k rays and each of the 10 scan columns is the nearest return
        of k consecutive rays (pool_scan_reference states the rule; the env is that of 10 k beams, its rows pooled); k in 1..4, 1 =
        off.  Before or after set_map / set_movers, in any order.  Rows, nets, history rows and checkpoints keep their shape.  The
        pooled world is HARDER: obstacles the 10 beams passed by are seen, and hit.  Waits for the device; the world changed:
        ``generation`` is bumped."""
        k = check_scan_pool(k, self.B, getattr(self, "per_env", False))
        with torch.cuda.device(self.device):
            check(lib().navsim_set_scan_pool(self._h, k), "navsim_set_scan_pool")
        self.scan_pool = k
        self.generation += 1

    def set_shape(self, envs_per_workgroup=0, pair_cast=None):
        """navsim_set_shape: force the workgroup shape (0 = rule; 4 | 8 | 16 | 32 | 64) / the 128-segment passes of this handle."""
        check(lib().navsim_set_shape(self._h, int(envs_per_workgroup), -1 if pair_cast is None else int(bool(pair_cast))),
              "navsim_set_shape")
        self.generation += 1   # a captured hipGraph froze the old instantiation

    def info(self):
        """navsim_get_info as a dict: handle facts + the (envs, waves, cast variant) each entry point launches right now."""
        inf = NavsimInfo()
        check(lib().navsim_get_info(self._h, C.byref(inf)), "navsim_get_info")
        d = {n: getattr(inf, n) for n, _ in NavsimInfo._fields_ if n != "reserved"}
        d["scan_pool"] = int(inf.reserved[0])
        return d

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            lib().navsim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- world
    def set_map(self, seg, per_env=None):
        """seg [S,4] (shared) or [N,S,4] (per env) float32 segments (ax, ay, bx, by).  The handle BORROWS the device tensor it
        is given (kept alive here) -- except for shared maps of 65..4096 segments, of which navsim_set_map takes its own
        Morton-ordered SNAPSHOT with tile bounding boxes (a blocking copy + host sort).  So: after editing a map tensor in
        place (domain randomisation), call set_map again; never call it inside a stream capture or a hot loop."""
        seg = torch.as_tensor(np.asarray(seg, dtype=np.float32) if not torch.is_tensor(seg) else seg)
        seg = seg.to(device=self.device, dtype=torch.float32).contiguous()
        if per_env is None:
            per_env = seg.dim() == 3
        if seg.shape[-1] != 4 or seg.dim() != (3 if per_env else 2) or (per_env and seg.shape[0] != self.N):
            raise NavsimError(f"bad map shape {tuple(seg.shape)} for per_env={per_env}, N={self.N}")
        with torch.cuda.device(self.device):
            check(lib().navsim_set_map(self._h, _ptr(seg), int(seg.shape[-2]), int(bool(per_env)), _stream()), "navsim_set_map")
        self._seg = seg
        self.S, self.per_env = int(seg.shape[-2]), bool(per_env)
        self.generation += 1

    def set_movers(self, tape, phase0=None):
        """Moving obstacles (navsim_set_movers): tape [P, M, 4] float32 segments (ax, ay, bx, by), P phases of M segments (M <= 64,
        P <= 65536; pad a phase with NaN segments: ONE NaN coordinate suffices to make a segment absent, everywhere -- infinite coordinates
        are undefined), cast beside the static map: a step's scan of env i sees
        tape[(k + 1 + phase0[i]) % P] with k its episode step counter before the step, every reset observation tape[phase0[i]].
        phase0: [N] integers in [0, P) or None (all zero).  tape=None turns movers off.  Call after set_map (10 beams, a shared static
        map).  The handle BORROWS the tape tensor -- a float32, contiguous, 16-byte aligned tensor on the handle's device is used where it lies, a
        view into a larger allocation included (kept alive here; after editing it in place nothing needs to be called unless phase
        tape[phase0[i]] changed, which the spawn scans have cached: then call set_movers again) and copies phase0."""
        if tape is None:
            with torch.cuda.device(self.device):
                check(lib().navsim_set_movers(self._h, None, 0, 0, None, _stream()), "navsim_set_movers")
            self._mov_tape = self._mov_phase0 = self._mov_bank = None
            self.movers_period = self.movers_segments = 0
            self.movers_tapes, self.movers_tape_id = 0, None
            self.generation += 1
            return
        tape = torch.as_tensor(np.asarray(tape, dtype=np.float32) if not torch.is_tensor(tape) else tape)
        tape = tape.to(device=self.device, dtype=torch.float32).contiguous()
        if tape.dim() != 3 or tape.shape[-1] != 4 or tape.shape[0] < 1 or tape.shape[1] < 1:
            raise NavsimError(f"set_movers: tape must be [P, M, 4], got {tuple(tape.shape)}")
        if tape.data_ptr() % 16:
            raise NavsimError("set_movers: the tape must be 16-byte aligned")
        if phase0 is not None:
            ph = torch.as_tensor(np.asarray(phase0) if not torch.is_tensor(phase0) else phase0)
            if ph.is_floating_point() or ph.numel() != self.N:
                raise NavsimError(f"set_movers: phase0 must be {self.N} integers, got {ph.dtype} {tuple(ph.shape)}")
            phase0 = ph.reshape(self.N).to(device=self.device, dtype=torch.int32).contiguous()
            self._chk("set_movers: phase0", phase0, torch.int32, self.N)
        self._chk("set_movers: tape", tape, torch.float32, tape.numel())
        with torch.cuda.device(self.device):
            check(lib().navsim_set_movers(self._h, _ptr(tape), int(tape.shape[0]), int(tape.shape[1]), _ptr(phase0), _stream()),
                  "navsim_set_movers")
        self._mov_tape, self._mov_phase0, self._mov_bank = tape, phase0, None
        self.movers_period, self.movers_segments = int(tape.shape[0]), int(tape.shape[1])
        self.movers_tapes, self.movers_tape_id = 1, None
        self.generation += 1

    def set_mover_bank(self, bank, periods=None, tape_id=None, phase0=None, goal_rects=None):
        """A bank of tapes, one scenario per env (navsim_set_mover_bank): bank [K, Pmax, M, 4] float32 (maps.mover_bank pads it),
        periods [K] integers in [1, Pmax] (None: all Pmax), tape_id [N] integers in [0, K) (None: all 0), phase0 [N] integers in
        [0, periods[tape_id[i]]) (None: all 0), goal_rects [K, R, 4] float64 (xmin, xmax, ymin, ymax), R <= 8, a row with a NaN absent
        (None: none).  Env i's scan sees bank[t][(k + 1 + phase0[i]) % periods[t]], t = tape_id[i]: set_movers' rule per env; a
        uniform-box goal draw of env i is also rejected inside its tape's rectangles.  Rows periods[k] .. Pmax-1 of a tape are never
        read.  The bank is BORROWED exactly as set_movers borrows its tape; ids, phases, periods and rectangles are copied.  A call
        of either replaces what the other set; bank=None turns movers off."""
        if bank is None:
            return self.set_movers(None)
        bank = torch.as_tensor(np.asarray(bank, dtype=np.float32) if not torch.is_tensor(bank) else bank)
        bank = bank.to(device=self.device, dtype=torch.float32).contiguous()
        if bank.dim() != 4 or bank.shape[-1] != 4 or min(bank.shape[:3]) < 1:
            raise NavsimError(f"set_mover_bank: bank must be [K, Pmax, M, 4], got {tuple(bank.shape)}")
        K, Pmax, M = (int(v) for v in bank.shape[:3])
        if bank.data_ptr() % 16:
            raise NavsimError("set_mover_bank: the bank must be 16-byte aligned")
        per = np.full(K, Pmax, dtype=np.int32) if periods is None else np.ascontiguousarray(np.asarray(periods).reshape(-1))
        if per.size != K or not np.issubdtype(per.dtype, np.integer):
            raise NavsimError(f"set_mover_bank: periods must be {K} integers, got {per.dtype} {per.shape}")
        per = np.ascontiguousarray(per, dtype=np.int32)

        def per_env(name, v):
            if v is None:
                return None
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
            if t.is_floating_point() or t.numel() != self.N:
                raise NavsimError(f"set_mover_bank: {name} must be {self.N} integers, got {t.dtype} {tuple(t.shape)}")
            t = t.reshape(self.N).to(device=self.device, dtype=torch.int32).contiguous()
            self._chk(f"set_mover_bank: {name}", t, torch.int32, self.N)
            return t
        tape_id, phase0 = per_env("tape_id", tape_id), per_env("phase0", phase0)
        rects, n_rects = None, 0
        if goal_rects is not None:
            rects = np.ascontiguousarray(goal_rects, dtype=np.float64)
            if rects.ndim != 3 or rects.shape[0] != K or rects.shape[2] != 4 or rects.shape[1] > 8:
                raise NavsimError(f"set_mover_bank: goal_rects must be [{K}, R <= 8, 4], got {rects.shape}")
            n_rects = int(rects.shape[1])
            if n_rects == 0:
                rects = None
        self._chk("set_mover_bank: bank", bank, torch.float32, bank.numel())
        with torch.cuda.device(self.device):
            check(lib().navsim_set_mover_bank(self._h, _ptr(bank), K, Pmax, M, _np_ptr(per), _ptr(tape_id), _ptr(phase0),
                                              _np_ptr(rects), n_rects, _stream()), "navsim_set_mover_bank")
        self._mov_tape, self._mov_phase0 = bank, phase0
        self._mov_bank = (per, rects, n_rects)   # what set_mover_assignment hands in again (host copies)
        self.movers_period, self.movers_segments = Pmax, M
        self.movers_tapes, self.movers_tape_id = K, tape_id
        self.generation += 1

    def set_mover_assignment(self, tape_id, phase0=None):
        """Re-points the envs at the tapes of the bank the handle already holds: tape_id [N] integers in [0, K), phase0 [N] integers in
        [0, periods[tape_id[i]]) (None: all 0).  The bank on the device, the periods and the goal rectangles stay what set_mover_bank
        was given (the same navsim_set_mover_bank entry point with the same bank pointer: no upload of the bank); the per-env spawn
        scans are rebuilt for the new tapes and phases.  The world changed: ``generation`` is bumped.  Waits for the stream."""
        if self._mov_bank is None:
            raise NavsimError("set_mover_assignment: the handle holds no bank of tapes (call set_mover_bank first)")
        if tape_id is None:
            raise NavsimError("set_mover_assignment: tape_id: required")
        per, rects, _ = self._mov_bank
        self.set_mover_bank(self._mov_tape, per, tape_id, phase0, rects)

    def set_goal_rects(self, which, rects):
        r = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        with torch.cuda.device(self.device):   # the call synchronises the CURRENT device before touching the rectangles
            check(lib().navsim_set_goal_rects(self._h, int(which), _np_ptr(r), r.shape[0]), "navsim_set_goal_rects")
        self.generation += 1

    def set_spawn_sampler(self, starts, goals=None, min_dist=1.5, max_dist=6.0):
        """GoalSpawnSampler tables (spawn_goal_sampler.py:37-62): start poses [K,3], goal points [G,2] or None."""
        st = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        g = None if goals is None else np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        with torch.cuda.device(self.device):
            check(lib().navsim_set_spawn_sampler(self._h, _np_ptr(st), st.shape[0], _np_ptr(g), 0 if g is None else g.shape[0],
                                                 float(min_dist), float(max_dist), _stream()), "navsim_set_spawn_sampler")
        self.generation += 1

    # -- buffers
    def alloc_io(self):
        dev, N = self.device, self.N
        return types.SimpleNamespace(
            obs=torch.zeros((N, self.D), dtype=self.obs_dtype, device=dev),
            reward=torch.zeros(N, dtype=torch.float32, device=dev),
            done=torch.zeros(N, dtype=torch.uint8, device=dev),
            arrive=torch.zeros(N, dtype=torch.uint8, device=dev),
            ended=torch.zeros(N, dtype=torch.uint8, device=dev),
            ep_return=torch.zeros(N, dtype=torch.float32, device=dev),
            ep_length=torch.zeros(N, dtype=torch.int32, device=dev),
            ep_path=torch.zeros(N, dtype=torch.float32, device=dev))

    # -- calls (all asynchronous on torch's current stream)
    # The C ABI takes raw device pointers and cannot know what is behind them: every tensor is checked HERE -- device, dtype,
    # element count, contiguity -- before its data_ptr() crosses the boundary (a float32 buffer handed to an f16 handle, or rows of
    # the wrong width, would otherwise be overwritten or overrun silently).
    def _chk(self, name, t, dtype, numel, optional=False):
        if t is None:
            if optional:
                return
            raise NavsimError(f"{name}: required")
        if not torch.is_tensor(t) or t.device != self.device:
            raise NavsimError(f"{name}: expected a tensor on {self.device}, got {getattr(t, 'device', type(t))}")
        if t.dtype != dtype:
            raise NavsimError(f"{name}: expected {dtype}, got {t.dtype}"
                              + (" (this handle writes float16 observations: obs_f16=True)" if dtype == torch.float16 else ""))
        if t.numel() != numel or not t.is_contiguous():
            raise NavsimError(f"{name}: expected {numel} contiguous elements, got shape {tuple(t.shape)}"
                              f"{'' if t.is_contiguous() else ' (not contiguous)'}")

    def _chk_step_io(self, rows, obs, reward, done, arrive, ended, ep_return, ep_length, ep_path, what):
        n = rows * self.N
        self._chk(f"{what}: obs", obs, self.obs_dtype, n * self.D)
        self._chk(f"{what}: reward", reward, torch.float32, n)
        self._chk(f"{what}: done", done, torch.uint8, n)
        self._chk(f"{what}: arrive", arrive, torch.uint8, n)
        self._chk(f"{what}: ended", ended, torch.uint8, n, optional=True)
        self._chk(f"{what}: ep_return", ep_return, torch.float32, n, optional=True)
        self._chk(f"{what}: ep_length", ep_length, torch.int32, n, optional=True)
        self._chk(f"{what}: ep_path", ep_path, torch.float32, n, optional=True)

    def reset(self, obs, mask=None):
        self._chk("reset: obs", obs, self.obs_dtype, self.N * self.D)
        self._chk("reset: mask", mask, torch.uint8, self.N, optional=True)
        with torch.cuda.device(self.device):
            check(lib().navsim_reset(self._h, _ptr(mask), _ptr(obs), _stream()), "navsim_reset")
        return obs

    def step(self, action, obs, reward, done, arrive, ended=None, ep_return=None, ep_length=None, past_action=None,
             ep_path=None):
        self._chk("step: action", action, torch.float32, 2 * self.N)
        self._chk("step: past_action", past_action, torch.float32, 2 * self.N, optional=True)
        self._chk_step_io(1, obs, reward, done, arrive, ended, ep_return, ep_length, ep_path, "step")
        with torch.cuda.device(self.device):
            check(lib().navsim_step(self._h, _ptr(action), _ptr(past_action), _ptr(obs), _ptr(reward), _ptr(done),
                                    _ptr(arrive), _ptr(ended), _ptr(ep_return), _ptr(ep_length), _ptr(ep_path), _stream()),
                  "navsim_step")

    def step_seq(self, actions, obs, reward, done, arrive, ended=None, ep_return=None, ep_length=None, ep_path=None):
        """All steps of an action tape in ONE launch (navsim_step_seq): actions [T, N, 2] float32; every output is [T, N, ...]
        and row t is what ``step(actions[t], ...)`` would have written.  For loops whose actions do not depend on the
        observations they produce (recorded tapes, scripted / random policies): the workgroups keep their envs on chip
        between the steps, so the launch ramp and the kernel boundaries of T launches are paid once."""
        T = int(actions.shape[0])
        if tuple(actions.shape) != (T, self.N, 2):
            raise NavsimError(f"step_seq: actions must be [T, {self.N}, 2], got {tuple(actions.shape)}")
        self._chk("step_seq: actions", actions, torch.float32, 2 * T * self.N)
        self._chk_step_io(T, obs, reward, done, arrive, ended, ep_return, ep_length, ep_path, "step_seq")
        with torch.cuda.device(self.device):
            check(lib().navsim_step_seq(self._h, _ptr(actions), T, _ptr(obs), _ptr(reward), _ptr(done), _ptr(arrive), _ptr(ended),
                                        _ptr(ep_return), _ptr(ep_length), _ptr(ep_path), _stream()), "navsim_step_seq")

    def raycast(self, pose):
        pose = pose.to(device=self.device, dtype=torch.float64).contiguous()
        out = torch.empty((self.N, self.B), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().navsim_raycast(self._h, _ptr(pose), _ptr(out), _stream()), "navsim_raycast")
        return out

    def get_state(self):
        N = self.N
        st = dict(pose=np.empty((N, 3)), goal=np.empty((N, 2)), past_dist=np.empty(N),
                  past_action=np.empty((N, 2), np.float32), ep_step=np.empty(N, np.int32), rng_ctr=np.empty(N, np.uint32))
        with torch.cuda.device(self.device):
            check(lib().navsim_get_state(self._h, *[_np_ptr(st[k]) for k in
                                                    ("pose", "goal", "past_dist", "past_action", "ep_step", "rng_ctr")],
                                         _stream()), "navsim_get_state")
        return st

    def set_state(self, pose=None, goal=None, past_dist=None, past_action=None, ep_step=None, rng_ctr=None):
        def cv(a, dt, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.shape != shape:
                raise NavsimError(f"set_state: expected shape {shape}, got {a.shape}")
            return a
        N = self.N
        arrs = [cv(pose, np.float64, (N, 3)), cv(goal, np.float64, (N, 2)), cv(past_dist, np.float64, (N,)),
                cv(past_action, np.float32, (N, 2)), cv(ep_step, np.int32, (N,)), cv(rng_ctr, np.uint32, (N,))]
        with torch.cuda.device(self.device):
            check(lib().navsim_set_state(self._h, *[_np_ptr(a) for a in arrs], _stream()), "navsim_set_state")


def rtg_scan(rew, ended, gamma, out=None, exact=False):
    """PPO.compute_rtgs (ppo.py:643-671) on [T,N] device tensors; see navsim_rtg_scan.  exact: the serial recurrence (every
    bit the reference's) instead of the T-split scan (<= 1 float32 ulp)."""
    if not rew.is_cuda:
        raise NavsimError("rtg_scan needs device tensors; there is no CPU path")
    T, N = rew.shape
    rew = rew.contiguous()
    ended = ended.contiguous()
    assert rew.dtype == torch.float32 and ended.dtype == torch.uint8 and ended.shape == rew.shape
    if out is None:
        out = torch.empty_like(rew)
    with torch.cuda.device(rew.device):
        check(lib().navsim_rtg_scan(_ptr(rew), _ptr(ended), T, N, float(gamma), _ptr(out), int(bool(exact)), _stream()), "navsim_rtg_scan")
    return out


def odometry(x, y, quat, goal):
    """Env.getOdometry (environment_new.py:138-181) for n samples on the device: x, y [n], quat [n,4] = (qx, qy, qz, qw),
    goal [n,2], all float64 -> [n,3] float64 (yaw, rel_theta, diff_angle); see navsim_odometry."""
    if not x.is_cuda:
        raise NavsimError("odometry needs device tensors; there is no CPU path")
    x, y, quat, goal = (t.to(torch.float64).contiguous() for t in (x, y, quat, goal))
    n = x.shape[0]
    assert y.shape == (n,) and quat.shape == (n, 4) and goal.shape == (n, 2)
    out = torch.empty((n, 3), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().navsim_odometry(n, _ptr(x), _ptr(y), _ptr(quat), _ptr(goal), _ptr(out), _stream()), "navsim_odometry")
    return out


def gae_scan(rew, ended, value, gamma, lam, last_value=None, want_returns=True, exact=False):
    """GAE(lambda) on [T,N] device tensors (navsim_gae_scan): returns (adv, lambda_returns).  lam = 1 without `last_value`
    is PPO.compute_rtgs followed by A = rtgs - V (ppo.py:277, 643-671), bit for bit."""
    if not rew.is_cuda:
        raise NavsimError("gae_scan needs device tensors; there is no CPU path")
    T, N = rew.shape
    rew, ended, value = rew.contiguous(), ended.contiguous(), value.contiguous()
    assert rew.dtype == torch.float32 and ended.dtype == torch.uint8 and value.dtype == torch.float32
    assert ended.shape == rew.shape == value.shape and (last_value is None or last_value.shape == (N,))
    if last_value is not None:
        last_value = last_value.to(torch.float32).contiguous()
    adv = torch.empty_like(rew)
    ret = torch.empty_like(rew) if want_returns else None
    with torch.cuda.device(rew.device):
        check(lib().navsim_gae_scan(_ptr(rew), _ptr(ended), _ptr(value), _ptr(last_value), T, N, float(gamma), float(lam),
                                    _ptr(adv), _ptr(ret), int(bool(exact)), _stream()), "navsim_gae_scan")
    return adv, ret


def gae_scan_trunc(rew, ended, done, arrive, value, gamma, lam, last_value=None, want_returns=True, exact=False):
    """gae_scan with time-outs bootstrapped (navsim_gae_scan_trunc): on a row with `ended` set and neither `done` nor `arrive` the
    value of the unseen next state is estimated by V of the row itself (rsl_rl's rule; truncated_returns_reference states it).
    Returns (adv, lambda_returns); without such a row both are gae_scan's, bit for bit."""
    if not rew.is_cuda:
        raise NavsimError("gae_scan_trunc needs device tensors; there is no CPU path")
    T, N = rew.shape
    rew, ended, done, arrive, value = (t.contiguous() for t in (rew, ended, done, arrive, value))
    assert rew.dtype == torch.float32 and value.dtype == torch.float32 and all(f.dtype == torch.uint8 for f in (ended, done, arrive))
    assert ended.shape == done.shape == arrive.shape == rew.shape == value.shape and (last_value is None or last_value.shape == (N,))
    if last_value is not None:
        last_value = last_value.to(torch.float32).contiguous()
    adv = torch.empty_like(rew)
    ret = torch.empty_like(rew) if want_returns else None
    with torch.cuda.device(rew.device):
        check(lib().navsim_gae_scan_trunc(_ptr(rew), _ptr(ended), _ptr(done), _ptr(arrive), _ptr(value), _ptr(last_value), T, N,
                                          float(gamma), float(lam), _ptr(adv), _ptr(ret), int(bool(exact)), _stream()),
              "navsim_gae_scan_trunc")
    return adv, ret


def truncated_returns_reference(rew, ended, done, arrive, value, gamma, lam, last_value=None):
    """Host mirror of navsim_gae_scan_trunc, numpy float64 -- the statement of the rule.  rew, value [T, N] float32; ended, done,
    arrive [T, N] (non-zero = set); last_value [N] float32 or None (= zeros: the batch end is terminal).  Per column, backwards:
        trunc[t] = ended[t] and not done[t] and not arrive[t]                    (a time-out, as navppo_episode_sums counts them)
        add      = rew[t] + (gamma V[t] if trunc[t] else 0 if ended[t] else gamma (1 - lam) V[t+1])        V[T] = last_value
        R[t]     = add + R[t+1] * (0 if ended[t] else gamma lam)                                           R[T] = last_value
    Returns (adv, ret) as float32 arrays: ret = float32(R), adv = ret - V."""
    rew = np.asarray(rew, dtype=np.float32)
    V = np.asarray(value, dtype=np.float32)
    T, N = rew.shape
    end = np.asarray(ended).reshape(T, N) != 0
    trunc = end & ~(np.asarray(done).reshape(T, N) != 0) & ~(np.asarray(arrive).reshape(T, N) != 0)
    g, lm = np.float64(gamma), np.float64(lam)
    gl, gv = g * lm, g * (np.float64(1.0) - lm)
    vnext = np.zeros(N, dtype=np.float32) if last_value is None else np.asarray(last_value, dtype=np.float32).reshape(N)
    R = vnext.astype(np.float64)
    ret = np.empty((T, N), dtype=np.float32)
    for t in range(T - 1, -1, -1):
        boot = np.where(trunc[t], g * V[t].astype(np.float64), np.where(end[t], 0.0, gv * vnext.astype(np.float64)))
        R = (rew[t].astype(np.float64) + boot) + R * np.where(end[t], 0.0, gl)
        ret[t] = R.astype(np.float32)
        vnext = V[t]
    return ret - V, ret


def stack_rows_reference(obs, ended=None, carry=None):
    """Host mirror of navsim_stack_rows / navsim_stack_rows_cont, numpy -- the statement of the scan-history rule.  obs [R, N, 16] (float32 or float16) are
    ordinary rows (10 beams / 3.5, past_action, 4 goal columns), ended [R - 1, N] (non-zero = the step between rows t and t + 1 ended
    the episode; None allowed when R == 1).  Returns [R, N, 42] of obs's dtype, every entry a copy:
        out[t, :,  0:16] = obs[t]                  the ordinary row
        out[t, :, 16:26] = obs[i1, :, 0:10]        the previous scan,          i1 = max(t - 1, r(t))
        out[t, :, 26:36] = obs[i2, :, 0:10]        the scan before it,         i2 = max(t - 2, r(t))
        out[t, :, 36:38] = obs[i1, :, 10:12]       the action between the two older scans
        out[t, :, 38:42] = 0
    r(t) = the latest s <= t with s == 0 or ended[s - 1] != 0: frames never reach across an episode's first row, and row 0 of the
    buffer counts as one -- unless ``carry`` [N, 22] (float32; None = no carry) says what lay in front of it: columns 16..37 of row
    0's history row (the scan of row -1, the scan of row -2, past_action of row -1, each already clamped to the episode's first row).
    Then the call returns (rows, carry_out), carry_out [N, 22] float32 = columns 16..37 of the last row: the carry of that row,
    wherever it is row 0 of the next buffer.  The pieces of a buffer cut at row s (obs[:s + 1], ended[:s] | obs[s:], ended[s:]),
    chained through the carry, give the rows of the whole."""
    obs = np.asarray(obs)
    if obs.ndim != 3 or obs.shape[2] != 16:
        raise ValueError(f"stack_rows_reference: obs must be [R, N, 16], got {obs.shape}")
    R, N, _ = obs.shape
    if R < 1 or N < 1:
        raise ValueError("stack_rows_reference: R and N must be at least 1")
    if ended is None:
        if R > 1:
            raise ValueError("stack_rows_reference: ended may be None only when R == 1")
        end = np.zeros((0, N), dtype=bool)
    else:
        end = np.asarray(ended).reshape(R - 1, N) != 0
    out = np.zeros((R, N, HIST_DIM), dtype=obs.dtype)
    cols = np.arange(N)
    start = np.zeros(N, dtype=np.int64)   # r(t) per env
    for t in range(R):
        if t > 0:
            start = np.where(end[t - 1], t, start)
        i1, i2 = np.maximum(t - 1, start), np.maximum(t - 2, start)
        out[t, :, 0:16] = obs[t]
        out[t, :, 16:26] = obs[i1, cols, 0:10]
        out[t, :, 26:36] = obs[i2, cols, 0:10]
        out[t, :, 36:38] = obs[i1, cols, 10:12]
    if carry is None:
        return out
    carry = np.asarray(carry, dtype=np.float32)
    if carry.shape != (N, HIST_CARRY):
        raise ValueError(f"stack_rows_reference: carry must be [{N}, {HIST_CARRY}], got {carry.shape}")
    out[0, :, 16:38] = carry.astype(obs.dtype)          # row 0: what lay in front of it
    if R > 1:                                           # row 1, unless it starts an episode: its oldest frame is row -1's scan
        keep = ~end[0]
        out[1, keep, 26:36] = carry[keep, 0:10].astype(obs.dtype)
    return out, out[R - 1, :, 16:38].astype(np.float32)


def stack_rows(obs, ended=None, out=None, carry_in=None, carry_out=None):
    """navsim_stack_rows on device tensors: obs [R, N, 16] float32 or float16, ended [R - 1, N] uint8 (None allowed when R == 1)
    -> [R, N, 42] of obs's dtype (``out`` if given); stack_rows_reference states the rule.  Asynchronous on the current stream.
    carry_in / carry_out ([N, 22] float32, either may be None, both may be one tensor): navsim_stack_rows_cont -- row 0 continues
    from carry_in instead of starting the episodes, carry_out receives the carry of the last row."""
    if not torch.is_tensor(obs) or not obs.is_cuda:
        raise NavsimError("stack_rows needs device tensors; there is no CPU path (stack_rows_reference is the host mirror)")
    if obs.dim() != 3 or obs.shape[2] != 16 or obs.dtype not in (torch.float32, torch.float16) or not obs.is_contiguous():
        raise NavsimError(f"stack_rows: obs must be contiguous [R, N, 16] float32 or float16 rows, got {obs.dtype} {tuple(obs.shape)}")
    R, N = int(obs.shape[0]), int(obs.shape[1])
    if ended is not None and (not torch.is_tensor(ended) or ended.device != obs.device or ended.dtype != torch.uint8
                              or ended.numel() != (R - 1) * N or not ended.is_contiguous()):
        raise NavsimError(f"stack_rows: ended must be {(R - 1) * N} contiguous uint8 values on {obs.device}")
    if ended is not None and R == 1:
        ended = None
    if out is None:
        out = torch.empty((R, N, HIST_DIM), dtype=obs.dtype, device=obs.device)
    elif (not torch.is_tensor(out) or out.device != obs.device or out.dtype != obs.dtype or out.numel() != R * N * HIST_DIM
          or not out.is_contiguous()):
        raise NavsimError(f"stack_rows: out must be {R * N * HIST_DIM} contiguous {obs.dtype} values on {obs.device}")
    _chk_carry("stack_rows: carry_in", carry_in, N, obs.device)
    _chk_carry("stack_rows: carry_out", carry_out, N, obs.device)
    with torch.cuda.device(obs.device):
        if carry_in is None and carry_out is None:
            check(lib().navsim_stack_rows(_ptr(obs), int(obs.dtype == torch.float16), _ptr(ended), R, N, _ptr(out), _stream()),
                  "navsim_stack_rows")
        else:
            check(lib().navsim_stack_rows_cont(_ptr(obs), int(obs.dtype == torch.float16), _ptr(ended), R, N, _ptr(out),
                                               _ptr(carry_in), _ptr(carry_out), _stream()), "navsim_stack_rows_cont")
    return out


class HistoryWindow:
    """The last three ordinary rows and the flags between them, for a loop that steps the envs itself: ``reset(obs)`` starts every
    env's episode, ``push(obs, ended)`` adds the row a step left (``ended`` [N] uint8: that step's flag); both return the current
    [N, 42] history row -- the last row navsim_stack_rows makes of the window, which is exact whatever lies in front of it."""

    def __init__(self, n_envs, device, dtype=torch.float32):
        self.N = int(n_envs)
        self.rows = torch.zeros((3, self.N, 16), dtype=dtype, device=device)
        self.flags = torch.zeros((2, self.N), dtype=torch.uint8, device=device)
        # one output per window length, each an allocation of its own (a tail of a [3, N, 42] buffer is 16-byte aligned for even N only)
        self.out = [torch.zeros((R, self.N, HIST_DIM), dtype=dtype, device=device) for R in (1, 2, 3)]
        self.row = torch.zeros((self.N, HIST_DIM), dtype=dtype, device=device)   # the current history row
        self.count = 0

    def reset(self, obs):
        self.count = 0
        return self.push(obs)

    def push(self, obs, ended=None):
        if self.count and ended is None:
            raise NavsimError("HistoryWindow.push: the flag of the step that produced the row is required")
        if self.count:
            self.rows[0].copy_(self.rows[1])
            self.rows[1].copy_(self.rows[2])
            self.flags[0].copy_(self.flags[1])
            self.flags[1].copy_(ended.reshape(self.N))
        self.rows[2].copy_(obs.reshape(self.N, 16))
        self.count = min(self.count + 1, 3)
        R = self.count
        out = self.out[R - 1]
        stack_rows(self.rows[3 - R:], self.flags[3 - R:] if R > 1 else None, out=out)
        self.row.copy_(out[R - 1])   # (an allocation of its own: aligned for every N, as the act entry points want their rows)
        return self.row


class HostHistoryWindow:
    """HistoryWindow for ONE env on the host (Env(scan_history=True)): a three-row deque of 16-vectors and the flags between them,
    the rule applied through stack_rows_reference.  reset(row) / push(row, ended) return the 42-vector in the rows' dtype."""

    def __init__(self):
        import collections
        self.rows, self.flags = collections.deque(maxlen=3), collections.deque(maxlen=2)

    def reset(self, row):
        self.rows.clear()
        self.flags.clear()
        return self._row(row)

    def push(self, row, ended):
        if not self.rows:
            raise ValueError("HostHistoryWindow.push before reset")
        self.flags.append(bool(ended))
        return self._row(row)

    def _row(self, row):
        self.rows.append(np.array(row).reshape(16))
        obs = np.stack(self.rows)[:, None, :]
        flags = list(self.flags)[-(len(self.rows) - 1):] if len(self.rows) > 1 else None
        end = None if flags is None else np.array(flags, dtype=np.uint8).reshape(-1, 1)
        return stack_rows_reference(obs, end)[-1, 0]


class VecEnv:
    """N environments stepped by one kernel launch; tensors stay on the GPU.

    ``step(action)`` mirrors ``Env.step`` per env and the episode bookkeeping of
    ``PPO.rollout`` (ppo.py:543-593): past_action tracking, timeout after
    ``max_episode_steps``, and -- with ``auto_reset`` -- the reset, in which case the returned
    observation is the post-reset one (what ``rollout`` stores next, ppo.py:508,593).
    """

    def __init__(self, n_envs, map="stage_1", n_beams=10, max_episode_steps=500, auto_reset=True, is_training=True,
                 seed=0, env_id_base=0, per_env_map=False, map_seed=0, obs_f16=False, device=None, sampler=None,
                 lidar_below_min="clamp", lidar_noise_sigma=0.0, respawn_on_arrive=False, envs_per_workgroup=None, pair_cast=None,
                 movers=None, scan_pool=1):
        """movers: moving obstacles (NavSim.set_movers) -- a name of maps.movers_by_name ("orbit4"), a tape [P, M, 4], or a dict:
        tape=... or name=... (+ period=...), phase="random" (default: phase0[i] drawn from (map_seed, env_id_base + i) only, so
        the shards of a multi-GPU run and the single-GPU run give every global env the same phase) | "zero".
        A BANK of tapes, one scenario per env (NavSim.set_mover_bank, maps.resolve_movers): dict(bank=..., periods=..., rects=...,
        assign="random" (default: the tape id from the same hash) | "cycle" | [N] ids), "random:K" (dict(name="random:K", seed=...))
        or "bank:orbit4,patrol2,...".
        scan_pool: sector LiDAR (NavSim.set_scan_pool): k rays min-pooled into each of the 10 scan columns; 1 = off."""
        scan_pool = check_scan_pool(scan_pool, n_beams, per_env_map or (torch.is_tensor(map) and map.dim() == 3) or
                                    (not isinstance(map, str) and np.ndim(map) == 3))
        thr = 0.2 if is_training else 0.4  # environment_new.py:44-47
        # what a sibling env on the same world is built from (PPOTrainer's evaluation env: same map / beams / row type / sensor)
        self._world_args = dict(map=map, n_beams=n_beams, per_env_map=per_env_map, map_seed=map_seed, obs_f16=obs_f16,
                                sampler=sampler, lidar_below_min=lidar_below_min, lidar_noise_sigma=lidar_noise_sigma,
                                respawn_on_arrive=respawn_on_arrive, movers=movers)
        self.sim = NavSim(n_envs, n_beams=n_beams, max_episode_steps=max_episode_steps, auto_reset=auto_reset,
                          respawn_on_arrive=respawn_on_arrive, seed=seed, env_id_base=env_id_base, threshold_arrive=thr,
                          obs_f16=obs_f16, device=device, lidar_below_min=lidar_below_min,
                          lidar_noise_sigma=lidar_noise_sigma, envs_per_workgroup=envs_per_workgroup, pair_cast=pair_cast,
                          scan_pool=scan_pool)
        self.N, self.B, self.D, self.device = self.sim.N, self.sim.B, self.sim.D, self.sim.device
        self.threshold_arrive = thr
        self.use_vision = False
        if isinstance(map, str):
            seg = _maps.by_name(map)
            reset_rects, respawn_rects = _maps.goal_rects(map)
            self.sim.set_goal_rects(0, reset_rects)
            self.sim.set_goal_rects(1, respawn_rects)
        else:
            seg = map
        if per_env_map and not (torch.is_tensor(seg) and seg.dim() == 3) and np.ndim(seg) == 2:
            seg = _maps.replicate_per_env(seg, self.N, seed=map_seed)
        self.sim.set_map(seg)
        if sampler is not None:  # e.g. "stage1" / "small_house" (spawn_goal_sampler.py) or a (starts, goals, min, max) tuple
            if isinstance(sampler, str):
                sampler = _maps.spawn_tables(sampler)
            self.sim.set_spawn_sampler(*sampler)
        self.mover_bank = None   # the resolved bank of tapes, if the movers are one (assign_scenarios)
        self._mover_phase, self._map_seed, self._env_id_base = "random", map_seed, env_id_base
        if movers is not None:
            tape, phase = _maps.resolve_movers(movers)
            if isinstance(tape, _maps.MoverBank):   # one scenario per env: ids and phases from (map_seed, global env id) only
                self.mover_bank, self._mover_phase = tape, phase
                ids = tape.tape_ids(self.N, map_seed=map_seed, env_id_base=env_id_base)
                phase0 = None if phase == "zero" else _maps.mover_bank_phases(tape.periods[ids], map_seed=map_seed, env_id_base=env_id_base)
                self.sim.set_mover_bank(tape.bank, tape.periods, ids, phase0, tape.rects)
            else:
                phase0 = None if phase == "zero" else _maps.mover_phases(tape.shape[0], self.N, map_seed=map_seed, env_id_base=env_id_base)
                self.sim.set_movers(tape, phase0)
        self.io = self.sim.alloc_io()

    def close(self):
        self.sim.close()

    @property
    def scan_pool(self):
        """the handle's scan_pool as it stands (NavSim.set_scan_pool may have changed it since the constructor)"""
        return self.sim.scan_pool

    @property
    def world_args(self):
        """the constructor's world, with the handle's current scan_pool when it is on (off: the dict is what it was)"""
        w = dict(self._world_args)
        if self.sim.scan_pool != 1:
            w["scan_pool"] = self.sim.scan_pool
        return w

    def set_scan_pool(self, k):
        """NavSim.set_scan_pool on the env's handle; scan_pool and world_args follow it"""
        self.sim.set_scan_pool(k)

    def assign_scenarios(self, ids):
        """Gives every env another tape of the bank (NavSim.set_mover_assignment): ids [N] integers in [0, K), the phases redrawn by
        the constructor's rule -- maps.mover_bank_phases of the new tapes' periods from (map_seed, global env id), or none for
        phase="zero" -- so a shard still gives a global env what the single-GPU run gives it.  The envs keep their state; reset them
        before stepping on (PPOTrainer does: the handle's generation changed)."""
        if self.mover_bank is None:
            raise NavsimError("assign_scenarios: the env's movers are not a bank of tapes")
        K = len(self.mover_bank.periods)
        ids = np.asarray(ids.cpu() if torch.is_tensor(ids) else ids)
        if ids.shape != (self.N,) or not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= K:
            raise NavsimError(f"assign_scenarios: {self.N} tape ids in [0, {K})")
        ids = ids.astype(np.int32)
        phase0 = None if self._mover_phase == "zero" else _maps.mover_bank_phases(
            np.asarray(self.mover_bank.periods)[ids], map_seed=self._map_seed, env_id_base=self._env_id_base)
        self.sim.set_mover_assignment(ids, phase0)

    def reset(self, mask=None):
        return self.sim.reset(self.io.obs, mask)

    def step(self, action, io=None):
        """action: [N,2] float32 device tensor.  Returns (obs, reward, done, arrive); `ended`,
        `ep_return`, `ep_length` are in ``self.io`` (or the `io` passed in)."""
        io = io or self.io
        action = action.to(device=self.device, dtype=torch.float32).contiguous()
        self.sim.step(action, io.obs, io.reward, io.done, io.arrive, io.ended, io.ep_return, io.ep_length, ep_path=io.ep_path)
        return io.obs, io.reward, io.done, io.arrive


    def step_seq(self, actions):
        """A whole action tape in ONE launch (navsim_step_seq): actions [T, N, 2] float32 on the device.  Returns a namespace of
        [T, N, ...] tensors (obs after each step, reward, done, arrive, ended, ep_return, ep_length, ep_path); row t is what
        ``step(actions[t])`` would have produced.  For loops whose actions do not depend on the observations they produce."""
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        T, N, dev = int(actions.shape[0]), self.N, self.device
        out = types.SimpleNamespace(
            obs=torch.empty((T, N, self.sim.D), dtype=self.sim.obs_dtype, device=dev), reward=torch.empty((T, N), device=dev),
            done=torch.empty((T, N), dtype=torch.uint8, device=dev), arrive=torch.empty((T, N), dtype=torch.uint8, device=dev),
            ended=torch.empty((T, N), dtype=torch.uint8, device=dev), ep_return=torch.zeros((T, N), device=dev),
            ep_length=torch.zeros((T, N), dtype=torch.int32, device=dev), ep_path=torch.zeros((T, N), device=dev))
        self.sim.step_seq(actions, out.obs, out.reward, out.done, out.arrive, out.ended, out.ep_return, out.ep_length, out.ep_path)
        return out


    def rollout_mlp64(self, actor_params, n_steps, var, seed=0, step_base=0, obs0=None, history=False, hist_in=None, hist_out=None):
        """PPO.rollout's hot loop (ppo.py:505-594) for the (B + 6)-64-64 policy in ONE launch (navsim_rollout_mlp64): per step
        PPO.get_action (ppo.py:673-706) on the observation the previous step left on chip, then the env step.
        actor_params: flat float32 device tensor [5378] (10 beams) / [7042] (36 beams) in nn.Module.named_parameters order
        (include/navppo.h); var: exploration variance (float or device scalar); action noise = Philox(seed, global env id,
        step_base + t).  obs0 [N, B + 6]: the observations to start from (default: a fresh reset).  Returns a namespace: obs
        [T + 1, N, B + 6] (row 0 = obs0; float16 on an obs_f16 env), act [T, N, 2], logp / reward / done / arrive / ended /
        ep_return / ep_length / ep_path [T, N] -- bit-identical to T pairs of navppo_mlp64_act / step calls.
        history=True (10 beams): navsim_rollout_mlp64_hist -- actor_params is the [7042] 42-64-64 actor, which reads the scan-history
        row of every step (stack_rows_reference); every returned buffer keeps its shape, obs stays [T + 1, N, 16].
        hist_in / hist_out (history=True; [N, 22] float32, either may be None, both may be one tensor): navsim_rollout_mlp64_hist_cont
        -- obs0 continues the envs' episodes with the history carry hist_in (None: obs0 starts them), hist_out receives the carry of
        row T.  A rollout cut in pieces (obs0 = the previous piece's last row, step_base advanced, the carry handed on) writes the
        bits of the whole."""
        if self.B not in (10, 36):
            raise NavsimError("rollout_mlp64 needs 10 or 36 beams")
        if history and self.B != 10:
            raise NavsimError("rollout_mlp64(history=True) needs 10 beams: the history row stacks 10-beam scans")
        T, N, D, dev = int(n_steps), self.N, self.D, self.device
        n_actor = 64 * (HIST_DIM if history else D) + 64 + 64 * 64 + 64 + 2 * (64 + 1)
        cont = hist_in is not None or hist_out is not None
        if cont and not history:
            raise NavsimError("rollout_mlp64: hist_in / hist_out need history=True")
        _chk_carry("rollout_mlp64: hist_in", hist_in, N, dev)
        _chk_carry("rollout_mlp64: hist_out", hist_out, N, dev)
        entry = ("navsim_rollout_mlp64_hist_cont" if cont else "navsim_rollout_mlp64_hist") if history else "navsim_rollout_mlp64"
        prm = actor_params.to(device=dev, dtype=torch.float32).contiguous()
        if prm.numel() != n_actor or prm.data_ptr() % 16:
            raise NavsimError(f"actor_params: {n_actor} float32 values, 16-byte aligned")
        out = types.SimpleNamespace(
            obs=torch.empty((T + 1, N, D), dtype=self.sim.obs_dtype, device=dev), act=torch.empty((T, N, 2), device=dev),
            logp=torch.empty((T, N), device=dev),
            reward=torch.empty((T, N), device=dev), done=torch.empty((T, N), dtype=torch.uint8, device=dev),
            arrive=torch.empty((T, N), dtype=torch.uint8, device=dev), ended=torch.empty((T, N), dtype=torch.uint8, device=dev),
            ep_return=torch.zeros((T, N), device=dev), ep_length=torch.zeros((T, N), dtype=torch.int32, device=dev),
            ep_path=torch.zeros((T, N), device=dev))
        if obs0 is None:
            self.sim.reset(out.obs[0])
        else:
            out.obs[0].copy_(obs0)
        var_t = var if torch.is_tensor(var) else torch.tensor(float(var), device=dev)
        var_t = var_t.to(device=dev, dtype=torch.float32).reshape(())
        base_t = torch.tensor(int(step_base), dtype=torch.int32, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            check(getattr(lib(), entry)(self.sim._h, p(prm), p(out.obs), p(out.act), p(out.logp), p(out.reward), p(out.done),
                                        p(out.arrive), p(out.ended), p(out.ep_return), p(out.ep_length), p(out.ep_path), p(var_t),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, p(base_t), T, *((_ptr(hist_in), _ptr(hist_out)) if cont else ()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), entry)
            torch.cuda.current_stream().synchronize()   # var_t / base_t / prm may be temporaries of this call
        return out

    EVAL_POLICIES = {"mlp64x2": "navsim_evaluate_mlp64", "resmlp512": "navsim_evaluate_resmlp512"}

    def evaluate_policy(self, actor_params, quota, n_steps=None, policy="mlp64x2", fill=0, history=False):
        """The evaluation loop (main.py:135-252) in ONE launch (navsim_evaluate_mlp64 / navsim_evaluate_resmlp512): a fresh
        reset, then every env plays whole episodes back to back with the DETERMINISTIC action (the clamped mean of the actor,
        main.py:197-199) and records its first ``quota`` of them; a workgroup of 16 envs stops once all of its envs are done,
        at the latest after ``n_steps`` steps (default quota * max_episode_steps: always enough, every episode ends by its
        time-out).  actor_params: the flat float32 actor as for rollout_mlp64 (policy "mlp64x2") or the [50290] 512-wide one
        ("resmlp512", 10 beams).  Returns a namespace: flags [quota, N] uint8 (1 success, 2 collision, 4 timeout), length
        [quota, N] int32, ret / path [quota, N] float32, count [N] int32 (episodes recorded), steps [ceil(N / 16)] int32 (steps
        each workgroup executed); slots that were not reached hold ``fill``.  The env state afterwards is unspecified (the envs
        ran on past their quota): reset before stepping this env again.
        history=True (policy "mlp64x2", 10 beams): navsim_evaluate_mlp64_hist -- the [7042] 42-64-64 actor on scan-history rows."""
        if history and (policy != "mlp64x2" or self.B != 10):
            raise ValueError("evaluate_policy(history=True): the scan-history evaluation runs the 42-64-64 actor (policy 'mlp64x2') "
                             f"on 10 beams, not policy {policy!r} on {self.B} beams")
        if policy not in self.EVAL_POLICIES:
            raise ValueError(f"evaluate_policy: no evaluation kernel for policy {policy!r} (have {sorted(self.EVAL_POLICIES)})")
        if policy == "resmlp512" and self.B != 10:
            raise ValueError("evaluate_policy: the 512-wide actor reads 16-wide observations (10 beams): no evaluation kernel "
                             f"for {self.B} beams")
        if policy == "mlp64x2" and self.B not in (10, 36):
            raise ValueError(f"evaluate_policy: the (B + 6)-64-64 actor has evaluation kernels for 10 and 36 beams, not {self.B}")
        N, D, dev, sim = self.N, self.D, self.device, self.sim
        quota = int(quota)
        n_steps = quota * int(sim.cfg.max_episode_steps) if n_steps is None else int(n_steps)
        n_actor = 50290 if policy == "resmlp512" else 64 * (HIST_DIM if history else D) + 64 + 64 * 64 + 64 + 2 * (64 + 1)
        entry = "navsim_evaluate_mlp64_hist" if history else self.EVAL_POLICIES[policy]
        if not torch.is_tensor(actor_params):
            raise NavsimError("evaluate_policy: actor_params: expected a tensor")
        prm = actor_params.detach().to(device=dev, dtype=torch.float32).contiguous()
        if prm.numel() < n_actor or prm.data_ptr() % 16:
            raise NavsimError(f"evaluate_policy: actor_params: at least {n_actor} float32 values, 16-byte aligned")
        q = max(quota, 1)   # (quota < 1 is refused by the library, with its message)
        out = types.SimpleNamespace(
            flags=torch.full((q, N), int(fill), dtype=torch.uint8, device=dev),
            length=torch.full((q, N), int(fill), dtype=torch.int32, device=dev),
            ret=torch.full((q, N), float(fill), dtype=torch.float32, device=dev),
            path=torch.full((q, N), float(fill), dtype=torch.float32, device=dev),
            count=torch.zeros(N, dtype=torch.int32, device=dev),
            steps=torch.zeros((N + 15) // 16, dtype=torch.int32, device=dev))
        obs0 = torch.empty((N, D), dtype=sim.obs_dtype, device=dev)
        sim._chk("evaluate_policy: actor_params", prm, torch.float32, prm.numel())
        sim._chk("evaluate_policy: flags", out.flags, torch.uint8, q * N)
        sim._chk("evaluate_policy: length", out.length, torch.int32, q * N)
        sim._chk("evaluate_policy: ret", out.ret, torch.float32, q * N)
        sim._chk("evaluate_policy: path", out.path, torch.float32, q * N)
        sim.reset(obs0)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            check(getattr(lib(), entry)(
                sim._h, p(prm), p(obs0), quota, n_steps, p(out.flags), p(out.length), p(out.ret), p(out.path), p(out.count),
                p(out.steps), C.c_void_p(torch.cuda.current_stream().cuda_stream)), entry)
            if prm.data_ptr() != actor_params.data_ptr():
                torch.cuda.current_stream().synchronize()   # prm is a temporary of this call
        return out


class _XY:
    __slots__ = ("x", "y", "z")

    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = x, y, z


class _Pose:
    def __init__(self):
        self.position = _XY()


def resolve_env_movers(movers):
    """Env's ``movers`` argument -> (tape [P, M, 4] float32, phase offset in [0, P)): a name of maps.movers_by_name ("orbit4"), a tape
    [P, M, 4], or a dict tape=... | name=... (+ period=...) with phase=int (default 0: the one env's scans start at the tape's row 0
    after every reset, unlike VecEnv's hashed per-env offsets)."""
    spec = dict(movers) if isinstance(movers, dict) else ({"name": movers} if isinstance(movers, str) else {"tape": movers})
    phase = spec.pop("phase", 0)
    period = spec.pop("period", None)
    if sum(k in spec for k in ("tape", "name")) != 1 or len(spec) != 1:
        raise ValueError("movers: give a tape or a name (and, in a dict, period=... with a name, phase=int)")
    if "name" in spec:
        tape = _maps.movers_by_name(spec["name"], period)
    elif period is not None:
        raise ValueError("movers: period goes with a name (a tape has its own)")
    else:
        tape = spec["tape"]
    tape = tape.detach().cpu().numpy() if torch.is_tensor(tape) else np.asarray(tape)
    tape = np.ascontiguousarray(tape, dtype=np.float32)
    if tape.ndim != 3 or tape.shape[2] != 4 or tape.shape[0] < 1:
        raise ValueError(f"movers: a tape is [P, M, 4], got {tape.shape}")
    if isinstance(phase, (bool, str)) or not isinstance(phase, (int, np.integer)) or not 0 <= int(phase) < tape.shape[0]:
        raise ValueError(f"movers: phase must be an integer in [0, {tape.shape[0]}), got {phase!r}")
    return tape, int(phase)


class Env:
    """Single-env drop-in for the reference ``Env`` (environment_new.py:26-382).

    >>> env = Env(is_training=True)
    >>> obs = env.reset()                              # np.ndarray (16,) float64
    >>> obs, reward, done, arrive = env.step(action, past_action)

    Differences from the reference, all deliberate: the world is simulated on the GPU instead of
    Gazebo (so ``step`` does not block on a 5 Hz scan), goal sampling uses a seeded counter-based
    RNG instead of the unseeded global ``random``, and service failures raise instead of being
    swallowed.  The episode loop stays with the caller exactly as in ``PPO.rollout``: ``step`` never
    resets, and on arrival it re-spawns the goal like ``setReward`` does (environment_new.py:245-267).
    """

    def __init__(self, is_training, use_vision=False, vision_dim=64, map="stage_1", seed=0, device=None, movers=None,
                 scan_history=False, scan_pool=1):
        """movers: moving obstacles (an extension, NavSim.set_movers; resolve_env_movers: a scene name, a tape [P, M, 4] or
        dict(tape=... | name=..., phase=int)).  The scan of a step sees tape[(k + 1 + phase) mod P], k = the steps taken since the last
        reset(); the reset observation sees tape[phase].  None: the static world, exactly as without the keyword.
        scan_history: reset() / step() return the 42-vector of stack_rows_reference (the last three scans, cut where the step's
        `ended` flag -- collision or arrival here -- was set and at every reset()) instead of the 16-vector.  Host code only.
        scan_pool: sector LiDAR (NavSim.set_scan_pool): 10 k rays min-pooled into the 10 scan entries; 1 = off."""
        scan_pool = check_scan_pool(scan_pool)
        if use_vision:
            raise NotImplementedError("camera modality is outside the LiDAR hot path (SURVEY.md 2a)")
        if not isinstance(scan_history, bool):
            raise ValueError(f"scan_history {scan_history!r}: True or False")
        self.scan_history = scan_history
        self._hist = HostHistoryWindow() if scan_history else None
        self.use_vision = False
        self.vision_dim = vision_dim
        self.threshold_arrive = 0.2 if is_training else 0.4
        self._sim = NavSim(1, n_beams=10, max_episode_steps=0, auto_reset=False, respawn_on_arrive=True, seed=seed,
                           threshold_arrive=self.threshold_arrive, device=device, scan_pool=scan_pool)
        self.scan_pool = scan_pool
        if isinstance(map, str):
            seg = _maps.by_name(map)
            rr, rs = _maps.goal_rects(map)
            self._sim.set_goal_rects(0, rr)
            self._sim.set_goal_rects(1, rs)
        else:
            seg = map
        self._sim.set_map(seg)
        self.movers_phase0 = 0
        if movers is not None:
            tape, self.movers_phase0 = resolve_env_movers(movers)
            self._sim.set_movers(tape, np.full(1, self.movers_phase0, np.int32) if self.movers_phase0 else None)
        # One pinned (host-mapped, device-visible) block carries a step's inputs and outputs: the kernel reads the action pair
        # from it and stores observation, reward and flags into it, so a step is one launch + a poll of the block (_wait_results), no copies.
        self._pin = torch.zeros(48, dtype=torch.float32).pin_memory()
        self._pin_u8 = torch.zeros(16, dtype=torch.uint8).pin_memory()
        self._pin_np, self._pin_u8_np = self._pin.numpy(), self._pin_u8.numpy()
        self._pin_i32 = self._pin_np.view(np.int32)   # the same block as bit patterns (the "not delivered yet" marker below)
        self._act_t, self._past_t = self._pin[0:2].view(1, 2), self._pin[2:4].view(1, 2)
        self._obs_t, self._rew_t = self._pin[16:32].view(1, 16), self._pin[32:33]
        self._done_t, self._arrive_t, self._ended_t = self._pin_u8[0:1], self._pin_u8[1:2], self._pin_u8[2:3]
        self._state = None   # host copy of pose / goal / past_distance, fetched when an attribute is read
        # One env step from Python is launch-latency bound (kernel 6 us, the rest is the way there and back): the argument list of
        # navsim_step / navsim_reset is built ONCE -- ctypes pointers of the pinned block, the stream the env was created on -- so
        # that a step is one foreign call and one wait (building twelve c_void_p objects, looking up the current stream and
        # entering a device context per step were 5 of the 25 us).  The stream is therefore FROZEN at construction: an Env built
        # under torch.cuda.stream(s) launches on s for its whole life (as do its attribute reads, which wait on that stream).
        dev = self._sim.device
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._stream_obj = torch.cuda.current_stream(dev)
        st = C.c_void_p(self._stream_obj.cuda_stream)
        self._lib = lib()
        self._step_args = (self._sim._h, _ptr(self._act_t), _ptr(self._past_t), _ptr(self._obs_t), _ptr(self._rew_t), _ptr(self._done_t),
                           _ptr(self._arrive_t), _ptr(self._ended_t), None, None, None, st)
        self._reset_args = (self._sim._h, None, _ptr(self._obs_t), st)

    # -- attributes the reference's callers read (ppo.py:535, main.py:202; environment_new.py:29-41): fetched lazily, one
    #    navsim_get_state per step at most, and none at all for callers that never look
    def _st(self):
        if self._state is None:
            with torch.cuda.stream(self._stream_obj):   # the stream the steps were launched on (frozen at construction)
                self._state = self._sim.get_state()
        return self._state

    @property
    def position(self):
        p = self._st()["pose"][0]
        return _XY(float(p[0]), float(p[1]))

    @property
    def yaw_rad(self):
        return float(self._st()["pose"][0, 2])

    @property
    def goal_position(self):
        g = self._st()["goal"][0]
        pose = _Pose()
        pose.position.x, pose.position.y = float(g[0]), float(g[1])
        return pose

    @property
    def past_distance(self):
        return float(self._st()["past_dist"][0])

    @property
    def mover_phase(self):
        """the tape row the NEXT step's scan sees, (k + 1 + phase) mod P with k the steps since the last reset (None without movers)"""
        P = self._sim.movers_period
        return (int(self._st()["ep_step"][0]) + 1 + self.movers_phase0) % P if P else None

    def _wait(self):
        self._stream_obj.synchronize()

    # A step's results are waited for where they land.  The pinned block is host-coherent memory: the kernel's stores reach it while
    # the kernel runs, so the caller plants a bit pattern the kernel never writes in every output slot -- _PLANT, a quiet NaN with a
    # payload no arithmetic produces (a diverged policy's NaN observation or reward is the canonical 0x7fc00000 / a propagated
    # input payload, and is returned to the caller like the reference's Env.step returns it), 0xFF in the flags -- and polls until
    # all of them are gone, each slot checked for itself, no assumption on the order the stores arrive in.
    # Measured (tools/time_env_n1_parts.py): launch + stream.synchronize() 23.5 us, launch + this 14.1 us.
    # A step that has not delivered after _POLLS polls (a stalled queue, a fault) falls back to the stream wait, which reports it.
    # The poll returns when the RESULTS have landed, which can be before the kernel has retired: later readers of the handle's
    # device state are ordered behind it by the stream (get_state and every other call run on the stream the Env was built on).
    _POLLS = 1 << 20
    _PLANT = np.int32(0x7FC0DEAD)

    def _plant(self):
        self._pin_i32[16:33] = self._PLANT
        self._pin_u8_np[0:3] = 255

    def _wait_results(self, obs_only=False):
        pin, u8, plant = self._pin_i32, self._pin_u8_np, self._PLANT
        for _ in range(self._POLLS):
            if pin[31] != plant and (obs_only or (pin[32] != plant and u8[0] != 255 and u8[1] != 255 and u8[2] != 255)) \
                    and not (pin[16:32] == plant).any():
                return
        self._wait()
        if (pin[16:32] == plant).any() or (not obs_only and (pin[32] == plant or (u8[0:3] == 255).any())):
            raise RuntimeError("the launch finished without delivering its results to the pinned block")

    def _call(self, fn, args, what):
        if args is None:
            raise NavsimError(f"{what}: the env is closed")
        if torch.cuda.current_device() == self._dev_index:
            check(fn(*args), what)
        else:
            with torch.cuda.device(self._dev_index):
                check(fn(*args), what)

    def reset(self):
        self._pin_i32[16:32] = self._PLANT
        self._call(self._lib.navsim_reset, self._reset_args, "navsim_reset")
        self._wait_results(obs_only=True)
        self._state = None
        if self._hist is not None:
            return self._hist.reset(self._pin_np[16:32]).astype(np.float64)
        return self._pin_np[16:32].astype(np.float64)

    def step(self, action, past_action):
        a = np.asarray(action, dtype=np.float32).reshape(-1)
        p = np.asarray(past_action, dtype=np.float32).reshape(-1)
        if a.shape[0] < 2 or p.shape[0] < 2:
            raise IndexError("action and past_action need two components")  # as action[1] would in the reference
        self._pin_np[0:2] = a[:2]
        self._pin_np[2:4] = p[:2]
        self._plant()
        self._call(self._lib.navsim_step, self._step_args, "navsim_step")
        self._wait_results()
        self._state = None
        if self._hist is not None:
            return (self._hist.push(self._pin_np[16:32], self._pin_u8_np[2]).astype(np.float64), float(self._pin_np[32]),
                    bool(self._pin_u8_np[0]), bool(self._pin_u8_np[1]))
        return (self._pin_np[16:32].astype(np.float64), float(self._pin_np[32]), bool(self._pin_u8_np[0]),
                bool(self._pin_u8_np[1]))

    def getLatestImage(self):
        return None

    def close(self):
        self._step_args = self._reset_args = None   # they hold the native handle: a step after close() raises instead of using it
        self._sim.close()
