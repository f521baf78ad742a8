"""Moving obstacles off the beaten path of tests/test_gpu_movers.py: every packing of the mover pass (64 .. 1 envs per 64-lane pass,
non-power-of-two M inside a packed pass), ragged and tiny workgroups, the sensor options (the MOV kernels are always the SENS
instantiation), float16 rows, a tripwire on both ends of the tape, shards (env_id_base), and the small contracts that the docstring
of NavSim.set_movers states: one NaN coordinate makes a segment absent, the tape is borrowed, a second set_movers replaces the first.

Nothing here has a tolerance of its own.  Both sides HIP kernels: torch.equal / bit patterns.  Against the oracle on per-step
composed maps (tests/_movers.py): flags exact and observations at OBS_ATOL through test_gpu_parity._lockstep, and the share of
bit-exact rows only where the sensor noise is off (the device's and glibc's logf / sinf may differ in the last ulp)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _movers import (RANGE_MIN, MoverOracle, below_min_poses, blade_tape, compose, embed_with_tripwires, partial_nan_tape)
from navbot_ppo_amd import maps
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, VecEnv
from oracle import navsim_oracle as O
from test_gpu_movers import (CAP_LOCK, R_NEAR, T_LOCK, _gpu, _phase0, _rollouts_equal, _seq_equals_steps, _tape, _vs_static_kernels,
                              bits)
from test_gpu_parity import OBS_ATOL, _actions, _lockstep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SENS = dict(lidar_noise_sigma=0.01, lidar_below_min="gazebo")
NOISE, GAZEBO = dict(lidar_noise_sigma=0.01), dict(lidar_below_min="gazebo")


def P_(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _acts(N):
    return _actions(np.random.default_rng(31), T_LOCK, N)


def _oracle(N, map_name, tape, ph0, **kw):
    cpu = MoverOracle(N, maps.by_name(map_name), tape, ph0, **kw)
    rr, rs = maps.goal_rects(map_name)
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    return cpu


@functools.lru_cache(maxsize=None)
def _static_done(map_name, N, opts=()):
    """collisions of the lock-step actions on the static map alone, on the oracle (once per case)"""
    s = O.OracleSim(N, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5, **dict(opts))
    s.set_map(maps.by_name(map_name))
    rr, rs = maps.goal_rects(map_name)
    s.set_goal_rects(0, rr)
    s.set_goal_rects(1, rs)
    s.reset()
    return sum(int(s.step(a)["done"].sum()) for a in _acts(N))


def _lock(map_name, N, P, M, watch=False, **kw):
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    gpu = _gpu(N, map_name, tape, ph0, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5, **kw)
    inf = gpu.info()
    assert (inf["step_epb"], inf["step_waves"], inf["step_cast"]) == (16, 8, 3 if map_name == "stage_2" else 0), inf
    cpu = _oracle(N, map_name, tape, ph0, watch=watch, max_episode_steps=CAP_LOCK, seed=5, **kw)
    st = _lockstep(gpu, cpu, _acts(N))   # flags exact, observations 1e-6, state as the static lock-step tests
    gpu.close()
    static = _static_done(map_name, N, tuple(sorted(kw.items())))
    print(f"{map_name} N={N} P={P} M={M} {kw}: done {st['done']} (static map {static}) ended {st['ended']} "
          f"exact rows {st['exact_obs']}/{st['total']}" + (f" tape in sight in {sum(cpu.seen)} of {len(cpu.seen)} steps" if watch else ""))
    return st, static, cpu


# ---------------------------------------------------------------- 1. every packing, ragged and tiny workgroups
# envs per 64-lane mover pass = 64 >> log2(pow2ceil(M)): M = 2 -> 32, 3 -> 16, 5 and 8 -> 8, 9 and 16 -> 4, 17 and 31 -> 2, 33 and
# 63 -> 1; all but 2, 8 and 16 leave idle lanes between the envs of a pass.  N = 37: two full 16-env workgroups and one of 5.
# (The oracle alone, these actions: 60 to 70 collisions per case against 0 on the static map.)
PACK_CASES = [("stage_1", M) for M in (2, 3, 5, 8, 9, 16, 17, 31, 33, 63)] + [("stage_2", M) for M in (3, 9, 33)]


@pytest.mark.parametrize("map_name,M", PACK_CASES)
def test_lockstep_at_every_packing(map_name, M):
    st, static, _ = _lock(map_name, 37, 7, M)
    assert st["exact_obs"] > 0.99 * st["total"]
    assert st["done"] >= 10            # the movers end episodes ...
    assert st["done"] != static        # ... that the static map does not
    _lock_case_through_step_seq(map_name, 37, M)


@pytest.mark.parametrize("M", [1, 3, 17, 64])
@pytest.mark.parametrize("N", [1, 5, 17])
def test_lockstep_in_workgroups_smaller_than_a_pass(N, M):
    """fewer envs than one mover pass covers: the clamp of the pass's env index.  (The oracle alone: N = 1: 4 collisions, N = 5: 7
    to 9, N = 17: 17 to 29, the static map 0; a tape segment in some env's scan in 44 of 60 steps at N = 1, M = 1, in all 60 else.)"""
    st, static, cpu = _lock("stage_1", N, 7, M, watch=True)
    assert st["exact_obs"] > 0.99 * st["total"]
    assert st["done"] >= 1 and st["done"] != static
    assert sum(cpu.seen) >= T_LOCK // 2   # the composed scans are not the static map's
    _lock_case_through_step_seq("stage_1", N, M)


def _lock_case_through_step_seq(map_name, N, M):
    """... and the persistent form of the same case (steps_mov_kernel stages phase0 of each workgroup's envs in LDS): one
    navsim_step_seq launch over the lock-step actions against the step launches the oracle has just vouched for, bit for bit"""
    _seq_equals_steps(map_name, 7, M, N=N, T=T_LOCK, cap=CAP_LOCK, radius=0.75, acts=_acts(N), seed=5)


# ---------------------------------------------------------------- 2. sensor options with a tape
@pytest.mark.parametrize("map_name,M,opts", [(m, M, SENS) for m in ("stage_1", "stage_2") for M in (5, 32, 64)] +
                         [("stage_1", 5, NOISE), ("stage_1", 5, GAZEBO)], ids=lambda v: "-".join(v) if isinstance(v, dict) else str(v))
def test_lockstep_with_sensor_options(map_name, M, opts):
    """(The oracle alone: 62 to 74 collisions per case against 0 on the static map, 48 to 74 -inf readings where gazebo is set.)"""
    st, static, _ = _lock(map_name, 40, 7, M, **opts)
    assert st["done"] >= 10 and st["done"] != static
    if "lidar_noise_sigma" not in opts:
        assert st["exact_obs"] > 0.99 * st["total"]


@pytest.mark.parametrize("map_name,P,M", [("stage_1", 7, 5), ("stage_1", 40, 37), ("stage_2", 7, 64)])
def test_sensor_options_bit_identical_to_the_static_kernels(map_name, P, M):
    _vs_static_kernels(map_name, P, M, **SENS)


@pytest.mark.parametrize("M", [5, 64])
def test_below_range_reading_from_a_tape_segment(M):
    """Every env looks nose-first at a blade of the phase its next step casts from 7 cm: the beams beside straight ahead read -inf
    (Gazebo's ray sensor below range_min) and the collision rule does not fire -- as the static test has it for the inner wall."""
    N, P = 40, 7
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    gpu = _gpu(N, "stage_1", tape, ph0, seed=3, **SENS)
    cpu = _oracle(N, "stage_1", tape, ph0, seed=3, **SENS)
    io = gpu.alloc_io()
    gpu.reset(io.obs)
    cpu.reset()
    pose = below_min_poses(tape, cpu.step_phases())
    for s in (gpu, cpu):
        s.set_state(pose=pose, goal=np.full((N, 2), 3.0), past_dist=np.full(N, 3.0))
    a = np.zeros((N, 2), np.float32)
    gpu.step(torch.from_numpy(a).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
    out = cpu.step(a, auto_reset=False)
    og = io.obs.cpu().numpy()
    low = np.isneginf(out["obs"][:, :10])
    assert low.any(axis=1).mean() >= 0.5                                      # from a tape segment: the static map alone ...
    assert all((O.raycast(maps.stage_1(), *p) > RANGE_MIN).all() for p in pose)   # ... reads nothing under range_min there
    np.testing.assert_array_equal(np.isneginf(og), np.isneginf(out["obs"]))
    fin = np.isfinite(out["obs"])
    np.testing.assert_allclose(og[fin], out["obs"][fin], rtol=0, atol=OBS_ATOL)
    np.testing.assert_array_equal(io.done.cpu().numpy(), out["done"])
    assert not io.done.cpu().numpy()[low.any(axis=1)].any()
    gpu.close()


@pytest.mark.parametrize("map_name,P,M", [("stage_1", 7, 32), ("stage_2", 40, 64)])
def test_step_seq_equals_step_launches_with_sensor_options(map_name, P, M):
    _seq_equals_steps(map_name, P, M, **SENS)


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
@pytest.mark.parametrize("map_name", ["stage_1", "stage_2"])
def test_persistent_rollout_equals_per_step_rollout_with_sensor_options(policy, map_name):
    _rollouts_equal(policy, map_name, **SENS)


# ---------------------------------------------------------------- 3. float16 rows with a tape
F16_OPTS = [dict(obs_f16=True), dict(obs_f16=True, **SENS)]
_f16_id = lambda v: ("f16-sens" if "lidar_below_min" in v else "f16") if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("map_name,P,M,opts", [("stage_1", 7, 32, F16_OPTS[0]), ("stage_2", 7, 5, F16_OPTS[0]), ("stage_1", 40, 37, F16_OPTS[1])],
                         ids=_f16_id)
def test_f16_rows_bit_identical_to_the_static_kernels(map_name, P, M, opts):
    _vs_static_kernels(map_name, P, M, **opts)


@pytest.mark.parametrize("map_name,P,M,opts", [("stage_1", 7, 32, F16_OPTS[0]), ("stage_2", 40, 64, F16_OPTS[1])], ids=_f16_id)
def test_f16_rows_step_seq_equals_step_launches(map_name, P, M, opts):
    _seq_equals_steps(map_name, P, M, **opts)


@pytest.mark.parametrize("policy,map_name,opts", [("mlp64x2", "stage_1", F16_OPTS[0]), ("resmlp512", "stage_1", F16_OPTS[0]),
                                                  ("mlp64x2", "stage_2", F16_OPTS[1]), ("resmlp512", "stage_2", F16_OPTS[1])], ids=_f16_id)
def test_f16_rows_persistent_rollout_equals_per_step_rollout(policy, map_name, opts):
    _rollouts_equal(policy, map_name, **opts)


# ---------------------------------------------------------------- 4. a tripwire on both ends of the tape
def _every_entry_point(tape_t, N, P, ph0, flats):
    """reset, 10 steps, a step_seq, a ray cast and both persistent rollouts on a handle that borrows `tape_t`; every output"""
    T, cap = 12, 9
    s = NavSim(N, max_episode_steps=cap, auto_reset=True, seed=6, device=DEV)
    rr, rs = maps.goal_rects("stage_1")
    s.set_goal_rects(0, rr)
    s.set_goal_rects(1, rs)
    s.set_map(maps.stage_1())
    s.set_movers(tape_t, ph0)
    assert s._mov_tape.data_ptr() == tape_t.data_ptr()   # borrowed where it lies, not copied
    io = s.alloc_io()
    out = [s.reset(io.obs).clone()]
    k = np.zeros(N, np.int32)
    k[N // 2:] = P - 1                                   # phase0 0 and P - 1 at step counter 0 and at P - 1: both ends of the tape are
    s.set_state(ep_step=k)                               # the current phase of some env, and the next one of another
    out.append(s.raycast(torch.zeros((N, 3), dtype=torch.float64)))
    acts = torch.from_numpy(_actions(np.random.default_rng(52), 10 + T, N)).to(DEV)
    for t in range(10):
        s.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
        out += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.ended.clone()]
    z = lambda dt=torch.float32, *sh: torch.zeros((T, N) + sh, dtype=dt, device=DEV)
    seq = [z(torch.float32, 16), z(), z(torch.uint8), z(torch.uint8), z(torch.uint8)]
    s.step_seq(acts[10:], *seq)
    out += seq
    out.append(s.raycast(torch.from_numpy(np.tile([0.1, 0.05, 0.4], (N, 1)))))
    var = torch.tensor([0.5], device=DEV)
    for entry, flat in zip(("navsim_rollout_mlp64", "navsim_rollout_resmlp512"), flats):
        ob = torch.zeros((T + 1, N, 16), device=DEV)
        s.reset(ob[0])
        act, lp, rw = torch.zeros((T, N, 2), device=DEV), z(), z()
        fl = [z(torch.uint8) for _ in range(3)]
        rc = getattr(lib(), entry)(s._h, P_(flat), P_(ob), P_(act), P_(lp), P_(rw), *[P_(f) for f in fl], None, None, None, P_(var), 9, None,
                                   T, _st())
        assert rc == 0, lib().navsim_last_error().decode()
        out += [ob, act, lp, rw] + fl
    torch.cuda.synchronize()
    s.close()
    return out


@pytest.mark.parametrize("M", [5, 37])
def test_tripwires_around_the_tape_are_never_cast(M):
    """The tape as rows 1..P of a [P + 2, M, 4] tensor whose rows 0 and P + 1 are a wall 0.3 m around the spawn pose (a read of a
    neighbouring row changes scans; NaN poison would be culled), against a plain copy of the tape: every output bit-identical."""
    from test_gpu_evaluate import _actor
    N, P = 40, 7
    tape = _tape(P, M, R_NEAR)
    ph0 = (np.arange(N) % P).astype(np.int32)
    ph0[:4] = [0, P - 1, P - 1, 0]
    flats = [_actor(pol, 16)[1] for pol in ("mlp64x2", "resmlp512")]
    whole = torch.from_numpy(embed_with_tripwires(tape)).to(DEV)
    inner = whole[1:P + 1]
    assert inner.is_contiguous() and inner.data_ptr() % 16 == 0 and inner.data_ptr() == whole.data_ptr() + 16 * tape.shape[1]
    got = _every_entry_point(inner, N, P, ph0, flats)
    want = _every_entry_point(torch.from_numpy(tape).to(DEV), N, P, ph0, flats)
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(bits(x), bits(y)), i
    # ... and a handle that does read the wall sees it: the tripwire rows as the tape of phase 0 change the reset scan
    wired = _gpu(N, "stage_1", whole[:1].contiguous(), None)
    obs = wired.reset(wired.alloc_io().obs)
    assert bool((obs[:, :10] != want[0][:, :10]).all())
    wired.close()


# ---------------------------------------------------------------- 5. shards
def test_shards_reproduce_the_whole():
    """phase0 is indexed by the handle's local env, maps.mover_phases hashes the global id, the noise streams key on env_id_base + i:
    two shards (24 envs from 0, 16 from 24) reproduce one handle of 40, per step and in one persistent rollout."""
    from test_gpu_evaluate import _actor
    N, T, TR, cap, cut = 40, 30, 24, 9, 24
    flat = _actor("mlp64x2", 16)[1]
    kw = dict(map="stage_1", max_episode_steps=cap, movers=dict(tape=_tape(7, 32, R_NEAR), phase="random"), map_seed=5, seed=3,
              lidar_noise_sigma=0.01)
    acts = torch.from_numpy(_actions(np.random.default_rng(53), T, N)).to(DEV)

    def run(n, base, sl):
        env = VecEnv(n, env_id_base=base, **kw)
        rows = [env.reset().clone()]
        for t in range(T):
            env.step(acts[t, sl].contiguous())
            rows.append(torch.cat([bits(env.io.obs), bits(env.io.reward)[:, None], env.io.done[:, None].int(), env.io.arrive[:, None].int(),
                                   env.io.ended[:, None].int()], 1))
        r = env.rollout_mlp64(flat, TR, 0.5, seed=7, step_base=11)
        roll = [r.obs, r.act, r.logp, r.reward, r.done, r.arrive, r.ended]
        ph = env.sim._mov_phase0.clone()
        ended = int(torch.stack([x[:, -1] for x in rows[1:]]).sum()), int(torch.stack([x[:, -3] for x in rows[1:]]).sum())
        env.close()
        return rows, roll, ph, ended

    rows, roll, ph, (ended, done) = run(N, 0, slice(0, N))
    assert ended > 2 * N and done > 0 and len(set(ph.tolist())) > 3
    ra, la, pa, _ = run(cut, 0, slice(0, cut))
    rb, lb, pb, _ = run(N - cut, cut, slice(cut, N))
    assert torch.equal(ph, torch.cat([pa, pb]))
    for t, (w, a, b) in enumerate(zip(rows, ra, rb)):
        assert torch.equal(bits(w), torch.cat([bits(a), bits(b)])), t
    for w, a, b in zip(roll, la, lb):   # [T, N, ...]: the shards side by side along the env axis
        assert torch.equal(bits(w), torch.cat([bits(a), bits(b)], 1))
    assert int(roll[6].sum()) > 2 * N


# ---------------------------------------------------------------- 6. small contracts
def test_one_nan_coordinate_makes_a_segment_absent():
    """Four segments per phase with exactly one NaN coordinate, one per position, where a wall 0.25 m ahead of the spawn pose would
    stand: the spawn table (raycast_kernel), the step's cull (a sum test), navsim_raycast and the oracle (comparisons) agree that
    they are not there -- the handle behaves as one on the tape without them, and as the oracle on the composed map WITH them."""
    N, P, M, T = 40, 7, 12, 30
    tape, whole = partial_nan_tape(P, M)
    plain = blade_tape(P, M - 4)
    ph0 = _phase0(P, M, N)
    acts = _actions(np.random.default_rng(54), T, N)
    outs = []
    for tp in (tape, plain, whole):
        g = _gpu(N, "stage_1", tp, ph0, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5)
        io = g.alloc_io()
        rows = [g.reset(io.obs).clone(), g.raycast(torch.zeros((N, 3), dtype=torch.float64))]
        for t in range(T):
            g.step(torch.from_numpy(acts[t]).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
            rows += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.ended.clone()]
        rows.append(g.raycast(torch.from_numpy(np.tile([0.0, 0.0, 0.3], (N, 1)))))
        outs.append(rows)
        g.close()
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(outs[0], outs[1]))
    # placed where they would be hit: with the NaN coordinates restored the wall is in the reset scan of every env
    assert bool((outs[2][0][:, :10] != outs[0][0][:, :10]).any(dim=1).all())
    gpu = _gpu(N, "stage_1", tape, ph0, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5)
    st = _lockstep(gpu, _oracle(N, "stage_1", tape, ph0, max_episode_steps=CAP_LOCK, seed=5), acts)
    gpu.close()
    assert st["exact_obs"] > 0.99 * st["total"] and st["done"] >= 10
    segs = compose(maps.stage_1(), tape, ph0 % P)
    want = np.stack([O.raycast(segs[i], 0.0, 0.0, 0.0) for i in range(N)])
    got = outs[0][1].cpu().numpy()
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    np.testing.assert_allclose(got[np.isfinite(want)], want[np.isfinite(want)], rtol=0, atol=OBS_ATOL)


def _drive(g, acts, io=None):
    io = io or g.alloc_io()
    rows = []
    for a in acts:
        g.step(a, io.obs, io.reward, io.done, io.arrive, io.ended)
        rows += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.arrive.clone(), io.ended.clone()]
    return rows


def test_in_place_edit_of_the_tape_is_seen_by_the_next_step():
    """The tape is borrowed: after 5 steps every phase but the reset phases tape[phase0[i]] is overwritten in place with blades on
    another radius, and the next 5 steps equal those of a fresh handle on the edited tape brought to the same state."""
    N, P, M, cap = 40, 7, 32, 4
    ph0 = np.where(np.arange(N) % 2 == 0, 0, 3).astype(np.int32)   # the reset phases: 0 and 3
    t0, t1 = _tape(P, M, R_NEAR), _tape(P, M, 0.3)
    t1[[0, 3]] = t0[[0, 3]]
    acts = torch.from_numpy(_actions(np.random.default_rng(55), 10, N)).to(DEV)
    tape_t = torch.from_numpy(t0).to(DEV)
    a = _gpu(N, "stage_1", tape_t, ph0, max_episode_steps=cap, auto_reset=True, seed=7)
    assert a._mov_tape.data_ptr() == tape_t.data_ptr()
    ia = a.alloc_io()
    a.reset(ia.obs)
    first = _drive(a, acts[:5], ia)
    tape_t[...] = torch.from_numpy(t1).to(DEV)
    st = a.get_state()
    got = _drive(a, acts[5:], ia)
    b = _gpu(N, "stage_1", t1, ph0, max_episode_steps=cap, auto_reset=True, seed=7)
    ib = b.alloc_io()
    b.reset(ib.obs)
    b.set_state(**st)
    want = _drive(b, acts[5:], ib)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, want))
    assert sum(int(r.sum()) for r in got[4::5]) >= N                    # every env resets (into an unchanged phase) after the edit
    # the edit matters: the unedited tape from the same state gives other scans
    c = _gpu(N, "stage_1", t0, ph0, max_episode_steps=cap, auto_reset=True, seed=7)
    ic = c.alloc_io()
    c.reset(ic.obs)
    c.set_state(**st)
    other = _drive(c, acts[5:], ic)
    assert not all(torch.equal(x, y) for x, y in zip(got[0::5], other[0::5]))
    for g in (a, b, c):
        g.close()
    assert len(first) == 25


def test_a_second_set_movers_replaces_the_first():
    """set_movers(tape_a, phase0), set_movers(tape_b) with another (P, M) and no phase0 (the phase copy is freed, the spawn tables go
    from [N][K][B] back to [K][B]), set_movers(tape_a, phase0) again: after each call the handle is a fresh handle with that tape."""
    N, T, cap = 40, 20, 9
    tape_a, ph_a, tape_b = _tape(7, 37, R_NEAR), _phase0(7, 37, N), _tape(3, 5, 0.6)
    acts = torch.from_numpy(_actions(np.random.default_rng(56), T, N)).to(DEV)

    def play(g):
        io = g.alloc_io()
        return [g.reset(io.obs).clone()] + _drive(g, acts, io)

    fresh = {}
    for key, (tp, ph) in dict(a=(tape_a, ph_a), b=(tape_b, None)).items():
        g = _gpu(N, "stage_1", tp, ph, max_episode_steps=cap, auto_reset=True, seed=8)
        fresh[key] = (play(g), g.info(), (g.movers_period, g.movers_segments))
        g.close()
    assert not torch.equal(fresh["a"][0][0], fresh["b"][0][0])
    g = _gpu(N, "stage_1", max_episode_steps=cap, auto_reset=True, seed=8)
    for key, (tp, ph) in (("a", (tape_a, ph_a)), ("b", (tape_b, None)), ("a", (tape_a, ph_a))):
        g.set_movers(tp, ph)
        g.set_state(rng_ctr=np.zeros(N, np.uint32))   # the goal stream of a fresh handle
        rows, inf, pm = fresh[key]
        assert (g.movers_period, g.movers_segments) == pm and g.info() == inf
        assert all(torch.equal(x, y) for x, y in zip(play(g), rows)), key
    g.close()
