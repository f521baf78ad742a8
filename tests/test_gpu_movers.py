"""Moving obstacles (navsim_set_movers): a periodic segment tape cast beside the static map by every step kernel.

The scan of a step must equal, bit for bit, the scan of a static map that holds the static segments plus the tape phase the rule
prescribes -- so every check here has an exact reference that already exists: the oracle on a per-env map composed per step
(tests/_movers.py), the static kernels on such a map, and the per-step entry points for the persistent forms."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _movers import MoverOracle, blade_tape, blade_tape_m1, compose
from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import NavSim, NavsimError, VecEnv
from oracle import navsim_oracle as O
from test_gpu_parity import _actions, _lockstep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_LOCK, T_LOCK, CAP_LOCK = 40, 60, 25   # two full 16-env workgroups and a ragged one


def _phase0(P, M, N):
    return np.random.default_rng(1000 * P + M).integers(0, P, N).astype(np.int32)


def _tape(P, M, radius=0.75):
    """the tape of case (P, M): M = 37 is padded to 40 rows with NaN segments"""
    return blade_tape(P, M, pad_to=40 if M == 37 else None, radius=radius)


# The persistent-form tests cap an episode at 9 steps (0.45 m of travel at most): their blades turn 0.45 m from the spawn pose, so
# that a robot driving straight reaches them inside an episode (0.22 m to go before a reading drops under 0.2 m) while the reset scan
# (0.42 m) stays clear.  With the 0.75 m circle of the other tests no mover could end an episode there.
R_NEAR = 0.45


def _gpu(N, map_name, tape=None, phase0=None, **kw):
    g = NavSim(N, device=DEV, **kw)
    rr, rs = maps.goal_rects(map_name)
    g.set_goal_rects(0, rr)
    g.set_goal_rects(1, rs)
    g.set_map(maps.by_name(map_name))
    if tape is not None:
        g.set_movers(tape, phase0)
    return g


@functools.lru_cache(maxsize=None)
def _lock_actions(map_name):
    return _actions(np.random.default_rng(31), T_LOCK, N_LOCK)


@functools.lru_cache(maxsize=None)
def _static_done(map_name):
    """collisions of the lock-step actions on the static map alone (the GPU's own count, once per map)"""
    g = _gpu(N_LOCK, map_name, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5)
    io = g.alloc_io()
    g.reset(io.obs)
    n = 0
    for a in _lock_actions(map_name):
        g.step(torch.from_numpy(a).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
        n += int(io.done.sum())
    g.close()
    return n


# ---------------------------------------------------------------- 1. lock step against the composed-map oracle
@pytest.mark.parametrize("M", [1, 32, 37, 64])
@pytest.mark.parametrize("P", [1, 7, 40])
@pytest.mark.parametrize("map_name", ["stage_1", "stage_4", "stage_2"])   # 32 segments (several envs per pass), 64 (one tile), 128 (tile boxes)
def test_lockstep_against_the_composed_oracle(map_name, P, M):
    tape, ph0 = _tape(P, M), _phase0(P, M, N_LOCK)
    gpu = _gpu(N_LOCK, map_name, tape, ph0, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5)
    inf = gpu.info()
    assert (inf["step_epb"], inf["step_waves"], inf["step_cast"]) == (16, 8, 3 if map_name == "stage_2" else 0), inf
    assert gpu.movers_period == P and gpu.movers_segments == tape.shape[1]
    cpu = MoverOracle(N_LOCK, maps.by_name(map_name), tape, ph0, max_episode_steps=CAP_LOCK, seed=5)
    rr, rs = maps.goal_rects(map_name)
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    st = _lockstep(gpu, cpu, _lock_actions(map_name))   # flags exact, observations 1e-6, state as the static lock-step tests
    gpu.close()
    static = _static_done(map_name)
    print(f"{map_name} P={P} M={M}: done {st['done']} (static map {static}) ended {st['ended']} exact rows {st['exact_obs']}/{st['total']}")
    assert st["exact_obs"] > 0.99 * st["total"]
    assert st["done"] >= 10            # the movers end episodes ...
    assert st["done"] != static        # ... that the static map does not


# ---------------------------------------------------------------- 2. bit identity against the static kernels
def bits(x):
    """float tensors as bit patterns (the NaN log-prob of a -inf reading compares equal to itself)"""
    return x.view({4: torch.int32, 2: torch.int16}[x.element_size()]) if x.is_floating_point() else x


def _vs_static_kernels(map_name, P, M, **kw):
    """MOV path against a second handle (same options kw: the static per-env kernel) whose per-env map is rewritten from the host
    before every step"""
    N, T = 40, 30
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    static = maps.by_name(map_name)
    a = _gpu(N, map_name, tape, ph0, seed=9, **kw)
    b = NavSim(N, device=DEV, seed=9, **kw)
    rr, rs = maps.goal_rects(map_name)
    b.set_goal_rects(0, rr)
    b.set_goal_rects(1, rs)
    seg_b = torch.from_numpy(compose(static, tape, ph0 % P)).to(DEV)
    b.set_map(seg_b, per_env=True)   # borrowed: rewritten in place below
    assert b._seg.data_ptr() == seg_b.data_ptr()
    ia, ib = a.alloc_io(), b.alloc_io()
    assert torch.equal(a.reset(ia.obs), b.reset(ib.obs))
    acts = _actions(np.random.default_rng(41), T, N)
    hits = 0
    for t in range(T):   # no auto-reset, no time-out: every env's step counter is t
        seg_b.copy_(torch.from_numpy(compose(static, tape, (t + 1 + ph0) % P)))
        act = torch.from_numpy(acts[t]).to(DEV)
        a.step(act, ia.obs, ia.reward, ia.done, ia.arrive, ia.ended)
        b.step(act, ib.obs, ib.reward, ib.done, ib.arrive, ib.ended)
        for k in ("obs", "reward", "done", "arrive", "ended"):
            assert torch.equal(bits(getattr(ia, k)), bits(getattr(ib, k))), (k, t)
        hits += int(ia.done.sum())
    assert hits > 0
    a.close()
    b.close()


@pytest.mark.parametrize("map_name,P,M", [("stage_1", 7, 32), ("stage_1", 40, 37), ("stage_4", 7, 64), ("stage_2", 40, 32), ("stage_2", 1, 1)])
def test_bit_identical_to_the_static_kernels_on_the_composed_map(map_name, P, M):
    _vs_static_kernels(map_name, P, M)


# ---------------------------------------------------------------- 3. phase arithmetic
@pytest.mark.parametrize("P,M,k0", [pytest.param(7, 32, "P-1", id="P-1"), pytest.param(7, 32, "P", id="P"),
                                    pytest.param(7, 32, "2**20+3", id="2**20+3"), pytest.param(7, 32, "2**30-2", id="2**30-2"),
                                    pytest.param(65536, 1, "P-1", id="P65536-P-1"), pytest.param(65536, 1, "2**30-2", id="P65536-2**30-2")])
def test_phase_follows_the_episode_step_counter(P, M, k0):
    """2**30-2: the step counter one short of the 30-bit mask of the ep_step word.  P = 65536: the host's upper bound on the period
    (a 1 MB tape of one blade, built without a loop), with phase0 values at both ends of the range."""
    N = 24
    k = {"P-1": P - 1, "P": P, "2**20+3": 2 ** 20 + 3, "2**30-2": 2 ** 30 - 2}[k0]
    tape, ph0 = (blade_tape_m1(P), _phase0(P, M, N)) if P == 65536 else (_tape(P, M), _phase0(P, M, N))
    if P == 65536:
        ph0[:4] = [65535, 0, 65535, 1]
    gpu = _gpu(N, "stage_1", tape, ph0, seed=3)
    cpu = MoverOracle(N, maps.stage_1(), tape, ph0, seed=3)
    io = gpu.alloc_io()
    np.testing.assert_allclose(gpu.reset(io.obs).cpu().numpy(), cpu.reset(), rtol=0, atol=1e-6)
    # somewhere the movers are in sight: 0.3 m behind the circle the blades turn on, looking outwards in every direction
    ang = np.linspace(0, 2 * np.pi, N, endpoint=False)
    pose = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), ang], 1)
    steps = np.full(N, k, np.int32)
    gpu.set_state(pose=pose, ep_step=steps)
    cpu.set_state(pose=pose, ep_step=steps)
    np.testing.assert_array_equal(cpu.step_phases(), (k + 1 + ph0) % P)
    act = np.zeros((N, 2), np.float32)
    gpu.step(torch.from_numpy(act).to(DEV), io.obs, io.reward, io.done, io.arrive, io.ended)
    out = cpu.step(act, auto_reset=False)
    got = io.obs.cpu().numpy()
    np.testing.assert_allclose(got, out["obs"], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(io.done.cpu().numpy(), out["done"])
    assert (got[:, :10] == out["obs"][:, :10]).all(axis=1).mean() > 0.99
    # ... and the scan at the NEIGHBOURING phase is a different one (the check above can tell the phases apart)
    other = MoverOracle(N, maps.stage_1(), tape, (ph0 + 1) % P, seed=3)
    other.reset()
    other.set_state(pose=pose, ep_step=steps)
    assert (other.step(act, auto_reset=False)["obs"][:, :10] != out["obs"][:, :10]).any(axis=1).mean() > 0.5
    gpu.close()


def test_no_phase0_is_all_zero_phase0():
    N, T, P, M = 40, 20, 7, 32
    tape = _tape(P, M)
    acts = torch.from_numpy(_actions(np.random.default_rng(43), T, N)).to(DEV)
    outs = []
    for ph0 in (None, np.zeros(N, np.int32)):
        g = _gpu(N, "stage_1", tape, ph0, max_episode_steps=9, auto_reset=True, seed=4)
        io = g.alloc_io()
        rows = [g.reset(io.obs).clone()]
        for t in range(T):
            g.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
            rows += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.ended.clone()]
        outs.append(rows)
        g.close()
    assert all(torch.equal(x, y) for x, y in zip(*outs))


def test_raycast_sees_the_phase_the_env_last_observed():
    N, P, M = 50, 7, 37
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    gpu = _gpu(N, "stage_2", tape, ph0, seed=6)
    io = gpu.alloc_io()
    gpu.reset(io.obs)
    rng = np.random.default_rng(44)
    k = rng.integers(0, 50, N).astype(np.int32)
    gpu.set_state(ep_step=k)
    pose = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(-7, 7, N)], 1)
    got = gpu.raycast(torch.from_numpy(pose)).cpu().numpy()
    segs = compose(maps.stage_2(), tape, (k + ph0) % P)
    want = np.stack([O.raycast(segs[i], *pose[i]) for i in range(N)])
    static = np.stack([O.raycast(maps.stage_2(), *pose[i]) for i in range(N)])
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=1e-6)
    assert (got[fin] == want[fin]).mean() > 0.999
    assert (want != static).any(axis=1).mean() > 0.5   # the tape is in most of these scans
    gpu.close()


# ---------------------------------------------------------------- 4. persistent forms
def _seq_equals_steps(map_name, P, M, N=40, T=24, cap=9, radius=R_NEAR, acts=None, seed=8, **kw):
    """navsim_step_seq against T navsim_step launches, any handle options kw.  Defaults: auto-resets and the wrap of the phase both
    happen inside the launch."""
    tape, ph0 = _tape(P, M, radius), _phase0(P, M, N)
    acts = torch.from_numpy(_actions(np.random.default_rng(45), T, N) if acts is None else acts).to(DEV)
    a = _gpu(N, map_name, tape, ph0, max_episode_steps=cap, auto_reset=True, seed=seed, **kw)
    b = _gpu(N, map_name, tape, ph0, max_episode_steps=cap, auto_reset=True, seed=seed, **kw)
    inf = a.info()
    assert (inf["seq_epb"], inf["seq_waves"]) == (16, 8), inf
    ia, ib = a.alloc_io(), b.alloc_io()
    assert torch.equal(a.reset(ia.obs), b.reset(ib.obs))
    z = lambda dt=torch.float32, *s: torch.zeros((T, N) + s, dtype=dt, device=DEV)
    seq = dict(obs=z(a.obs_dtype, 16), reward=z(), done=z(torch.uint8), arrive=z(torch.uint8), ended=z(torch.uint8), ep_return=z(),
               ep_length=z(torch.int32), ep_path=z())
    a.step_seq(acts, seq["obs"], seq["reward"], seq["done"], seq["arrive"], seq["ended"], seq["ep_return"], seq["ep_length"], seq["ep_path"])
    for t in range(T):
        b.step(acts[t], ib.obs, ib.reward, ib.done, ib.arrive, ib.ended, ib.ep_return, ib.ep_length, ep_path=ib.ep_path)
        for k in ("obs", "reward", "done", "arrive", "ended"):
            assert torch.equal(bits(seq[k][t]), bits(getattr(ib, k))), (k, t)
        e = ib.ended.bool()
        for k in ("ep_return", "ep_length", "ep_path"):
            assert torch.equal(bits(seq[k][t][e]), bits(getattr(ib, k)[e])), (k, t)
    # (defaults: every env times out twice in 24 steps at the latest;) the movers end episodes earlier
    assert int(seq["ended"].sum()) > 2 * N and int(seq["done"].sum()) > 0
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k])
    a.close()
    b.close()


@pytest.mark.parametrize("map_name,P,M", [("stage_1", 7, 32), ("stage_2", 40, 64)])
def test_step_seq_equals_step_launches(map_name, P, M):
    _seq_equals_steps(map_name, P, M)


def _rollouts_equal(policy, map_name, **kw):
    """navsim_rollout_mlp64 / navsim_rollout_resmlp512 with a tape against T pairs of navppo_*_act / navsim_step (the pattern of
    test_gpu_ppo.test_persistent_rollout_equals_per_step_rollout): every buffer and the state bit-identical, two rollouts.  kw: env
    options (sensor, float16 rows)."""
    N, T, cap = 40, 24, 9
    movers = dict(tape=_tape(7, 32, R_NEAR), phase="random")
    outs = []
    for persistent in (True, False):
        env = VecEnv(N, map=map_name, max_episode_steps=cap, seed=3, map_seed=5, movers=movers, **kw)
        cfg = ppo.PPOConfig(rollout_len=T, max_episode_steps=cap, n_updates_per_iteration=1, policy=policy, seed=5,
                            persistent_rollout=persistent, use_graph=False)
        tr = ppo.PPOTrainer(env, cfg)
        assert tr.uses_persistent_rollout is persistent
        inf = env.sim.info()
        assert (inf["rollout_kind"], inf["rollout_epb"], inf["rollout_waves"]) == (1, 16, 8), inf
        bufs = []
        for _ in range(2):
            tr.rollout()
            torch.cuda.synchronize()
            bufs.append([b.clone() for b in (tr.obs_buf, tr.act_buf, tr.logp_buf, tr.rew_buf, tr.done_buf, tr.arrive_buf, tr.ended_buf)] +
                        [torch.where(tr.ended_buf.bool(), b, torch.zeros_like(b)) for b in (tr.epret_buf, tr.eplen_buf, tr.eppath_buf)])
        outs.append((bufs, env.sim.get_state()))
        env.close()
    (a, sa), (b, sb) = outs
    assert a[0][0].dtype == (torch.float16 if kw.get("obs_f16") else torch.float32)
    assert int(a[0][6].sum()) >= 2 * N   # cap 9, 24 steps: every env ends twice at least -- resets and phase wraps inside the launch
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert torch.equal(bits(x), bits(y))
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k])


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
@pytest.mark.parametrize("map_name", ["stage_1", "stage_2"])
def test_persistent_rollout_equals_per_step_rollout(policy, map_name):
    _rollouts_equal(policy, map_name)


@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
@pytest.mark.parametrize("map_name", ["stage_1", "stage_2"])
def test_evaluation_table_equals_the_stepping_loop(policy, map_name):
    """navsim_evaluate_mlp64 / navsim_evaluate_resmlp512 with a tape: the episode table of a loop of navppo_*_act (zero noise) +
    navsim_step launches, bit for bit (the reference and the comparison of tests/test_gpu_evaluate.py)."""
    from test_gpu_evaluate import _actor, assert_tables_equal, kernel_table, reference_table
    N, quota, cap, P, M = 24, 2, 20, 7, 32
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    flat = _actor(policy, 16)[1]
    tabs = []
    for fn in (reference_table, kernel_table):
        s = _gpu(N, map_name, tape, ph0, max_episode_steps=cap, auto_reset=True, seed=12, threshold_arrive=0.4)
        r = fn(s, policy, flat, quota, quota * cap)
        tabs.append(r[0] if isinstance(r, tuple) else r)
        s.close()
    want, got = tabs
    assert (want["count"] == quota).all()
    assert_tables_equal(got, want, f"{policy} {map_name}")


# ---------------------------------------------------------------- 5. refusals and switching off
def _rc(fn, *a):
    return fn(*a), lib().navsim_last_error().decode()


def test_refusals():
    tape = torch.from_numpy(_tape(7, 32)).to(DEV)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    L = lib()
    g = NavSim(32, device=DEV)
    assert _rc(L.navsim_set_movers, g._h, P(tape), 7, 32, None, None)[0] == -3           # NAVSIM_E_STATE: before set_map
    with pytest.raises(NavsimError, match="code -3"):
        g.set_movers(tape)
    g.set_map(maps.stage_1())
    assert _rc(L.navsim_set_movers, g._h, P(tape), 7, 32, None, None)[0] == 0
    big = torch.zeros((2, 65, 4), device=DEV)
    rc, msg = _rc(L.navsim_set_movers, g._h, P(big), 2, 65, None, None)                  # M = 65
    assert rc == -1 and "n_segments" in msg
    with pytest.raises(NavsimError, match="code -1"):
        g.set_movers(big)
    assert _rc(L.navsim_set_movers, g._h, P(tape), 0, 32, None, None)[0] == -1
    assert _rc(L.navsim_set_movers, g._h, P(tape), 65537, 32, None, None)[0] == -1
    ph = torch.zeros(32, dtype=torch.int32, device=DEV)
    ph[17] = 7                                                                           # a phase0 value equal to P
    rc, msg = _rc(L.navsim_set_movers, g._h, P(tape), 7, 32, P(ph), None)
    assert rc == -1 and "phase0" in msg
    ph[17] = -1
    assert _rc(L.navsim_set_movers, g._h, P(tape), 7, 32, P(ph), None)[0] == -1
    ph[17] = 6
    assert _rc(L.navsim_set_movers, g._h, P(tape), 7, 32, P(ph), None)[0] == 0
    with pytest.raises(NavsimError):   # the Python layer checks the tensors before a pointer crosses the ABI
        g.set_movers(torch.zeros((7, 32, 3)))
    with pytest.raises(NavsimError):
        g.set_movers(tape, np.zeros(31, np.int32))
    with pytest.raises(NavsimError):
        g.set_movers(tape, np.zeros(32, np.float32))
    # a refused call leaves the movers that were set
    assert g.info()["step_epb"] == 16 and g.info()["step_waves"] == 8
    g.close()

    g36 = NavSim(32, n_beams=36, device=DEV)                                             # 36 beams
    g36.set_map(maps.stage_1())
    rc, msg = _rc(L.navsim_set_movers, g36._h, P(tape), 7, 32, None, None)
    assert rc == -1 and "36 beams" in msg and "not built" in msg
    g36.close()

    gp = NavSim(32, device=DEV)                                                          # a per-env static map
    gp.set_map(maps.replicate_per_env(maps.stage_1(), 32), per_env=True)
    rc, msg = _rc(L.navsim_set_movers, gp._h, P(tape), 7, 32, None, None)
    assert rc == -1 and "per-env static map" in msg and "not built" in msg
    gp.set_map(maps.stage_1())
    gp.set_movers(tape)
    with pytest.raises(NavsimError, match="not built"):                                  # ... and the other way round
        gp.set_map(maps.replicate_per_env(maps.stage_1(), 32), per_env=True)
    gp.close()


def test_set_map_after_set_movers_keeps_the_tape():
    N, P, M = 40, 7, 32
    tape, ph0 = _tape(P, M), _phase0(P, M, N)
    g = _gpu(N, "stage_1", tape, ph0, max_episode_steps=CAP_LOCK, auto_reset=True, seed=5)
    g.set_map(maps.stage_4())   # the tape stays, the spawn tables are rebuilt for the new static map
    cpu = MoverOracle(N, maps.stage_4(), tape, ph0, max_episode_steps=CAP_LOCK, seed=5)
    rr, rs = maps.goal_rects("stage_1")
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    st = _lockstep(g, cpu, _lock_actions("stage_1")[:40])
    assert st["done"] >= 10
    g.close()


@pytest.mark.parametrize("map_name", ["stage_1", "stage_2"])
def test_switching_movers_off_restores_the_static_handle(map_name):
    N, T = 40, 30
    acts = torch.from_numpy(_actions(np.random.default_rng(47), T, N)).to(DEV)
    outs, infos = [], []
    for had_tape in (True, False):
        g = _gpu(N, map_name, max_episode_steps=9, auto_reset=True, seed=2)
        if had_tape:
            g.set_movers(_tape(7, 32), _phase0(7, 32, N))
            assert g.info()["step_waves"] == 8 and g.raycast(torch.zeros((N, 3), dtype=torch.float64)).min() < 0.8   # the blades are there
            g.set_movers(None)
            assert g.movers_period == 0
        infos.append(g.info())
        io = g.alloc_io()
        rows = [g.reset(io.obs).clone()]
        for t in range(T):
            g.step(acts[t], io.obs, io.reward, io.done, io.arrive, io.ended)
            rows += [io.obs.clone(), io.reward.clone(), io.done.clone(), io.arrive.clone(), io.ended.clone()]
        outs.append(rows)
        g.close()
    assert infos[0] == infos[1]   # the same instantiations as a handle that never had a tape
    assert all(torch.equal(x, y) for x, y in zip(*outs))


# ---------------------------------------------------------------- 6. the trainer
@pytest.mark.parametrize("policy", ["mlp64x2", "resmlp512"])
def test_trainer_with_movers(policy, tmp_path):
    env = VecEnv(64, map="stage_1", max_episode_steps=30, seed=3, movers="orbit4")
    cfg = ppo.PPOConfig(rollout_len=32, max_episode_steps=30, n_updates_per_iteration=2, policy=policy, seed=1, eval_every=1,
                        eval_episodes=32, output_dir=str(tmp_path))
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.uses_persistent_rollout and env.sim.movers_period == maps.MOVERS_DEFAULT_PERIOD
    with torch.no_grad():   # drive: a forward bias on the linear-velocity head, so that the robots reach the pillars' orbit
        (tr.actor.layer3 if policy == "mlp64x2" else tr.actor.out1).bias.add_(2.0)
    done = 0
    for _ in range(2):
        lg = tr.iteration()
        assert np.isfinite([lg["actor_loss"], lg["critic_loss"]]).all(), lg
        done += int(tr.done_buf.sum())
        assert "eval_success" in lg
    assert done > 0
    ev = tr._eval_env
    assert ev is not None and ev.sim.movers_period == env.sim.movers_period and ev.sim.movers_segments == env.sim.movers_segments == 32
    assert ev.world_args["movers"] == "orbit4"
    env.close()
    ev.close()
