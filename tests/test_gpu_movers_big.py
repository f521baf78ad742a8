"""Movers in the big shapes of the persistent mlp64 rollout (rollout_big_mov_kernel: 64 envs on 16 waves, 32 on 8), and the ``movers``
keyword of the single-env ``Env``.

The reference of the big twins is the 16-env twin (rollout_mov_kernel) on the same handle left to the rule -- which
tests/test_gpu_movers*.py hold to the per-step launches and to the composed-map oracle: every buffer must keep its bits.  N = 72
forced to 64 envs per workgroup is one full workgroup and one of 8 envs; forced to 32 it is 32 + 32 + 8."""
import functools

import numpy as np
import pytest
import torch

from _guards import canary_of, is_canary, run_both
from _movers import MoverOracle, blade_tape, tripwire_rows
from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import Env, VecEnv
from test_gpu_mover_bank import QUADS, SPECS
from test_gpu_movers import R_NEAR, _gpu, _phase0, _tape, bits
from test_gpu_parity import OBS_ATOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, T, CAP, P7 = 72, 24, 9, 7


def _info3(g):
    inf = g.info()
    return inf["rollout_kind"], inf["rollout_epb"], inf["rollout_waves"]


# ---------------------------------------------------------------- 1. kernel selection
@pytest.mark.parametrize("map_name,cast", [("stage_1", 0), ("stage_2", 3)])
def test_kernel_selection(map_name, cast):
    g = _gpu(N, map_name, _tape(P7, 32), _phase0(P7, 32, N), max_episode_steps=CAP, auto_reset=True, seed=5)
    assert _info3(g) == (1, 16, 8), g.info()            # the rule at 72 envs: the 16-env twin
    for epb, waves in ((64, 16), (32, 8)):
        g.set_shape(epb)
        inf = g.info()
        assert _info3(g) == (2, epb, waves), inf
        assert inf["rollout_cast"] == cast, inf           # stage_2: 128 segments, tile boxes
        # a forced shape applies to the rollout only: every other stepping entry point keeps the 16-env twins
        assert (inf["step_epb"], inf["step_waves"], inf["seq_epb"], inf["seq_waves"]) == (16, 8, 16, 8), inf
        assert inf["step_cast"] == cast and inf["seq_cast"] == cast
    for epb in (4, 8, 16):                                # the small forced shapes: the 16-env twin, as before
        g.set_shape(epb)
        assert _info3(g) == (1, 16, 8), g.info()
    g.set_shape(0)
    assert _info3(g) == (1, 16, 8)
    g.set_movers(None)                                    # without the tape the forced shape is the static kernel's
    g.set_shape(64)
    assert _info3(g) == (2, 64, 16) and g.info()["step_epb"] == 64
    g.close()


# ---------------------------------------------------------------- 2. bit identity against the 16-env twin
OPTS = {"plain": {}, "noise-gazebo": dict(lidar_noise_sigma=0.01, lidar_below_min="gazebo"), "f16": dict(obs_f16=True)}


def _trainer_rollouts(env, shape, persistent=True, n=2):
    """n consecutive rollouts of a trainer on `env` with the rollout shape forced (0: the rule): every buffer, and the state"""
    env.sim.set_shape(shape)
    cfg = ppo.PPOConfig(rollout_len=T, max_episode_steps=CAP, n_updates_per_iteration=1, policy="mlp64x2", seed=5,
                        persistent_rollout=persistent, use_graph=False)
    tr = ppo.PPOTrainer(env, cfg)
    assert tr.uses_persistent_rollout is persistent
    bufs = []
    for _ in range(n):
        tr.rollout()
        torch.cuda.synchronize()
        bufs.append([b.clone() for b in (tr.obs_buf, tr.act_buf, tr.logp_buf, tr.rew_buf, tr.done_buf, tr.arrive_buf, tr.ended_buf)] +
                    [torch.where(tr.ended_buf.bool(), b, torch.zeros_like(b)) for b in (tr.epret_buf, tr.eplen_buf, tr.eppath_buf)])
    return bufs, env.sim.get_state(), _info3(env.sim)


def _assert_same(a, b, what):
    (ba, sa, _), (bb, sb, _) = a, b
    for r, (ra, rb) in enumerate(zip(ba, bb)):
        for j, (x, y) in enumerate(zip(ra, rb)):
            assert torch.equal(bits(x), bits(y)), f"{what}: rollout {r}, buffer #{j}"
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=f"{what}: state {k}")


@functools.lru_cache(maxsize=None)
def _single_tape_run(map_name, M, opts, shape):
    env = VecEnv(N, map=map_name, max_episode_steps=CAP, seed=3, map_seed=5, movers=dict(tape=_tape(P7, M, R_NEAR), phase="random"),
                 **OPTS[opts])
    out = _trainer_rollouts(env, shape)
    env.close()
    return out


CASES = [(m, M, "plain") for m in ("stage_1", "stage_2") for M in (3, 17, 32, 33, 64)] + [("stage_1", 32, "noise-gazebo"),
                                                                                            ("stage_2", 17, "f16")]


@pytest.mark.parametrize("shape", [64, 32])
@pytest.mark.parametrize("map_name,M,opts", CASES, ids=[f"{m}-M{M}-{o}" for m, M, o in CASES])
def test_rollout_bit_identical_to_the_16_env_twin(map_name, M, opts, shape):
    """M at P = 7: the mover pass holds 16 envs (M = 3), 2 (17, 32) or 1 (33, with idle lanes, and 64)."""
    want = _single_tape_run(map_name, M, opts, 0)
    assert want[2] == (1, 16, 8)
    got = _single_tape_run(map_name, M, opts, shape)
    assert got[2] == (2, shape, 16 if shape == 64 else 8)
    ended = want[0][0][6]
    assert want[0][0][0].dtype == (torch.float16 if opts == "f16" else torch.float32)
    assert int(ended.sum()) >= 2 * N       # cap 9, 24 steps: resets and phase wraps inside the launch
    _assert_same(got, want, f"{map_name} M={M} {opts} forced {shape}")


# ---------------------------------------------------------------- 3. the forced-64 rollout replayed on the oracle
def test_forced_64_rollout_replays_on_the_oracle():
    M, seed, map_seed = 32, 3, 5
    tape = _tape(P7, M, R_NEAR)
    env = VecEnv(N, map="stage_1", max_episode_steps=CAP, seed=seed, map_seed=map_seed, movers=dict(tape=tape, phase="random"))
    env.sim.set_shape(64)
    assert _info3(env.sim) == (2, 64, 16)
    from test_gpu_evaluate import _actor
    flat = _actor("mlp64x2", 16)[1]
    out = env.rollout_mlp64(flat, T, 0.3, seed=11)
    torch.cuda.synchronize()
    ph0 = maps.mover_phases(P7, N, map_seed=map_seed, env_id_base=0)
    cpu = MoverOracle(N, maps.stage_1(), tape, ph0, max_episode_steps=CAP, seed=seed, threshold_arrive=env.threshold_arrive)
    rr, rs = maps.goal_rects("stage_1")
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    np.testing.assert_allclose(out.obs[0].cpu().numpy(), cpu.reset(), rtol=0, atol=OBS_ATOL)
    acts = out.act.cpu().numpy()
    exact = total = seen = 0
    for t in range(T):
        np.testing.assert_array_equal(cpu.step_phases(), (cpu.get_state()["ep_step"].astype(np.int64) + 1 + ph0) % P7)
        o = cpu.step(acts[t])
        seen += int(cpu.tape_in_scan().sum())   # the oracle alone: at these poses the tape changes the scan of the static map
        for f in ("done", "arrive", "ended"):
            np.testing.assert_array_equal(getattr(out, f)[t].cpu().numpy(), o[f], err_msg=f"{f}, step {t}")
        got = out.obs[t + 1].cpu().numpy()
        np.testing.assert_allclose(got, o["obs"], rtol=0, atol=OBS_ATOL, err_msg=f"obs, step {t}")
        np.testing.assert_allclose(out.reward[t].cpu().numpy(), o["reward"], rtol=1e-5, atol=1e-5, err_msg=f"reward, step {t}")
        exact += int((got == o["obs"]).all(axis=1).sum())
        total += N
    sg, sc = env.sim.get_state(), cpu.get_state()
    np.testing.assert_allclose(sg["pose"], sc["pose"], rtol=0, atol=1e-11)
    for f in ("goal", "ep_step", "rng_ctr"):
        np.testing.assert_array_equal(sg[f], sc[f])
    assert int(out.ended.sum()) >= 2 * N
    assert exact > 0.99 * total
    assert seen > 0.5 * total               # the tape is in more than half of the compared rows' scans
    env.close()


# ---------------------------------------------------------------- 4. a bank of tapes mixed inside the 64-env workgroup
TID = np.random.default_rng(72).integers(0, len(SPECS), N).astype(np.int32)
PH0 = np.array([_phase0(SPECS[k][0], SPECS[k][1], N)[i] for i, k in enumerate(TID)], np.int32)
for _k, (_P, _, _) in enumerate(SPECS):   # both ends of every tape's range occur
    _c = np.flatnonzero(TID == _k)
    PH0[_c[0]], PH0[_c[1]] = 0, _P - 1


def _trapped_bank():
    """[K * Pmax + 2, M, 4] on the device: the NaN-padded bank with a tripwire phase (a wall 0.3 m round the spawn pose) in front of
    tape 0, behind the last tape, and in rows period[k] .. Pmax - 1 of every tape; the kernels get rows 1 .. K * Pmax"""
    bank, periods, _ = maps.mover_bank([blade_tape(P, M, radius=R_NEAR) for P, M, _ in SPECS])
    K, Pmax, M, _ = bank.shape
    wire = tripwire_rows(M)
    trap = bank.copy()
    for k in range(K):
        trap[k, periods[k]:] = wire
    big = torch.from_numpy(np.ascontiguousarray(np.concatenate([wire[None], trap.reshape(K * Pmax, M, 4), wire[None]]))).to(DEV)
    return big, big[1:-1].view(K, Pmax, M, 4), [int(p) for p in periods]


@functools.lru_cache(maxsize=None)
def _bank_run(shape):
    big, inner, periods = _trapped_bank()
    assert inner.data_ptr() % 16 == 0 and inner.data_ptr() == big.data_ptr() + inner.shape[2] * 16
    env = VecEnv(N, map="stage_1", max_episode_steps=CAP, seed=3)
    env.sim.set_mover_bank(inner, periods, TID, PH0, QUADS)
    out = _trainer_rollouts(env, shape)
    env.close()
    return out


@pytest.mark.parametrize("shape", [64, 32])
def test_bank_bit_identical_to_the_16_env_twin(shape):
    assert len(set(TID[:64].tolist())) == 3 and len(set(TID[64:].tolist())) >= 2   # the tapes mix inside both workgroups
    want, got = _bank_run(0), _bank_run(shape)
    assert want[2] == (1, 16, 8) and got[2] == (2, shape, 16 if shape == 64 else 8)
    assert int(want[0][0][6].sum()) >= 2 * N
    _assert_same(got, want, f"bank forced {shape}")


# ---------------------------------------------------------------- 5. the trainer
def test_trainer_on_a_forced_64_handle_equals_the_per_step_path():
    outs = []
    for persistent in (True, False):
        env = VecEnv(N, map="stage_1", max_episode_steps=CAP, seed=3, map_seed=5, movers=dict(tape=_tape(P7, 32, R_NEAR), phase="random"))
        outs.append(_trainer_rollouts(env, 64, persistent))
        env.close()
    assert outs[0][2] == (2, 64, 16)
    assert int(outs[0][0][0][6].sum()) >= 2 * N
    _assert_same(outs[0], outs[1], "trainer, forced 64: persistent against per-step")


# ---------------------------------------------------------------- 6. guarded allocations
@pytest.mark.parametrize("epb,f16,M", [(64, 0, 37), (32, 1, 5), (64, 1, 64)])
def test_big_mover_rollout_guarded(epb, f16, M):
    """navsim_rollout_mlp64 on the big twins through the harness of tests/test_gpu_tails.py: the tape at its 16-byte minimum alignment
    (borrowed where it lies, poisoned guards round it), phase0 at 4, every [T, N, .] output guarded after its last row, N no multiple
    of the workgroup's envs; the bits of both placements equal."""
    from test_gpu_tails import P, _map, _mlp64_flat, _sim, _st
    n, t_, D = 203, 5, 16
    odt = torch.float16 if f16 else torch.float32
    flat = _mlp64_flat(D, 1)[2]
    PA = 64 * D + 4354

    def call(g):
        s = _sim(n, 10, f16, 5, epb)
        try:
            s.set_map(_map(n, False, g))
            tape = g.inp(torch.from_numpy(blade_tape(P7, M, pad_to=40 if M == 37 else None, radius=R_NEAR)).to(DEV), 16)
            ph0 = g.inp((torch.arange(n, dtype=torch.int32) * 5 % P7).to(DEV), 4)
            s.set_movers(tape, ph0)
            assert s._mov_tape.data_ptr() == tape.data_ptr()
            assert _info3(s) == (2, epb, 16 if epb == 64 else 8) and n % epb != 0
            al = 16 if g.minimal else 256
            o0 = g.out((n, D), odt, al)
            s.reset(o0)
            start = torch.cat([o0[None], canary_of(odt).to(DEV).expand(t_, n, D)]).contiguous()
            ob = g.io(start, al)
            pr = g.inp(flat[:PA], 16)
            act = g.out((t_, n, 2), torch.float32, 8 if g.minimal else 256)
            lp, rw = g.out((t_, n), torch.float32, al), g.out((t_, n), torch.float32, al)
            fl = [g.out((t_, n), torch.uint8, al) for _ in range(3)]
            var = g.inp(torch.tensor([0.5], device=DEV), 4)
            assert lib().navsim_rollout_mlp64(s._h, P(pr), P(ob), P(act), P(lp), P(rw), *[P(f) for f in fl], None, None, None, P(var), 9,
                                              None, t_, _st()) == 0
            torch.cuda.synchronize()
            assert not bool(is_canary(ob[1:]).any())
            assert bool(torch.isfinite(ob.float()).all())   # a read of a poisoned guard would be a NaN
            return ob, act, lp
        finally:
            s.close()

    run_both(DEV, call, f"rollout_big_mov epb={epb} f16={f16} M={M}")


# ---------------------------------------------------------------- 7. Env(..., movers=...)
def _drive(k):
    return np.array([0.9, 0.3 * np.sin(0.7 * k)], np.float32)


def test_env_with_movers_against_the_oracle():
    Pn, phase = 7, 3
    tape = blade_tape(Pn, 5)
    env = Env(True, movers=dict(tape=tape, phase=phase))
    cpu = MoverOracle(1, maps.stage_1(), tape, [phase], respawn_on_arrive=True, threshold_arrive=0.2, seed=0)
    rr, rs = maps.goal_rects("stage_1")
    cpu.set_goal_rects(0, rr)
    cpu.set_goal_rects(1, rs)
    inf = env._sim.info()
    assert (inf["step_epb"], inf["step_waves"]) == (16, 8) and env._sim.movers_period == Pn
    static_rows = tape_rows = 0
    k = 0
    past = np.zeros(2, np.float32)
    np.testing.assert_allclose(env.reset(), cpu.reset()[0], rtol=0, atol=OBS_ATOL)
    for s in range(30):
        if s == 14:   # a reset in the middle: the step counter, and with it the phase, starts again
            np.testing.assert_allclose(env.reset(), cpu.reset()[0], rtol=0, atol=OBS_ATOL)
            k, past = 0, np.zeros(2, np.float32)
        assert env.mover_phase == (k + 1 + phase) % Pn == int(cpu.step_phases()[0])
        a = _drive(s)
        obs, rew, done, arrive = env.step(a, past)
        o = cpu.step(a[None], auto_reset=False)
        assert (done, arrive) == (bool(o["done"][0]), bool(o["arrive"][0])), s
        np.testing.assert_allclose(obs, o["obs"][0], rtol=0, atol=OBS_ATOL, err_msg=f"step {s}")
        np.testing.assert_allclose(rew, o["reward"][0], rtol=1e-5, atol=1e-5)
        tape_rows += int(cpu.tape_in_scan()[0])
        static_rows += 1
        past, k = a, k + 1
    assert tape_rows > static_rows // 2   # the blades are in most of these scans
    np.testing.assert_allclose(np.array([env.position.x, env.position.y]), cpu.get_state()["pose"][0, :2], rtol=0, atol=1e-11)
    env.close()


def test_env_without_the_keyword_is_unchanged():
    a, b = Env(True), Env(True, movers=None)
    assert a._sim.info() == b._sim.info() and a._sim.movers_period == 0 and a.mover_phase is None
    rows = []
    for e in (a, b):
        r = [e.reset()]
        past = np.zeros(2, np.float32)
        for s in range(12):
            act = _drive(s)
            obs, rew, done, arrive = e.step(act, past)
            r += [obs, np.array([rew, done, arrive])]
            past = act
        rows.append(r)
        e.close()
    for x, y in zip(*rows):
        np.testing.assert_array_equal(x, y)
    # ... and a tape does change what the env sees
    c = Env(True, movers=blade_tape(7, 5, radius=R_NEAR))
    assert (c.reset()[:10] != rows[0][0][:10]).any()
    c.close()
