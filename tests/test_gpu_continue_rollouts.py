"""Rollouts that continue across launches, on the GPU: navsim_rollout_mlp64_hist_cont, navsim_stack_rows_cont and
PPOConfig.continue_rollouts.

Nothing is recomputed at a seam -- a history carry is 22 copies, the env state lives in the handle, the noise counter is a device
scalar -- so every comparison is bit for bit: k launches chained through row T -> row 0, step_base and the carry against ONE launch
of the whole length.  The common world: 40 envs (two full 16-env workgroups and one of 8) on stage_1, 24 steps, episodes capped at 7
steps, so that time-outs put an episode's first row on rows 7, 14 and 21.

The further worlds (SEAM_KINDS) are those of tests/test_gpu_scan_history.py, built by its make_sim and started by its start(): stage_2
with the robot in front of the inner wall, episodes capped at 7 steps and started at step count env mod 7, so that collisions,
arrivals and time-outs end episodes on every row.  Beside the comparison with ONE launch the final carry is held against
stack_rows_reference of the one-launch buffers on the host -- an expected value that no kernel of the project computed."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_scan_history as SH
from _guards import run_both
from _ranks import spawn_ranks
from navbot_ppo_amd import maps, nets, ppo
from navbot_ppo_amd._native import lib
from navbot_ppo_amd.env import HIST_CARRY, HIST_DIM, NavSim, NavsimError, VecEnv, stack_rows, stack_rows_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N, T, CAP = 40, 24, 7
ACT_SEED, STEP_BASE, VAR = 0x5EED1234ABCD, 5, 0.3
CUTS = [1, 5, 7, 8, 14, 23]
FIELDS = ("obs", "act", "logp", "reward", "done", "arrive", "ended", "ep_return", "ep_length", "ep_path")
KINDS = {   # name -> (NavSim options, movers)
    "plain": ({}, False),
    "tape": ({}, True),
    "f16": (dict(obs_f16=True), False),
    "noise": (dict(lidar_noise_sigma=0.02), False),
}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(x):
    return x.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[x.element_size()]) if x.is_floating_point() else x


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _actor(policy="hist", seed=3, scale=2.0):
    """a fixed random actor of the entry point's policy, as its flat parameters"""
    torch.manual_seed(seed)
    a, _ = nets.make_policy("resmlp512", 16) if policy == "resmlp512" else nets.make_policy("mlp64x2", HIST_DIM if policy == "hist" else 16)
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(scale)
    return nets.flat_actor_params(a).to(DEV)


def make_sim(kind="plain", n=N, cap=CAP, **kw):
    if kind not in KINDS:   # a world of tests/test_gpu_scan_history.py (its cap is this file's)
        assert kind in SH.KINDS and cap == CAP == SH.CAP
        return SH.make_sim(kind, n, **kw)
    opts, movers = KINDS[kind]
    s = NavSim(n, n_beams=10, max_episode_steps=cap, auto_reset=True, seed=11, device=DEV, **opts, **kw)
    rr, rs = maps.goal_rects("stage_1")
    s.set_goal_rects(0, rr)
    s.set_goal_rects(1, rs)
    s.set_map(maps.by_name("stage_1"))
    if movers:   # two pillars, five phases: a small tape whose period is no divisor of the cap or of a cut
        tape = maps.orbit_movers(5, n=2, sides=4)
        s.set_movers(tape, maps.mover_phases(tape.shape[0], n, map_seed=2))
    return s


def _buffers(sim, n_steps):
    n = sim.N
    z = lambda dt, *s: torch.zeros((n_steps, n) + s, dtype=dt, device=DEV)
    return dict(obs=torch.zeros((n_steps + 1, n, 16), dtype=sim.obs_dtype, device=DEV), act=z(torch.float32, 2), logp=z(torch.float32),
                reward=z(torch.float32), done=z(torch.uint8), arrive=z(torch.uint8), ended=z(torch.uint8), ep_return=z(torch.float32),
                ep_length=z(torch.int32), ep_path=z(torch.float32))


def launch(entry, sim, flat, b, n_steps, step_base, carries=None):
    """one launch of a rollout entry point through the C ABI; carries = (hist_in, hist_out) for the _cont entry point"""
    var = torch.tensor(VAR, device=DEV)
    base = torch.tensor(step_base, dtype=torch.int32, device=DEV)
    extra = () if carries is None else (P(carries[0]), P(carries[1]))
    rc = getattr(lib(), entry)(sim._h, P(flat), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]), P(b["arrive"]),
                               P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var), ACT_SEED, P(base),
                               n_steps, *extra, _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()


def start_of(kind):
    """how a rollout in the world `kind` begins: a reset, in the worlds of the scan-history file its start() (staggered step counts)"""
    return (lambda sim, obs0: sim.reset(obs0)) if kind in KINDS else SH.start


def chained(entry, sim, flat, cuts, n_steps=T, cont=False, inplace=True, start=start_of("plain")):
    """the rollout in pieces cut at the rows `cuts`: a reset, then per piece a launch on buffers of its own whose row 0 is a copy of
    the piece before's last row, step_base advanced by the steps taken, the carry handed on (cont).  Returns the concatenation -- the
    seam rows once -- and the last carry."""
    edges = [0] + list(cuts) + [n_steps]
    parts, prev, carry = [], None, None
    if cont:
        carry = [torch.full((sim.N, HIST_CARRY), float("nan"), device=DEV) for _ in range(2)]
    for k, (a, e) in enumerate(zip(edges[:-1], edges[1:])):
        b = _buffers(sim, e - a)
        if prev is None:
            start(sim, b["obs"][0])
        else:
            b["obs"][0].copy_(prev["obs"][-1])
        cs = None
        if cont:   # in place: one buffer in and out; else the two take turns
            cs = (None if k == 0 else carry[0], carry[0] if inplace else carry[1])
        launch(entry, sim, flat, b, e - a, STEP_BASE + a, cs)
        if cont and not inplace:
            carry.reverse()
        parts.append(b)
        prev = b
    out = {f: torch.cat([p[f] if (f != "obs" or k == 0) else p[f][1:] for k, p in enumerate(parts)]) for f in FIELDS}
    return out, (carry[0] if cont else None)


@functools.lru_cache(maxsize=None)
def _whole(kind, n=N, n_steps=T, cap=CAP, env_id_base=0):
    """ONE launch of T steps of navsim_rollout_mlp64_hist_cont (no carry in), its carry-out, and the history rows of its buffer"""
    s = make_sim(kind, n, cap, env_id_base=env_id_base)
    try:
        b, carry = chained("navsim_rollout_mlp64_hist_cont", s, _actor(), [], n_steps, cont=True, start=start_of(kind))
    finally:
        s.close()
    hist = stack_rows(b["obs"], b["ended"])
    torch.cuda.synchronize()
    return b, carry, hist


def mirror_carry(b):
    """the carry of the last row of a rollout's buffers by the host mirror: columns 16..37 of its last history row, as float32"""
    rows = stack_rows_reference(b["obs"].cpu().numpy(), b["ended"].cpu().numpy())
    return torch.from_numpy(rows[-1, :, 16:38].astype(np.float32)).to(DEV)


def assert_chain_is_one_launch(kind, cuts, inplace=True, n=N, n_steps=T, cap=CAP, env_id_base=0):
    """the launches chained at `cuts` write the bits of ONE launch, carry included, and that carry is the host mirror's; returns the
    chain's buffers and carry"""
    want, carry, _ = _whole(kind, n, n_steps, cap, env_id_base)
    s = make_sim(kind, n, cap, env_id_base=env_id_base)
    try:
        got, c = chained("navsim_rollout_mlp64_hist_cont", s, _actor(), cuts, n_steps, cont=True, inplace=inplace, start=start_of(kind))
    finally:
        s.close()
    _assert_same_rollout(got, want, (kind, cuts, inplace, n))
    assert same(c, carry), (kind, cuts, inplace, n)
    assert same(carry, mirror_carry(want)), (kind, n)
    return got, c


def _assert_same_rollout(got, want, what):
    for f in FIELDS:
        assert same(got[f], want[f]), (what, f)


# ---------------------------------------------------------------- 1. split invariance of the history rollout
def test_the_cut_set_meets_an_episode_start_a_second_row_and_a_mid_episode_row():
    ended = _whole("plain")[0]["ended"].cpu().numpy() != 0
    assert 7 in CUTS and 8 in CUTS and 5 in CUTS
    assert ended[6].any()                                # cut 7: the seam row is an episode's first row
    assert (ended[6] & ~ended[7]).any()                  # cut 8: ... its second row
    assert (~ended[2] & ~ended[3] & ~ended[4]).any()     # cut 5: two rows and more into an episode: both older frames are real
    assert ended[13].any() and ended[20].any()           # the time-outs of the cap put first rows on 14 and 21 too
    assert 0 < ended.sum() < ended.size


@pytest.mark.parametrize("cuts", [[s] for s in CUTS] + [[7, 8]], ids=lambda c: "-".join(map(str, c)))
def test_chained_launches_write_the_bits_of_one(cuts):
    want, carry, hist = _whole("plain")
    for inplace in (True, False):
        s = make_sim("plain")
        try:
            got, c = chained("navsim_rollout_mlp64_hist_cont", s, _actor(), cuts, cont=True, inplace=inplace)
        finally:
            s.close()
        _assert_same_rollout(got, want, (cuts, inplace))
        assert same(c, carry), (cuts, inplace)
    # the carry of row T is columns 16..37 of the last history row of the whole buffer
    assert same(carry, hist[-1, :, 16:38].float())


def test_without_the_carry_the_seam_shows():
    """the check above is not vacuous: chained WITHOUT the carry (row 0 of every piece an episode start, the rule of the entry point
    without _cont) the actions behind a mid-episode seam differ"""
    want = _whole("plain")[0]
    s = make_sim("plain")
    try:
        got, _ = chained("navsim_rollout_mlp64_hist", s, _actor(), [5])
    finally:
        s.close()
    assert same(got["act"][:5], want["act"][:5]) and same(got["logp"][:5], want["logp"][:5])
    assert not (same(got["act"][5], want["act"][5]) and same(got["logp"][5], want["logp"][5]))


def test_null_carries_are_the_entry_point_without_them():
    want = _whole("plain")[0]
    for entry, cont in (("navsim_rollout_mlp64_hist", False), ("navsim_rollout_mlp64_hist_cont", None)):
        s = make_sim("plain")
        try:
            b = _buffers(s, T)
            s.reset(b["obs"][0])
            launch(entry, s, _actor(), b, T, STEP_BASE, None if cont is False else (None, None))
        finally:
            s.close()
        _assert_same_rollout(b, want, entry)


@pytest.mark.parametrize("kind,cut", [("tape", 8), ("f16", 5), ("noise", 7)])
def test_one_cut_with_a_tape_float16_rows_and_lidar_noise(kind, cut):
    want, carry, hist = _whole(kind)
    s = make_sim(kind)
    try:
        got, c = chained("navsim_rollout_mlp64_hist_cont", s, _actor(), [cut], cont=True)
    finally:
        s.close()
    _assert_same_rollout(got, want, kind)
    assert same(c, carry) and same(carry, hist[-1, :, 16:38].float())
    assert bool(want["ended"].any()) and not bool(want["ended"].all())
    if kind == "f16":
        assert want["obs"].dtype == torch.float16
    if kind == "tape":   # the tape is seen: the same world without it scans differently
        assert not same(want["obs"], _whole("plain")[0]["obs"])


def test_misaligned_carries_are_refused_before_any_launch():
    s = make_sim("plain")
    try:
        b = _buffers(s, 2)
        s.reset(b["obs"][0])
        before = s.get_state()
        big = torch.zeros(N * HIST_CARRY + 4, device=DEV)
        off = big[1:1 + N * HIST_CARRY]   # 4 bytes past a 16-byte boundary
        var, base = torch.tensor(VAR, device=DEV), torch.tensor(0, dtype=torch.int32, device=DEV)
        for cs in ((P(off), None), (None, P(off))):
            rc = lib().navsim_rollout_mlp64_hist_cont(s._h, P(_actor()), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]),
                                                      P(b["done"]), P(b["arrive"]), P(b["ended"]), None, None, None, P(var), ACT_SEED,
                                                      P(base), 2, *cs, _st())
            assert rc == -1 and b"aligned" in lib().navsim_last_error()
        torch.cuda.synchronize()
        after = s.get_state()
        assert all(np.array_equal(before[k], after[k]) for k in before) and not bool(b["act"].any())
        with pytest.raises(NavsimError, match="16-byte"):   # the shim checks a carry before its pointer crosses the ABI
            stack_rows(b["obs"], b["ended"], carry_in=off.view(N, HIST_CARRY))
        with pytest.raises(NavsimError, match="carry_out"):
            stack_rows(b["obs"], b["ended"], carry_out=torch.zeros((N, HIST_CARRY), dtype=torch.float64, device=DEV))
    finally:
        s.close()


# ---------------------------------------------------------------- 1b. seams in the further worlds, on every row, in every placement
SEAM_KINDS = {   # a world of tests/test_gpu_scan_history.py -> the row it is cut at
    "bank3-respawn": 9,      # three tapes with per-env ids, goal rectangles, respawn on arrival (sp_scan[1])
    "noise-gazebo": 10,      # range noise with the below-minimum mode (sm.neg)
    "noise-f16": 11,         # ... on float16 rows
    "per-env": 9,            # every env its own copy of stage_2
    "house-boxes": 10,       # the tile-box cast of a 256-segment shared map
    "no-reset": 4,           # auto_reset off: an ended env keeps its row, hist_leave copies it
}


def seam_facts(b, s):
    """what the one-launch rollout holds around a cut at row s, per env: the step in front of the cut ended an episode (row s is an
    episode's first row); row s lies two rows and more into an episode (both older frames are real rows of it); the env ended
    before the cut and is still ended behind it; an arrival lies in front of the cut"""
    e, a = b["ended"].cpu().numpy() != 0, b["arrive"].cpu().numpy() != 0
    return dict(first=e[s - 1], deep=~e[s - 3] & ~e[s - 2] & ~e[s - 1], stays=e[s - 2] & e[s - 1] & e[s], arrived=a[:s].any(axis=0))


@pytest.mark.parametrize("kind", list(SEAM_KINDS))
def test_one_cut_in_the_further_worlds(kind):
    s = SEAM_KINDS[kind]
    want = _whole(kind)[0]
    f = seam_facts(want, s)
    print(f"{kind}, cut {s}: {SH.cut_facts(want)}; at the cut: " + ", ".join(f"{k} {int(v.sum())}" for k, v in f.items()))
    assert 3 <= s < T and f["first"].any() and f["deep"].any()       # the case means something: else it fails, it does not pass empty
    w = SH.world_of(kind)
    if not w["auto_reset"]:
        assert f["stays"].any()
    if w.get("respawn_on_arrive"):
        assert f["arrived"].any()
    if w.get("obs_f16"):
        assert want["obs"].dtype == torch.float16
    assert 0 < int(want["ended"].sum()) < want["ended"].numel()
    assert_chain_is_one_launch(kind, [s])


@pytest.mark.parametrize("inplace", [True, False], ids=["in-place", "two-buffers"])
@pytest.mark.parametrize("kind", ["plain", "bank3-respawn", "noise-f16"])
def test_every_row_a_seam(kind, inplace):
    """T launches of ONE step: hist_shift never runs (no step is followed by another), hist_enter and hist_leave alone move the carry"""
    assert_chain_is_one_launch(kind, list(range(1, T)), inplace)


PLACED = {"plain": (5, 7), "bank3-noise-f16": (11,)}    # kind -> the cuts, one per chain (this file's plain world ends episodes by
# its cap alone, all envs at once: row 7 is an episode's first row, row 5 lies five rows into one)


@pytest.mark.parametrize("kind", list(PLACED))
def test_shards_with_carries_concatenate_to_the_whole(kind):
    """one handle of 40 envs against two of 24 and 16 (env_id_base 0 and 24), each chained over one cut with a carry of its own"""
    want, carry, _ = _whole(kind)
    facts = [seam_facts(want, s) for s in PLACED[kind]]
    assert any(f["first"].any() for f in facts) and any(f["deep"].any() for f in facts)
    for s in PLACED[kind]:
        parts = [assert_chain_is_one_launch(kind, [s], n=n, env_id_base=base) for base, n in SH.SHARDS]
        assert not same(parts[1][0]["act"], want["act"][:, :16])     # (the second shard is not the first 16 envs again)
        for fld in FIELDS:
            assert same(torch.cat([p[0][fld] for p in parts], dim=1), want[fld]), (kind, s, fld)
        assert same(torch.cat([p[1] for p in parts]), carry), (kind, s)


@pytest.mark.parametrize("n", [1, 5, 17])
@pytest.mark.parametrize("kind", list(PLACED))
def test_one_handle_of_1_5_and_17_envs(kind, n):
    for s in PLACED[kind]:
        assert_chain_is_one_launch(kind, [s], n=n)
        assert_chain_is_one_launch(kind, [s], inplace=False, n=n)


def test_more_workgroups_than_one_round_with_carries():
    """4117 envs: 258 workgroups -- the grid runs in rounds -- the last one of 5 envs; episodes capped at 3 steps, one cut at row 3"""
    n, steps, cap = 4117, 6, 3
    want = _whole("plain", n, steps, cap)[0]
    e = want["ended"].cpu().numpy() != 0
    print(f"N = {n}, cap {cap}: episode ends per row {e.sum(axis=1).tolist()}")
    assert e[2].any() and e[2, -5:].any() and not e[0].all()     # the cap makes row 3 an episode's first row, in the last workgroup too
    assert_chain_is_one_launch("plain", [3], n=n, n_steps=steps, cap=cap)


def _zero_step_call(s, b, cin, cout):
    var, base = torch.tensor(VAR, device=DEV), torch.tensor(STEP_BASE, dtype=torch.int32, device=DEV)
    rc = lib().navsim_rollout_mlp64_hist_cont(s._h, P(_actor()), P(b["obs"]), P(b["act"]), P(b["logp"]), P(b["reward"]), P(b["done"]),
                                              P(b["arrive"]), P(b["ended"]), P(b["ep_return"]), P(b["ep_length"]), P(b["ep_path"]), P(var),
                                              ACT_SEED, P(base), 0, P(cin), P(cout), _st())
    torch.cuda.synchronize()
    return rc


def test_zero_steps_with_carries():
    s = make_sim("plain")
    try:
        b = _buffers(s, 2)
        s.reset(b["obs"][0])
        for f in FIELDS[1:]:
            b[f].fill_(7)
        torch.cuda.synchronize()
        before, state = {f: b[f].clone() for f in FIELDS}, s.get_state()
        carry = torch.randn((N, HIST_CARRY), device=DEV)
        kept = carry.clone()
        # one buffer in and out: accepted, nothing moves
        assert _zero_step_call(s, b, carry, carry) == 0, lib().navsim_last_error().decode()
        assert same(carry, kept)
        # a carry in alone: accepted as well
        assert _zero_step_call(s, b, carry, None) == 0, lib().navsim_last_error().decode()
        # two buffers (both 16-byte aligned): no row to write a carry for -- refused by name, nothing launched
        other = torch.full((N, HIST_CARRY), 7.0, device=DEV)
        assert carry.data_ptr() % 16 == 0 and other.data_ptr() % 16 == 0 and other.data_ptr() != carry.data_ptr()
        assert _zero_step_call(s, b, carry, other) == -1
        err = lib().navsim_last_error().decode()
        assert err.startswith("navsim_rollout_mlp64_hist_cont: ") and "n_steps == 0" in err
        assert _zero_step_call(s, b, None, other) == -1 and b"navsim_rollout_mlp64_hist_cont" in lib().navsim_last_error()
        assert bool((other == 7.0).all()) and same(carry, kept)
        after = s.get_state()
        assert all(np.array_equal(state[k], after[k]) for k in state)
        for f in FIELDS:
            assert same(b[f], before[f]), f
    finally:
        s.close()


# ---------------------------------------------------------------- 2. navsim_stack_rows_cont
@pytest.mark.parametrize("kind", ["plain", "f16"])
def test_stack_rows_cont_against_the_host_mirror(kind):
    b, _, hist = _whole(kind)
    obs, ended = b["obs"], b["ended"]
    obs_h, ended_h = obs.cpu().numpy(), ended.cpu().numpy()
    full_h = stack_rows_reference(obs_h, ended_h)
    assert np.array_equal(hist.cpu().numpy().view(np.uint8), full_h.view(np.uint8))
    for s in CUTS + [T]:
        carry = hist[s, :, 16:38].float().contiguous()
        want_h, carry_out_h = stack_rows_reference(obs_h[s:], ended_h[s:] if s < T else None, carry=carry.cpu().numpy())
        assert np.array_equal(want_h.view(np.uint8), full_h[s:].view(np.uint8)), s   # (the mirror itself, on these rows)
        out_c = torch.full((N, HIST_CARRY), float("nan"), device=DEV)
        got = stack_rows(obs[s:].contiguous(), ended[s:].contiguous() if s < T else None, carry_in=carry, carry_out=out_c)
        assert same(got, hist[s:]), s
        assert np.array_equal(out_c.cpu().numpy().view(np.uint8), carry_out_h.view(np.uint8)), s
        # in place: the carry-out lands in the buffer the carry-in came from
        inpl = carry.clone()
        got2 = stack_rows(obs[s:].contiguous(), ended[s:].contiguous() if s < T else None, carry_in=inpl, carry_out=inpl)
        assert same(got2, hist[s:]) and same(inpl, out_c), s
    # a carry out alone: the first piece of a chain
    c0 = torch.full((N, HIST_CARRY), float("nan"), device=DEV)
    assert same(stack_rows(obs[:9].contiguous(), ended[:8].contiguous(), carry_out=c0), hist[:9]) and same(c0, hist[8, :, 16:38].float())


@pytest.mark.parametrize("kind", ["plain", "f16"])
def test_stack_rows_cont_with_null_carries_is_stack_rows(kind):
    b, _, hist = _whole(kind)
    out = torch.zeros_like(hist)
    rc = lib().navsim_stack_rows_cont(P(b["obs"]), int(kind == "f16"), P(b["ended"]), T + 1, N, P(out), None, None, _st())
    assert rc == 0, lib().navsim_last_error().decode()
    torch.cuda.synchronize()
    assert same(out, hist)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("R,n", [(1, 37), (2, 37), (3, 1), (3, 37), (3, 4099)])
def test_stack_rows_cont_at_its_sizes_inside_guards(R, n, f16):
    """R = 1: no step at all -- ended_dev is NULL, row 0's columns 16..37 ARE the carry and the carry goes out as it came in; R = 2:
    the one flag decides, per env, whether row 1 reads its oldest frame from the carry; R = 3 with 1, 37 and 4099 envs.  Against
    stack_rows_reference, with separate carries and with one buffer for both."""
    rng = np.random.default_rng(100 * R + n)
    dt = np.float16 if f16 else np.float32
    obs = rng.standard_normal((R, n, 16)).astype(dt)
    carry = rng.standard_normal((n, HIST_CARRY)).astype(dt).astype(np.float32)     # (values the rows' dtype holds)
    ended = (rng.random((R - 1, n)) < 0.4).astype(np.uint8) if R > 1 else None
    if R == 2:
        assert ended[0].any() and not ended[0].all()
    want, want_carry = stack_rows_reference(obs, ended, carry=carry)
    tdt = torch.float16 if f16 else torch.float32

    def call(g, inplace):
        o = g.inp(torch.from_numpy(obs), 16)
        e = g.inp(torch.from_numpy(ended), 1) if R > 1 else None
        cin = g.io(torch.from_numpy(carry), 16) if inplace else g.inp(torch.from_numpy(carry), 16)
        cout = cin if inplace else g.out((n, HIST_CARRY), torch.float32, 16)
        out = g.out((R, n, HIST_DIM), tdt, 16)
        rc = lib().navsim_stack_rows_cont(P(o), int(f16), P(e), R, n, P(out), P(cin), P(cout), _st())
        assert rc == 0, lib().navsim_last_error().decode()
        torch.cuda.synchronize()
        return out.clone(), cout.clone()

    for inplace in (False, True):
        out, cout = run_both(DEV, lambda g: call(g, inplace), f"navsim_stack_rows_cont R={R} N={n} f16={f16} inplace={inplace}")
        assert np.array_equal(out.cpu().numpy().view(np.uint8), want.view(np.uint8)), (R, n, f16, inplace)
        assert np.array_equal(cout.cpu().numpy().view(np.uint8), want_carry.view(np.uint8)), (R, n, f16, inplace)
        if R == 1:
            assert np.array_equal(out.cpu().numpy()[0, :, 16:38].astype(np.float32).view(np.uint8), carry.view(np.uint8))
            assert np.array_equal(cout.cpu().numpy().view(np.uint8), carry.view(np.uint8))


# ---------------------------------------------------------------- 3. the carries inside guarded allocations
@pytest.mark.parametrize("kind", ["plain", "f16"])
def test_stack_rows_cont_inside_guards(kind):
    b, _, hist = _whole(kind)
    s = 5
    R = T + 1 - s
    carry = hist[s, :, 16:38].float().contiguous()

    def call(g):
        obs, ended = g.inp(b["obs"][s:].contiguous(), 16), g.inp(b["ended"][s:].contiguous(), 1)
        cin, cout = g.inp(carry, 16), g.out((N, HIST_CARRY), torch.float32, 16)
        out = g.out((R, N, HIST_DIM), b["obs"].dtype, 16)
        rc = lib().navsim_stack_rows_cont(P(obs), int(kind == "f16"), P(ended), R, N, P(out), P(cin), P(cout), _st())
        assert rc == 0, lib().navsim_last_error().decode()
        torch.cuda.synchronize()
        return out.clone(), cout.clone()

    out, cout = run_both(DEV, call, "navsim_stack_rows_cont")
    assert same(out, hist[s:]) and same(cout, hist[-1, :, 16:38].float())


@pytest.mark.parametrize("kind", ["plain", "tape"])
def test_rollout_carries_inside_guards(kind):
    want, carry, hist = _whole(kind)
    s = 7
    cin0 = hist[s, :, 16:38].float().contiguous()

    def call(g):
        sim = make_sim(kind)
        try:
            head, c = chained("navsim_rollout_mlp64_hist_cont", sim, _actor(), [], n_steps=s, cont=True)
            assert same(c, cin0)
            cin, cout = g.inp(cin0, 16), g.out((N, HIST_CARRY), torch.float32, 16)
            b = _buffers(sim, T - s)
            b["obs"][0].copy_(head["obs"][-1])
            launch("navsim_rollout_mlp64_hist_cont", sim, _actor(), b, T - s, STEP_BASE + s, (cin, cout))
        finally:
            sim.close()
        return b, cout.clone()

    b, cout = run_both(DEV, call, "navsim_rollout_mlp64_hist_cont")
    for f in FIELDS:
        assert same(b[f][1:] if f == "obs" else b[f], want[f][s + 1:] if f == "obs" else want[f][s:]), f
    assert same(cout, carry)


# ---------------------------------------------------------------- 4. the contract the trainer rests on, for the other rollouts
@pytest.mark.parametrize("entry,policy,n,epb,cut", [("navsim_rollout_mlp64", "mlp64", N, None, 8),
                                                    ("navsim_rollout_mlp64", "mlp64", 72, 64, 5),
                                                    ("navsim_rollout_resmlp512", "resmlp512", N, None, 7)],
                         ids=["mlp64", "mlp64-64env-shape", "resmlp512"])
def test_the_other_rollouts_continue_from_the_handle(entry, policy, n, epb, cut):
    """env state in the handle, row T -> row 0, step_base advanced: two launches write what one writes"""
    kw = {} if epb is None else dict(envs_per_workgroup=epb)
    s = make_sim("plain", n, **kw)
    try:
        if epb:
            assert s.info()["rollout_epb"] == epb
        want, _ = chained(entry, s, _actor(policy), [])
    finally:
        s.close()
    s = make_sim("plain", n, **kw)
    try:
        got, _ = chained(entry, s, _actor(policy), [cut])
    finally:
        s.close()
    _assert_same_rollout(got, want, entry)
    assert bool(want["ended"].any()) and not bool(want["ended"].all())


# ---------------------------------------------------------------- 5. the trainer
TR = dict(policy="mlp64x2", scan_history=True, rollout_len=8, max_episode_steps=20, n_updates_per_iteration=2, seed=2,
          bootstrap_truncated=True)


ENV = dict(map="stage_1", max_episode_steps=20, seed=1, device=DEV)


def _trainer(env_kw=None, **cfg):
    env = VecEnv(40, **{**ENV, **(env_kw or {})})
    return ppo.PPOTrainer(env, ppo.PPOConfig(**{**TR, **cfg}))


def _run(tr, iters):
    snaps = []
    for _ in range(iters):
        lg = tr.iteration()
        torch.cuda.synchronize()
        snaps.append({k: getattr(tr, k + "_buf").clone() for k in ("obs", "act", "rew", "ended", "hist", "eplen")
                      if getattr(tr, k + "_buf") is not None})
        snaps[-1]["log"] = dict(lg)
        snaps[-1]["starts"] = tr.episode_starts
        snaps[-1]["did_reset"] = tr._did_reset
    return snaps


def _replay(actions_per_reset, env_kw=None, state=None):
    """the observations and flags of a fresh env of the trainer's world under recorded actions: a reset in front of every tape
    (state: the envs' state behind it -- NavSim.get_state -- where the trainer's envs did more than reset before the tape)"""
    env = VecEnv(40, **{**ENV, **(env_kw or {})})
    try:
        out = []
        for act in actions_per_reset:
            obs0 = env.reset().clone()
            if state is not None:
                env.sim.set_state(**state)
            r = env.step_seq(act)
            torch.cuda.synchronize()
            out.append((torch.cat([obs0[None], r.obs]), r.ended))
    finally:
        env.close()
    return out


def test_trainer_continues_across_iterations():
    tr = _trainer(continue_rollouts=True, norm_reward=True)
    try:
        snaps = _run(tr, 3)
        ret_rms = tr.ret_rms.tolist()
        gamma = tr.cfg.gamma
    finally:
        tr.env.close()
    Tr = TR["rollout_len"]
    for a, b in zip(snaps[:-1], snaps[1:]):
        assert same(b["obs"][0], a["obs"][Tr])   # row 0 is the row the last rollout stopped at
    # the three iterations are ONE trajectory: a single reset and the recorded actions reproduce every row and flag
    (obs, ended), = _replay([torch.cat([s["act"] for s in snaps])])
    assert same(obs, torch.cat([snaps[0]["obs"]] + [s["obs"][1:] for s in snaps[1:]]))
    assert same(ended, torch.cat([s["ended"] for s in snaps]))
    # every iteration's history rows are the rule applied to the whole trajectory (no weights in this check)
    full = stack_rows_reference(obs.cpu().numpy(), ended.cpu().numpy())
    for k, s in enumerate(snaps):
        assert np.array_equal(s["hist"].cpu().numpy(), full[k * Tr:(k + 1) * Tr + 1]), k
    # ... which differ from the rows of a buffer whose row 0 starts the episodes, on the rows behind a seam
    assert not np.array_equal(full[Tr:2 * Tr + 1], stack_rows_reference(obs.cpu().numpy()[Tr:2 * Tr + 1], ended.cpu().numpy()[Tr:2 * Tr]))
    # episodes longer than a rollout end: impossible when every rollout starts from a reset
    assert max(int(s["eplen"].max()) for s in snaps) > Tr
    # the exploration decay counts the reset's N episode starts once
    eps = [int(s["ended"].sum()) for s in snaps]
    assert [s["starts"] for s in snaps] == [eps[0] + 40, eps[1], eps[2]]
    # norm_reward: the running return crosses the seams -- the host mirror chained through its carry
    want, carry = ppo.RET_RMS_INIT, None
    for s in snaps:
        r = ppo.reward_norm_reference(s["rew"].cpu().numpy(), s["ended"].cpu().numpy(), gamma, rms=want[:3], carry=carry)
        want, carry = r.rms, r.carry
    assert abs(ret_rms[0] - want[0]) <= 1e-12 * np.sqrt(want[1]) and abs(ret_rms[1] - want[1]) <= 1e-12 * want[1]
    assert ret_rms[2] == want[2]
    cold = ppo.RET_RMS_INIT
    for s in snaps:
        cold = ppo.reward_norm_reference(s["rew"].cpu().numpy(), s["ended"].cpu().numpy(), gamma, rms=cold[:3]).rms
    assert abs(cold[1] - want[1]) > 1e-9 * want[1]   # (without the carry the statistics are others: the check can fail)


def test_trainer_resets_again_when_told_or_when_the_world_changes():
    tr = _trainer(continue_rollouts=True)
    try:
        snaps = _run(tr, 2)
        tr.reset_envs()
        snaps += _run(tr, 1)
        tr.env.sim.set_map(maps.by_name("stage_1"))   # bumps sim.generation
        snaps += _run(tr, 1)
        snaps += _run(tr, 1)
    finally:
        tr.env.close()
    Tr = TR["rollout_len"]
    assert same(snaps[1]["obs"][0], snaps[0]["obs"][Tr])
    for k in (2, 3):   # reset rows: past_action zero, and not the row the last rollout stopped at
        assert not same(snaps[k]["obs"][0], snaps[k - 1]["obs"][Tr]) and not bool(snaps[k]["obs"][0][:, 10:12].any())
        assert same(snaps[k]["hist"][0, :, 16:26], snaps[k]["obs"][0][:, 0:10])
    assert same(snaps[4]["obs"][0], snaps[3]["obs"][Tr])
    acts = [torch.cat([snaps[0]["act"], snaps[1]["act"]]), snaps[2]["act"], torch.cat([snaps[3]["act"], snaps[4]["act"]])]
    rep = _replay(acts)
    assert same(rep[0][0], torch.cat([snaps[0]["obs"], snaps[1]["obs"][1:]])) and same(rep[1][0], snaps[2]["obs"])
    assert same(rep[2][0], torch.cat([snaps[3]["obs"], snaps[4]["obs"][1:]]))


def test_option_off_every_rollout_starts_from_a_reset():
    tr = _trainer()
    try:
        assert tr.continue_rollouts is False and not hasattr(tr, "_hist_carry")
        snaps = _run(tr, 2)
    finally:
        tr.env.close()
    Tr = TR["rollout_len"]
    assert not same(snaps[1]["obs"][0], snaps[0]["obs"][Tr])
    rep = _replay([s["act"] for s in snaps])
    for k, s in enumerate(snaps):   # the parent's rule: row 0 is a reset row each time, history rows start there
        assert same(rep[k][0], s["obs"]) and same(rep[k][1], s["ended"]), k
        assert np.array_equal(s["hist"].cpu().numpy(), stack_rows_reference(s["obs"].cpu().numpy(), s["ended"].cpu().numpy())), k
        assert int(s["eplen"].max()) <= Tr
        assert s["starts"] == int(s["ended"].sum()) + 40


CONT_CASES = {   # name -> (PPOConfig options over TR + continue_rollouts, VecEnv options)
    "mlp64x2-16-columns": (dict(scan_history=False), {}),
    "resmlp512": (dict(policy="resmlp512", scan_history=False), {}),
    "history-float16": (dict(), dict(obs_f16=True)),
    "graph": (dict(scan_history=False, persistent_rollout=False), {}),
    "per-step": (dict(scan_history=False, persistent_rollout=False, use_graph=False), {}),
}


@pytest.mark.parametrize("case", list(CONT_CASES))
def test_trainer_continues_on_every_rollout_path(case):
    """test_trainer_continues_across_iterations' trajectory check for the other nets, row formats and rollout paths: three iterations
    are ONE trajectory.  On the hipGraph path the first rollout captures -- the warm-up steps the envs, so it resets a second time --
    and the two behind it replay the graph and continue; the replay of that case starts from the state the envs had behind that
    second reset (a fresh env's reset alone is not where they stood)."""
    cfg_kw, env_kw = CONT_CASES[case]
    tr = _trainer(env_kw, continue_rollouts=True, **cfg_kw)
    states = []
    try:
        reset = tr.env.sim.reset

        def recording_reset(obs, mask=None):
            out = reset(obs, mask)
            torch.cuda.synchronize()
            states.append(tr.env.sim.get_state())
            return out

        tr.env.sim.reset = recording_reset
        persistent, graph = tr.uses_persistent_rollout, tr._graph
        snaps = _run(tr, 3)
        graph_after = tr._graph
    finally:
        tr.env.close()
    Tr = TR["rollout_len"]
    on_graph = case == "graph"
    assert persistent == (case not in ("graph", "per-step")) and graph is None and (graph_after is not None) == on_graph
    assert [s["did_reset"] for s in snaps] == [True, False, False]
    assert len(states) == (2 if on_graph else 1)
    for a, b in zip(snaps[:-1], snaps[1:]):
        assert same(b["obs"][0], a["obs"][Tr])   # row 0 is the row the last rollout stopped at
    (obs, ended), = _replay([torch.cat([s["act"] for s in snaps])], env_kw, state=states[-1] if on_graph else None)
    if on_graph:   # (row 0 is the second reset's; the replaying env wrote its own first one)
        assert same(obs[1:], torch.cat([s["obs"][1:] for s in snaps]))
    else:
        assert same(obs, torch.cat([snaps[0]["obs"]] + [s["obs"][1:] for s in snaps[1:]]))
    assert same(ended, torch.cat([s["ended"] for s in snaps]))
    assert max(int(s["eplen"].max()) for s in snaps) > Tr     # episodes longer than a rollout end
    assert 0 < int(ended.sum()) < ended.numel()
    if case == "history-float16":
        assert snaps[0]["obs"].dtype == torch.float16 and snaps[0]["hist"].dtype == torch.float16
        full = stack_rows_reference(obs.cpu().numpy(), ended.cpu().numpy())
        for k, s in enumerate(snaps):
            assert np.array_equal(s["hist"].cpu().numpy().view(np.uint16), full[k * Tr:(k + 1) * Tr + 1].view(np.uint16)), k
    else:
        assert "hist" not in snaps[0]
    eps = [int(s["ended"].sum()) for s in snaps]
    assert [s["starts"] for s in snaps] == [eps[0] + 40, eps[1], eps[2]]


def test_history_off_the_persistent_rollout_is_refused():
    """scan_history lives in the persistent rollout kernel alone: with continue_rollouts as without, the other paths refuse it"""
    for kw in (dict(persistent_rollout=False), dict(persistent_rollout=False, use_graph=False), dict(fused_update=False)):
        with pytest.raises(ValueError, match="scan_history needs persistent_rollout=True and fused_update=True"):
            ppo.PPOConfig(**{**TR, **kw}, continue_rollouts=True)
    with pytest.raises(ValueError, match="scan_history with policy='resmlp512'"):
        ppo.PPOConfig(**{**TR, "policy": "resmlp512"}, continue_rollouts=True)


# ---------------------------------------------------------------- 6. two ranks
RANKS_CAP = 12   # two iterations are 16 steps: under the cap of 20 no episode would time out, under this one every env's does on row 11


def _cont_rank_worker(rank, world, port, path):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      NAVBOT_DIST_BACKEND="gloo")   # RCCL refuses two ranks on one device: gloo carries the all-reduce here
    ctx = ppo.DistCtx(device="cuda:0")
    lo, hi = ctx.shard(40)
    env = VecEnv(hi - lo, **{**ENV, "max_episode_steps": RANKS_CAP}, env_id_base=lo)
    tr = ppo.PPOTrainer(env, ppo.PPOConfig(**{**TR, "max_episode_steps": RANKS_CAP}, continue_rollouts=True), ctx)
    try:
        snaps = _run(tr, 2)
        torch.save({"snaps": [{k: v.cpu() if torch.is_tensor(v) else v for k, v in s.items()} for s in snaps],
                    "flat": tr.updater.fp.flat.cpu(), "base": tr._env_id_base}, f"{path}.{rank}")
    finally:
        env.close()
    ctx.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_continue_like_one_process_that_plays_both(tmp_path):
    """Shards of 20 + 20 envs with scan_history, two iterations: every rank's rows, flags and history rows are those of ONE env of
    all 40 under the recorded actions -- a single reset -- and the ranks hold the same weights."""
    path = str(tmp_path / "cont")
    spawn_ranks(_cont_rank_worker, 2, lambda port: (2, port, path))
    ranks = [torch.load(f"{path}.{r}", weights_only=False) for r in range(2)]
    assert [r["base"] for r in ranks] == [0, 20]
    assert same(ranks[0]["flat"], ranks[1]["flat"])
    Tr = TR["rollout_len"]
    cat = lambda k, it: torch.cat([r["snaps"][it][k] for r in ranks], dim=1)
    (obs, ended), = _replay([torch.cat([cat("act", 0), cat("act", 1)]).to(DEV)], dict(max_episode_steps=RANKS_CAP))
    obs, ended = obs.cpu(), ended.cpu()
    assert bool(ended[RANKS_CAP - 1].any()) and 0 < int(ended.sum()) < ended.numel()
    full = stack_rows_reference(obs.numpy(), ended.numpy())
    for it in range(2):
        assert [r["snaps"][it]["did_reset"] for r in ranks] == [it == 0] * 2
        assert same(cat("obs", it), obs[it * Tr:(it + 1) * Tr + 1]), it
        assert same(cat("ended", it), ended[it * Tr:(it + 1) * Tr]), it
        assert np.array_equal(cat("hist", it).numpy().view(np.uint32), full[it * Tr:(it + 1) * Tr + 1].view(np.uint32)), it
    assert not np.array_equal(full[Tr:], stack_rows_reference(obs.numpy()[Tr:], ended.numpy()[Tr:]))   # the carry mattered
    assert max(int(cat("eplen", it).max()) for it in range(2)) == RANKS_CAP > Tr     # an episode longer than a rollout ended
