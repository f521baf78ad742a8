"""navppo_group_sums (csrc/ppo_group_sums.hip): navppo_episode_sums per group of envs, against its host mirror.

Shapes (T, N, K): (1, 1, 1) the smallest; (3, 17, 4) with one empty group; (37, 40, 3) N ragged to 16 and 64; (64, 129, 5) N % 4 != 0;
(40, 4112, 32) more columns than one workgroup of lanes per row (17 workgroups along N, the last one 16 columns wide) and several
chunks of T.  Each with and without advantages, the ids in no order.  Columns 0-4 and 7 are integers and must be exact; columns 5 and 6
are float64 sums of float32 terms in an order of the kernel's own, so |got - ref| <= n 2^-53 sum|x| with n the number of summands --
the bound that holds for any summation order in float64.  Every buffer of every call sits inside guarded allocations.

CHUNKS: the shapes that exist for the way T is cut (gs_cut in the kernel's file: the rows of a chunk and the chunk count, which the
workspace size and both launches share).  group_sums_final gives wave w of its 16 the chunks w, w + 16, ...; each case names the
count it needs -- read back from navppo_group_sums_ws_bytes -- so that another cut fails the case instead of hollowing it out.
(137, 40, 3): 18 chunks, waves 0 and 1 take two, the last chunk is one row; (300, 40, 3): 38, waves 0..5 take three; (2049, 5, 2):
256 aimed for, 9 rows each, so 228 with a last one of 6 rows; (2048, 17, 2): 256, the maximum, 16 per wave.  The 4096-column tile of
group_sums_final: N = 4096 (one tile exactly), 4097 (a second tile of one column: every other id load of it is clamped to N - 1),
8200 (three tiles, the last one 8 columns).  K = 1024, the maximum (at most 48 groups hold an env), and K = 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _guards import ptr, run_both
from _movers import blade_tape
from navbot_ppo_amd import maps, ppo
from navbot_ppo_amd._native import NavsimError, _navppo, lib
from navbot_ppo_amd.env import VecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F64 = torch.float64
CHUNKS = {(137, 40, 3): 18, (300, 40, 3): 38, (2049, 5, 2): 228, (2048, 17, 2): 256, (9, 4096, 4): 2, (9, 4097, 4): 2, (9, 8200, 7): 2,
          (24, 48, 1024): 3, (24, 48, 1): 3}
SHAPES = [(1, 1, 1), (3, 17, 4), (37, 40, 3), (64, 129, 5), (40, 4112, 32)] + list(CHUNKS)
U = 2.0 ** -53
NAN_BYTE = 0xFF      # eight of them: a NaN double (sign, exponent and mantissa all ones)


def n_chunks(T, N, K):
    """how many chunks the entry point cuts T into: its workspace is [chunks][7][N] float64"""
    nbytes = int(lib().navppo_group_sums_ws_bytes(T, N, K))
    assert nbytes > 0 and nbytes % (7 * N * 8) == 0
    return nbytes // (7 * N * 8)


@functools.lru_cache(maxsize=None)
def _case(T, N, K):
    """random rollout buffers with all four outcomes (flags also set on rows that did not end), ids in no order, and the reference"""
    rng = np.random.default_rng(1000 * T + N)
    b = dict(ended=(rng.random((T, N)) < 0.3).astype(np.uint8),
             arrive=((rng.random((T, N)) < 0.4) * rng.integers(1, 256, (T, N))).astype(np.uint8),
             done=(rng.random((T, N)) < 0.5).astype(np.uint8),
             ep_length=rng.integers(0, 501, (T, N)).astype(np.int32),
             ep_return=(rng.standard_normal((T, N)) * 100).astype(np.float32),
             adv=rng.standard_normal((T, N)).astype(np.float32),
             group=rng.integers(0, K, N).astype(np.int32))
    if (T, N, K) == (3, 17, 4):
        b["group"][b["group"] == 2] = 3          # group 2 has no env
        b["group"][:3] = [3, 0, 1]
    for v in b.values():
        v.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _reference(T, N, K, with_adv):
    b = _case(T, N, K)
    return ppo.group_sums_reference(b["ended"], b["arrive"], b["done"], b["ep_length"], b["ep_return"], b["group"], K,
                                    adv=b["adv"] if with_adv else None)


def _bounds(b, K, with_adv):
    """[K, 2]: n 2^-53 sum|x| for columns 5 (the ended entries' returns) and 6 (every entry's |adv|)"""
    out = np.zeros((K, 2))
    e = b["ended"] != 0
    for k in range(K):
        c = b["group"] == k
        out[k, 0] = e[:, c].sum() * U * np.abs(np.where(e, b["ep_return"].astype(np.float64), 0.0)[:, c]).sum()
        if with_adv:
            out[k, 1] = e[:, c].size * U * np.abs(b["adv"].astype(np.float64)[:, c]).sum()
    return out


def _assert_sums(got, want, bounds, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    exact = [0, 1, 2, 3, 4, 7]
    assert np.array_equal(got[:, exact], want[:, exact]), f"{what}: counts\n{got[:, exact]}\n{want[:, exact]}"
    err = np.abs(got[:, 5:7] - want[:, 5:7])
    print(f"{what}: max |got - ref| = {err.max(axis=0)} of bound {bounds.max(axis=0)}")
    assert (err <= bounds).all(), f"{what}: {err} > {bounds}"


def _guarded_call(b, T, N, K, with_adv, twice=False, ws_fill=None):
    """ws_fill: the byte the workspace holds before the call (default: the guards' canary)"""
    def call(g):
        t = {k: g.inp(torch.from_numpy(np.array(v)), 4 if v.dtype.itemsize == 4 else 1) for k, v in b.items() if k != "adv" or with_adv}
        ws = g.scratch(int(lib().navppo_group_sums_ws_bytes(T, N, K)), 8)
        if ws_fill is not None:
            ws.fill_(ws_fill)
        out = g.out((K, 8), F64, 8)
        args = (t["ended"], t["arrive"], t["done"], t["ep_length"], t["ep_return"], t["group"], K)
        ppo.group_sums(*args, adv=t.get("adv"), out=out, workspace=ws)
        if twice:   # the same buffers, the same workspace, another output: the same bits
            again = g.out((K, 8), F64, 8)
            ppo.group_sums(*args, adv=t.get("adv"), out=again, workspace=ws)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), again.view(torch.int64))
        return out
    return run_both(DEV, call, f"navppo_group_sums {(T, N, K)} adv={with_adv}")   # guards intact, no canary left, both placements equal


@pytest.mark.parametrize("with_adv", [False, True], ids=["noadv", "adv"])
@pytest.mark.parametrize("T, N, K", SHAPES)
def test_against_the_host_mirror_inside_guards(T, N, K, with_adv):
    b = _case(T, N, K)
    want = _reference(T, N, K, with_adv)
    got = _guarded_call(b, T, N, K, with_adv, twice=True)
    _assert_sums(got, want, _bounds(b, K, with_adv), f"{(T, N, K)} adv={with_adv}")
    if (T, N, K) == (3, 17, 4):
        assert not got[2].cpu().numpy().any()        # a group without envs: a zero row
    if not with_adv:
        assert not got[:, 6].cpu().numpy().any()
    assert want[:, 7].sum() == T * N
    if (T, N, K) in CHUNKS:     # the case reaches what it is here for
        c = n_chunks(T, N, K)
        assert c == CHUNKS[(T, N, K)], (c, CHUNKS[(T, N, K)])
        if T >= 137:
            assert c > 16       # some wave of group_sums_final takes a second chunk
        if (T, N, K) == (2049, 5, 2):
            assert c < 256      # fewer chunks than the 256 aimed for
        if K == 1024:
            assert 1 < (want[:, 7] > 0).sum() <= N and not got.cpu().numpy()[want[:, 7] == 0].any()
        if K == 1:
            assert want[0, 7] == T * N


def _bits(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else x).view(np.int64)


# ---------------------------------------------------------------- what the contract allows the buffers and the workspace to hold
@pytest.mark.parametrize("T, N, K", [(37, 40, 3), (137, 40, 3), (9, 4097, 4)])
def test_garbage_where_no_episode_ended_is_not_read(T, N, K):
    """ep_return is written only where an episode ended (include/navppo.h): everywhere else a real buffer holds whatever it held.
    NaN, +inf, -inf and -0.0 there, with arrive and done set as well: the sums are the clean buffers' -- the mirror's within the
    file's bounds, and bit for bit the kernel's own on the clean buffers (it masks the return's bits, so a not-ended entry adds +0.0
    either way, in the same order)."""
    b = _case(T, N, K)
    quiet = b["ended"] == 0
    dirty = dict(b)
    junk = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)[(np.arange(T)[:, None] + np.arange(N)[None, :]) % 4]
    dirty["ep_return"] = np.where(quiet, junk, b["ep_return"]).astype(np.float32)
    dirty["arrive"] = np.where(quiet, 0xFF, b["arrive"]).astype(np.uint8)
    dirty["done"] = np.where(quiet, 1, b["done"]).astype(np.uint8)
    for k in range(K):      # every group holds each of the four values on an entry that did not end
        col = b["group"] == k
        if col.any():
            q = quiet[:, col]
            x = dirty["ep_return"][:, col][q]
            assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any() and (np.signbit(x) & (x == 0)).any(), k
    want = _reference(T, N, K, True)
    assert np.isfinite(want).all()
    got = _guarded_call(dirty, T, N, K, True)
    _assert_sums(got, want, _bounds(b, K, True), f"garbage on not-ended entries {(T, N, K)}")
    clean = _guarded_call(b, T, N, K, True)
    assert np.array_equal(_bits(got), _bits(clean))
    # (the mirror states the same rule)
    mirror = ppo.group_sums_reference(dirty["ended"], dirty["arrive"], dirty["done"], dirty["ep_length"], dirty["ep_return"],
                                      dirty["group"], K, adv=dirty["adv"])
    assert np.array_equal(_bits(mirror), _bits(want))


@pytest.mark.parametrize("T, N, K", [(37, 40, 3), (300, 40, 3)])
def test_a_non_finite_advantage_stays_in_its_group(T, N, K):
    b = _case(T, N, K)
    clean = _guarded_call(b, T, N, K, True).cpu().numpy()
    n = N - 3                     # (a column of the ragged last wave)
    k = int(b["group"][n])
    adv = np.array(b["adv"])
    adv[T - 1, n] = np.nan        # the last row: at T = 300 the one chunk of wave 5's third trip
    bad = dict(b, adv=adv)
    want = ppo.group_sums_reference(bad["ended"], bad["arrive"], bad["done"], bad["ep_length"], bad["ep_return"], bad["group"], K, adv=adv)
    assert np.isnan(want[k, 6]) and np.isnan(want).sum() == 1
    got = _guarded_call(bad, T, N, K, True).cpu().numpy()
    assert np.isnan(got[k, 6])
    others = np.arange(K) != k
    assert np.array_equal(_bits(got[others]), _bits(clean[others]))                       # no other group sees it
    assert np.array_equal(_bits(got[k, [0, 1, 2, 3, 4, 5, 7]]), _bits(clean[k, [0, 1, 2, 3, 4, 5, 7]]))   # and no count changes


@pytest.mark.parametrize("with_adv", [False, True], ids=["noadv", "adv"])
@pytest.mark.parametrize("T, N, K", [(37, 40, 3), (300, 40, 3)])
def test_a_stale_workspace_does_not_leak(T, N, K, with_adv):
    """The trainer keeps one workspace for the whole run.  Every double of it a NaN before the call: the sums are the bits of a call
    on a zeroed workspace -- also without advantages, where figure 6 of the workspace is neither written nor read."""
    b = _case(T, N, K)
    zeroed = _guarded_call(b, T, N, K, with_adv, ws_fill=0)
    stale = _guarded_call(b, T, N, K, with_adv, ws_fill=NAN_BYTE, twice=True)
    assert np.array_equal(_bits(stale), _bits(zeroed))
    assert np.isfinite(stale.cpu().numpy()).all()
    _assert_sums(stale, _reference(T, N, K, with_adv), _bounds(b, K, with_adv), f"stale workspace {(T, N, K)} adv={with_adv}")
    if not with_adv:
        assert np.array_equal(_bits(stale[:, 6]), np.zeros(K, np.int64))      # +0.0 exactly


@pytest.mark.parametrize("T, N, K", [(37, 40, 3), (300, 40, 3)])
def test_one_workspace_with_and_then_without_advantages(T, N, K):
    """with adv the call fills figure 6 of the workspace; the next call without adv must not pick it up"""
    b = _case(T, N, K)
    fresh = _guarded_call(b, T, N, K, False)

    def call(g):
        t = {k: g.inp(torch.from_numpy(np.array(v)), 4 if v.dtype.itemsize == 4 else 1) for k, v in b.items()}
        ws = g.scratch(int(lib().navppo_group_sums_ws_bytes(T, N, K)), 8)
        first, second = g.out((K, 8), F64, 8), g.out((K, 8), F64, 8)
        args = (t["ended"], t["arrive"], t["done"], t["ep_length"], t["ep_return"], t["group"], K)
        ppo.group_sums(*args, adv=t["adv"], out=first, workspace=ws)
        ppo.group_sums(*args, adv=None, out=second, workspace=ws)
        torch.cuda.synchronize()
        assert bool((first[:, 6] > 0).all())
        return second
    second = run_both(DEV, call, f"navppo_group_sums {(T, N, K)} adv, then none, one workspace")
    assert np.array_equal(_bits(second), _bits(fresh))
    assert np.array_equal(_bits(second[:, 6]), np.zeros(K, np.int64))


@pytest.mark.parametrize("T, N, K", SHAPES)
def test_rows_add_up_to_navppo_episode_sums(T, N, K):
    b = _case(T, N, K)
    t = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in b.items()}
    got = ppo.group_sums(t["ended"], t["arrive"], t["done"], t["ep_length"], t["ep_return"], t["group"], K).cpu().numpy()
    six = torch.empty(6, dtype=F64, device=DEV)
    ws = torch.empty(256 * 6, dtype=F64, device=DEV)
    _navppo("navppo_episode_sums", ptr(t["ended"]), ptr(t["arrive"]), ptr(t["done"]), ptr(t["ep_length"]), ptr(t["ep_return"]), T * N,
            ptr(six), ptr(ws))
    six = six.cpu().numpy()
    assert np.array_equal(got[:, :5].sum(axis=0), six[:5])
    e = b["ended"] != 0
    bound = e.sum() * U * np.abs(np.where(e, b["ep_return"].astype(np.float64), 0.0)).sum()
    assert abs(got[:, 5].sum() - six[5]) <= bound


def test_ids_outside_the_groups_are_dropped():
    T, N, K = 37, 40, 3
    b = dict(_case(T, N, K))
    g = np.array(b["group"])
    g[[0, 7, 16, 39]] = [-1, K, -1, K]      # (in the first, the ragged and the last lanes of a wave)
    b["group"] = g
    keep = (g >= 0) & (g < K)
    sub = {k: (v[keep] if k == "group" else np.ascontiguousarray(v[:, keep])) for k, v in b.items()}
    want = ppo.group_sums_reference(sub["ended"], sub["arrive"], sub["done"], sub["ep_length"], sub["ep_return"], sub["group"], K,
                                    adv=sub["adv"])
    got = _guarded_call(b, T, N, K, True)
    _assert_sums(got, want, _bounds(sub, K, True), "ids -1 and K")
    assert got[:, 7].sum().item() == T * keep.sum()
    # ids far outside: nothing is indexed by them (the guards of every buffer stay intact), every row is zero
    b["group"] = np.full(N, np.iinfo(np.int32).max, dtype=np.int32)
    b["group"][::2] = np.iinfo(np.int32).min
    assert not _guarded_call(b, T, N, K, True).cpu().numpy().any()


def test_the_shim_refuses_before_any_pointer_crosses():
    T, N, K = 5, 12, 3
    b = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in _case(37, 40, 3).items()}
    b = {k: (v[:N] if k == "group" else v[:T, :N]).contiguous() for k, v in b.items()}
    order = ("ended", "arrive", "done", "ep_length", "ep_return", "group")

    def call(**kw):
        a = dict(b, **kw)
        return ppo.group_sums(*[a[k] for k in order], a.get("K", K), adv=a.get("adv_"), out=a.get("out"), workspace=a.get("workspace"))
    call()
    call(adv_=b["adv"])
    bad = [dict(ended=b["ended"].int()), dict(arrive=b["arrive"].bool()), dict(done=b["done"].float()),
           dict(ep_length=b["ep_length"].long()), dict(ep_return=b["ep_return"].double()), dict(group=b["group"].long()),
           dict(adv_=b["adv"].double()), dict(out=torch.empty((K, 8), device=DEV)),                     # dtypes
           dict(arrive=b["arrive"][:, :N - 1].contiguous()), dict(ep_length=b["ep_length"][:T - 1]), dict(group=b["group"][:N - 1]),
           dict(ended=b["ended"].reshape(-1)), dict(adv_=b["adv"].reshape(N, T)), dict(out=torch.empty((K, 6), dtype=F64, device=DEV)),
           dict(out=torch.empty((K + 1, 8), dtype=F64, device=DEV)),                                     # shapes
           dict(done=b["done"].cpu()), dict(group=b["group"].cpu()), dict(ended=b["ended"].cpu()),
           dict(out=torch.empty((K, 8), dtype=F64)),                                                     # devices
           dict(ep_return=b["ep_return"].t().contiguous().t()), dict(group=torch.zeros(2 * N, dtype=torch.int32, device=DEV)[::2]),
           dict(adv_=torch.zeros((T, 2 * N), device=DEV)[:, ::2]),                                       # not contiguous
           dict(K=0), dict(K=1025), dict(K=2.0), dict(K=True),
           dict(workspace=torch.empty(8, dtype=torch.uint8, device=DEV)), dict(workspace=torch.empty(1 << 16, dtype=F64, device=DEV))]
    for kw in bad:
        with pytest.raises(NavsimError, match="group_sums"):
            call(**kw)


def test_the_entry_point_refuses_nulls_and_bad_sizes():
    L = lib()
    assert L.navppo_group_sums_ws_bytes(0, 4, 2) == 0 and L.navppo_group_sums_ws_bytes(4, 0, 2) == 0
    assert L.navppo_group_sums_ws_bytes(4, 4, 0) == 0 and L.navppo_group_sums_ws_bytes(4, 4, 1025) == 0
    assert L.navppo_group_sums_ws_bytes(-1, 4, 2) == 0 and L.navppo_group_sums_ws_bytes(4, 4, 1024) > 0
    T, N, K = 4, 8, 2
    u8 = [torch.zeros((T, N), dtype=torch.uint8, device=DEV) for _ in range(3)]
    ln, rt = torch.zeros((T, N), dtype=torch.int32, device=DEV), torch.zeros((T, N), device=DEV)
    grp, out = torch.zeros(N, dtype=torch.int32, device=DEV), torch.full((K, 8), -1.0, dtype=F64, device=DEV)
    ws = torch.empty(int(L.navppo_group_sums_ws_bytes(T, N, K)), dtype=torch.uint8, device=DEV)
    good = [ptr(u8[0]), ptr(u8[1]), ptr(u8[2]), ptr(ln), ptr(rt), None, ptr(grp), T, N, K, ptr(out), ptr(ws)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.navppo_group_sums(*good, stream) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[0, 0, 0, 0, 0, 0, 0, T * N], [0] * 8]
    out.fill_(-1.0)
    for i in (0, 1, 2, 3, 4, 6, 10, 11):          # every required pointer, the workspace included (adv, 5, may be null)
        a = list(good)
        a[i] = None
        assert L.navppo_group_sums(*a, stream) == -1
        assert L.navppo_last_error().decode().startswith("navppo_group_sums: ")
    for i, v in ((7, 0), (8, 0), (9, 0), (9, 1025), (7, -3)):
        a = list(good)
        a[i] = v
        assert L.navppo_group_sums(*a, stream) == -1 and b"navppo_group_sums" in L.navppo_last_error()
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())              # a refused call launched nothing


# ---------------------------------------------------------------- the buffers of a real rollout over three blade tapes
def test_on_a_real_rollout_over_three_blade_tapes():
    N, T, K = 40, 60, 3
    bank, periods, _ = maps.mover_bank([blade_tape(P, M, radius=r) for P, M, r in ((5, 3, 0.75), (8, 17, 0.60), (13, 32, 0.90))])
    tid = np.random.default_rng(7).integers(0, K, N).astype(np.int32)
    env = VecEnv(N, map="stage_1", max_episode_steps=25, seed=5, device=DEV, movers=dict(bank=bank, periods=periods, assign=tid))
    try:
        torch.manual_seed(11)
        r = env.rollout_mlp64(torch.randn(5378, device=DEV) * 0.3, T, 0.8, seed=9)
        grp = env.sim.movers_tape_id
        assert np.array_equal(grp.cpu().numpy(), tid)
        adv = torch.randn((T, N), device=DEV)
        got = ppo.group_sums(r.ended, r.arrive, r.done, r.ep_length, r.ep_return, grp, K, adv=adv).cpu().numpy()
        h = {k: getattr(r, k).cpu().numpy() for k in ("ended", "arrive", "done", "ep_length", "ep_return")}
        h.update(adv=adv.cpu().numpy(), group=tid)
    finally:
        env.close()
    want = ppo.group_sums_reference(h["ended"], h["arrive"], h["done"], h["ep_length"], h["ep_return"], tid, K, adv=h["adv"])
    _assert_sums(got, want, _bounds(h, K, True), "rollout over three blade tapes")
    assert (got[:, 0] > 0).all() and got[:, 0].sum() == (h["ended"] != 0).sum()      # every tape ended episodes
    assert got[:, 2].sum() > 0 and got[:, 3].sum() > 0                               # collisions (the blades) and time-outs
    assert np.array_equal(got[:, 7], T * np.bincount(tid, minlength=K))
