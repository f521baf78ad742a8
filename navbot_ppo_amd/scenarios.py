"""Scenario-prioritised training on a bank of mover tapes (PPOConfig.scenario_stats / scenario_priority): the per-scenario sums of a
rollout on the device (navppo_group_sums) with their host mirror, and the rule that turns them into the next assignment of envs to
scenarios (ScenarioSampler: rank-prioritised level replay, Jiang et al. 2021, with a uniform floor in place of the staleness term and
one assignment per iteration in place of one draw per episode)."""
import numpy as np

from .config import SCENARIO_PRIORITIES  # noqa: F401

GROUP_SUMS_COLS = 8   # NAVPPO_GROUP_SUMS_COLS: episodes, successes, collisions, time-outs, sum ep_length, sum ep_return, sum |adv|, rows
SCENARIO_CSV_HEADER = ["iteration", "scenario", "envs", "episodes", "success_rate", "collision_rate", "timeout_rate", "score", "weight"]
_MASK = 0xFFFFFFFFFFFFFFFF
_SALT = 0x3C6EF372FE94F82B    # the sampler's own salt of maps._env_hash (the phases' and the tape ids' are others)
_STEP = 0xA0761D6478BD642F    # what one re-assignment adds to it


def group_sums_reference(ended, arrive, done, ep_length, ep_return, group, K, adv=None):
    """Host mirror of navppo_group_sums, numpy float64 -- the statement of the rule.  ended, arrive, done [T, N] (non-zero = set),
    ep_length [T, N] integers, ep_return [T, N] float32, adv [T, N] float32 or None, group [N] integers.  Returns [K, 8] float64, row k
    over the columns n with group[n] == k (an id outside [0, K) is counted in no row; a group without envs gives a zero row):
        0 episodes    = sum ended                         4 sum of ep_length over ALL entries
        1 successes   = sum ended & arrive                5 sum of ep_return over ended entries
        2 collisions  = sum ended & done & ~arrive        6 sum of |adv| over all entries (0 without adv)
        3 time-outs   = sum ended & ~done & ~arrive       7 rows = T x the number of envs of the group
    -- entry by entry the figures of navppo_episode_sums, which the rows add up to."""
    e = np.asarray(ended) != 0
    T, N = e.shape
    a = (np.asarray(arrive).reshape(T, N) != 0) & e
    d = (np.asarray(done).reshape(T, N) != 0) & e
    ln = np.asarray(ep_length).reshape(T, N).astype(np.float64)
    rt = np.where(e, np.asarray(ep_return, dtype=np.float32).reshape(T, N).astype(np.float64), 0.0)
    ab = None if adv is None else np.abs(np.asarray(adv, dtype=np.float32).reshape(T, N).astype(np.float64))
    g = np.asarray(group).reshape(N)
    out = np.zeros((int(K), GROUP_SUMS_COLS), dtype=np.float64)
    for k in range(int(K)):
        c = g == k
        out[k] = [e[:, c].sum(), a[:, c].sum(), (d & ~a)[:, c].sum(), (e & ~d & ~a)[:, c].sum(), ln[:, c].sum(), rt[:, c].sum(),
                  0.0 if ab is None else ab[:, c].sum(), float(T) * int(c.sum())]
    return out


def group_sums(ended, arrive, done, ep_length, ep_return, group, K, adv=None, out=None, workspace=None):
    """navppo_group_sums on device tensors: ended / arrive / done [T, N] uint8, ep_length [T, N] int32, ep_return [T, N] float32,
    adv [T, N] float32 or None, group [N] int32 -> [K, 8] float64 (``out`` if given); group_sums_reference states the rule.  Every
    tensor is checked -- dtype, shape, device, contiguity -- before its pointer crosses the ABI.  workspace: a contiguous uint8 tensor of
    at least navppo_group_sums_ws_bytes(T, N, K) bytes to reuse (default: allocated here).  Asynchronous on the current stream."""
    import torch
    from ._native import NavsimError, _navppo, _ptr, lib
    what = "group_sums"
    if not torch.is_tensor(ended) or not ended.is_cuda:
        raise NavsimError(f"{what} needs device tensors; there is no CPU path (group_sums_reference is the host mirror)")
    if ended.dim() != 2:
        raise NavsimError(f"{what}: ended must be [T, N], got {tuple(ended.shape)}")
    T, N, dev = int(ended.shape[0]), int(ended.shape[1]), ended.device
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= 1024:
        raise NavsimError(f"{what}: K {K!r}: an integer in [1, 1024]")
    K = int(K)
    if T < 1 or N < 1 or T >= 1 << 31 or N >= 1 << 31:
        raise NavsimError(f"{what}: T and N must lie in [1, 2^31), got {(T, N)}")

    def chk(name, t, dtype, shape, align):
        if (not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                or t.data_ptr() % align):
            raise NavsimError(f"{what}: {name} must be a contiguous {dtype} tensor {tuple(shape)} on {dev}, {align}-byte aligned, got "
                              f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}"
                              f"{'' if not torch.is_tensor(t) or t.is_contiguous() else ' (not contiguous)'}")
    chk("ended", ended, torch.uint8, (T, N), 1)
    chk("arrive", arrive, torch.uint8, (T, N), 1)
    chk("done", done, torch.uint8, (T, N), 1)
    chk("ep_length", ep_length, torch.int32, (T, N), 4)
    chk("ep_return", ep_return, torch.float32, (T, N), 4)
    chk("group", group, torch.int32, (N,), 4)
    if adv is not None:
        chk("adv", adv, torch.float32, (T, N), 4)
    if out is None:
        out = torch.empty((K, GROUP_SUMS_COLS), dtype=torch.float64, device=dev)
    chk("out", out, torch.float64, (K, GROUP_SUMS_COLS), 8)
    need = int(lib().navppo_group_sums_ws_bytes(T, N, K))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if (not torch.is_tensor(workspace) or workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
            or workspace.numel() < need or workspace.data_ptr() % 8):
        raise NavsimError(f"{what}: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {need} bytes on {dev}")
    with torch.cuda.device(dev):
        _navppo("navppo_group_sums", _ptr(ended), _ptr(arrive), _ptr(done), _ptr(ep_length), _ptr(ep_return), _ptr(adv), _ptr(group),
                T, N, K, _ptr(out), _ptr(workspace))
    return out


def scenario_rows(G, envs_per_scenario, sampler, iteration):
    """One dict per scenario for <method>_train_scenarios.csv (SCENARIO_CSV_HEADER): evaluate.scenario_report's fields (scenario,
    episodes and the success, collision and time-out rate, NaN where no episode ended) plus iteration, envs, score and weight, from the
    global [K, 8] sums G, the [K] envs per scenario over all ranks and the sampler's scores."""
    w, nan = sampler.weights(), float("nan")
    rows = []
    for k in range(sampler.K):
        ep = G[k, 0]
        rows.append(dict(iteration=iteration, scenario=k, envs=int(envs_per_scenario[k]), episodes=int(ep),
                         success_rate=float(G[k, 1] / ep) if ep else nan, collision_rate=float(G[k, 2] / ep) if ep else nan,
                         timeout_rate=float(G[k, 3] / ep) if ep else nan, score=float(sampler.score[k]), weight=float(w[k])))
    return rows


class ScenarioSampler:
    """Scores per scenario from the [K, 8] sums of navppo_group_sums, and the assignment of envs to scenarios they lead to.  Pure
    numpy, deterministic, no generator streams: the same on every rank and under every numpy version.

    State: ``score`` [K] float64 (NaN = not measured yet) and ``counter``, the re-assignments made so far.
      observe(G)  raw score of scenario k --  "failure": 1 - successes / episodes where episodes > 0;  "abs_adv": sum |adv| / rows where
                  rows > 0 (PLR's L1 value-loss score: where the critic still mispredicts, not merely where the policy fails) --
                  score = raw at first sight, else (1 - alpha) score + alpha raw; a scenario the sums did not observe keeps its score.
      assign(n)   rank the scenarios by score, descending, unmeasured ones first, ties to the lower id;  p_k ~ (1 / rank_k)^(1 / beta);
                  w_k = (1 - u) p_k + u / K (the floor keeps every scenario's statistics fresh: PLR's staleness term in a setting
                  where every scenario can play every iteration);  every scenario gets one env, the other n - K are apportioned by
                  largest remainder of w (ties to the lower id);  the list "count_0 times 0, count_1 times 1, ..." is spread over the
                  GLOBAL env ids 0 .. n - 1 by sorting them on a splitmix64 hash of (seed, counter, global id) -- maps._env_hash with
                  a salt of its own.  A rank takes the slice of its envs, so every shard gives a global env the scenario the
                  single-GPU run gives it."""

    def __init__(self, K, mode="failure", alpha=0.5, temperature=0.3, uniform_mix=0.25, seed=0):
        if mode not in ("failure", "abs_adv"):
            raise ValueError(f"ScenarioSampler: mode {mode!r}: 'failure' or 'abs_adv'")
        if int(K) < 1:
            raise ValueError("ScenarioSampler: K must be at least 1")
        if not 0.0 <= alpha <= 1.0 or not 0.0 <= uniform_mix <= 1.0 or not 0.0 < temperature < float("inf"):
            raise ValueError("ScenarioSampler: alpha and uniform_mix lie in [0, 1], temperature is a finite number > 0")
        self.K, self.mode, self.seed = int(K), mode, int(seed)
        self.alpha, self.temperature, self.uniform_mix = float(alpha), float(temperature), float(uniform_mix)
        self.score = np.full(self.K, np.nan, dtype=np.float64)
        self.counter = 0

    def raw_scores(self, G):
        """(raw [K], seen [K] bool) of one iteration's sums"""
        G = np.asarray(G, dtype=np.float64).reshape(self.K, GROUP_SUMS_COLS)
        num, den = (G[:, 0] - G[:, 1], G[:, 0]) if self.mode == "failure" else (G[:, 6], G[:, 7])
        seen = den > 0
        return np.where(seen, num / np.where(seen, den, 1.0), np.nan), seen

    def observe(self, G):
        raw, seen = self.raw_scores(G)
        first = seen & np.isnan(self.score)
        again = seen & ~first
        self.score[again] = (1.0 - self.alpha) * self.score[again] + self.alpha * raw[again]
        self.score[first] = raw[first]
        return self.score

    def ranks(self):
        """[K] ranks 1 .. K: by score descending, unmeasured scenarios first, ties to the lower id"""
        unset = np.isnan(self.score)
        order = np.lexsort((np.arange(self.K), -np.where(unset, 0.0, self.score), ~unset))
        rank = np.empty(self.K, dtype=np.int64)
        rank[order] = np.arange(1, self.K + 1)
        return rank

    def weights(self):
        p = (1.0 / self.ranks().astype(np.float64)) ** (1.0 / self.temperature)
        return (1.0 - self.uniform_mix) * (p / p.sum()) + self.uniform_mix / self.K

    def counts(self, n_global):
        """[K] envs per scenario: one each, the rest by largest remainder of the weights"""
        n_global = int(n_global)
        if n_global < self.K:
            raise ValueError(f"ScenarioSampler: {n_global} envs cannot play {self.K} scenarios (every scenario gets at least one env)")
        quota = (n_global - self.K) * self.weights()
        base = np.floor(quota).astype(np.int64)
        left = (n_global - self.K) - int(base.sum())
        counts = 1 + base
        if left > 0:
            order = np.lexsort((np.arange(self.K), -(quota - base)))
            counts[order[np.arange(left) % self.K]] += 1
        elif left < 0:   # (rounding let the floors overshoot: take back from the smallest remainders)
            order = np.lexsort((-np.arange(self.K), quota - base))
            order = order[base[order] > 0]
            counts[order[:-left]] -= 1
        return counts

    def permutation(self, n_global):
        """the global env ids sorted on the hash of (seed, counter, global id), ties to the lower id"""
        from . import maps
        h = maps._env_hash(int(n_global), self.seed, 0, (_SALT + self.counter * _STEP) & _MASK)
        return np.argsort(h, kind="stable")

    def assign(self, n_global, env_id_base=0, n_envs=None):
        """The next assignment: [n_envs] int32 scenario ids of the envs env_id_base .. env_id_base + n_envs - 1 of n_global (default:
        all of them).  Counts one re-assignment."""
        n_global = int(n_global)
        ids = np.empty(n_global, dtype=np.int32)
        ids[self.permutation(n_global)] = np.repeat(np.arange(self.K, dtype=np.int32), self.counts(n_global))
        self.counter += 1
        lo = int(env_id_base)
        hi = n_global if n_envs is None else lo + int(n_envs)
        if lo < 0 or hi > n_global:
            raise ValueError(f"ScenarioSampler.assign: envs [{lo}, {hi}) lie outside [0, {n_global})")
        return ids[lo:hi].copy()

    def state_dict(self):
        return {"score": self.score.copy(), "counter": int(self.counter), "mode": self.mode}

    def load_state_dict(self, state):
        if state.get("mode", self.mode) != self.mode:
            raise ValueError(f"ScenarioSampler: the stored scores are {state['mode']!r} scores, this run's are {self.mode!r}")
        score = np.asarray(state["score"], dtype=np.float64).reshape(-1)
        if score.shape != (self.K,):
            raise ValueError(f"ScenarioSampler: the stored scores are of {score.size} scenarios, the bank has {self.K}")
        self.score, self.counter = score.copy(), int(state["counter"])
