"""PPOUpdater.update's four execution paths without a device: a CPU updater whose fused attributes are set by hand and whose kernel
wrappers are recorders that write known numbers into the rows they are given.  Per case: the exact order of the calls (with the
_fhist / clip_stats row and the optimiser step of each), _adam_t, loss_history, clip_stats, kl_state and the whole statistics
dictionary -- its values worked out here from the planted numbers, its keys and their order spelled out.  With minibatches a row is an
optimiser STEP's: the log also holds every shuffle with its counter, every prepare with the tensor it saw, and per step the slice (its
source, first row and length) with the byte offset into the prepared buffer its kernel arguments carry; with the adaptive learning rate
the `adapt` flag of every step launch."""
import sys
import types

import numpy as np
import pytest
import torch

from navbot_ppo_amd import nets, ppo

CPU = torch.device("cpu")
N_A, N_C = 5378, 5313
T0 = 10                                     # _adam_t before the update
V0 = torch.arange(8.0) * 0.25               # what the fake value pass returns (repeated to the batch): mean 0.875
N_MB = 96                                   # samples of the minibatch cases: slices of 32 (K = 3) or 64 (K = 2, the last one shorter)
PREP_ROW = 100                              # bytes per row the fake navppo_mlp64_bf16x3_prep_bytes answers with
DESIRED_KL = 0.05                           # adaptive rate: the planted approx_kl 0.01 (e + 1) asks for a raise at steps 0 and 1
# what the fake kernels plant for epoch e.  Three DIFFERENT sources of gradient norms, so that the statistics show which one was read:
ROW = lambda e: (0.5 * (e + 1), 0.01 * (e + 1), 0.125 * (e + 1), 10.0 + e)   # actor loss, approx_kl, clip_frac, critic loss
G = lambda e: (3.0 * (e + 1), 4.0 * (e + 1), 5.0 * (e + 1))    # the gradient as it stands after epoch e: (actor, critic, total) norms
P = lambda e: (5.0 * e, 12.0 * e, 13.0 * e)                    # row e's columns 3 / 7: "the epoch before" (square roots)
S = lambda e: (8.0 * (e + 1), 15.0 * (e + 1), 17.0 * (e + 1))  # the clip statistics' pre-clip norms (square roots)
COEF = ((1.0, 0.25), (0.5, 1.0), (0.5, 0.25))                  # the clip coefficients (actor, critic) of a stepped epoch, e modulo 3
KEYS = ["actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "value_mean",
        "actor_grad_norm", "critic_grad_norm", "actor_param_delta", "critic_param_delta"]
CLIP_KEYS = ["grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic"]
KL_KEYS = ["kl_stop_epoch", "kl_stopped"]
LR_KEYS = ["lr", "lr_ups", "lr_downs"]
MODES = [(None, None), (0.5, None), (None, 0.01), (0.5, 0.01)]   # (max_grad_norm, target_kl)


# ---- how the recorders see what the update hands a step beside its tensors: the ONE place that follows PPOUpdater's internals
def adapt_seen(up, kw):
    """the `adapt` flag the step launch receives"""
    return int(kw["adapt"])


def prep_offset(up, sl, var, kw):
    """the byte offset into the prepared buffer that the kernel arguments of this step carry (PPOUpdater._batch_args builds them)"""
    return up._batch_args(*sl, var, kw.get("first_row"))[1][0].value - up._prep.data_ptr()


class Fakes:
    """The recorders.  A KL-gated step trips when ONE step has been taken: an update of 3 epochs stops after 1 of 3 steps."""

    def __init__(self, monkeypatch, path, n_ep, max_norm, target_kl, mb=None, shuffle="epoch", lr_schedule=None):
        torch.manual_seed(0)
        a, c = nets.make_policy("mlp64x2")
        self.log = []
        self.ctx = None
        if path != "single":
            self.ctx = types.SimpleNamespace(world=2, rank=0, enabled=True, broadcast=lambda t, src=0: t, all_reduce_sum=self.all_reduce_sum)
            if mb is not None:   # (the plan's collective: every rank holds the same number of samples)
                self.ctx.all_reduce_max = self.all_reduce_max
        cfg = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, max_grad_norm=max_norm, target_kl=target_kl,
                            overlap_allreduce=path == "pipelined", minibatch_size=mb, minibatch_shuffle=shuffle, lr_schedule=lr_schedule,
                            desired_kl=DESIRED_KL)
        self.up = up = ppo.PPOUpdater(a, c, cfg, self.ctx, CPU)
        assert tuple(up.fp.module_numel) == (N_A, N_C) and up.fused is None
        up.fused, up.fused_mlp64, up.bf16x3, up._n_actor, up._adam_t = "navppo_mlp64", True, True, N_A, T0
        up._fstats, up._fhist = torch.zeros(8), torch.zeros((max(n_ep, 1), 8))
        up._adam_m, up._adam_v = torch.zeros_like(up.fp.flat), torch.zeros_like(up.fp.flat)
        if up.lr_adaptive:
            up.lr_state = torch.zeros(4)
        for name in ("_fused_epoch", "_fused_loss_grad", "_fused_loss_grad_net", "_fused_adam", "_fused_value", "prepare"):
            monkeypatch.setattr(up, name, getattr(self, name))
        monkeypatch.setattr(ppo.dist, "all_reduce", self.all_reduce_async)
        # the native library as the module of the updater sees it: the shuffle's launch is recorded, a prepared row is PREP_ROW bytes
        mod = sys.modules[ppo.PPOUpdater.__module__]
        monkeypatch.setattr(mod, "_navppo", self.navppo)
        monkeypatch.setattr(mod, "lib", lambda: types.SimpleNamespace(navppo_mlp64_bf16x3_prep_bytes=lambda n, d: PREP_ROW * n))

    def row(self, t, of, width):
        assert t.untyped_storage().data_ptr() == of.untyped_storage().data_ptr()
        return t.storage_offset() // width

    def where(self, obs):
        """(source, first row, rows) of the observations a call was given: the batch as the caller passed it, or the one permuted copy"""
        sh = self.up._shuf
        shuf = sh is not None and obs.untyped_storage().data_ptr() == sh[0].untyped_storage().data_ptr()
        return "shuf" if shuf else "batch", obs.storage_offset() // 16, int(obs.shape[0])

    def slice_of(self, sl, var, kw):
        return self.where(sl[0]) + (prep_offset(self.up, sl, var, kw),)

    # ---- collectives: two identical replicas, so a sum doubles and a maximum changes nothing
    def all_reduce_sum(self, t):
        same = t.untyped_storage().data_ptr() == self.up.fp.grad.untyped_storage().data_ptr()
        self.log.append(("all_reduce", "grad" if same else f"{str(t.dtype)[6:]}x{t.numel()}"))
        return t.mul_(2)

    def all_reduce_max(self, t):
        self.log.append(("all_reduce_max", f"{str(t.dtype)[6:]}x{t.numel()}"))
        return t

    def all_reduce_async(self, t, op=None, async_op=False):
        assert async_op and op == ppo.dist.ReduceOp.SUM
        sl = (self.row(t, self.up.fp.grad, 1), t.numel())
        self.log.append(("all_reduce_async", sl))
        t.mul_(2)
        return types.SimpleNamespace(wait=lambda: self.log.append(("wait", sl)))

    # ---- the native calls the real methods make (PPOUpdater._shuffled is not replaced: its launch is)
    def navppo(self, entry, *args):
        assert entry == "navppo_shuffle_batch" and args[7] == N_MB and args[8] == ppo.minibatch_key(0, 0)
        assert (args[-1] is None) == (self.up.kl_state is None)   # (gated by kl_state when there is one)
        self.log.append(("shuffle", args[9]))

    # ---- the passes
    def _pass(self, stats, nets_):
        e = self.row(stats, self.up._fhist, 8)
        a, kl, cf, c = ROW(e)
        if 0 in nets_:
            stats[0], stats[1], stats[2], self.up.fp.grad[0] = a, kl, cf, G(e)[0]
        if 1 in nets_:
            stats[4], self.up.fp.grad[N_A] = c, G(e)[1]
        return e

    def _fused_value(self, obs):
        self.log.append(("value",))
        return V0.repeat(obs.shape[0] // 8)

    def prepare(self, obs):
        up = self.up
        self.log.append(("prepare", self.where(obs)[0]))
        if up._prep is None or up._prep.numel() < PREP_ROW * obs.shape[0]:
            up._prep = torch.zeros(PREP_ROW * obs.shape[0], dtype=torch.uint8)
        up._prep_key = (obs.data_ptr(), tuple(obs.shape), obs.dtype, obs._version)

    def _fused_loss_grad(self, obs, acts, logp_old, rtg, adv, var, stats=None, **kw):
        assert var == float(torch.tensor(0.6))
        sl = self.slice_of((obs, acts, logp_old, rtg, adv), var, kw)
        self.log.append(("pass", self._pass(stats, (0, 1)), sl))

    def _fused_loss_grad_net(self, net, obs, acts, logp_old, rtg, adv, var, stats):
        assert var == float(torch.tensor(0.6))
        self.log.append(("pass_net", net, self._pass(stats, (net,))))

    # ---- the steps
    def _step(self, e, nets_, step, cstats, kl, adapt=None):
        """the optimiser step of epoch e on `nets_`; kl: the global approx_kl of a gated or rate-adapting step, or None"""
        up = self.up
        coef = COEF[e % 3]
        if up.lr_adaptive:   # the rule on the device state: the step reads the rate of slot step & 1 (0 = cfg.lr) and writes the other
            ls, cfg = up.lr_state, up.cfg
            d = ppo.adaptive_lr_direction(kl, DESIRED_KL, adapt)
            ls[(step + 1) & 1] = ppo.adaptive_lr_reference(float(ls[step & 1]) or cfg.lr, kl, DESIRED_KL, cfg.lr_min, cfg.lr_max, adapt)
            ls[2] += d > 0
            ls[3] += d < 0
        elif kl is not None:
            ks = up.kl_state
            if float(ks[0]) != 0.0:
                return                                   # stopped: the launch returns at its entry
            if float(ks[1]) == 1.0:                      # the trip: nothing is stepped, coefficients 0, the gradient stays as it is
                ks[0], ks[2], ks[3] = 1.0, kl, float(step)
                coef = (0.0, 0.0)
            else:
                ks[1] += 1.0
        for k in nets_:
            if cstats is not None:
                cstats[k], cstats[2 + k] = S(e)[k] ** 2, coef[k]
            if coef[k] != 0.0:
                up.fp.flat[k * N_A] += (0.5, 0.25)[k]

    def _fused_epoch(self, obs, acts, logp_old, rtg, adv, var, stats, cstats=None, **kw):
        up = self.up
        up._adam_t += 1
        assert var == float(torch.tensor(0.6))
        e = self.row(stats, up._fhist, 8)
        adapt = adapt_seen(up, kw) if up.lr_adaptive else None
        self.log.append(("epoch", e, None if cstats is None else self.row(cstats, up.clip_stats, 4), up._adam_t,
                         self.slice_of((obs, acts, logp_old, rtg, adv), var, kw), adapt))
        kl_on = up.kl_limit is not None
        if kl_on and float(up.kl_state[0]) != 0.0:
            return                                       # stopped: every launch of the epoch returns at its entry
        self._pass(stats, (0, 1))
        stats[3], stats[7] = P(e)[0] ** 2, P(e)[1] ** 2
        self._step(e, (0, 1), up._adam_t, cstats, float(stats[1]) if kl_on or up.lr_adaptive else None, adapt)

    def _fused_adam(self, grad_scale, lo=0, n=None, step=None, cstats=None, kl_dev=None, **kw):
        up = self.up
        assert grad_scale == 0.5
        if step is None:
            up._adam_t += 1
            step = up._adam_t
        crow = None
        if cstats is not None:   # (the pipelined epochs step into rows of their own: (epoch, net) pairs)
            crow = cstats.storage_offset() // 4 if lo or n is not None else self.row(cstats, up.clip_stats, 4)
        adapt = adapt_seen(up, kw) if up.lr_adaptive else None
        self.log.append(("adam", (lo, n), step, crow, None if kl_dev is None else kl_dev.storage_offset() // 2, adapt))
        nets_ = (0, 1) if n is None else (0,) if lo == 0 else (1,)
        self._step(step - T0 - 1, nets_, step, cstats, None if kl_dev is None else float(kl_dev[0]), adapt)


def batch(n=8):
    g = torch.Generator().manual_seed(3)
    return (torch.rand((n, 16), generator=g), torch.rand((n, 2), generator=g), -torch.rand(n, generator=g), torch.randn(n, generator=g),
            torch.tensor(0.6))


def want_log(path, n_ep, clipping, kl_on, n=8, mb=None, shuffle="epoch", adaptive=False, t0=T0, update=0):
    """The calls of one update() in order.  A step is an epoch, or with minibatches (mb < n) one of its K slices: its row of the per-step
    buffers is the step's index, its slice ("batch" as it lies or the "shuf" copy, first row, rows, byte offset of the prepared rows)."""
    multi, sliced = path != "single", mb is not None and mb < n
    shuffling = sliced and shuffle != "none"
    log = [("value",)] + ([("all_reduce", "float64x3")] if multi else []) + ([("all_reduce_max", "int64x2")] if multi and mb is not None else [])
    log += [("prepare", "batch")] if n_ep and not shuffling else []   # (shuffling: the permuted copy is prepared behind every shuffle)
    A, B = (0, N_A), (N_A, N_C)
    if path == "pipelined":   # each net's all-reduce under the other net's pass; the steps of epoch e behind the waits in round e + 1
        for e in range(n_ep + 1):
            for k, sl in enumerate((A, B)):
                if e > 0:
                    log += [("wait", sl), ("adam", sl, t0 + e, 2 * (e - 1) + k if clipping else None, None, None)]
                if e < n_ep:
                    log += [("pass_net", k, e), ("all_reduce_async", sl)]
        return log + [("all_reduce", "float32x6")]
    st = 0
    for ep in range(n_ep):
        if shuffling and (shuffle == "epoch" or ep == 0):
            log += [("shuffle", ppo.minibatch_counter(update, ep if shuffle == "epoch" else 0)), ("prepare", "shuf")]
        for lo in range(0, n, mb if sliced else n):
            sl = ("shuf" if shuffling else "batch", lo, min(mb if sliced else n, n - lo), PREP_ROW * lo)
            adapt = int(st > 0) if adaptive else None   # the first step of an update does not adapt
            crow, klrow = st if clipping else None, st if kl_on or adaptive else None
            if not multi:
                log += [("epoch", st, crow, t0 + 1 + st, sl, adapt)]
            else:
                log += [("pass", st, sl), ("all_reduce", "grad")] + ([("all_reduce", "float32x2")] if klrow is not None else [])
                log += [("adam", (0, None), t0 + 1 + st, crow, klrow, adapt)]
            st += 1
    return log + ([("all_reduce", "float32x6")] if multi else [])


def want_stats(path, n_st, max_norm, target_kl, K=1, adaptive=False):
    """(k, steps, stopped, the statistics) by the definitions of the keys, from the planted numbers; n_st: the optimiser steps queued"""
    kl_on, clipping = target_kl is not None, max_norm is not None or target_kl is not None or adaptive
    stopped = int(kl_on and n_st >= 2)
    steps = 1 if stopped else n_st
    k = steps + stopped                      # the steps whose passes count
    mean = lambda xs: sum(xs) / max(k, 1)
    rows = [ROW(e) for e in range(k)]
    last = n_st - 1                          # the gradient as it stands (read without clipping only: no stop, every pass ran)
    if clipping:                             # every step's norms from the clip statistics
        gn, net = [S(e)[2] for e in range(k)], [[S(e)[j] for e in range(k)] for j in (0, 1)]
    elif path == "single":                   # the steps before from the next row's columns 3 / 7, the last from the gradient
        gn = [P(e)[2] for e in range(1, n_st)] + [G(last)[2]] * min(n_st, 1)
        net = [[P(e)[j] for e in range(1, n_st)] + [G(last)[j]] * min(n_st, 1) for j in (0, 1)]
    else:                                    # every step's norms of the mean gradient
        gn, net = [G(e)[2] for e in range(k)], [[G(e)[j] for e in range(k)] for j in (0, 1)]
    vals = [mean([r[0] for r in rows]), mean([r[3] for r in rows]), mean([r[1] for r in rows]), mean([r[2] for r in rows]),
            mean(gn), mean([0.875] * k), mean(net[0]), mean(net[1]), 0.5 * steps, 0.25 * steps]
    st = dict(zip(KEYS, vals))
    if max_norm is not None:
        stepped = range(k - stopped)         # the tripping step's coefficient 0 is not a clipped step
        st.update(zip(CLIP_KEYS, [sum(COEF[e % 3][0] < 1 for e in stepped) / max(k, 1), sum(COEF[e % 3][1] < 1 for e in stepped) / max(k, 1), 0, 0]))
    if kl_on:                                # (minibatches: whole epochs completed, and the steps)
        st.update(zip(KL_KEYS, [steps // K, stopped]))
        if K > 1:
            st["kl_stop_step"] = steps
    return k, steps, stopped, st


def check_update(f, out, path, n_ep, max_norm, target_kl, K=1, adaptive=False, st_extra=None):
    """everything an update() leaves behind but the log: _adam_t, loss_history, last_losses, the statistics, clip_stats, kl_state"""
    up, n_st = f.up, n_ep * K
    kl_on, clipping = target_kl is not None, max_norm is not None or target_kl is not None or adaptive
    k, steps, stopped, st = want_stats(path, n_st, max_norm, target_kl, K, adaptive)
    st.update(st_extra or {})
    assert up._adam_t == T0 + steps
    # loss_history: per epoch, the mean over its steps that count; NaN where none does
    h = up.loss_history
    assert tuple(h.shape) == (n_ep, 2)
    eps = -(-k // K)                         # epochs a step of which counts
    want_h = [[sum(ROW(e)[j] for e in range(ep * K, min(ep * K + K, k))) / (min(ep * K + K, k) - ep * K) for j in (0, 3)] for ep in range(eps)]
    torch.testing.assert_close(h[:eps], torch.tensor(want_h).reshape(eps, 2), rtol=0 if K == 1 else 1e-6, atol=0)
    assert bool(torch.isnan(h[eps:]).all())
    assert tuple(float(x) for x in up.last_losses) == (tuple(float(x) for x in h[eps - 1]) if k else (0.0, 0.0))
    # the statistics: values, key set and key order
    assert out is up.stats and list(out) == list(st)
    for key, v in st.items():   # float32 statistics of a handful of roundings each (2^-24 relative): 1e-6
        assert out[key] == pytest.approx(v, rel=1e-6, abs=0), key
        assert type(out[key]) is (int if key.startswith(("skipped", "kl_", "lr_")) else float), key
    # clip_stats and kl_state as the step launches left them
    if clipping:
        cs = up.clip_stats
        assert tuple(cs.shape) == ((n_ep if path == "pipelined" else max(n_st, 1)), 4)
        coef = [COEF[e % 3] if e < k - stopped else (0.0, 0.0) for e in range(k)]
        assert cs[:k].tolist() == [[S(e)[0] ** 2, S(e)[1] ** 2, coef[e][0], coef[e][1]] for e in range(k)]
    else:
        assert up.clip_stats is None
    if kl_on:   # (stopped, steps taken, tripping approx_kl, its step)
        assert up.kl_state.tolist() == pytest.approx([1.0, 1.0, ROW(1)[1], T0 + 2.0] if stopped else [0.0, float(n_st), 0.0, 0.0], rel=1e-6)
    else:
        assert up.kl_state is None


@pytest.mark.parametrize("max_norm,target_kl", MODES)
@pytest.mark.parametrize("n_ep", [0, 1, 3])
@pytest.mark.parametrize("path", ["single", "multi", "pipelined"])
def test_fused_paths_call_order_and_statistics(monkeypatch, path, n_ep, max_norm, target_kl):
    if path == "pipelined" and target_kl is not None:
        with pytest.raises(ValueError, match="overlap_allreduce"):
            Fakes(monkeypatch, path, n_ep, max_norm, target_kl)
        return
    f = Fakes(monkeypatch, path, n_ep, max_norm, target_kl)
    up = f.up
    kl_on, clipping = target_kl is not None, max_norm is not None or target_kl is not None
    out = up.update(*batch())
    assert f.log == want_log(path, n_ep, clipping, kl_on)
    assert list(out) == KEYS + (CLIP_KEYS if max_norm is not None else []) + (KL_KEYS if kl_on else [])
    check_update(f, out, path, n_ep, max_norm, target_kl)
    k = want_stats(path, n_ep, max_norm, target_kl)[0]
    torch.testing.assert_close(up.loss_history[:k], torch.tensor([[ROW(e)[0], ROW(e)[3]] for e in range(k)]).reshape(k, 2), rtol=0, atol=0)
    assert tuple(float(x) for x in up.last_losses) == ((ROW(k - 1)[0], ROW(k - 1)[3]) if k else (0.0, 0.0))
    assert up._shuf is None   # whole-batch epochs: no permuted copy, no shuffle (the log), one prepare per update


@pytest.mark.parametrize("max_norm,target_kl", MODES)
@pytest.mark.parametrize("shuffle", ["epoch", "update", "none"])
@pytest.mark.parametrize("mb", [32, 64])
@pytest.mark.parametrize("path", ["single", "multi"])
def test_minibatch_steps_slices_shuffles_and_statistics(monkeypatch, path, mb, shuffle, max_norm, target_kl):
    """2 epochs of K = 3 (32) or K = 2 (64 and a shorter last slice of 32) steps over 96 samples on the split-bf16 arithmetic."""
    n_ep, K = 2, -(-N_MB // mb)
    f = Fakes(monkeypatch, path, n_ep, max_norm, target_kl, mb=mb, shuffle=shuffle)
    up = f.up
    kl_on, clipping = target_kl is not None, max_norm is not None or target_kl is not None
    out = up.update(*batch(N_MB))
    assert f.log == want_log(path, n_ep, clipping, kl_on, n=N_MB, mb=mb, shuffle=shuffle)
    assert list(out) == (KEYS + (CLIP_KEYS if max_norm is not None else []) + (KL_KEYS + ["kl_stop_step"] if kl_on else []))
    check_update(f, out, path, n_ep, max_norm, target_kl, K=K)
    if kl_on:   # the trip at the second step of epoch 0: one step taken, no whole epoch; the mean of that epoch's two rows that count
        assert (out["kl_stop_epoch"], out["kl_stopped"], out["kl_stop_step"]) == (0, 1, 1)
        torch.testing.assert_close(up.loss_history[0], torch.tensor([0.75, 10.5]), rtol=1e-6, atol=0)
        assert bool(torch.isnan(up.loss_history[1]).all())
    assert (up._shuf is None) == (shuffle == "none") and up.update_index == 1


@pytest.mark.parametrize("mb", [None, 32])
@pytest.mark.parametrize("path", ["single", "multi"])
def test_adaptive_rate_flag_collective_and_statistics(monkeypatch, path, mb):
    """lr_schedule="adaptive": every step launch gets adapt = 0 on the first step of an update() and 1 afterwards, the several-rank path
    runs its 2-float collective per step, kl_steps holds every step's approx_kl and lr / lr_ups / lr_downs follow the base keys."""
    n_ep, K = 2, 1 if mb is None else 3
    n_st = n_ep * K
    f = Fakes(monkeypatch, path, n_ep, None, None, mb=mb, lr_schedule="adaptive")
    up = f.up
    f32 = np.float32
    lr, t0 = 3e-4, T0
    for update in (0, 1):   # (the second update: the flag is 0 again on its first step, the rate carries over, the counts do not)
        del f.log[:]
        out = up.update(*batch(N_MB))
        assert f.log == want_log(path, n_ep, True, False, n=N_MB, mb=mb, adaptive=True, t0=t0, update=update)
        kls = [float(f32(ROW(e)[1])) for e in range(n_st)]
        assert up.kl_steps.tolist() == pytest.approx(kls, rel=1e-6)   # (several ranks: sum(kl_r n_r) / sum(n_r) rounds twice)
        ups = 0
        for e, kl in enumerate(kls):   # step 0 asks for a raise (0.01 < DESIRED_KL / 2) and must not get it
            new = ppo.adaptive_lr_reference(lr, kl, DESIRED_KL, 1e-5, 1e-2, adapt=e > 0)
            ups, lr = ups + (new > float(f32(lr))), new
        assert ups == 1 and list(out) == KEYS + LR_KEYS
        assert (out["lr"], out["lr_ups"], out["lr_downs"]) == (lr, 1, 0) and up.lr_value == lr
        t0 += n_st
        assert up._adam_t == t0
        if update == 0:
            check_update(f, out, path, n_ep, None, None, K=K, adaptive=True, st_extra=dict(lr=lr, lr_ups=1, lr_downs=0))


def _pytorch_update(n_ep):
    torch.manual_seed(0)
    a, c = nets.make_policy("mlp64x2")
    g = torch.Generator().manual_seed(12)
    obs = torch.rand((8, 16), generator=g)
    acts = torch.stack([torch.rand(8, generator=g), torch.rand(8, generator=g) * 2 - 1], 1)
    rtg, var = torch.randn(8, generator=g) * 3, torch.tensor(0.6)
    with torch.no_grad():   # the start policy's own log-probabilities: approx_kl is 0 in epoch 0 and positive after the first step
        logp = ppo.gaussian_log_prob(a(obs), acts, var)
    up = ppo.PPOUpdater(a, c, ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, max_grad_norm=0.5, target_kl=1e-9), None, CPU)
    assert up.fused is None
    return up, up.update(obs, acts, logp, rtg, var)


def test_pytorch_path_trip_leaves_the_weights_of_the_last_step_taken():
    up, st = _pytorch_update(3)
    assert list(st) == KEYS + CLIP_KEYS + KL_KEYS
    assert st["kl_stop_epoch"] == 1 and st["kl_stopped"] == 1
    h = up.loss_history
    assert tuple(h.shape) == (3, 2) and bool(torch.isfinite(h[:2]).all()) and bool(torch.isnan(h[2:]).all())
    one, st1 = _pytorch_update(1)
    assert st1["kl_stop_epoch"] == 1 and st1["kl_stopped"] == 0
    assert torch.equal(up.fp.flat, one.fp.flat)
