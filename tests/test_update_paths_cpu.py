"""PPOUpdater.update's four execution paths without a device: a CPU updater whose fused attributes are set by hand and whose kernel
wrappers are recorders that write known numbers into the rows they are given.  Per case: the exact order of the calls (with the
_fhist / clip_stats row and the optimiser step of each), _adam_t, loss_history, clip_stats, kl_state and the whole statistics
dictionary -- its values worked out here from the planted numbers, its keys and their order spelled out."""
import types

import pytest
import torch

from navbot_ppo_amd import nets, ppo

CPU = torch.device("cpu")
N_A, N_C = 5378, 5313
T0 = 10                                     # _adam_t before the update
V0 = torch.arange(8.0) * 0.25               # what the fake value pass returns: mean 0.875
# what the fake kernels plant for epoch e.  Three DIFFERENT sources of gradient norms, so that the statistics show which one was read:
ROW = lambda e: (0.5 * (e + 1), 0.01 * (e + 1), 0.125 * (e + 1), 10.0 + e)   # actor loss, approx_kl, clip_frac, critic loss
G = lambda e: (3.0 * (e + 1), 4.0 * (e + 1), 5.0 * (e + 1))    # the gradient as it stands after epoch e: (actor, critic, total) norms
P = lambda e: (5.0 * e, 12.0 * e, 13.0 * e)                    # row e's columns 3 / 7: "the epoch before" (square roots)
S = lambda e: (8.0 * (e + 1), 15.0 * (e + 1), 17.0 * (e + 1))  # the clip statistics' pre-clip norms (square roots)
COEF = ((1.0, 0.25), (0.5, 1.0), (0.5, 0.25))                  # the clip coefficients (actor, critic) of a stepped epoch
KEYS = ["actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "value_mean",
        "actor_grad_norm", "critic_grad_norm", "actor_param_delta", "critic_param_delta"]
CLIP_KEYS = ["grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic"]
KL_KEYS = ["kl_stop_epoch", "kl_stopped"]
MODES = [(None, None), (0.5, None), (None, 0.01), (0.5, 0.01)]   # (max_grad_norm, target_kl)


class Fakes:
    """The recorders.  A KL-gated step trips when ONE step has been taken: an update of 3 epochs stops after 1 of 3 steps."""

    def __init__(self, monkeypatch, path, n_ep, max_norm, target_kl):
        torch.manual_seed(0)
        a, c = nets.make_policy("mlp64x2")
        self.log = []
        self.ctx = None
        if path != "single":
            self.ctx = types.SimpleNamespace(world=2, rank=0, enabled=True, broadcast=lambda t, src=0: t, all_reduce_sum=self.all_reduce_sum)
        cfg = ppo.PPOConfig(policy="mlp64x2", n_updates_per_iteration=n_ep, max_grad_norm=max_norm, target_kl=target_kl,
                            overlap_allreduce=path == "pipelined")
        self.up = up = ppo.PPOUpdater(a, c, cfg, self.ctx, CPU)
        assert tuple(up.fp.module_numel) == (N_A, N_C) and up.fused is None
        up.fused, up.fused_mlp64, up.bf16x3, up._n_actor, up._adam_t = "navppo_mlp64", True, True, N_A, T0
        up._fstats, up._fhist = torch.zeros(8), torch.zeros((max(n_ep, 1), 8))
        up._adam_m, up._adam_v = torch.zeros_like(up.fp.flat), torch.zeros_like(up.fp.flat)
        for name in ("_fused_epoch", "_fused_loss_grad", "_fused_loss_grad_net", "_fused_adam", "_fused_value", "prepare"):
            monkeypatch.setattr(up, name, getattr(self, name))
        monkeypatch.setattr(ppo.dist, "all_reduce", self.all_reduce_async)

    def row(self, t, of, width):
        assert t.untyped_storage().data_ptr() == of.untyped_storage().data_ptr()
        return t.storage_offset() // width

    # ---- collectives: two identical replicas, so a sum doubles
    def all_reduce_sum(self, t):
        same = t.untyped_storage().data_ptr() == self.up.fp.grad.untyped_storage().data_ptr()
        self.log.append(("all_reduce", "grad" if same else f"{str(t.dtype)[6:]}x{t.numel()}"))
        return t.mul_(2)

    def all_reduce_async(self, t, op=None, async_op=False):
        assert async_op and op == ppo.dist.ReduceOp.SUM
        sl = (self.row(t, self.up.fp.grad, 1), t.numel())
        self.log.append(("all_reduce_async", sl))
        t.mul_(2)
        return types.SimpleNamespace(wait=lambda: self.log.append(("wait", sl)))

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
        return V0.clone()

    def prepare(self, obs):
        self.log.append(("prepare",))

    def _fused_loss_grad(self, obs, acts, logp_old, rtg, adv, var, stats=None):
        assert var == float(torch.tensor(0.6))
        self.log.append(("pass", self._pass(stats, (0, 1))))

    def _fused_loss_grad_net(self, net, obs, acts, logp_old, rtg, adv, var, stats):
        assert var == float(torch.tensor(0.6))
        self.log.append(("pass_net", net, self._pass(stats, (net,))))

    # ---- the steps
    def _step(self, e, nets_, step, cstats, kl):
        """the optimiser step of epoch e on `nets_`; kl: the global approx_kl of a gated step, or None"""
        up = self.up
        coef = COEF[e]
        if kl is not None:
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

    def _fused_epoch(self, obs, acts, logp_old, rtg, adv, var, stats, cstats=None):
        up = self.up
        up._adam_t += 1
        assert var == float(torch.tensor(0.6))
        e = self.row(stats, up._fhist, 8)
        self.log.append(("epoch", e, None if cstats is None else self.row(cstats, up.clip_stats, 4), up._adam_t))
        kl_on = up.kl_limit is not None
        if kl_on and float(up.kl_state[0]) != 0.0:
            return                                       # stopped: every launch of the epoch returns at its entry
        self._pass(stats, (0, 1))
        stats[3], stats[7] = P(e)[0] ** 2, P(e)[1] ** 2
        self._step(e, (0, 1), up._adam_t, cstats, float(stats[1]) if kl_on else None)

    def _fused_adam(self, grad_scale, lo=0, n=None, step=None, cstats=None, kl_dev=None):
        up = self.up
        assert grad_scale == 0.5
        if step is None:
            up._adam_t += 1
            step = up._adam_t
        crow = None
        if cstats is not None:   # (the pipelined epochs step into rows of their own: (epoch, net) pairs)
            crow = cstats.storage_offset() // 4 if lo or n is not None else self.row(cstats, up.clip_stats, 4)
        self.log.append(("adam", (lo, n), step, crow, None if kl_dev is None else kl_dev.storage_offset() // 2))
        nets_ = (0, 1) if n is None else (0,) if lo == 0 else (1,)
        self._step(step - T0 - 1, nets_, step, cstats, None if kl_dev is None else float(kl_dev[0]))


def batch():
    g = torch.Generator().manual_seed(3)
    return (torch.rand((8, 16), generator=g), torch.rand((8, 2), generator=g), -torch.rand(8, generator=g), torch.randn(8, generator=g),
            torch.tensor(0.6))


def want_log(path, n_ep, clipping, kl_on):
    log = [("value",)] + ([("all_reduce", "float64x3")] if path != "single" else []) + ([("prepare",)] if n_ep else [])
    A, B = (0, N_A), (N_A, N_C)
    if path == "single":
        log += [("epoch", e, e if clipping else None, T0 + 1 + e) for e in range(n_ep)]
    elif path == "multi":
        for e in range(n_ep):
            log += [("pass", e), ("all_reduce", "grad")] + ([("all_reduce", "float32x2")] if kl_on else [])
            log += [("adam", (0, None), T0 + 1 + e, e if clipping else None, e if kl_on else None)]
    else:   # each net's all-reduce under the other net's pass; the steps of epoch e behind the waits in round e + 1
        for e in range(n_ep + 1):
            for k, sl in enumerate((A, B)):
                if e > 0:
                    log += [("wait", sl), ("adam", sl, T0 + e, 2 * (e - 1) + k if clipping else None, None)]
                if e < n_ep:
                    log += [("pass_net", k, e), ("all_reduce_async", sl)]
    return log + ([("all_reduce", "float32x6")] if path != "single" else [])


def want_stats(path, n_ep, max_norm, target_kl):
    """(k, steps, stopped, the statistics) by the definitions of the keys, from the planted numbers"""
    kl_on, clipping = target_kl is not None, max_norm is not None or target_kl is not None
    stopped = int(kl_on and n_ep == 3)
    steps = 1 if stopped else n_ep
    k = steps + stopped                      # the epochs whose passes count
    mean = lambda xs: sum(xs) / max(k, 1)
    rows = [ROW(e) for e in range(k)]
    last = n_ep - 1                          # the gradient as it stands (read without clipping only: no stop, every pass ran)
    if clipping:                             # every epoch's norms from the clip statistics
        gn, net = [S(e)[2] for e in range(k)], [[S(e)[j] for e in range(k)] for j in (0, 1)]
    elif path == "single":                   # the epochs before from the next row's columns 3 / 7, the last from the gradient
        gn = [P(e)[2] for e in range(1, n_ep)] + [G(last)[2]] * min(n_ep, 1)
        net = [[P(e)[j] for e in range(1, n_ep)] + [G(last)[j]] * min(n_ep, 1) for j in (0, 1)]
    else:                                    # every epoch's norms of the mean gradient
        gn, net = [G(e)[2] for e in range(k)], [[G(e)[j] for e in range(k)] for j in (0, 1)]
    vals = [mean([r[0] for r in rows]), mean([r[3] for r in rows]), mean([r[1] for r in rows]), mean([r[2] for r in rows]),
            mean(gn), mean([0.875] * k), mean(net[0]), mean(net[1]), 0.5 * steps, 0.25 * steps]
    st = dict(zip(KEYS, vals))
    if max_norm is not None:
        stepped = range(k - stopped)         # the tripping epoch's coefficient 0 is not a clipped epoch
        st.update(zip(CLIP_KEYS, [sum(COEF[e][0] < 1 for e in stepped) / max(k, 1), sum(COEF[e][1] < 1 for e in stepped) / max(k, 1), 0, 0]))
    if kl_on:
        st.update(zip(KL_KEYS, [steps, stopped]))
    return k, steps, stopped, st


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
    k, steps, stopped, st = want_stats(path, n_ep, max_norm, target_kl)
    assert f.log == want_log(path, n_ep, clipping, kl_on)
    assert up._adam_t == T0 + steps
    # loss_history: the rows that count, NaN behind a stop
    h = up.loss_history
    assert tuple(h.shape) == (n_ep, 2)
    torch.testing.assert_close(h[:k], torch.tensor([[ROW(e)[0], ROW(e)[3]] for e in range(k)]).reshape(k, 2), rtol=0, atol=0)
    assert bool(torch.isnan(h[k:]).all())
    want_last = (ROW(k - 1)[0], ROW(k - 1)[3]) if k else (0.0, 0.0)
    assert tuple(float(x) for x in up.last_losses) == want_last
    # the statistics: values, key set and key order
    assert out is up.stats and list(out) == KEYS + (CLIP_KEYS if max_norm is not None else []) + (KL_KEYS if kl_on else [])
    assert list(out) == list(st)
    for key, v in st.items():   # float32 statistics of a handful of roundings each (2^-24 relative): 1e-6
        assert out[key] == pytest.approx(v, rel=1e-6, abs=0), key
        assert type(out[key]) is (int if key.startswith(("skipped", "kl_")) else float), key
    # clip_stats and kl_state as the step launches left them
    if clipping:
        cs = up.clip_stats
        assert tuple(cs.shape) == ((n_ep if path == "pipelined" else max(n_ep, 1)), 4)
        coef = [COEF[e] if e < k - stopped else (0.0, 0.0) for e in range(k)]
        assert cs[:k].tolist() == [[S(e)[0] ** 2, S(e)[1] ** 2, coef[e][0], coef[e][1]] for e in range(k)]
    else:
        assert up.clip_stats is None
    if kl_on:   # (stopped, steps taken, tripping approx_kl, its step)
        assert up.kl_state.tolist() == pytest.approx([1.0, 1.0, ROW(1)[1], T0 + 2.0] if stopped else [0.0, float(n_ep), 0.0, 0.0], rel=1e-6)
    else:
        assert up.kl_state is None


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
