"""The update half of PPO.learn (ppo.py:275-397): the flat parameter buffer, the losses, and PPOUpdater -- the host side of the fused
HIP update (include/navppo.h) and its PyTorch formulation."""
import collections
import dataclasses
import math

import torch
import torch.distributed as dist

from . import nets
from ._native import _navppo, _ptr, lib
from .config import check_learn_var_config, check_lr_schedule_config, check_minibatch_config, check_update_config
from .distributed import as_ctx, global_mean
from .explore_var import (ADAM_M, ADAM_V, ENTROPY_AT_ZERO, GRAD, SKIPPED, STEPS, THETA, VAR, VAR_STATE_LEN, learned_var_reference,
                          var_state_init)
from .lr_schedule import adaptive_lr_direction, adaptive_lr_reference
from .minibatch import batch_permutation, minibatch_counter, minibatch_key

LOG_2PI = math.log(2.0 * math.pi)
ADAM_HYPER = (0.9, 0.999, 1e-8)   # Adam's (beta1, beta2, eps), torch's defaults (ppo.py:116-117): torch.optim.Adam and the fused steps

# The step mode of an updater, the counterpart of NavppoMode on the native side: what an optimiser step does beside Adam.  A constant of
# the config -- target_kl and lr_schedule="adaptive" exclude each other and both are refused with overlap_allreduce -- resolved once, in
# PPOUpdater.__init__.  The value is the suffix of the entry points of a mode: navppo_*_update_epoch<mode>, navppo_adam_step<mode>;
# PPOUpdater._mode_args holds the arguments a mode adds.  Every mode but the plain one runs the clipped machinery and fills clip_stats:
# target_kl or the adaptive rate without max_grad_norm clip at max_norm = +inf, the unclipped epochs' bits.
PLAIN, CLIP, KL_STOP, ADAPTIVE_LR = "", "_clipped", "_kl", "_lr"
# PPOConfig.learn_var (one rank only): the *_var entry points -- the clipped machinery, or with lr_schedule="adaptive" the adaptive
# rate's, with the passes reading the variance from the device state and one more launch that steps it
LEARN_VAR = "_var"


class FlatParams:
    """All trainable tensors of actor + critic as views into ONE flat buffer, and their gradients as
    views into ONE flat gradient buffer: a single all-reduce and a single Adam update per epoch.
    (The reference's unused BatchNorm parameters never receive gradients -- net_actor.py:44,48 -- and
    stay ordinary tensors so state_dict keys are unchanged.)"""

    def __init__(self, modules, device):
        per_module = [[p for n, p in m.named_parameters() if ".bn" not in "." + n and not n.startswith("bn")] for m in modules]
        self.params = [p for ps in per_module for p in ps]
        self.module_numel = [sum(p.numel() for p in ps) for ps in per_module]   # [actor, critic] slices of the flat buffers
        total = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view_as(p)
            p.grad = self.grad[off:off + n].view_as(p)
            off += n
        self.numel = total
        self.proxy = torch.nn.Parameter(self.flat, requires_grad=True)
        self.proxy.data = self.flat
        self.proxy.grad = self.grad


def gaussian_log_prob(mean, action, var):
    """log N(action; mean, var*I) for a 2-D isotropic Gaussian = MultivariateNormal(mean, diag(var)).log_prob
    (ppo.py:696,704,734-735)."""
    k = mean.shape[-1]
    return -0.5 * (((action - mean) ** 2).sum(-1) / var) - 0.5 * k * LOG_2PI - 0.5 * k * torch.log(var)


def ppo_losses(actor, critic, obs, acts, logp_old, rtg, adv, var, clip):
    """One evaluation of ppo.py:307-343.  Returns (actor_loss, critic_loss, ratios, logp)."""
    V = critic(obs).squeeze(-1)
    mean = actor(obs)
    lo = mean.new_tensor([0.0, -1.0])
    hi = mean.new_tensor([1.0, 1.0])
    mean = torch.max(torch.min(mean, hi), lo)              # ppo.py:730-733 (no-op after sigmoid/tanh)
    logp = gaussian_log_prob(mean, acts, var)
    ratios = torch.exp(logp - logp_old)                    # ppo.py:316
    surr1 = ratios * adv                                   # ppo.py:319
    surr2 = torch.clamp(ratios, 1 - clip, 1 + clip) * adv  # ppo.py:320
    actor_loss = (-torch.min(surr1, surr2)).mean()         # ppo.py:342
    critic_loss = torch.nn.functional.mse_loss(V, rtg)     # ppo.py:343
    return actor_loss, critic_loss, ratios, logp, V


def normalise_advantages(adv, ctx=None):
    """(A - mean) / (std + 1e-10) with torch.std's unbiased estimator (ppo.py:284); with several ranks the
    moments are all-reduced so every rank uses the global mean/std."""
    a64 = adv.double()
    m = torch.stack([a64.sum(), (a64 * a64).sum(), torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device)])
    as_ctx(ctx).all_reduce_sum(m)
    n = m[2]
    mean = m[0] / n
    var = (m[1] - n * mean * mean) / (n - 1)
    std = torch.sqrt(torch.clamp(var, min=0.0))
    return ((adv - mean.float()) / (std.float() + 1e-10))


# What each of PPOUpdater's four epoch runners hands to _summarise.  k: the epochs whose passes ran = the rows the statistics are taken
# over; steps, stopped: optimiser steps taken, whether target_kl stopped the update early (k = steps + stopped); losses: [n_ep, 2] per-epoch
# (actor, critic) loss, NaN behind a stop; sums: [4] sums over the k epochs of (actor loss, critic loss, approx_kl, clip_frac); gn_sum, v_sum:
# the same of the whole gradient's norm and the mean value; net_gn: [2] of the per-net norms, if the runner has them; net_gn_open: less the last's.
# Minibatches (K = slices per epoch > 1): k, steps and the sums count optimiser STEPS (K to an epoch); losses stays per epoch -- a row is
# the mean over the steps of its epoch that ran, NaN where none did
_Epochs = dataclasses.make_dataclass("_Epochs", ["k", "steps", "stopped", "losses", "sums", "gn_sum", "v_sum",
                                                 ("net_gn", object, None), ("net_gn_open", bool, False), ("K", int, 1)])

# The optimiser steps of ONE update(), fixed before its first launch (PPOUpdater._plan): n samples, n_ep epochs of K slices of `size`
# samples (the last one shorter if n is no multiple), n_steps = n_ep K steps -- a row of every per-step buffer each; shuffle: which
# samples a slice holds (PPOConfig.minibatch_shuffle); update: the index of this update, the high word of its shuffles' counters.
# Whole-batch epochs (minibatch_size None or >= n) are K = 1, size = n, shuffle = "none": today's launches and nothing else.
_StepPlan = dataclasses.make_dataclass("_StepPlan", ["n", "n_ep", "size", "K", "shuffle", "n_steps", "update"], frozen=True)
# One optimiser step of a plan: its index (the row of the per-step buffers), its epoch, the first row of its slice in the batch the
# slices are cut from (0: a whole batch), and the tensors (obs, acts, logp_old, rtg, adv) of the slice
_Step = collections.namedtuple("_Step", ["index", "epoch", "first_row", "batch"])


class PPOUpdater:
    """The update half of PPO.learn (ppo.py:275-397) on a fixed batch: the host side of the fused HIP update and its PyTorch formulation."""

    def __init__(self, actor, critic, cfg, ctx=None, device=None):
        self.actor, self.critic, self.cfg, self.ctx = actor, critic, cfg, as_ctx(ctx)
        self.device = device or next(actor.parameters()).device
        self.fp = FlatParams([actor, critic], self.device)
        self.ctx.broadcast(self.fp.flat, 0)  # identical replicas; identical Adam steps keep them in sync
        fused = self.device.type == "cuda"
        self.opt = torch.optim.Adam([self.fp.proxy], lr=cfg.lr, betas=ADAM_HYPER[:2], eps=ADAM_HYPER[2], fused=fused)  # == ppo.py:116-117
        self.stats = {}
        self._last_adv = self._last_V0 = None   # the last update()'s normalised advantages, and with norm_reward its V0 (the trainer's logs)
        # HIP paths: fused f32-MFMA kernels instead of ~40 (mlp64x2) / ~120 (resmlp512) PyTorch kernels per epoch
        on_gpu = self.device.type == "cuda" and cfg.fused_update
        # the D-64-64 heads: D = 16 (10 beams) or 42 (36 beams), rows float32 or float16 (obs_f16 envs) -- include/navppo.h
        self.fused_mlp64 = (on_gpu and cfg.policy == "mlp64x2" and isinstance(actor, nets.MLP64Actor)
                            and actor.layer1.in_features in (16, 42))
        self.obs_dim = actor.layer1.in_features if isinstance(actor, nets.MLP64Actor) else actor.rb1.f_in
        check_update_config(cfg)
        check_minibatch_config(cfg)
        check_lr_schedule_config(cfg)
        check_learn_var_config(cfg, self.ctx.world)
        self.max_norm = None if cfg.max_grad_norm is None else float(cfg.max_grad_norm)
        self.kl_limit = None if cfg.target_kl is None else 1.5 * float(cfg.target_kl)   # Stable-Baselines3's factor
        # lr_schedule: lr_adaptive = the rule runs after every optimiser step; lr_value = the rate the next step starts from (adaptive),
        # or the rate set_lr() put in force ("linear": the trainer, per iteration); None = cfg.lr as it stands at every call
        self.lr_adaptive = cfg.lr_schedule == "adaptive"
        self.lr_value = float(cfg.lr) if self.lr_adaptive else None
        self.lr_state = None     # adaptive, fused: [4] (two rate slots, raises, lowerings) on the device, zeroed here: the first step starts at cfg.lr
        self.lr_counts = (0, 0)  # adaptive: raises and lowerings since construction
        self.kl_steps = None     # adaptive: [steps] the approx_kl (global, on several ranks) of every optimiser step of the last update()
        self.mode = ADAPTIVE_LR if self.lr_adaptive else KL_STOP if self.kl_limit is not None else CLIP if self.max_norm is not None else PLAIN
        # learn_var: [8] (theta, var, m, v, gradient, steps taken, steps skipped, entropy), on the updater's device; after this only the
        # *_var entry points (fused) or the mirror's step (PyTorch) write it.  The trainer's variance is a view of slot 1.
        self.learn_var = bool(cfg.learn_var)
        self.var_state = None
        if self.learn_var:
            self.mode = LEARN_VAR
            self.var_state = torch.tensor(var_state_init(cfg.init_var), dtype=torch.float32, device=self.device)
            self._var_t = 0   # (the PyTorch path: optimiser steps so far, Adam's count for the mirror)
            self._var_skipped0 = 0   # the skipped steps the last summary saw (the state counts since its initialisation)
        self._clipping = self.mode != PLAIN   # the clipped machinery runs and fills clip_stats
        self.update_index = 0    # updates run so far: the high word of the shuffle's counter
        self._mb_key = minibatch_key(cfg.seed, self.ctx.rank)
        self._shuf = self._shuf_key = None   # the ONE permuted copy of the batch (navppo_shuffle_batch's outputs), regrown like _prep
        self.kl_state = None     # target_kl on, fused: [4] (stopped, steps taken, tripping approx_kl, its step) of the last update(), on the device
        self.clip_stats = None   # clipping on: [n_ep, 4] (s_actor, s_critic, coef_actor, coef_critic) of the last update(), on the device
        self.fused_resmlp512 = (on_gpu and cfg.policy == "resmlp512" and isinstance(actor, nets.ResMLPActor)
                                and actor.rb1.f_in == 16 and actor.rb1.fc1.out_features == 512)
        if self.fused_resmlp512 and cfg.update_arith == "f32":
            # the fused 512-wide kernels exist in ONE arithmetic (csrc/ppo_resmlp512.hip: the products that fill a k-step of the
            # bf16 MFMA are split-bf16 float32 products, the rest f32-input MFMA).  A caller who asks for native float32
            # products gets them -- from PyTorch's float32 GEMMs, ~4 x slower per epoch -- instead of being ignored.
            import warnings
            warnings.warn("update_arith='f32' with policy='resmlp512': the fused 512-wide kernels have no all-f32-MFMA build; "
                          "this updater runs the PyTorch float32 path (slower).  Use update_arith='bf16x3' (default) for the fused kernels.")
            self.fused_resmlp512 = False
        self.fused = "navppo_mlp64" if self.fused_mlp64 else "navppo_resmlp512" if self.fused_resmlp512 else None
        self.bf16x3 = self.fused_mlp64 and cfg.update_arith == "bf16x3"   # (16- and 42-column rows, float32 or float16)
        self._prep = self._prep_key = None
        self._n_actor = self.fp.module_numel[0]   # the actor's slice of the flat buffers is [0, _n_actor), the critic's the rest
        if self.fused:
            d = self.obs_dim
            assert tuple(self.fp.module_numel) == ((64 * d + 4354, 64 * d + 4289) if self.fused_mlp64 else (50290, 50257))
            self._ws = None
            if self.fused_mlp64:
                self._ws = torch.empty(lib().navppo_mlp64_workspace_bytes(d) // 4, dtype=torch.float32, device=self.device)
            self._fstats = torch.zeros(8, dtype=torch.float32, device=self.device)
            self._fhist = torch.zeros((max(cfg.n_updates_per_iteration, 1), 8), dtype=torch.float32, device=self.device)
            # single GPU: Adam runs inside the kernel that sums the partial gradients (navppo_*_update_epoch)
            self._adam_m = torch.zeros_like(self.fp.flat)
            self._adam_v = torch.zeros_like(self.fp.flat)
            self._adam_t = 0
            if self.lr_adaptive:
                self.lr_state = torch.zeros(4, dtype=torch.float32, device=self.device)

    def _lr(self):
        """the `lr` argument of the fused entry points (adaptive: where a zeroed state starts)"""
        return float(self.cfg.lr if self.lr_value is None or self.lr_adaptive else self.lr_value)

    def set_lr(self, lr):
        """Puts a learning rate in force: lr_schedule="linear" (the trainer, per iteration), and the resumed rate of "adaptive" -- into
        BOTH slots of the device state, whichever the next step reads."""
        self.lr_value = float(lr)
        self.opt.param_groups[0]["lr"] = self.lr_value
        if self.lr_state is not None:
            self.lr_state[:2] = self.lr_value

    def _mode_args(self, cstats, adapt=False):
        """The arguments the step mode puts behind an entry point's own -- the one place that knows them.  Plain Adam: none.  Every
        other mode: max_norm (+inf = no clipping) and the step's clip-statistics row `cstats` [4], then the KL stop's (kl_limit,
        kl_state_dev) or the adaptive rate's (kl_target, lr_min, lr_max, adapt, lr_state_dev).  adapt: whether this step adapts the
        rate -- the first step of an update does not."""
        if (cstats is None) != (self.mode == PLAIN):
            raise ValueError(f"step mode {self.mode or 'plain'!r}: a clip-statistics row goes with every mode but the plain one, and only with them")
        if self.mode == PLAIN:
            return ()
        cfg, args = self.cfg, (math.inf if self.max_norm is None else self.max_norm, _ptr(cstats))
        if self.mode == KL_STOP:
            args += (self.kl_limit, _ptr(self.kl_state))
        elif self.mode == ADAPTIVE_LR:
            args += (float(cfg.desired_kl), float(cfg.lr_min), float(cfg.lr_max), int(adapt), _ptr(self.lr_state))
        elif self.mode == LEARN_VAR:   # (lr_state None: the constant rate, the adaptive rule's arguments are not read)
            args += (float(cfg.desired_kl), float(cfg.lr_min), float(cfg.lr_max), int(adapt), _ptr(self.lr_state),
                     float(cfg.ent_coef), float(cfg.var_min), float(cfg.var_max), _ptr(self.var_state))
        return args

    def _step_kw(self, plan, st):
        """What a step's launches get beside today's positional arguments, as two keyword dictionaries: where a slice starts in the
        prepared batch (minibatches), and whether the adaptive rate adapts -- on every step but the first of an update.  Both empty on
        whole-batch epochs of the other modes."""
        return ({"first_row": st.first_row} if plan.K > 1 else {}), ({"adapt": st.index > 0} if self.lr_adaptive else {})

    def _workspace(self, n):
        """Scratch of the fused kernels: fixed for the 2x64 heads, per-sample partial block outputs for the 512-wide nets."""
        if self.fused_resmlp512:
            need = lib().navppo_resmlp512_workspace_bytes(int(n)) // 4 + 4
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._ws

    def _obs_args(self, obs):
        """The observation arguments of the fused entry points -- (pointer, obs_dim, obs_f16) for the D-64-64 heads, (pointer, obs_f16)
        for the 512-wide nets -- after checking what is behind the pointer: rows of self.obs_dim columns, float32 or float16 (the
        kernels widen half rows as they load)."""
        ok = (torch.float32, torch.float16)
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim or obs.dtype not in ok or not obs.is_contiguous():
            raise ValueError(f"{self.fused}: observations must be contiguous [n, {self.obs_dim}] rows of {ok}, got "
                             f"{tuple(obs.shape)} {obs.dtype}")
        p = _ptr(obs)
        f16 = int(obs.dtype == torch.float16)
        return (p, self.obs_dim, f16) if self.fused_mlp64 else (p, f16)

    def prepare(self, obs):
        """bf16x3: split the batch's observations into bf16 pieces (navppo_mlp64_bf16x3_prepare) -- once per update, the rows do not
        change over the epochs.  The epoch entry points use the prepared buffer while `obs` is the tensor it was made from."""
        p, d, f16 = self._obs_args(obs)
        need = lib().navppo_mlp64_bf16x3_prep_bytes(int(obs.shape[0]), self.obs_dim)
        if self._prep is None or self._prep.numel() < need:
            self._prep = None
            self._prep = torch.empty(need, dtype=torch.uint8, device=self.device)
        _navppo("navppo_mlp64_bf16x3_prepare", p, d, f16, int(obs.shape[0]), _ptr(self._prep))
        self._prep_key = (obs.data_ptr(), tuple(obs.shape), obs.dtype, obs._version)

    def invalidate_prepared(self):
        """The rows behind a prepared tensor changed without torch noticing (the HIP rollout / step kernels write the trainer's
        buffers through raw pointers: no version bump).  PPOTrainer.rollout() calls this; any other writer of such a buffer must."""
        self._prep_key = None

    def _prepared(self, obs):
        """The pre-split pieces of `obs`.  Reused while `obs` is the very tensor prepare() saw, unchanged as far as torch knows
        (pointer, shape, dtype, version counter) AND nobody called invalidate_prepared() since."""
        if self._prep_key != (obs.data_ptr(), tuple(obs.shape), obs.dtype, obs._version):
            self.prepare(obs)
        return _ptr(self._prep)

    def _batch_args(self, obs, acts, logp_old, rtg, adv, var, first_row=None):
        """(family, the arguments every *_loss_grad / *_update_epoch entry point of it takes between params_dev and the step's): the
        rows -- obs, or their prepared pieces -- then acts, logp_old, rtg, adv, n, var, clip.  first_row: `obs` is the slice from that
        row on of the batch that was prepared (a multiple of 32: whole tile blocks in front of it); None: a batch of its own."""
        if self.bf16x3 and first_row is not None:
            rows = (_ptr(self._prep, lib().navppo_mlp64_bf16x3_prep_bytes(first_row, self.obs_dim)), self.obs_dim)   # (0 samples: 0 bytes)
        else:
            rows = (self._prepared(obs), self.obs_dim) if self.bf16x3 else self._obs_args(obs)
        fam = "navppo_mlp64_bf16x3" if self.bf16x3 else self.fused
        return fam, (*rows, _ptr(acts), _ptr(logp_old), _ptr(rtg), _ptr(adv), int(obs.shape[0]), float(var), float(self.cfg.clip))

    def _fused_loss_grad(self, obs, acts, logp_old, rtg, adv, var, stats=None, *, first_row=None):
        """evaluate + losses + backward of ppo.py:307-386 in the HIP kernels of csrc/ppo_mlp64.hip; gradients land
        in the flat gradient buffer, (actor_loss, approx_kl, clip_frac, -, critic_loss) in self._fstats."""
        for t in (acts, logp_old, rtg, adv):
            assert t.is_contiguous() and t.dtype == torch.float32
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, var, first_row)
        _navppo(fam + "_loss_grad", _ptr(self.fp.flat), *batch, _ptr(self.fp.grad), _ptr(self._fstats if stats is None else stats),
                _ptr(self._workspace(obs.shape[0])))

    def _fused_loss_grad_net(self, net, obs, acts, logp_old, rtg, adv, var, stats):
        """One net's half of _fused_loss_grad (navppo_mlp64[_bf16x3]_loss_grad_net): its slice of the flat gradient, its statistics."""
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, var)
        _navppo(fam + "_loss_grad_net", int(net), _ptr(self.fp.flat), *batch, _ptr(self.fp.grad), _ptr(stats),
                _ptr(self._workspace(obs.shape[0])))

    def _fused_adam(self, grad_scale, lo=0, n=None, step=None, cstats=None, kl_dev=None, *, adapt=False):
        """Scale + Adam on the flat buffer, or on the slice [lo, lo + n) at optimiser step `step` (one net of the pipelined epoch):
        navppo_adam_step of the updater's step mode.  cstats ([4], every mode but the plain one): per-net norm, guard and clip of the
        scaled gradient first.  kl_dev ([1], the KL stop and the adaptive rate): the global approx_kl the stop decision, or the step's
        rate (with the device state), is taken from."""
        mode = self._mode_args(cstats, adapt)
        if (kl_dev is None) == (self.mode in (KL_STOP, ADAPTIVE_LR)):
            raise ValueError(f"step mode {self.mode or 'plain'!r}: the global approx_kl goes with the KL stop and the adaptive rate, and only with them")
        if step is None:
            self._adam_t += 1
            step = self._adam_t
        n_ = int(self.fp.numel - lo if n is None else n)
        head = tuple(_ptr(t, 4 * lo) for t in (self.fp.flat, self.fp.grad, self._adam_m, self._adam_v)) + (n_,)
        hyper = (self._lr(), *ADAM_HYPER, int(step))
        if not mode:
            args = head + (float(grad_scale),) + hyper
        else:   # (the actor's share of the slice and max_norm go in front of Adam's own, the rest of the mode's behind)
            args = head + (max(0, min(n_, self._n_actor - lo)), float(grad_scale), mode[0]) + hyper + mode[1:]
            if kl_dev is not None:
                args += (_ptr(kl_dev),)
        _navppo("navppo_adam_step" + self.mode, *args)

    def _pipelined_epochs(self, n_ep, world, obs, acts, logp_old, rtg, adv, var_f):
        """The multi-GPU epochs of the 2x64 heads as a two-stage pipeline.  Actor and critic are disjoint nets whose losses share
        nothing inside the epoch loop (the advantages are fixed before it, ppo.py:275-284), so each net's all-reduce (RCCL's own
        stream) runs under the OTHER net's pass -- the actor's under the critic's pass of the same epoch, the critic's under the
        actor's pass of the next one -- and neither the wire time nor the cross-stream hand-over is on the compute stream's
        critical path.  Same kernels on the same data as the unpipelined order: the weights are bit-identical.
        Returns every epoch's squared norms of the mean (actor, critic) gradient.  Clipping on: each net's step is
        navppo_adam_step_clipped, which reports into its own row -- its net's columns are gathered into self.clip_stats at the end."""
        n_a = self._n_actor
        t0 = self._adam_t
        clipped = self._clipping   # (the pipeline runs plain or clipped: the other two modes are refused with it)
        nets_ = ((0, n_a, self.fp.grad[:n_a]), (n_a, self.fp.numel - n_a, self.fp.grad[n_a:]))   # (offset, parameters, gradient)
        if clipped:
            cs2 = torch.zeros((max(n_ep, 1), 2, 4), dtype=torch.float32, device=obs.device)
        else:
            gn_sq = torch.zeros((max(n_ep, 1), 2), device=obs.device)
        waits = [None, None]
        for ep in range(n_ep + 1):   # (the last round: only the steps of epoch n_ep - 1)
            for k, (lo, n, g) in enumerate(nets_):
                if waits[k] is not None:   # epoch ep - 1's gradient of net k has arrived (long ago: it had the other net's pass to do so)
                    waits[k].wait()
                    self._fused_adam(1.0 / world, lo, n, t0 + ep, cstats=cs2[ep - 1, k] if clipped else None)
                    if not clipped:
                        gn_sq[ep - 1, k] = torch.dot(g, g)
                if ep < n_ep:
                    self._fused_loss_grad_net(k, obs, acts, logp_old, rtg, adv, var_f, self._fhist[ep])
                    waits[k] = dist.all_reduce(g, op=dist.ReduceOp.SUM, async_op=True)
        self._adam_t = t0 + n_ep
        if clipped:
            self.clip_stats = torch.stack([cs2[:n_ep, 0, 0], cs2[:n_ep, 1, 1], cs2[:n_ep, 0, 2], cs2[:n_ep, 1, 3]], 1)
            return self.clip_stats[:, :2]   # squared norms of the MEAN gradient, per epoch and net
        return gn_sq / float(world) ** 2

    def _fused_value(self, obs):
        """V = critic(obs).squeeze() (ppo.py:275) by the forward half of the critic's fused pass."""
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=obs.device)
        ws = (_ptr(self._workspace(obs.shape[0])),) if self.fused_resmlp512 else ()
        _navppo(self.fused + "_value", _ptr(self.fp.flat, 4 * self._n_actor), *self._obs_args(obs), int(obs.shape[0]), _ptr(out), *ws)
        return out

    def _fused_epoch(self, obs, acts, logp_old, rtg, adv, var, stats, cstats=None, *, first_row=None, adapt=False):
        """One epoch of ppo.py:305-392 on one GPU: losses, gradients and both Adam steps in four launches -- the *_update_epoch entry
        point of the updater's step mode.  cstats ([4], every mode but the plain one): one more small launch clips and steps behind the
        reduction; the KL stop runs gated twins of the same launches with the stop decision in the step launch, the adaptive rate the
        clipped launches with a step launch that derives its rate on the device.  first_row: _batch_args; adapt: _mode_args."""
        mode = self._mode_args(cstats, adapt)
        self._adam_t += 1
        fam, batch = self._batch_args(obs, acts, logp_old, rtg, adv, 0.0 if self.learn_var else var, first_row)
        if self.learn_var:   # the *_var entry points have no by-value variance: (..., n, clip)
            batch = batch[:-2] + batch[-1:]
        _navppo(fam + "_update_epoch" + self.mode, _ptr(self.fp.flat), *batch, self._lr(), *ADAM_HYPER, int(self._adam_t),
                _ptr(self._adam_m), _ptr(self._adam_v), _ptr(self.fp.grad), _ptr(stats), _ptr(self._workspace(obs.shape[0])), *mode)

    def _clip_and_step(self, ep):
        """The PyTorch formulation of a clipped epoch's optimiser step (the CPU / gloo path and the tests' float32 reference), the
        contract of the navppo_*_clipped entry points per net: s = sum of squares of the net's gradient; s not finite: that net's
        slice of the parameters and of Adam's exp_avg / exp_avg_sq is restored after the step (the step counter advances), its
        coefficient is 0 and its gradient stays unclipped; else the gradient is scaled by min(1, max_norm / (sqrt(s) + 1e-6))."""
        n_a, cs = self._n_actor, self.clip_stats
        oks = []
        with torch.no_grad():
            for k, (lo, hi) in enumerate(((0, n_a), (n_a, self.fp.numel))):
                g = self.fp.grad[lo:hi]
                sq = (g * g).sum()
                ok = torch.isfinite(sq)
                coef = torch.where(ok, torch.clamp(self.max_norm / (sq.sqrt() + 1e-6), max=1.0), torch.zeros_like(sq))
                g.mul_(torch.where(ok, coef, torch.ones_like(coef)))
                cs[ep, k], cs[ep, 2 + k] = sq, coef
                oks.append(ok)
            st = self.opt.state.get(self.fp.proxy, {})
            keys = ("exp_avg", "exp_avg_sq")
            old = [self.fp.flat.clone()] + [st[key].clone() if key in st else torch.zeros_like(self.fp.flat) for key in keys]
        self.opt.step()
        with torch.no_grad():
            st = self.opt.state[self.fp.proxy]
            for k, (lo, hi) in enumerate(((0, n_a), (n_a, self.fp.numel))):
                for cur, was in zip([self.fp.flat] + [st[key] for key in keys], old):
                    cur[lo:hi].copy_(torch.where(oks[k], cur[lo:hi], was[lo:hi]))

    def value(self, obs):
        """V = critic(obs).squeeze() (ppo.py:275) for [n, D] rows."""
        with torch.no_grad():
            if self.fused and obs.is_contiguous() and obs.data_ptr() % 16 == 0 and obs.dtype in (torch.float32, torch.float16):
                return self._fused_value(obs)
            return self.critic(obs.float()).squeeze(-1)

    # ---- the steps of an update: the plan, the one permuted copy (PPOConfig.minibatch_size), the steps in order
    def _plan(self, n, n_ep):
        """The step plan of an update of n_ep epochs on n samples.  minibatch_size None or >= n: whole-batch epochs.  Several ranks: all
        must hold the same n (one collective, with minibatch_size set), else every rank raises."""
        cfg = self.cfg
        check_minibatch_config(cfg)
        size = cfg.minibatch_size
        if size is not None and self.ctx.enabled:
            nn = torch.tensor([n, -n], dtype=torch.int64, device=self.device)
            self.ctx.all_reduce_max(nn)
            hi, lo = int(nn[0]), -int(nn[1])
            if hi != lo:
                raise ValueError(f"minibatch_size: every rank must hold the same number of samples, got between {lo} and {hi} (this rank: {n})")
        if size is None or size >= n:
            return _StepPlan(n=n, n_ep=n_ep, size=n, K=1, shuffle="none", n_steps=n_ep, update=self.update_index)
        K = -(-n // size)
        return _StepPlan(n=n, n_ep=n_ep, size=size, K=K, shuffle=cfg.minibatch_shuffle, n_steps=n_ep * K, update=self.update_index)

    def _shuffled(self, batch, counter):
        """`batch` gathered by batch_permutation(n, key, counter): always from the ORIGINAL batch into the one permuted copy.  Fused: one
        navppo_shuffle_batch launch (gated by kl_state: behind an early stop it returns at its entry), then -- bf16x3 -- the split of the
        permuted rows into the prepared buffer.  PyTorch: index_select by the host mirror."""
        obs = batch[0]
        n = int(obs.shape[0])
        if not self.fused:
            perm = batch_permutation(n, self._mb_key, counter).to(obs.device)
            return tuple(t.index_select(0, perm) for t in batch)
        key = (obs.dtype, obs.shape[1])
        if self._shuf is None or self._shuf_key != key or self._shuf[1].shape[0] < n:
            self._shuf = None
            f32 = dict(dtype=torch.float32, device=self.device)
            self._shuf = (torch.empty((n, obs.shape[1]), dtype=obs.dtype, device=self.device), torch.empty((n, 2), **f32),
                          torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32))
            self._shuf_key = key
        out = tuple(t[:n] for t in self._shuf)
        p, d, f16 = self._obs_args(obs)[:1] + (self.obs_dim, int(obs.dtype == torch.float16))
        _navppo("navppo_shuffle_batch", p, d, f16, *(_ptr(t) for t in batch[1:]), n, self._mb_key, int(counter), *(_ptr(t) for t in out),
                _ptr(self.kl_state))
        if self.bf16x3:
            self.prepare(out[0])
        return out

    def _steps(self, plan, batch):
        """Every optimiser step of `plan` in order: n_ep times the whole batch, or -- minibatches -- per epoch its K slices, of the
        batch as it lies ("none") or of its permuted copy, drawn before every epoch ("epoch") or once ("update")."""
        if plan.K == 1:
            for ep in range(plan.n_ep):
                yield _Step(ep, ep, 0, batch)
            return
        src = batch
        for ep in range(plan.n_ep):
            if plan.shuffle == "epoch" or (plan.shuffle == "update" and ep == 0):
                src = self._shuffled(batch, minibatch_counter(plan.update, ep if plan.shuffle == "epoch" else 0))
            for k, lo in enumerate(range(0, plan.n, plan.size)):
                yield _Step(ep * plan.K + k, ep, lo, tuple(t[lo:lo + plan.size] for t in src))

    def _epoch_losses(self, rows, k, plan):
        """[n_ep, 2] per-epoch (actor, critic) losses from the first k rows of `rows`, one per step that ran: K = 1 the rows themselves;
        else row e is the mean over the steps of epoch e that ran; NaN where none ran."""
        n_ep, K = plan.n_ep, plan.K
        if K == 1:
            losses = rows[:k].clone()
            return losses if k >= n_ep else torch.cat([losses, torch.full((n_ep - k, 2), math.nan, device=rows.device)])
        ran = (torch.arange(n_ep * K, device=rows.device) < k).reshape(n_ep, K, 1)
        r = torch.where(ran, rows[:n_ep * K].reshape(n_ep, K, 2), torch.zeros((), device=rows.device))
        return r.sum(1) / ran.sum(1)   # (0 / 0: NaN)

    def _clip_row(self, ep, c):
        """This epoch's clip-statistics row from the gradient as it stands, coefficient c: 0 = the update stopped before this step, 1 = unclipped."""
        g_a, g_c = self.fp.grad[:self._n_actor], self.fp.grad[self._n_actor:]
        self.clip_stats[ep] = torch.stack([(g_a * g_a).sum(), (g_c * g_c).sum(), g_a.new_full((), c), g_a.new_full((), c)])

    def _var_step_host(self, grad_sum, coef):
        """learn_var on the PyTorch path: the step of log var through the kernel's host mirror, at the rate the nets just stepped with"""
        cfg = self.cfg
        self._var_t += 1
        new = learned_var_reference(self.var_state.tolist(), grad_sum, coef, cfg.ent_coef, self.opt.param_groups[0]["lr"], ADAM_HYPER[:2],
                                    ADAM_HYPER[2], self._var_t, cfg.var_min, cfg.var_max)
        self.var_state.copy_(torch.tensor(new, dtype=torch.float32))

    def var_state_dict(self):
        """learn_var: what a checkpoint keeps of the state -- theta, Adam's moments and the steps taken"""
        st = self.var_state.tolist()
        return {"theta": st[THETA], "m": st[ADAM_M], "v": st[ADAM_V], "steps": st[STEPS]}

    def load_var_state(self, d=None):
        """learn_var: the state of a checkpoint (var_state_dict), or -- None -- a fresh one from init_var.  Written IN PLACE: the
        trainer's variance is a view of slot 1, and captured graphs hold its address."""
        st = var_state_init(self.cfg.init_var)
        if d is not None:
            theta = torch.tensor(float(d["theta"]), dtype=torch.float32)
            st = [float(theta), float(torch.exp(theta)), float(d["m"]), float(d["v"]), 0.0, float(d["steps"]), 0.0, float(theta + ENTROPY_AT_ZERO)]
            self._var_t = int(d["steps"])
        self.var_state.copy_(torch.tensor(st, dtype=torch.float32))
        self._var_skipped0 = 0

    def _fused_record(self, plan, V0, r0, gn_sum=None, net_gn=None):
        """What every fused runner ends with: ONE synchronisation (kl_state) after the last epoch, then the record from the first k rows
        of _fhist.  gn_sum / net_gn: the runner's own sums of norms; the single-GPU epochs have none and take them from the rows."""
        if plan.n_ep == 0:
            return r0
        n_st = plan.n_steps   # optimiser steps queued: with minibatches every row below is a STEP's
        steps, stopped = n_st, 0
        if self.kl_limit is not None:   # (the update synchronises for its statistics anyway)
            st = self.kl_state.tolist()
            steps, stopped = int(st[1]), int(st[0] != 0.0)
            self._adam_t -= n_st - steps   # Adam's bias correction counts steps TAKEN: every step's launch counted one
        k = steps + stopped
        h = self._fhist[:k]
        losses = self._epoch_losses(self._fhist[:, 0:5:4], k, plan)   # columns 0 (actor loss) and 4 (critic loss)
        gn_last = self.fp.grad.norm() / self.ctx.world   # multi-GPU: fp.grad holds the all-reduced SUM (the 1 / world scale is inside navppo_adam_step)
        own = gn_sum is not None
        if not own and not self._clipping:
            # every epoch's norms as the reference logs them (ppo.py:351-352, 389-390) without a norm launch per epoch: the fused epoch leaves
            # the squared per-net norms of the epoch BEFORE in columns 3 / 7 of its row (reduce_adam / resmlp_reduce), the last epoch's stand
            # (minibatches: a row per step, the slots of the step before -- reduce_adam's lie at a fixed place of the workspace and its grid
            # does not depend on n, so a shorter last slice and an epoch boundary change nothing; resmlp_reduce's lie BEHIND the per-sample
            # part of the workspace and move with n: _run_fused_single takes that family's norms itself when the slices are not all equal)
            if n_st > 1:
                prev = h[1:, 3:8:4].clone()   # [n_st - 1, (actor, critic)]
                gn_sum, net_gn = prev.sum(1).sqrt().sum() + gn_last, prev.sqrt().sum(0)
            else:
                gn_sum = gn_last * n_st
        return _Epochs(k=k, steps=steps, stopped=stopped, losses=losses, sums=h.sum(0)[[0, 4, 1, 2]], gn_sum=gn_sum, v_sum=V0.mean() * k,
                       net_gn=net_gn, net_gn_open=not own, K=plan.K)

    def _run_fused_single(self, plan, batch, var_f, V0, r0):
        """One GPU: _fused_epoch.  Per-epoch diagnostics land in row ep of a device buffer: no extra launches inside the epoch loop."""
        # gn (resmlp512 on slices of two lengths, no clip statistics): every step's per-net norms by two small launches -- the slot of
        # the step before is read at the wrong place when n changes between two calls (the shorter last slice, the epoch boundary)
        n_a = self._n_actor
        gn = (torch.zeros((plan.n_steps, 2), device=self.device)
              if plan.K > 1 and self.fused_resmlp512 and not self._clipping and plan.n % plan.size else None)
        for st in self._steps(plan, batch):
            rows, adapt = self._step_kw(plan, st)
            self._fused_epoch(*st.batch, var_f, self._fhist[st.index], self.clip_stats[st.index] if self._clipping else None, **rows, **adapt)
            if gn is not None:
                gn[st.index] = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:]]))
        if self.lr_adaptive:
            self.kl_steps = self._fhist[:plan.n_steps, 1].clone()
        return self._fused_record(plan, V0, r0, *((gn.pow(2).sum(1).sqrt().sum(), gn.sum(0)) if gn is not None and plan.n_ep > 0 else ()))

    def _run_fused_multi(self, plan, batch, var_f, V0, r0):
        """Several GPUs: fused passes -> ONE all-reduce of the flat gradient (RCCL) -> scale + Adam in one launch."""
        ctx, n_a, gn = self.ctx, self._n_actor, None   # gn: step sums of the MEAN gradient's (actor, critic, whole) norm
        need_kl = self.mode in (KL_STOP, ADAPTIVE_LR)   # (adaptive lr: every rank must derive the same rate)
        kl_glob = torch.zeros((max(plan.n_steps, 1), 2), dtype=torch.float32, device=self.device) if need_kl else None
        for st in self._steps(plan, batch):
            i, (rows, adapt) = st.index, self._step_kw(plan, st)
            self._fused_loss_grad(*st.batch, var_f, stats=self._fhist[i], **rows)
            ctx.all_reduce_sum(self.fp.grad)
            if need_kl:   # the passes are ungated: a stop only keeps the weights
                n = float(st.batch[0].shape[0])
                global_mean(ctx, self._fhist[i, 1] * n, n, out=kl_glob[i])
            elif not self._clipping:   # every epoch's norms of the MEAN gradient (two small launches beside an all-reduce)
                g3 = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:], self.fp.grad])) / ctx.world
                gn = g3 if gn is None else gn + g3
            # (clipping: the norms of the mean gradient are in the clip statistics)
            self._fused_adam(1.0 / ctx.world, cstats=self.clip_stats[i] if self._clipping else None, kl_dev=kl_glob[i] if need_kl else None, **adapt)
        if self.lr_adaptive:
            self.kl_steps = kl_glob[:plan.n_steps, 0]
        return self._fused_record(plan, V0, r0, *((gn[2], gn[:2]) if gn is not None else ()))

    def _run_fused_pipelined(self, plan, batch, var_f, V0, r0):
        """Several GPUs, overlap_allreduce: every epoch runs in _pipelined_epochs; pg: its squared norms of the MEAN gradient."""
        pg = self._pipelined_epochs(plan.n_ep, self.ctx.world, *batch, var_f)
        gn = torch.cat([pg.sqrt().sum(0), pg.sum(1).sqrt().sum().reshape(1)]) if plan.n_ep > 0 else None
        return self._fused_record(plan, V0, r0, *((gn[2], gn[:2]) if gn is not None else ()))

    def _run_pytorch(self, plan, batch, var, V0, r0):
        """CPU, gloo, and resmlp512 with update_arith="f32": ppo.py:305-392 in PyTorch."""
        ctx, n_ep = self.ctx, plan.n_ep
        steps, stopped, losses = plan.n_steps, 0, torch.zeros((plan.n_steps, 2), device=batch[0].device)   # (a row per step)
        acc, net_gn = torch.zeros(6, device=batch[0].device), None  # sums over steps of the diagnostics and of the per-net gradient norms
        kls = []   # adaptive lr: every step's (global) approx_kl, float32
        for ep, _, _, (obs, acts, logp_old, rtg, adv) in self._steps(plan, batch):   # ppo.py:305 (ep: the step -- an epoch, or a slice of one)
            if self.learn_var:   # theta = log var as a leaf: autograd gives d(actor loss)/d theta, the entropy term is the mirror's
                log_var = self.var_state[THETA].detach().clone().requires_grad_(True)
                var = torch.exp(log_var)
            a_loss, c_loss, ratios, logp, _ = ppo_losses(self.actor, self.critic, obs, acts, logp_old, rtg, adv, var, self.cfg.clip)
            self.fp.grad.zero_()
            (a_loss + c_loss).backward()                       # disjoint nets: same grads as the two backward()s of :349,:386
            if ctx.enabled:
                ctx.all_reduce_sum(self.fp.grad)
                self.fp.grad.div_(ctx.world)
            ratios, lr_, trip = ratios.detach(), logp.detach() - logp_old, False
            if self.kl_limit is not None or self.lr_adaptive:   # both act before the step, on the global approx_kl (weighted by the ranks' batch sizes)
                kl = float(global_mean(ctx, ((ratios - 1) - lr_).sum(), float(lr_.numel())))
            if self.kl_limit is not None:   # a NaN trips
                trip = not (kl <= self.kl_limit)
            if self.lr_adaptive:   # the rule through the kernel's host mirror; not on an update's first step
                d = adaptive_lr_direction(kl, self.cfg.desired_kl, adapt=ep > 0)
                self.lr_value = adaptive_lr_reference(self.lr_value, kl, self.cfg.desired_kl, self.cfg.lr_min, self.cfg.lr_max, adapt=ep > 0)
                self.lr_counts = (self.lr_counts[0] + (d > 0), self.lr_counts[1] + (d < 0))
                self.opt.param_groups[0]["lr"] = self.lr_value
                kls.append(kl)
            if trip:   # neither net is stepped; the gradient stays unclipped, the coefficients are reported as 0, the remaining epochs do not run
                steps, stopped = ep, 1
                self._clip_row(ep, 0.0)
            elif self.max_norm is not None:
                self._clip_and_step(ep)
            else:
                self.opt.step()                                # ppo.py:381,392
                if self._clipping:   # (target_kl without max_grad_norm: the norms of every epoch, coefficient 1)
                    self._clip_row(ep, 1.0)
            if self.learn_var:   # theta follows the actor: its coefficient and rate of this step, Adam's count as torch's (steps so far)
                self._var_step_host(float(log_var.grad), float(self.clip_stats[ep, 2]))
            with torch.no_grad():                              # ppo.py:323-336
                losses[ep] = torch.stack([a_loss.detach(), c_loss.detach()])
                acc += torch.stack([a_loss.detach(), c_loss.detach(), ((ratios - 1) - lr_).mean(),
                                    ((ratios - 1).abs() > self.cfg.clip).float().mean(), self.fp.grad.norm(), V0.mean()])
                g2 = torch.stack(torch._foreach_norm([self.fp.grad[:self._n_actor], self.fp.grad[self._n_actor:]]))
                net_gn = g2 if net_gn is None else net_gn + g2
            if trip:
                break
        if self.lr_adaptive:
            self.kl_steps = torch.tensor(kls, dtype=torch.float32)
        return _Epochs(k=steps + stopped, steps=steps, stopped=stopped, losses=self._epoch_losses(losses, steps + stopped, plan), sums=acc[:4],
                       gn_sum=acc[4], v_sum=acc[5], net_gn=net_gn, K=plan.K)

    def _summarise(self, r, plan, flat_before):
        """The record of the epochs that ran -> the stats dict.  Gradient norms are means over the r.k epochs, from the first source
        that has them: the clip statistics (every epoch's pre-clip norms), the runner's own sums, the gradient as it stands."""
        k, n_a, clipping, multi, world = r.k, self._n_actor, self._clipping, self.ctx.enabled, self.ctx.world
        cs = self.clip_stats[:k] if clipping else None
        # every epoch's pre-clip norm of the whole gradient: folded in before the ranks' mean when fused, after it in PyTorch (not the same last bit)
        total = cs[:, :2].sum(1).sqrt() if clipping and k > 0 else None
        acc = torch.cat([r.sums, torch.stack([total.sum() if total is not None and self.fused else r.gn_sum, r.v_sum])]) / max(k, 1)
        if multi:
            self.ctx.all_reduce_sum(acc)
            acc = acc / world
        if total is not None and not self.fused:
            acc = torch.cat([acc[:4], total.mean().reshape(1), acc[5:]])
        d = self.fp.flat - flat_before                         # the parameter-delta diagnostics of ppo.py:402-403
        extra = torch.stack(torch._foreach_norm([self.fp.grad[:n_a], self.fp.grad[n_a:], d[:n_a], d[n_a:]]))
        if self.fused and multi:
            extra = extra * extra.new_tensor([1.0 / world, 1.0 / world, 1.0, 1.0])   # norms of the MEAN gradient, as on one GPU
        if total is not None:
            extra = torch.cat([cs[:, :2].sqrt().mean(0), extra[2:]])
        elif r.net_gn is not None:   # (open: the runner's sums lack the last epoch, whose gradient still stands)
            extra = torch.cat([(r.net_gn + extra[:2] if r.net_gn_open else r.net_gn) / k, extra[2:]])
        clip_cols = []
        if clipping:   # share of clipped epochs, skipped steps; identical on every rank
            # (not the tripping epoch: its coefficient is 0 because the update stopped, not because anything was clipped or skipped)
            clipped_ep = (cs[:, 2:] < 1.0)[:k - r.stopped]
            clip_cols = [clipped_ep.float().sum(0) / max(k, 1), (~torch.isfinite(cs[:, :2])).float().sum(0)]
            if k == 0:
                clip_cols = [torch.zeros(2, device=self.device)] * 2
        # (the last four keys exist with max_grad_norm only -- not with target_kl alone: without it the trainer's log dictionary is what it was)
        keys = ["actor_loss", "critic_loss", "approx_kl", "clip_frac", "grad_norm", "value_mean", "actor_grad_norm", "critic_grad_norm",
                "actor_param_delta", "critic_param_delta",
                "grad_clip_frac_actor", "grad_clip_frac_critic", "skipped_steps_actor", "skipped_steps_critic"]
        lr_cols = [self.lr_state] if self.lr_state is not None else []   # (adaptive lr, fused: the state rides on this read-back)
        var_cols = [self.var_state.to(acc.device)] if self.learn_var else []   # (learn_var: the state rides on this read-back too)
        vals = [float(v) for v in torch.cat([acc, extra] + (clip_cols if self.max_norm is not None else []) + lr_cols + var_cols).tolist()]
        if var_cols:
            vals, vs = vals[:-VAR_STATE_LEN], vals[-VAR_STATE_LEN:]
        if lr_cols:   # the slot the last step wrote; the counts are cumulative
            vals, st = vals[:-4], vals[-4:]
            if plan.n_steps > 0:
                self.lr_value = st[(self._adam_t + 1) & 1]
            ups, downs = int(st[2]), int(st[3])
        elif self.lr_adaptive:
            ups, downs = self.lr_counts
        stats = dict(zip(keys, vals[:12] + [int(v) for v in vals[12:]]))
        if self.lr_adaptive:   # the rate after the update's last step, the raises and lowerings of this update; identical on every rank
            stats["lr"], stats["lr_ups"], stats["lr_downs"] = self.lr_value, ups - self._lr_counts0[0], downs - self._lr_counts0[1]
            self.lr_counts = (ups, downs)
        elif self.lr_value is not None:   # ("linear": the rate this update ran with)
            stats["lr"] = self.lr_value
        if var_cols:   # the variance the NEXT rollout draws its noise with, the gradient of the last step taken, the steps skipped in this update
            stats.update(var=vs[VAR], std=math.sqrt(vs[VAR]), entropy=1.0 + LOG_2PI + vs[THETA], var_grad=vs[GRAD],
                         var_steps_skipped=int(vs[SKIPPED]) - self._var_skipped0)
            self._var_skipped0 = int(vs[SKIPPED])
        if self.kl_limit is not None:   # steps taken (n_ep if the update never stopped) and whether it stopped; identical on every rank
            # (minibatches: kl_stop_step counts the steps, kl_stop_epoch the whole epochs completed)
            stats["kl_stop_epoch"], stats["kl_stopped"] = r.steps // r.K, r.stopped
            if r.K > 1:
                stats["kl_stop_step"] = r.steps
        return stats

    def update(self, obs, acts, logp_old, rtg, var, adv_raw=None, V0=None):
        """adv_raw / V0: advantages (before normalisation) and values computed by the caller (GAE); default = the reference's
        A = rtg - V (ppo.py:275-277).  Prologue, the epochs on the one path that applies, the summary, the published results."""
        cfg, ctx, n_ep = self.cfg, self.ctx, self.cfg.n_updates_per_iteration
        multi = ctx.enabled   # collectives run (also one forced rank)
        with torch.no_grad():
            V0 = self.value(obs) if V0 is None else V0
            adv = normalise_advantages(rtg - V0 if adv_raw is None else adv_raw, ctx)          # ppo.py:275-284
        flat_before = self.fp.flat.clone()
        zero = torch.zeros((), device=obs.device)   # n_updates_per_iteration == 0: nothing to report
        r0 = _Epochs(k=0, steps=0, stopped=0, losses=torch.zeros((n_ep, 2), device=obs.device), sums=torch.zeros(4, device=obs.device),
                     gn_sum=zero, v_sum=zero)
        if not (self.fused and obs.dtype == torch.float16):
            obs = obs.float()   # half rows (obs_f16 envs) are consumed as they are by the fused kernels only
        batch = (obs, acts, logp_old, rtg, adv)
        plan = self._plan(int(obs.shape[0]), n_ep)
        self.update_index += 1
        self._lr_counts0 = self.lr_counts
        n_st = plan.n_steps   # optimiser steps: a row of every per-step buffer each
        if self.fused:
            batch = tuple(t.contiguous() for t in batch)
            if self.bf16x3 and n_ep > 0 and plan.shuffle == "none":   # (shuffling: the permuted copy is prepared behind every shuffle instead)
                self.prepare(batch[0])   # ALWAYS here: the rollout kernels fill the buffer behind torch's back (no version bump)
            if self._fhist.shape[0] < n_st:
                self._fhist = torch.zeros((n_st, 8), dtype=torch.float32, device=self.device)
            if self.kl_limit is not None:   # zeroed once per update; afterwards only the library writes it
                self.kl_state = torch.zeros(4, dtype=torch.float32, device=obs.device)
        if self._clipping:   # every step's (s_actor, s_critic, coef_actor, coef_critic): filled on the device, read once after the epochs
            self.clip_stats = torch.zeros((max(n_st, 1), 4), dtype=torch.float32, device=obs.device)
        self._last_adv = batch[4]   # (PPOTrainer._grad_guard's diagnostics)
        if cfg.norm_reward:
            self._last_V0 = V0      # (the trainer's explained_variance: the critic before this update)
        runner = (self._run_pytorch if not self.fused else self._run_fused_single if not multi else
                  self._run_fused_pipelined if self.fused_mlp64 and cfg.overlap_allreduce else self._run_fused_multi)
        # (learn_var: `var` is not read -- the variance is the state's, on the device -- and must not cost a synchronisation here)
        run = runner(plan, batch, None if self.learn_var else float(var) if self.fused else var, V0, r0)
        self.stats = self._summarise(run, plan, flat_before)
        self.loss_history = run.losses   # per-epoch (actor, critic) loss, ppo.py:396-397; NaN rows behind an early stop
        last = (run.k - 1) // run.K      # the last epoch a step of which ran
        self.last_losses = (run.losses[last, 0].detach(), run.losses[last, 1].detach()) if run.k else (zero, zero)
        return self.stats
