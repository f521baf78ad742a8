"""The ranks of a run: DistCtx wraps torch.distributed (one process per GPU), SingleProcessCtx stands in where there is none.
Multi-GPU is absent in the reference."""
import os

import torch
import torch.distributed as dist


class SingleProcessCtx:
    """The context of a run without torch.distributed -- what PPOUpdater and PPOTrainer install for ctx=None: one process, rank 0,
    every collective a no-op."""
    world, rank, local_rank, enabled = 1, 0, 0, False

    def all_reduce_sum(self, t):
        return t

    all_reduce_max = all_reduce_sum

    def broadcast(self, t, src=0):
        return t

    def barrier(self):
        pass


def as_ctx(ctx):
    """`ctx` itself, or the single-process context for None"""
    return SingleProcessCtx() if ctx is None else ctx


def global_mean(ctx, total, count, out=None):
    """sum(total_r) / sum(count_r) over the ranks r by ONE 2-float collective -- the global approx_kl = sum(kl_r n_r) / sum(n_r), every
    rank's samples weighing the same.  total: this rank's sum (a 0-dim tensor), count: its samples.  out: a [2] tensor to form the
    quotient in (it stays behind in out[0]); default a new one.  Returns the 0-dim quotient."""
    kg = total.new_empty(2) if out is None else out
    kg[0], kg[1] = total, count
    ctx.all_reduce_sum(kg)
    kg[0] /= kg[1]
    return kg[0]


class DistCtx:
    """torch.distributed wrapper that degrades to a no-op for a single process."""

    def __init__(self, device=None):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # NAVBOT_DIST_FORCE=1: a single rank still creates its process group and sends every collective through the backend --
        # on a one-GPU box this is how the RCCL branch (init with device_id, all-reduces on RCCL's stream, the overlap of the
        # actor's all-reduce with the critic pass, navppo_adam_step's 1/world scale) is executed at all
        self.enabled = self.world > 1 or os.environ.get("NAVBOT_DIST_FORCE") == "1"
        if device is None:
            if torch.cuda.is_available():
                device = torch.device(f"cuda:{self.local_rank % torch.cuda.device_count()}")
            else:
                device = torch.device("cpu")
        self.device = torch.device(device)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        self.backend, self.rccl_version = None, None
        if self.enabled and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            # "nccl" is RCCL on ROCm.  NAVBOT_DIST_BACKEND=gloo lets several ranks share one GPU (tests only:
            # RCCL refuses two ranks on the same device).
            backend = os.environ.get("NAVBOT_DIST_BACKEND") or ("nccl" if self.device.type == "cuda" else "gloo")
            kw = {"device_id": self.device} if backend == "nccl" else {}
            dist.init_process_group(backend=backend, rank=self.rank, world_size=self.world, **kw)
        if self.enabled:
            # a launcher may have created the group itself (backend=None or "cpu:gloo,cuda:nccl"): ask for the CUDA backend
            try:
                self.backend = dist.get_backend_config().get_device_backend_map().get("cuda", dist.get_backend())
            except Exception:
                self.backend = dist.get_backend()
            if self.device.type == "cuda" and not os.environ.get("NAVBOT_DIST_BACKEND") and "nccl" not in str(self.backend):
                import warnings
                warnings.warn(f"GPU ranks should talk RCCL (torch backend 'nccl'); the process group uses {self.backend!r}")
            if "nccl" in str(self.backend):
                self.backend = "nccl"
                try:
                    self.rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())
                except Exception:
                    self.rccl_version = "unknown"
                if self.rank == 0:   # one line per job: a scaling run shows how many ranks RCCL really connected
                    print(f"[navbot_ppo_amd] RCCL {self.rccl_version}: {dist.get_world_size()} ranks, one per GPU, "
                          f"flat-gradient all-reduce per epoch", flush=True)

    def all_reduce_sum(self, t):
        if self.enabled:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t

    def all_reduce_max(self, t):
        if self.enabled:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t

    def broadcast(self, t, src=0):
        if self.enabled:
            dist.broadcast(t, src=src)
        return t

    def barrier(self):
        if self.enabled:
            dist.barrier()

    def shard(self, n_total):
        """Contiguous env-id shard [lo, hi) of this rank."""
        per = n_total // self.world
        if per * self.world != n_total:
            raise ValueError(f"n_envs {n_total} not divisible by world size {self.world}")
        return self.rank * per, (self.rank + 1) * per
