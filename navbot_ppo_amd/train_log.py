"""What PPOTrainer writes about a run, from figures that are already on the host: the progress line of learn(), the reference's
TensorBoard scalars (ppo.py:892-939; also one JSON object per iteration in scalars.jsonl), the per-episode CSV (ppo.py:159-163,739-746),
the gradient check with its grad_diagnostics.txt (ppo.py:356-379, 414-416).  Functions of their inputs; RunLog holds what persists
across iterations."""
import csv
import json
import math
import os
import time

import torch

from .tb_writer import SummaryWriter
from .updater import LOG_2PI

EPISODE_CSV_HEADER = ["episode", "timestep", "success", "collision", "timeout", "length", "return", "path_length", "time"]
EVAL_HISTORY_HEADER = ["iteration", "timesteps", "episodes", "success_rate", "collision_rate", "timeout_rate", "mean_length",
                       "mean_return", "mean_path_length"]


def join_sections(parts):
    """The iteration's read-back, put together: [(name, 1-D device tensor), ...] -> (one tensor, [(name, length), ...]).  The parts
    are concatenated once; a single part is returned as it is, nothing launched."""
    return (parts[0][1] if len(parts) == 1 else torch.cat([t for _, t in parts])), [(name, t.numel()) for name, t in parts]


def split_sections(m, sections):
    """... and taken apart on the host, by name.  Several sections: ONE read-back of m, cut into a list of figures per section.  A
    single section: m itself, untouched, under its name (whoever takes it reads it)."""
    if len(sections) == 1:
        return {sections[0][0]: m}
    flat, out, lo = m.tolist(), {}, 0
    for name, n in sections:
        out[name], lo = flat[lo:lo + n], lo + n
    return out


def append_rows(path, header, rows):
    """Appends rows to the CSV at path; a file that does not exist yet (its directory is created) gets the header first."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    new = not os.path.exists(path)
    with open(path, "a", newline="") as f:
        w = csv.writer(f)
        if new:
            w.writerow(header)
        w.writerows(rows)
    return path


def append_json_line(path, record):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(record) + "\n")


def tb_scalars(lg, cfg):
    """The scalars the reference hands to SummaryWriter.add_scalar once per iteration, under its tag names (ppo.py:892-918), from the
    figures lg of one iteration (PPOTrainer.logger); an option's tags are there when its figures are."""
    ep = max(lg.get("episodes", 0), 1)
    n_ep = cfg.n_updates_per_iteration
    var = float(lg.get("var", cfg.init_var))
    sec_per_step = float(lg.get("rollout_time", 0.0)) / max(cfg.rollout_len, 1)
    return {"train/success_rate": lg.get("success_rate"), "train/collision_rate": lg.get("collisions", 0) / ep,
            "train/timeout_rate": lg.get("timeouts", 0) / ep, "train/mean_return": lg.get("avg_ep_rews"),
            "train/mean_ep_length": lg.get("avg_ep_lens"), "train/mean_ep_time": lg.get("avg_ep_lens", 0.0) * sec_per_step,
            "loss/actor": lg.get("actor_loss"), "loss/critic": lg.get("critic_loss"), "train/timesteps": lg.get("t_so_far"),
            "time/rollout": lg.get("rollout_time"), "time/update": lg.get("update_time"), "time/iteration": lg.get("iter_time"),
            "perf/steps_per_sec": lg.get("steps_per_sec"), "perf/actor_grad_steps": n_ep, "perf/critic_grad_steps": n_ep,
            "ppo/approx_kl": lg.get("approx_kl"),
            "ppo/entropy": 1.0 + LOG_2PI + math.log(max(var, 1e-30)),   # MultivariateNormal(mean, var I).entropy(), 2-D
            "ppo/clip_frac": lg.get("clip_frac"), "ppo/actor_grad_norm": lg.get("actor_grad_norm"),
            "ppo/critic_grad_norm": lg.get("critic_grad_norm"), "ppo/actor_param_delta": lg.get("actor_param_delta"),
            "ppo/critic_param_delta": lg.get("critic_param_delta"),
            "ppo/grad_clip_frac_actor": lg.get("grad_clip_frac_actor"), "ppo/grad_clip_frac_critic": lg.get("grad_clip_frac_critic"),
            "ppo/skipped_steps_actor": lg.get("skipped_steps_actor"), "ppo/skipped_steps_critic": lg.get("skipped_steps_critic"),
            "ppo/kl_stop_epoch": lg.get("kl_stop_epoch"), "ppo/kl_stopped": lg.get("kl_stopped"),   # (target_kl set)
            **({"ppo/kl_stop_step": lg["kl_stop_step"]} if "kl_stop_step" in lg else {}),           # (target_kl and minibatches)
            **({"ppo/" + k: lg[k] for k in ("lr", "lr_ups", "lr_downs") if k in lg}),               # (lr_schedule set)
            **({"ppo/" + k: lg[k] for k in ("reward_scale", "ret_rms_mean", "ret_rms_std", "explained_variance")}
               if "reward_scale" in lg else {}),                                                    # (norm_reward)
            **({"ppo/bootstrapped_frac": lg["bootstrapped_frac"]} if "bootstrapped_frac" in lg else {}),   # (bootstrap_truncated)
            **({"ppo/" + k: lg[k] for k in ("var", "std", "var_grad", "var_steps_skipped")} if "var_grad" in lg else {}),   # (learn_var)
            **({"env/scan_pool": lg["scan_pool"]} if "scan_pool" in lg else {}),                    # (sector LiDAR on)
            **({"scenarios/train_success_min": lg["train_scenario_success_min"],
                "scenarios/train_success_mean": lg["train_scenario_success_mean"]}
               if "train_scenario_success_min" in lg else {}),                                      # (scenario_stats / _priority)
            **({"eval/success_rate": lg["eval_success"], "eval/collision_rate": lg["eval_collision"],
                "eval/timeout_rate": lg["eval_timeout"], "eval/mean_return": lg["eval_return"],
                "eval/mean_ep_length": lg["eval_length"], "time/eval": lg["eval_time"]} if "eval_success" in lg else {})}


def progress_line(lg):
    """The line learn() logs per iteration; an option's part is there when its figures are."""
    return (f"[iter {lg['iteration']:4d}] t={lg['t_so_far']:>10d} mean_ep_rew={lg['avg_ep_rews']:8.2f} "
            f"succ={lg['success_rate']:.3f} ep_len={lg['avg_ep_lens']:6.1f} a_loss={lg['actor_loss']:.4f} "
            f"c_loss={lg['critic_loss']:.2f} kl={lg['approx_kl']:.4f} steps/s={lg['steps_per_sec']:.0f} "
            f"(rollout {lg['rollout_time']:.3f}s update {lg['update_time']:.3f}s)"
            + (f" kl_stop_epoch={lg['kl_stop_epoch']} kl_stopped={lg['kl_stopped']}" if "kl_stop_epoch" in lg else "")
            + (f" kl_stop_step={lg['kl_stop_step']}" if "kl_stop_step" in lg else "")
            + (f" lr={lg['lr']:.3e}" if "lr" in lg else "")
            + (f" lr_ups={lg['lr_ups']} lr_downs={lg['lr_downs']}" if "lr_ups" in lg else "")
            + (f" bootstrapped_frac={lg['bootstrapped_frac']:.4f}" if "bootstrapped_frac" in lg else "")
            + (f" var={lg['var']:.4f} std={lg['std']:.4f} entropy={lg['entropy']:.4f} var_grad={lg['var_grad']:.3e} "
               f"var_steps_skipped={lg['var_steps_skipped']}" if "var_grad" in lg else "")
            + (f" scan_pool={lg['scan_pool']}" if "scan_pool" in lg else "")
            + (f" train scenarios: min={lg['train_scenario_success_min']:.3f} mean={lg['train_scenario_success_mean']:.3f}"
               if "train_scenario_success_min" in lg else "")
            + (f" eval: succ={lg['eval_success']:.3f} coll={lg['eval_collision']:.3f} tmo={lg['eval_timeout']:.3f} "
               f"ret={lg['eval_return']:.2f} len={lg['eval_length']:.1f} ({lg['eval_time']:.3f}s)"
               if "eval_success" in lg else "")
            + (f" scenarios: min={lg['eval_scenario_success_min']:.3f} mean={lg['eval_scenario_success_mean']:.3f}"
               if "eval_scenario_success_min" in lg else ""))


def finished_episodes(ended_buf, cap=None):
    """(t_idx, n_idx) of the episodes that ended in the rollout, in (step, env) order, the first `cap` of them (None: all)"""
    t_idx, n_idx = torch.nonzero(ended_buf.bool(), as_tuple=True)
    return (t_idx, n_idx) if cap is None else (t_idx[:cap], n_idx[:cap])


def grad_diagnostics_block(net, grad_norm, loss, skipped, n_updates, iteration, adv_stats, clip_frac):
    """One block of grad_diagnostics.txt: a net whose update went wrong in an iteration; adv_stats = (mean, std, min, max)"""
    a = adv_stats
    return (f"\n[{net.upper()} GRAD ISSUE] Iteration {iteration}\n"
            f"  Net: {net}\n"
            f"  {net.capitalize()} grad norm: {grad_norm}\n"
            f"  {net.capitalize()} loss: {loss}\n"
            f"  Skipped steps: {skipped} of {n_updates}\n"
            f"  Advantage stats: mean={a[0]:.4f}, std={a[1]:.4f}, min={a[2]:.4f}, max={a[3]:.4f}\n"
            f"  Clip fraction: {clip_frac:.4f}\n")


def grad_guard(stats, cfg, iteration, adv, writes_files, log=print):
    """A per-net mean gradient norm that is <= 0 or not finite, a loss that is not finite, or a skipped step (max_grad_norm):
    the reference's warning line, and a block in <output_dir>/grad_diagnostics.txt.  No launch and no sync unless it triggers
    (then a few reductions over the advantages adv for the file); it reports only -- what happens to the weights is decided by
    PPOConfig.max_grad_norm inside the update -- and never raises.  Returns the nets that triggered."""
    if cfg.n_updates_per_iteration < 1:
        return []
    hit = []
    for net in ("actor", "critic"):
        gn, loss, sk = stats.get(net + "_grad_norm", 0.0), stats.get(net + "_loss", 0.0), stats.get("skipped_steps_" + net, 0)
        if gn <= 0 or not math.isfinite(gn) or not math.isfinite(loss) or sk > 0:
            hit.append((net, gn, loss, sk))
    if not hit or not writes_files:
        return [h[0] for h in hit]
    try:
        for net, gn, loss, sk in hit:
            if log:
                log(f"[WARNING] {net.capitalize()} grad norm invalid: {gn:.6f} at iteration {iteration}. Check grad_diagnostics.txt"
                    + (f" ({sk} of {cfg.n_updates_per_iteration} steps skipped)" if sk else ""), flush=True)
        if cfg.output_dir:
            a = [float("nan")] * 4 if adv is None else [float(x) for x in (adv.mean(), adv.std(), adv.min(), adv.max())]
            os.makedirs(cfg.output_dir, exist_ok=True)
            with open(os.path.join(cfg.output_dir, "grad_diagnostics.txt"), "a") as f:
                for net, gn, loss, sk in hit:
                    f.write(grad_diagnostics_block(net, gn, loss, sk, cfg.n_updates_per_iteration, iteration, a, stats.get("clip_frac", 0.0)))
    except Exception as e:   # a diagnostics file must never end a run
        try:
            print(f"[WARNING] grad diagnostics not written: {e}", flush=True)
        except Exception:
            pass
    return [h[0] for h in hit]


class RunLog:
    """The files of one run under <output_dir>/<method_name>, and what they carry from one iteration to the next: the running
    episode count of the CSV, the TensorBoard writer (opened at the first write) with the steps of its two per-point series, and
    what the last TensorBoard write cost (logged as time/log by the next one)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.log_dir = os.path.join(cfg.output_dir, cfg.method_name, "logs")
        self.tb_dir = os.path.join(cfg.output_dir, cfg.method_name, "tb")   # ppo.py:66
        self.episode_count = 0
        self.tb, self.tb_loss_steps, self.tb_ep_steps = None, 0, 0
        self.last_log_time = 0.0

    def path(self, suffix):
        """<log_dir>/<method_name>_<suffix>"""
        return os.path.join(self.log_dir, f"{self.cfg.method_name}_{suffix}")

    def write_episode_csv(self, ended, done, arrive, ep_length, ep_return, ep_path, env_steps, rollout_time, max_rows=None):
        """Appends the episodes finished in the last rollout ([T, N] buffers; env_steps counts it), in (step, env) order
        (ppo.py:739-746).  path_length is the simulator's per-episode accumulator (ppo.py:533-537 semantics: the final step's
        displacement is not part of it); time is the episode's share of the rollout wall clock, length x (rollout_time / T): the
        envs advance in lock step, so an episode of L steps occupied L / T of the rollout."""
        T, N = ended.shape
        t_idx, n_idx = finished_episodes(ended, max_rows)
        d, a, ln, rt, pl = (b[t_idx, n_idx].cpu().numpy() for b in (done, arrive, ep_length, ep_return, ep_path))
        tt = t_idx.cpu().numpy()
        sec_per_step = float(rollout_time) / max(T, 1)
        base = self.episode_count
        rows = [[base + k, env_steps - (T - int(tt[k]) - 1) * N, int(a[k]), int(d[k] and not a[k]), int(not d[k] and not a[k]),  # ppo.py:558-560
                 int(ln[k]), float(rt[k]), float(pl[k]), float(ln[k]) * sec_per_step] for k in range(len(tt))]
        self.episode_count = base + len(tt)
        return append_rows(self.path("train_episodes.csv"), EPISODE_CSV_HEADER, rows)

    def write_tensorboard(self, iteration, lg, loss_history, update_stats, ended, ep_return, ep_length):
        """The reference's TensorBoard stream (ppo.py:892-939): per-iteration scalars at step `iteration`, the per-epoch
        Actor_loss/train and Critic_loss/train series, Episode_Rewards/train (return / length of every finished episode,
        ppo.py:586, capped per iteration like the CSV) and avg_ep_rews/train."""
        if self.tb is None:
            self.tb = SummaryWriter(self.tb_dir)
        t0 = time.time()
        recs = [(k, float(v), iteration) for k, v in tb_scalars(lg, self.cfg).items() if v is not None]
        hist = loss_history.detach().cpu().numpy()
        hist = hist[:int(update_stats.get("kl_stop_epoch", hist.shape[0])) + int(update_stats.get("kl_stopped", 0))]   # (rows of epochs that ran)
        for k in range(hist.shape[0]):
            recs.append(("Actor_loss/train", float(hist[k, 0]), self.tb_loss_steps + k))
            recs.append(("Critic_loss/train", float(hist[k, 1]), self.tb_loss_steps + k))
        self.tb_loss_steps += hist.shape[0]
        cap = int(self.cfg.tb_episode_rows or 0)
        if cap:   # own cap, independent of the CSV's: with 4096 envs an iteration finishes ~1e5 episodes
            t_idx, n_idx = finished_episodes(ended, cap)
            per_step = (ep_return[t_idx, n_idx] / ep_length[t_idx, n_idx].clamp(min=1)).cpu().numpy()
            recs.extend(("Episode_Rewards/train", float(r), self.tb_ep_steps + k) for k, r in enumerate(per_step))
            self.tb_ep_steps += len(per_step)
        recs.append(("avg_ep_rews/train", float(lg.get("avg_ep_rews", 0.0)), iteration))
        recs.append(("time/log", float(self.last_log_time), iteration))   # the previous iteration's logging cost
        self.tb.add_scalars(recs)   # one TFRecord per point; CRCs vectorised over the records (tb_writer._masked_crc_many)
        self.tb.flush()
        self.last_log_time = time.time() - t0
