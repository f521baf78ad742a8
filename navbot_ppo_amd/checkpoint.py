"""Checkpoint files: the reference's two state_dicts (ppo.py:452-457 file naming, main.py:52-89 loading; the keys match the reference's
nets for policy resmlp512) and the sidecars PPOTrainer writes beside them -- <kind>_<tag>.pth, one per option with state of its own."""
import os
import warnings

import torch


def sidecar_path(kind, actor_path):
    """<kind>_<tag>.pth beside actor_<tag>.pth"""
    d, base = os.path.split(actor_path)
    return os.path.join(d, kind + "_" + (base[len("actor_"):] if base.startswith("actor_") else base))


def save_sidecar(kind, actor_path, payload):
    torch.save(payload, sidecar_path(kind, actor_path))


def load_sidecar(kind, actor_path, missing):
    """What was stored in the `kind` file beside the actor's, or -- no such file -- None after ONE warning line: `missing` with the
    file's path in its {}."""
    path = sidecar_path(kind, actor_path)
    if os.path.exists(path):
        return torch.load(path, map_location="cpu")
    warnings.warn(missing.format(path))
    return None


def save_nets(dir, tag, actor, critic):
    """actor_<tag> and critic_<tag> in dir (created): the state_dicts, on the host.  Returns the two paths."""
    os.makedirs(dir, exist_ok=True)
    pa, pc = os.path.join(dir, "actor_" + tag), os.path.join(dir, "critic_" + tag)
    for net, path in ((actor, pa), (critic, pc)):
        torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, path)
    return pa, pc


def load_nets(actor, critic, actor_path, critic_path):
    """state_dicts only (optimiser state and covariance are not part of a checkpoint), copied in place: parameters stay views of the
    flat buffer.  KeyError if a file lacks a key of its net."""
    sa = torch.load(actor_path, map_location="cpu")
    sc = torch.load(critic_path, map_location="cpu")
    with torch.no_grad():
        for mod, sd in ((actor, sa), (critic, sc)):
            own = mod.state_dict()
            missing = set(own) - set(sd)
            if missing:
                raise KeyError(f"checkpoint lacks keys {sorted(missing)}")
            for k, v in own.items():
                v.copy_(sd[k])
