"""Argument checks of the update's entry points (include/navppo.h) without a device: from one valid-looking argument tuple per entry
point, ONE defect at a time -- every such call returns -1 before any launch and navppo_last_error() starts with the name of the entry
point that was called.  Every call here carries a defect: the pointers are host memory and must never reach a kernel."""
import ctypes as C

import pytest

from navbot_ppo_amd import _native

# (argument, role) in the order of the prototypes.  Roles: p = a pointer that must not be null; obs / prep / act = such a pointer that
# must also be aligned; the scalars by their names; - = an argument with no defect of its own (clip, the Adam hyper-parameters, stream)
_BATCH = [("act_dev", "act"), ("logp_old_dev", "p"), ("rtg_dev", "p"), ("adv_dev", "p"), ("n_samples", "n"), ("var", "var"), ("clip", "-")]
_ADAM = [("lr", "-"), ("beta1", "-"), ("beta2", "-"), ("eps", "-"), ("step", "step"), ("adam_m_dev", "p"), ("adam_v_dev", "p")]
_OUT = [("grad_dev", "p"), ("stats_dev", "p"), ("workspace_dev", "p")]
_CLIP = [("max_norm", "max_norm"), ("clip_stats_dev", "p")]
_KL = [("kl_limit", "kl_limit"), ("kl_state_dev", "p")]
_STREAM = [("stream", "-")]
_ROWS = {"navppo_mlp64": [("obs_dev", "obs"), ("obs_dim", "obs_dim"), ("obs_f16", "-")],
         "navppo_mlp64_bf16x3": [("prep_dev", "prep"), ("obs_dim", "obs_dim")],
         "navppo_resmlp512": [("obs_dev", "obs"), ("obs_f16", "-")]}


def _entries():
    e = {}
    for fam, rows in _ROWS.items():
        head = [("params_dev", "p")] + rows + _BATCH
        e[fam + "_loss_grad"] = head + _OUT + _STREAM
        if fam != "navppo_resmlp512":
            e[fam + "_loss_grad_net"] = [("net", "net")] + head + _OUT + _STREAM
        e[fam + "_update_epoch"] = head + _ADAM + _OUT + _STREAM
        e[fam + "_update_epoch_clipped"] = head + _ADAM + _OUT + _CLIP + _STREAM
        e[fam + "_update_epoch_kl"] = head + _ADAM + _OUT + _CLIP + _KL + _STREAM
    flat = [("params_dev", "p"), ("grad_dev", "p"), ("adam_m_dev", "p"), ("adam_v_dev", "p"), ("n", "n")]
    hyper = [("lr", "-"), ("beta1", "-"), ("beta2", "-"), ("eps", "-"), ("step", "step")]
    e["navppo_adam_step"] = flat + [("grad_scale", "-")] + hyper + _STREAM
    clipped = flat + [("n_first", "n_first"), ("grad_scale", "-"), ("max_norm", "max_norm")] + hyper + [("clip_stats_dev", "p")]
    e["navppo_adam_step_clipped"] = clipped + _STREAM
    e["navppo_adam_step_kl"] = clipped + _KL + [("kl_dev", "p")] + _STREAM
    return e


ENTRIES = _entries()
_BUF = C.create_string_buffer(1 << 16)
_BASE = (C.addressof(_BUF) + 15) & ~15   # a 16-byte aligned host buffer behind every pointer
_VALID = {"n": 32, "var": 0.6, "clip": 0.2, "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "step": 1, "obs_dim": 16, "obs_f16": 0,
          "net": 0, "max_norm": 0.5, "kl_limit": 0.03, "n_first": 16, "grad_scale": 1.0, "stream": None}
# the words a message must name (besides the entry point in front)
_WORD = {"max_norm": "max_norm", "clip_stats_dev": "clip_stats_dev", "kl_limit": "kl_limit", "kl_state_dev": "kl_state_dev", "obs_dim": "obs_dim",
         "net": "net"}


def _valid(spec):
    return [_BASE if role in ("p", "obs", "prep", "act") else _VALID[role if role != "-" else name] for name, role in spec]


def _defects(spec):
    """(label, index, bad value, word the message must contain or None)"""
    nan = float("nan")
    for i, (name, role) in enumerate(spec):
        if role in ("p", "obs", "prep", "act"):
            yield f"{name} null", i, None, _WORD.get(name)
        if role in ("obs", "prep", "act"):
            yield f"{name} misaligned", i, _BASE + 4, None
        if role == "n":
            yield f"{name} 0", i, 0, None
        if role == "var":
            yield "var 0", i, 0.0, None
            yield "var NaN", i, nan, None
        if role == "step":
            yield "step 0", i, 0, None
        if role == "obs_dim":
            yield "obs_dim 17", i, 17, "obs_dim"
        if role == "net":
            yield "net 2", i, 2, "net"
        if role == "n_first":
            yield "n_first > n", i, 33, None
        if role in ("max_norm", "kl_limit"):
            for bad in (0.0, -1.0, nan):
                yield f"{role} {bad}", i, bad, role


def test_the_matrix_covers_every_update_entry_point_and_agrees_with_the_ctypes_table():
    assert len(ENTRIES) == 5 + 5 + 4 + 3   # mlp64, mlp64_bf16x3, resmlp512 (no per-net form), navppo_adam_step*
    table = {name: args for name, _, args in _native.SYMBOLS}
    for name, spec in ENTRIES.items():
        assert len(table[name]) == len(spec), name
        for (arg, role), ct in zip(spec, table[name]):   # pointers where the table has pointers, integers and floats likewise
            assert (ct is C.c_void_p) == (role in ("p", "obs", "prep", "act") or arg == "stream"), (name, arg)
        assert any(True for _ in _defects(spec))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_defect_is_refused_before_a_launch_under_the_entry_points_own_name(entry):
    L = _native.lib()
    fn, spec = getattr(L, entry), ENTRIES[entry]
    n = 0
    for label, i, bad, word in _defects(spec):
        args = _valid(spec)
        assert args[i] != bad, (entry, label)
        args[i] = bad
        rc = fn(*args)
        msg = L.navppo_last_error().decode()
        print(f"{entry}: {label}: rc {rc}, {msg!r}")
        assert rc == -1, (entry, label, rc)
        assert msg.startswith(entry + ":"), (entry, label, msg)
        if word is not None:
            assert word in msg[len(entry):], (entry, label, msg)
        n += 1
    assert n >= 6, (entry, n)   # (navppo_adam_step: four pointers, n and step; every other entry point has more)
