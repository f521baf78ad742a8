"""The persistent evaluation (navsim_evaluate_mlp64 / navsim_evaluate_resmlp512, evaluate(persistent=True), PPOConfig.eval_every)
as far as it can be checked without a device: a handle cannot be created without one, so this covers the argument checks that run
before anything touches the GPU, the configuration surface and the absence of a CPU fallback."""
import pytest
import torch

from navbot_ppo_amd import _native, evaluate as ev, main, nets, ppo


@pytest.mark.parametrize("name", ["navsim_evaluate_mlp64", "navsim_evaluate_resmlp512"])
def test_null_handle_is_an_argument_error(name):
    L = _native.lib()
    rc = getattr(L, name)(None, None, None, 1, 1, None, None, None, None, None, None, None)
    assert rc == -1   # NAVSIM_E_ARG
    msg = L.navsim_last_error().decode()
    assert name in msg and "handle" in msg


def test_entry_points_are_bound():
    names = [s[0] for s in _native.SYMBOLS]
    assert "navsim_evaluate_mlp64" in names and "navsim_evaluate_resmlp512" in names
    assert _native.NAVSIM_ABI_VERSION == 6   # new symbols only


def test_config_defaults_and_flags():
    cfg = ppo.PPOConfig()
    assert cfg.eval_every == 0 and cfg.eval_episodes == 100
    a = main.get_args(["--eval_every", "5", "--eval_persistent"])
    assert a.eval_every == 5 and a.eval_persistent is True
    a = main.get_args([])
    assert a.eval_every == 0 and a.eval_persistent is False


def test_flat_actor_params_layout():
    torch.manual_seed(0)
    a64, _ = nets.make_policy("mlp64x2", 16)
    assert ev.persistent_policy(a64)[1].numel() == 64 * 16 + 4354
    a512, _ = nets.make_policy("resmlp512", 16)
    policy, flat = ev.persistent_policy(a512)
    assert policy == "resmlp512" and flat.numel() == 50290
    assert torch.equal(flat[:512 * 16], a512.rb1.fc1.weight.detach().reshape(-1))


def test_persistent_refuses_what_has_no_kernel():
    """no silent fallback to the stepping loop: an actor or a beam count without an evaluation kernel is a ValueError that says why"""
    with pytest.raises(ValueError, match="no evaluation kernel"):
        ev.evaluate(torch.nn.Linear(16, 2), num_episodes=4, persistent=True, log=None)
    a42, _ = nets.make_policy("resmlp512", 42)
    with pytest.raises(ValueError, match="no evaluation kernel"):
        ev.evaluate(a42, num_episodes=4, persistent=True, log=None)


def test_persistent_has_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (a machine with a GPU checks the same refusal)
    actor, _ = nets.make_policy("mlp64x2", 16)
    with pytest.raises(_native.NavsimError):
        ev.evaluate(actor, num_episodes=4, max_timesteps_per_episode=10, persistent=True, log=None)
