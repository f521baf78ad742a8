"""The action-noise contract on the CPU: tests/_noise.py (the executable form of the stream every sampling kernel draws from,
mlp64::policy_noise) and the oracle's orc_philox4x32_10 (the reference behind the goal and LiDAR streams) against the published
Random123 known-answer vectors and against each other; the edges of the uniform mappings; and the arithmetic by which
tests/test_gpu_action_noise.py recovers a kernel's draws from its actions."""
import numpy as np
import pytest

import _noise
from oracle import navsim_oracle as O

# Random123 (kat_vectors, philox4x32 with 10 rounds): counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _ref(ctr, key):
    return tuple(int(w) for w in _noise.philox4x32_10(ctr, key))


def _orc(ctr, key):
    return tuple(int(w) for w in O.philox4x32_10(ctr, key))


@pytest.mark.parametrize("impl", [_ref, _orc], ids=["numpy", "oracle"])
@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(impl, ctr, key, want):
    assert impl(ctr, key) == want


def test_philox_known_answers_need_all_ten_rounds():
    """The vectors do discriminate: nine rounds give other words."""
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in _noise.philox4x32_10(ctr, key, rounds=9)) != want


def test_numpy_philox_agrees_with_the_oracle():
    g = np.random.default_rng(20240611)
    w = g.integers(0, 1 << 32, size=(4096, 6), dtype=np.uint64)
    w[:64] &= np.uint64(0xFFFF0000)   # words with zero halves and saturated words: the carries of the 32 x 32 products
    w[64:128] |= np.uint64(0xFFFF0000)
    got = np.stack(_noise.philox4x32_10(tuple(w[:, i] for i in range(4)), (w[:, 4], w[:, 5])), 1)
    want = np.stack([O.philox4x32_10(r[:4], r[4:]) for r in w]).astype(np.uint64)
    np.testing.assert_array_equal(got, want)


def test_uniform_mapping_edges():
    u1, u2 = _noise.uniforms(np.array([0xFFFFFFFF, 0, 0xFFFFFF00, 0xFF]), np.array([0xFFFFFFFF, 0, 0xFFFFFF00, 0xFF]))
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    # r0 = 0xffffffff: u1 = 1, the radius and both draws are 0 whatever the angle
    assert u1[0] == 1.0 and u1[2] == 1.0
    rad, e0, e1 = _noise.box_muller(u1, u2)
    assert rad[0] == 0.0 and e0[0] == 0.0 and e1[0] == 0.0
    # r0 = 0 (and every r0 < 256): u1 = 2^-24, never 0: the radius is finite, and it is the largest one
    assert u1[1] == np.float32(2.0 ** -24) and u1[3] == np.float32(2.0 ** -24)
    assert np.isfinite(rad).all() and rad.max() == rad[1] and 5.768 < rad[1] <= 5.7683
    # u2 < 1 always: its largest value is 1 - 2^-24, and the float32 angle stays below float32(2 pi)
    assert u2[0] == np.float32(1.0 - 2.0 ** -24) and u2[1] == 0.0 and (u2 < 1.0).all()
    assert (_noise.TWO_PI_F32 * u2).astype(np.float32).max() <= _noise.TWO_PI_F32


def test_action_noise_layout():
    """The counter and key layout as words: gid fills counter words 0 and 1, step is taken mod 2^32, the seed fills the key."""
    gid, seed, step = (0x12345678 << 32) | 0x9ABCDEF0, (0x0BADF00D << 32) | 0xDEADBEEF, (1 << 32) + 77
    r, u1, u2, e0, e1 = _noise.action_noise(seed, [gid], step)
    want = _noise.philox4x32_10((0x9ABCDEF0, 0x12345678, 77, 0x61637473), (0xDEADBEEF, 0x0BADF00D))
    assert [int(w[0]) for w in r] == [int(w) for w in want]
    assert [int(w[0]) for w in r] == [int(w) for w in O.philox4x32_10((0x9ABCDEF0, 0x12345678, 77, 0x61637473), (0xDEADBEEF, 0x0BADF00D))]
    # the carry of env_id_base + i into counter word 1
    r2 = _noise.action_noise(9, [(1 << 32) - 1, 1 << 32], 5)[0]
    assert [int(w[0]) for w in r2] == [int(w) for w in _noise.philox4x32_10((0xFFFFFFFF, 0, 5, 0x61637473), (9, 0))]
    assert [int(w[1]) for w in r2] == [int(w) for w in _noise.philox4x32_10((0, 1, 5, 0x61637473), (9, 0))]


def test_recovery_of_the_draws_from_the_actions():
    """What the GPU tests do with a zero actor and var = 2^-8, on the float32 emulation of the kernel's formula over 2^20 draws:
    a1 = e1 / 16 gives e1 back bit for bit, a0 = float32(0.5 + e0 / 16) gives e0 back within 2^-21; the float32 formula with
    correctly rounded library functions stays within 2^-22 max(1, rad) of the float64 reference (the GPU bound is 4 x that);
    and the sample is standard normal."""
    f = np.float32
    _, u1, u2, e0, e1 = _noise.action_noise(9, np.arange(1 << 20), 5)
    rad = _noise.rad_of(u1)
    g0, g1 = _noise.box_muller_f32(u1, u2)
    scale = np.maximum(1.0, rad)
    emu = max(float((np.abs(g0 - e0) / scale).max()), float((np.abs(g1 - e1) / scale).max()))
    print(f"float32 emulation vs float64 reference / max(1, rad): {emu:.3e}")
    assert emu <= 2.0 ** -22
    sd = f(2.0 ** -4)
    for g in (g0, g1):
        a_mid = (f(0.5) + sd * g).astype(f)          # fmaf(sd, e, 0.5): sd e is exact, one rounding
        a_zero = (sd * g).astype(f)                   # fmaf(sd, e, 0)
        assert (a_mid > 0.0).all() and (a_mid < 1.0).all() and (np.abs(a_zero) < 1.0).all()   # nothing clamps
        err = np.abs(_noise.recover_half(a_mid) - g.astype(np.float64)).max()
        print(f"recovery error of the 0.5 leg: {err:.3e}")
        assert err <= 2.0 ** -21
        assert np.array_equal(_noise.recover_exact(a_zero).astype(f), g) and np.array_equal(_noise.recover_exact(a_zero), g.astype(np.float64))
    e = np.stack([e0, e1], 1)
    # moments of 2^20 independent standard normals: every statistic below has a standard error of at most 2^-10; 0.005 is 5 of them
    print("mean", e.mean(0), "std", e.std(0), "corr", np.corrcoef(e0, e1)[0, 1])
    assert np.abs(e.mean(0)).max() < 0.005 and np.abs(e.std(0) - 1).max() < 0.005 and abs(np.corrcoef(e0, e1)[0, 1]) < 0.005
    assert np.abs(e).max() <= 5.7683
