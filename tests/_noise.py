"""The action-noise stream of the sampling kernels (mlp64::policy_noise, csrc/mlp64_policy.h) as an independent numpy reference.

Written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11 -- Philox4x32
with ten rounds), not by calling the oracle or the library:
    counter = (gid & 0xffffffff, gid >> 32, step mod 2^32, 0x61637473 "acts"),  key = (seed & 0xffffffff, seed >> 32)
    u1 = (float32(r0 >> 8) + 1) 2^-24 in (0, 1],  u2 = float32(r1 >> 8) 2^-24 in [0, 1)
    ang = float32(float32(2 pi) u2)            -- the float32 rounding of the angle belongs to the contract
    rad = sqrt(-2 ln u1),  e0 = rad cos(ang),  e1 = rad sin(ang)              (float64 here; the kernels evaluate them in float32)
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key schedule's Weyl increments (golden ratio, sqrt(3) - 1)
MASK = 0xFFFFFFFF
DOMAIN = 0x61637473                       # counter word 3 of the action stream
TWO_PI_F32 = np.float32(6.283185307179586)


def philox4x32_10(ctr, key, rounds=10):
    """ctr: four, key: two array-likes of 32-bit words (broadcast against each other).  Returns the four output words as uint64 arrays
    holding 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(MASK) for k in key)
    m, s32 = np.uint64(MASK), np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0              # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def uniforms(r0, r1):
    """The two float32 uniforms of a draw: u1 in (0, 1], u2 in [0, 1) (24 bits each, so every step below is exact in float32)."""
    r0, r1 = np.asarray(r0, dtype=np.uint64), np.asarray(r1, dtype=np.uint64)
    u1 = ((r0 >> np.uint64(8)).astype(np.float32) + np.float32(1.0)) * np.float32(2.0 ** -24)
    u2 = (r1 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u1, u2


def box_muller(u1, u2):
    """float64 Box-Muller on the float32 uniforms with the float32 angle.  Returns (rad, e0, e1)."""
    ang = (TWO_PI_F32 * np.asarray(u2, dtype=np.float32)).astype(np.float32).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(np.asarray(u1, dtype=np.float32).astype(np.float64)))
    return rad, rad * np.cos(ang), rad * np.sin(ang)


def action_noise(seed, gids, step):
    """The draws of the envs with global ids `gids` (Python ints or an integer array, up to 64 bits) at rollout step `step` under the
    64-bit `seed`.  Returns (r, u1, u2, e0, e1): r the four Philox words, u1 / u2 float32, e0 / e1 float64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if isinstance(gids, np.ndarray) and gids.dtype.kind in "iu":
        g = gids.reshape(-1).astype(np.uint64)
    else:   # Python ints beyond 2^63 do not survive a default conversion
        g = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in np.asarray(gids, dtype=object).reshape(-1)], dtype=np.uint64)
    ctr = (g & np.uint64(MASK), g >> np.uint64(32), np.uint64(int(step) & MASK), np.uint64(DOMAIN))
    r = philox4x32_10(ctr, (np.uint64(seed & MASK), np.uint64(seed >> 32)))
    r = tuple(np.broadcast_to(w, g.shape).copy() for w in r)
    u1, u2 = uniforms(r[0], r[1])
    _, e0, e1 = box_muller(u1, u2)
    return r, u1, u2, e0, e1


def rad_of(u1):
    return np.sqrt(-2.0 * np.log(np.asarray(u1, dtype=np.float32).astype(np.float64)))


def box_muller_f32(u1, u2):
    """The kernel's formula emulated in float32 step by step (correctly rounded log / sqrt / sin / cos of the float32 values): what a
    float32 implementation with exact library functions returns.  (e0, e1) as float32."""
    f = np.float32
    u1, u2 = np.asarray(u1, dtype=f), np.asarray(u2, dtype=f)
    lg = np.log(u1.astype(np.float64)).astype(f)
    rad = np.sqrt((f(-2.0) * lg).astype(np.float64)).astype(f)
    ang = (TWO_PI_F32 * u2).astype(f)
    c, s = np.cos(ang.astype(np.float64)).astype(f), np.sin(ang.astype(np.float64)).astype(f)
    return (rad * c).astype(f), (rad * s).astype(f)


def recover_half(a0):
    """e0 from a0 = float32(0.5 + e0 / 16) (zero actor, var = 2^-8): within 2^-21 of e0 (half an ulp of [0.5, 1) times 16)."""
    return 16.0 * (np.asarray(a0, dtype=np.float32).astype(np.float64) - 0.5)


def recover_exact(a):
    """e from a = e / 16 (a mean of exactly 0): the kernel's own float32 draw, bit for bit."""
    return 16.0 * np.asarray(a, dtype=np.float32).astype(np.float64)
