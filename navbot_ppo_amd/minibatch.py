"""Which samples a minibatch holds (PPOConfig.minibatch_size / minibatch_shuffle): the host mirror of navppo_shuffle_batch's
permutation, and the key and counter an updater draws its permutations with."""
import torch

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _philox4x32_10(ctr, key):
    """Philox4x32-10 of the kernels (csrc/mlp64_policy.h: philox10) on Python integers."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def batch_permutation(n, key, counter):
    """The permutation pi of navppo_shuffle_batch (include/navppo.h states it) as an int64 tensor on the CPU: out[i] = in[pi[i]].
    A pure function of (n, key, counter): a 6-round Feistel network on ceil(log2 n) bits whose halves trade places and widths every
    round, cycle-walked into [0, n); the round function is two of Philox's multiply-mix rounds, the round keys a Weyl sequence from
    Philox4x32-10 over (counter, n) keyed by `key`.  The kernel matches it exactly (tests/test_gpu_minibatch.py)."""
    import numpy as np
    n, key, counter = int(n), int(key) & _M64, int(counter) & _M64
    if not 1 <= n < 1 << 31:
        raise ValueError(f"batch_permutation: n = {n} outside [1, 2^31)")
    b = (n - 1).bit_length()
    a = b // 2
    c = b - a
    o = _philox4x32_10((counter & _M32, counter >> 32, n, 0x73687566), (key & _M32, key >> 32))
    u64 = np.uint64
    m32, s32 = u64(_M32), u64(32)

    def network(x):
        wl, wr, k0, k1 = a, c, o[0], o[1]
        for _ in range(6):
            left, r = x >> u64(wr), x & u64((1 << wr) - 1)
            p = u64(_PHILOX_M0) * ((r + u64(k0)) & m32)
            t = (p >> s32) ^ (p & m32) ^ u64(k1)
            q = u64(_PHILOX_M1) * t
            f = (q >> s32) ^ (q & m32)
            x = (r << u64(wl)) | (left ^ (f & u64((1 << wl) - 1)))
            wl, wr = wr, wl
            k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
        return x

    x = network(np.arange(n, dtype=u64))
    while True:   # cycle walking: the network is a bijection of [0, 2^b), so every walk from an index < n comes back below n
        walk = np.nonzero(x >= u64(n))[0]
        if walk.size == 0:
            break
        x[walk] = network(x[walk])
    return torch.from_numpy(x.astype(np.int64))


def minibatch_key(seed, rank=0):
    """`key` of an updater's permutations: PPOConfig.seed mixed with the global rank (every rank shuffles its own shard its own way)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + 0x6D6273 + int(rank) * 0xD1B54A32D192ED03) & _M64


def minibatch_counter(update_index, epoch_index):
    """`counter` of a permutation: (update index, epoch index) -- no two epochs of a run share one."""
    return ((int(update_index) & _M32) << 32) | (int(epoch_index) & _M32)
