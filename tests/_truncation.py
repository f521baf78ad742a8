"""Test helper: synthetic [T, N] batches for the truncation-aware return scan (tests of PPOConfig.bootstrap_truncated, CPU and GPU).

An episode end is one of three kinds -- a collision (done), an arrival (arrive), a time-out (ended alone) -- and only the last one
bootstraps.  `truncated_batch` draws 2 % episode ends, a third of each kind, adds rows that carry done or arrive WITHOUT ended (what
respawn_on_arrive and handles without auto_reset write: they must change nothing) and, with forced=True, the rows at which the
T-split kernel can go wrong, each family on columns of its own (column j takes family j % 7, so 16 columns hold all of them)."""
import numpy as np

CHUNK, SUPER = 32, 512   # rows per chunk and per super-chunk of the T-split scan, counted from the batch end


def truncated_batch(T, N, seed=0, forced=False, v_std=100.0):
    """(rew, ended, done, arrive, value [T, N], last_value [N]): float32 rewards and values (V ~ N(0, v_std)), uint8 flags."""
    g = np.random.default_rng(seed + 1000 * T + N)
    rew = (500.0 * g.uniform(-0.05, 0.05, (T, N))).astype(np.float32)
    ended = g.random((T, N)) < 0.02
    kind = g.integers(0, 3, (T, N))   # 0 = collision, 1 = arrival, 2 = time-out
    done, arrive = ended & (kind == 0), ended & (kind == 1)
    rew[done], rew[arrive] = -100.0, 120.0
    arrive |= ~ended & (g.random((T, N)) < 0.01)   # flags without an episode end
    done |= ~ended & (g.random((T, N)) < 0.01)
    value = g.normal(0.0, v_std, (T, N)).astype(np.float32)
    last_value = g.normal(0.0, v_std, N).astype(np.float32)

    def put(t, n, k):
        """row t of column n: 2 = a time-out, 0 = a collision, 1 = an arrival, 3 / 4 = arrive / done without an episode end"""
        if not 0 <= t < T:
            return
        ended[t, n], done[t, n], arrive[t, n] = k <= 2, k in (0, 4), k in (1, 3)

    if forced:
        for n, fam in ((n, fam) for n in range(N) for fam in ([n % 7] if N >= 7 else [5, 6, 1, 2, 3, 4, 0])):   # (few columns: each takes all)
            if fam == 0:     # the first and the last row of the batch
                put(0, n, 2), put(T - 1, n, 2)
            elif fam == 1:   # both sides of every chunk edge
                for t in range(T - CHUNK, -1, -CHUNK):
                    put(t, n, 2), put(t - 1, n, 2)
            elif fam == 2:   # both sides of the super-chunk edge
                put(T - SUPER, n, 2), put(T - SUPER - 1, n, 2)
            elif fam == 3:   # two time-outs inside one chunk (the last one of the batch; with a ragged T also the first)
                put(T - 5, n, 2), put(T - 9, n, 2), put(1, n, 2), put(3, n, 2)
            elif fam == 4:   # a time-out on the row before a collision
                tc = min(T - 1, T // 2 + 1)
                put(tc, n, 0), put(tc - 1, n, 2)
            elif fam == 5:   # arrive without ended, beside a time-out
                put(T // 3, n, 3), put(T // 3 + 1, n, 2)
            else:            # done without ended, and an arrival that does end the episode
                put(T // 3, n, 4), put(T // 3 + 2, n, 1)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    return rew, u8(ended), u8(done), u8(arrive), value, last_value


def truncated_rows(ended, done, arrive):
    """the time-outs: ended, neither done nor arrive (navppo_episode_sums' definition)"""
    return (ended != 0) & (done == 0) & (arrive == 0)
