#!/usr/bin/env python3
"""Record the golden vectors of the sector-LiDAR rule from the REFERENCE's own down-sampler (run in the build container only).

    python3 -B tests/golden/generate_golden_pick.py

Imports /root/reference/project_ppo/src/pick_laser.py at run time, calls its Pick(scan, len_batch) on random and crafted scans of
20, 30 and 40 samples (len_batch 2, 3, 4) and stores inputs and outputs as G11_pick.npz next to this script.  No reference source is
copied: the fixture is data.  Crafted rows: ties inside a chunk, readings at the range limits (3.5, 0.12), -inf readings (Gazebo's
below-range value) alone and beside finite ones, a chunk of +inf only."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

sys.path.insert(0, "/root/reference/project_ppo/src")
import pick_laser  # noqa: E402


def scans(k, rng):
    n = 10 * k
    rows = [rng.uniform(0.12, 3.5, n) for _ in range(24)]
    tie = rng.uniform(0.2, 3.0, n)
    tie[:k] = tie[0]                       # a whole chunk of equal readings
    tie[k:2 * k] = np.sort(tie[k:2 * k])
    tie[2 * k] = tie[2 * k + 1]            # two equal readings, the minimum of their chunk or not
    rows.append(tie)
    lim = rng.uniform(0.12, 3.5, n)
    lim[::3] = 3.5
    lim[1::5] = 0.12
    rows.append(lim)
    rows.append(np.full(n, 3.5))
    rows.append(np.full(n, 0.12))
    neg = rng.uniform(0.12, 3.5, n)
    neg[k - 1] = -np.inf                   # last ray of column 0
    neg[3 * k] = -np.inf                   # first ray of column 3
    neg[5 * k:6 * k] = -np.inf             # a whole column
    rows.append(neg)
    inf = rng.uniform(0.12, 3.5, n)
    inf[2 * k:3 * k] = np.inf              # a raw scan before the sanitiser: a column without a return
    inf[4 * k] = np.inf
    rows.append(inf)
    return np.asarray(rows, dtype=np.float32)


def main():
    rng = np.random.default_rng(20261021)
    out = {}
    for k in (2, 3, 4):
        s = scans(k, rng)
        picked = np.asarray([pick_laser.Pick(list(row), k) for row in s], dtype=np.float32)
        assert picked.shape == (s.shape[0], 10)
        out[f"scan_{k}"] = s
        out[f"pick_{k}"] = picked
    np.savez(os.path.join(HERE, "G11_pick.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
