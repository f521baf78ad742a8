"""Static line-segment obstacle maps for the batched LiDAR simulator.

A map is a float32 array ``[S, 4]`` of segments ``(ax, ay, bx, by)`` in world metres; a
per-env map buffer is ``[N, S, 4]``.  Geometry is computed in float64 and rounded once.

Only ``stage_1`` has reference geometry
(``turtlebot3_simulations/turtlebot3_gazebo/worlds/train_world_new.world:85-416``: 4 outer
walls + 4 inner boxes, the obstacles the env's goal-rejection rectangles at
``project_ppo/src/environment_new.py:248-251,340-343`` are drawn around).  ``stage_2`` and
``stage_4`` are AUTHORED here (the reference's ``turtlebot3_stage_2.world`` is referenced by
``launch/turtlebot3_stage_2.launch:8`` but missing from the tree; "stage_4" appears nowhere),
so results on them are "parity unpinned (no reference geometry)".
"""
import math

import numpy as np

# Reference goal-rejection rectangles (xmin, xmax, ymin, ymax), inclusive.
RESET_RECTS_STAGE1 = np.array(  # environment_new.py:340-343
    [[1.7, 2.3, -1.2, 1.2], [-2.3, -1.7, -1.2, 1.2], [-1.2, 1.2, 1.7, 2.3], [-1.2, 1.2, -2.3, -1.7]], dtype=np.float64)
RESPAWN_RECTS_STAGE1 = np.array(  # environment_new.py:248-251
    [[1.6, 2.4, -1.4, 1.4], [-2.4, -1.6, -1.4, 1.4], [-1.4, 1.4, 1.6, 2.4], [-1.4, 1.4, -2.4, -1.6]], dtype=np.float64)


def box_to_segments(length, width, cx, cy, yaw):
    """Footprint of an SDF ``<box><size>length width h</size>`` posed at (cx, cy, yaw): 4 segments, CCW."""
    c, s = math.cos(yaw), math.sin(yaw)
    hx, hy = length / 2.0, width / 2.0
    corners = [(-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy)]
    pts = [(cx + c * px - s * py, cy + s * px + c * py) for px, py in corners]
    return [[pts[i][0], pts[i][1], pts[(i + 1) % 4][0], pts[(i + 1) % 4][1]] for i in range(4)]


def cylinder_to_segments(radius, cx, cy, sides=24, phase=0.0):
    """Regular ``sides``-gon inscribed in an SDF ``<cylinder>`` footprint, CCW."""
    pts = [(cx + radius * math.cos(phase + 2 * math.pi * k / sides), cy + radius * math.sin(phase + 2 * math.pi * k / sides))
           for k in range(sides)]
    return [[pts[k][0], pts[k][1], pts[(k + 1) % sides][0], pts[(k + 1) % sides][1]] for k in range(sides)]


def _as_map(segs):
    return np.asarray(segs, dtype=np.float64).astype(np.float32).reshape(-1, 4)


# (length, width, cx, cy, yaw) exactly as written in train_world_new.world (link poses at
# :122,:164,:206,:248,:290,:332,:374,:416; collision sizes at :89,:131,:173,:215,:257,:299,:341,:383)
_STAGE1_BOXES = [
    (8.0, 0.2, 4.0, 0.0, -1.5708),
    (8.0002, 0.2, 0.0, -4.0, 3.14159),
    (8.0, 0.2, -4.0, 0.0, 1.5708),
    (8.0, 0.2, 0.0, 4.0, 0.0),
    (2.0, 0.2, 2.0, 0.0, -1.5708),
    (2.0, 0.2, 0.0, -2.0, 3.14159),
    (2.0, 0.2, -2.0, 0.0, 1.5708),
    (2.0, 0.2, 0.0, 2.0, 0.0),
]


def stage_1():
    """8 boxes = 32 segments (reference geometry)."""
    segs = []
    for b in _STAGE1_BOXES:
        segs += box_to_segments(*b)
    return _as_map(segs)


def stage_2(sides=24):
    """AUTHORED: stage_1 shell + four r=0.3 m pillars at (+-2.6, +-2.6); 32 + 4*sides segments (128 by default)."""
    segs = []
    for b in _STAGE1_BOXES:
        segs += box_to_segments(*b)
    for sx in (1, -1):
        for sy in (1, -1):
            segs += cylinder_to_segments(0.3, 2.6 * sx, 2.6 * sy, sides=sides, phase=math.pi / sides)
    return _as_map(segs)


STAGE2_EXTRA_RECTS = np.array([[sx * 2.6 - 0.6, sx * 2.6 + 0.6, sy * 2.6 - 0.6, sy * 2.6 + 0.6]
                               for sx in (1, -1) for sy in (1, -1)], dtype=np.float64)


def stage_4():
    """AUTHORED: stage_1 shell + a pinwheel of four 1.6 m walls and four corner posts; 64 segments."""
    segs = []
    for b in _STAGE1_BOXES:
        segs += box_to_segments(*b)
    for k in range(4):
        a = k * math.pi / 2
        cx, cy = 2.9 * math.cos(a + math.pi / 4), 2.9 * math.sin(a + math.pi / 4)
        segs += box_to_segments(1.6, 0.15, cx, cy, a + 3 * math.pi / 4)
        segs += box_to_segments(0.3, 0.3, 3.3 * math.cos(a + 0.35), 3.3 * math.sin(a + 0.35), a)
    return _as_map(segs)


STAGE4_EXTRA_RECTS = np.array(
    [[2.05 * sx - 1.0, 2.05 * sx + 1.0, 2.05 * sy - 1.0, 2.05 * sy + 1.0] for sx in (1, -1) for sy in (1, -1)],
    dtype=np.float64)


def house_base():
    """The reference's ``models/turtlebot3_house/model.sdf`` cut at the LiDAR plane: 52 boxes + 4 cylinders (12-gons) = 256
    segments, produced by ``tools/gen_house_map.py`` with ``sdf_ingest`` (4 mesh collisions have no footprint and are
    skipped).  15 x 10.7 m."""
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "turtlebot3_house_segments.npy"))


def house(n_segments=2048, seed=0, keep_clear=None, clear_radius=0.6):
    """AUTHORED "small_house ~2k segments" map of BASELINE cfg 5 (``aws_robomaker_small_house_world`` is not vendored in
    the reference, ``navbot_small_house.launch:11``): ``house_base()`` furnished with seeded clutter -- thin table/chair
    legs (5 cm boxes) and round stools/plant pots (16-gons) -- until the map has exactly ``n_segments`` segments.  Clutter
    keeps ``clear_radius`` metres away from every point of ``keep_clear`` (default: the small_house start/goal tables)."""
    base = house_base()
    if keep_clear is None:
        keep_clear = np.concatenate([np.array(_HOUSE_STARTS)[:, :2], np.array(_HOUSE_GOALS)])
    rng = np.random.default_rng(seed)
    segs = [base.astype(np.float64)]
    n = base.shape[0]
    xmin, xmax, ymin, ymax = -7.3, 7.3, -5.1, 5.1
    placed = []
    while n < n_segments:
        left = n_segments - n
        x, y = rng.uniform(xmin, xmax), rng.uniform(ymin, ymax)
        if np.min(np.hypot(keep_clear[:, 0] - x, keep_clear[:, 1] - y)) < clear_radius:
            continue
        if placed and np.min(np.hypot(np.array(placed)[:, 0] - x, np.array(placed)[:, 1] - y)) < 0.25:
            continue
        if left >= 16 and rng.random() < 0.35:
            segs.append(np.array(cylinder_to_segments(rng.uniform(0.1, 0.2), x, y, sides=16, phase=rng.uniform(0, 1))))
            n += 16
        elif left >= 4:
            segs.append(np.array(box_to_segments(0.05, 0.05, x, y, rng.uniform(0, math.pi / 2))))
            n += 4
        else:  # 1..3 segments left: a short free-standing panel per segment
            a = rng.uniform(0, math.pi)
            segs.append(np.array([[x, y, x + 0.3 * math.cos(a), y + 0.3 * math.sin(a)]]))
            n += 1
        placed.append((x, y))
    return _as_map(np.concatenate(segs))


def open_tables(seg, starts, goals, n_beams=10, open_thresh=0.4):
    """Keeps the start poses / goal points whose surroundings are open in map ``seg`` (validate_open_space rule,
    spawn_goal_sampler.py:64-72) using a float64 numpy ray-caster (host-side tooling, not the simulation path)."""
    seg = np.asarray(seg, dtype=np.float64)

    def min_range(x, y):
        ang = np.linspace(-math.pi, math.pi, 72, endpoint=False)
        dx, dy = np.cos(ang)[:, None], np.sin(ang)[:, None]
        ax, ay, bx, by = seg.T
        ex, ey = bx - ax, by - ay
        den = dx * ey - dy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((ax - x) * ey - (ay - y) * ex) / den
            u = ((ax - x) * dy - (ay - y) * dx) / den
        t = np.where((den != 0) & (t >= 0) & (u >= 0) & (u <= 1), t, np.inf)
        return t.min()

    ks = [k for k, p in enumerate(starts) if min_range(p[0], p[1]) > open_thresh]
    kg = [k for k, p in enumerate(goals) if min_range(p[0], p[1]) > open_thresh]
    return np.asarray(starts)[ks], np.asarray(goals)[kg]


# ---------------------------------------------------------------------------------------------------------------
# Moving obstacles (NavSim.set_movers): a tape [P, M, 4] of P phases with M segments each.  Everything here is AUTHORED:
# results on it are "parity unpinned (no reference geometry)".
def mover_tape(frames):
    """frames: P phases, each M segments (ax, ay, bx, by) -> float32 [P, M, 4]; computed in float64 and rounded once, like a
    map.  Pad a phase that has fewer segments with NaN rows (a segment with a NaN coordinate is never hit)."""
    t = np.asarray(frames, dtype=np.float64)
    if t.ndim != 3 or t.shape[-1] != 4:
        raise ValueError(f"mover_tape: frames must be [P, M, 4], got {t.shape}")
    return t.astype(np.float32)


def orbit_frame(p, period, n=4, orbit_radius=1.0, radius=0.15, sides=8, centre=(0.0, 0.0)):
    """Phase p of orbit_movers: pillar k is a regular ``sides``-gon of circumradius ``radius`` (not turning about its own axis)
    centred at centre + orbit_radius (cos a, sin a), a = 2 pi ((p mod period) / period + k / n).  float64 [n * sides, 4]."""
    segs = []
    for k in range(n):
        a = 2.0 * math.pi * ((p % period) / period + k / n)
        segs += cylinder_to_segments(radius, centre[0] + orbit_radius * math.cos(a), centre[1] + orbit_radius * math.sin(a),
                                     sides=sides)
    return np.asarray(segs, dtype=np.float64)


def orbit_movers(period, n=4, orbit_radius=1.0, radius=0.15, sides=8, centre=(0.0, 0.0)):
    """AUTHORED: ``n`` regular-polygon pillars on a circle about ``centre``, one revolution per ``period`` steps.  Tape
    [period, n * sides, 4] float32.  With the defaults the pillars pass 0.85 m from the stage spawn pose (0, 0): the reset scans
    stay clear of them, a robot that drives outwards has to cross their orbit."""
    return mover_tape([orbit_frame(p, period, n, orbit_radius, radius, sides, centre) for p in range(period)])


MOVERS_DEFAULT_PERIOD = 64


def patrol_frame(p, period, ends, radius=0.15, sides=8):
    """Phase p of patrol_movers: pillar k stands at a + s (b - a) of ends[k] = (ax, ay, bx, by), s = 1 - |1 - 2 (p mod period) / period|
    (a at phase 0, b at half the period, back at a after one period).  float64 [len(ends) * sides, 4]."""
    s = 1.0 - abs(1.0 - 2.0 * (p % period) / period)
    segs = []
    for ax, ay, bx, by in np.asarray(ends, dtype=np.float64).reshape(-1, 4):
        segs += cylinder_to_segments(radius, ax + s * (bx - ax), ay + s * (by - ay), sides=sides)
    return np.asarray(segs, dtype=np.float64)


def patrol_movers(period, ends, radius=0.15, sides=8):
    """AUTHORED: regular-polygon pillars going back and forth along the segments ``ends`` [n, 4] (ax, ay, bx, by), one round trip per
    ``period`` steps.  Tape [period, n * sides, 4] float32."""
    return mover_tape([patrol_frame(p, period, ends, radius, sides) for p in range(period)])


def clutter_tape(centres, radius=0.15, sides=8):
    """AUTHORED: standing pillars at ``centres`` [n, 2] as a tape of period 1 -- extra STATIC obstacles that differ from env to env
    when they come from a bank.  Tape [1, n * sides, 4] float32."""
    segs = []
    for cx, cy in np.asarray(centres, dtype=np.float64).reshape(-1, 2):
        segs += cylinder_to_segments(radius, cx, cy, sides=sides)
    return mover_tape([segs])


def clutter_rects(centres, radius=0.15, margin=0.3):
    """Goal-rejection rectangles [n, 4] (xmin, xmax, ymin, ymax) round the pillars of clutter_tape: the pillar's bounding square
    grown by ``margin`` (stage_2's rectangles: radius 0.3, margin 0.3)."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 2)
    h = float(radius) + float(margin)
    return np.stack([c[:, 0] - h, c[:, 0] + h, c[:, 1] - h, c[:, 1] + h], axis=1)


def mover_bank(tapes, rects=None):
    """A bank of tapes for NavSim.set_mover_bank: tapes = K arrays [P_k, M_k, 4], rects = None or K lists of rectangles
    (xmin, xmax, ymin, ymax), possibly empty -> (bank [K, Pmax, Mmax, 4] float32, periods [K] int32, rects [K, R, 4] float64).
    What a tape or a rectangle list does not fill is NaN: a segment with a NaN coordinate is never hit, a rectangle row with one
    is absent, and rows periods[k] .. Pmax-1 of tape k are never read."""
    tapes = [np.asarray(t, dtype=np.float32) for t in tapes]
    if not tapes or any(t.ndim != 3 or t.shape[-1] != 4 or t.shape[0] < 1 or t.shape[1] < 1 for t in tapes):
        raise ValueError("mover_bank: tapes must be a non-empty list of [P, M, 4] arrays")
    K = len(tapes)
    bank = np.full((K, max(t.shape[0] for t in tapes), max(t.shape[1] for t in tapes), 4), np.nan, dtype=np.float32)
    for k, t in enumerate(tapes):
        bank[k, :t.shape[0], :t.shape[1]] = t
    periods = np.array([t.shape[0] for t in tapes], dtype=np.int32)
    rl = [np.zeros((0, 4))] * K if rects is None else [np.asarray(r, dtype=np.float64).reshape(-1, 4) for r in rects]
    if len(rl) != K:
        raise ValueError(f"mover_bank: {len(rl)} rectangle lists for {K} tapes")
    out = np.full((K, max(r.shape[0] for r in rl), 4), np.nan, dtype=np.float64)
    for k, r in enumerate(rl):
        out[k, :r.shape[0]] = r
    return bank, periods, out


def _scene_patrol2(P):
    return patrol_movers(P, [(1.0, -1.0, 1.0, 1.0), (-1.0, 1.0, -1.0, -1.0)])


_CLUTTER4 = [(2.6, 2.6), (-2.6, 2.6), (-2.6, -2.6), (2.6, -2.6)]   # where stage_2 has its pillars

# name -> (tape of period P, goal rectangles or None).  All AUTHORED: parity unpinned (no reference geometry).
_SCENES = {"orbit4": (lambda P: orbit_movers(P, n=4), None),
           "orbit2": (lambda P: orbit_movers(P, n=2, orbit_radius=1.4), None),
           "patrol2": (_scene_patrol2, None),
           "clutter4": (lambda P: clutter_tape(_CLUTTER4, radius=0.3), clutter_rects(_CLUTTER4, 0.3, 0.3))}


def movers_by_name(name, period=None):
    if name not in _SCENES:
        raise KeyError(f"unknown movers {name!r}; have {sorted(_SCENES)}")
    return _SCENES[name][0](int(period or MOVERS_DEFAULT_PERIOD))


def _seg_point_dist(ax, ay, bx, by, px, py):
    ex, ey = bx - ax, by - ay
    t = np.clip(((px - ax) * ex + (py - ay) * ey) / np.maximum(ex * ex + ey * ey, 1e-300), 0.0, 1.0)
    return np.hypot(ax + t * ex - px, ay + t * ey - py)


def mover_clearance(tape, starts=((0.0, 0.0),)):
    """The smallest distance between a segment of any phase of ``tape`` [..., 4] and a start pose (NaN segments are absent)."""
    g = np.asarray(tape, dtype=np.float64).reshape(-1, 4)
    g = g[~np.isnan(g).any(axis=1)]
    return min(float(_seg_point_dist(g[:, 0], g[:, 1], g[:, 2], g[:, 3], p[0], p[1]).min()) for p in starts) if g.size else math.inf


def random_scenario(rng, period, goal_box=3.6, start=(0.0, 0.0), clear_radius=0.6, radius=0.15, sides=8, pillars=4):
    """One AUTHORED scenario from ``rng``: ``pillars`` pillars, each an orbiter about the start pose, a patrol between two points of
    the goal box or a standing pillar (period 1: standing pillars only), none of which comes within ``clear_radius`` of the start
    pose in any phase.  -> (tape [period, pillars * sides, 4], rectangles round the standing pillars [n, 4])."""
    keep = clear_radius + radius + 0.05

    def point():
        while True:
            q = rng.uniform(-goal_box, goal_box, 2)
            if math.hypot(q[0] - start[0], q[1] - start[1]) >= keep:
                return q
    kinds = ["clutter"] * pillars if period == 1 else list(rng.choice(["orbit", "patrol", "clutter"], size=pillars))
    orbit, patrol, clutter = [], [], []
    for kind in kinds:
        if kind == "orbit":
            orbit.append((rng.uniform(keep + 0.15, 1.6), rng.uniform(0.0, 2.0 * math.pi), rng.choice([-1.0, 1.0])))
        elif kind == "patrol":
            while True:
                a, b = point(), point()
                if _seg_point_dist(a[0], a[1], b[0], b[1], start[0], start[1]) >= keep:
                    break
            patrol.append((a[0], a[1], b[0], b[1]))
        else:
            clutter.append(point())
    frames = []
    for p in range(period):
        segs = []
        for r, a0, sgn in orbit:
            a = a0 + sgn * 2.0 * math.pi * p / period
            segs += cylinder_to_segments(radius, start[0] + r * math.cos(a), start[1] + r * math.sin(a), sides=sides)
        if patrol:
            segs += patrol_frame(p, period, patrol, radius, sides).tolist()
        for cx, cy in clutter:
            segs += cylinder_to_segments(radius, cx, cy, sides=sides)
        frames.append(segs)
    return mover_tape(frames), (clutter_rects(clutter, radius, 0.3) if clutter else np.zeros((0, 4)))


def random_mover_bank(K, seed=0, period_choices=(1, 32, 64, 128), goal_box=3.6, start=(0.0, 0.0), clear_radius=0.6, radius=0.15,
                      sides=8, pillars=4):
    """AUTHORED: K scenarios, scenario k a pure function of (seed, k): a period drawn from ``period_choices`` and
    random_scenario's mix of orbiters, patrols and standing clutter inside the goal box (period 1: clutter only, i.e. extra static
    obstacles that differ from env to env).  Standing pillars come with their goal rectangles.  -> mover_bank's triple, every
    tape with pillars * sides segments (32: orbit4's)."""
    tapes, rects = [], []
    for k in range(int(K)):
        rng = np.random.default_rng([int(seed), k])
        period = int(rng.choice(np.asarray(period_choices)))
        t, r = random_scenario(rng, period, goal_box, start, clear_radius, radius, sides, pillars)
        tapes.append(t)
        rects.append(r)
    return mover_bank(tapes, rects)


class MoverBank:
    """What resolve_movers returns for a bank: the arrays of mover_bank and how the envs are given their tapes."""

    def __init__(self, bank, periods, rects, assign):
        self.bank, self.periods, self.rects, self.assign = bank, periods, rects, assign

    def tape_ids(self, n_envs, map_seed=0, env_id_base=0):
        K = len(self.periods)
        if isinstance(self.assign, str):
            if self.assign == "random":
                return mover_tape_ids(K, n_envs, map_seed, env_id_base)
            return ((int(env_id_base) + np.arange(int(n_envs))) % K).astype(np.int32)   # "cycle", by the GLOBAL env id
        ids = np.asarray(self.assign)
        if ids.shape != (int(n_envs),) or not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= K:
            raise ValueError(f"movers: assign must be 'random', 'cycle' or {n_envs} tape ids in [0, {K})")
        return ids.astype(np.int32)


def resolve_movers(movers):
    """VecEnv's ``movers`` argument -> (tape [P, M, 4], phase rule "random" | "zero") for a single tape -- a tape, a scene name
    ("orbit4"), dict(tape=... | name=..., period=...) -- or (MoverBank, phase rule) for a bank of tapes, one scenario per env:
    dict(bank=[K, Pmax, M, 4], periods=[K], rects=[K, R, 4], assign="random" | "cycle" | [N] ids), the name "random:K"
    (random_mover_bank(K, seed), dict(name="random:K", seed=...)) or "bank:orbit4,patrol2,..." (one tape per listed scene)."""
    spec = dict(movers) if isinstance(movers, dict) else ({"name": movers} if isinstance(movers, str) else {"tape": movers})
    phase = spec.pop("phase", "random")
    if phase not in ("random", "zero"):
        raise ValueError(f"movers: phase must be 'random' or 'zero', got {phase!r}")
    if sum(k in spec for k in ("tape", "name", "bank")) != 1:
        raise ValueError("movers: give a tape or a name" if "bank" not in spec else "movers: give a bank, a tape or a name")
    out = None
    name = spec.get("name")
    if "bank" in spec:
        bank = np.asarray(spec.pop("bank"), dtype=np.float32)
        if bank.ndim != 4 or bank.shape[-1] != 4:
            raise ValueError(f"movers: bank must be [K, Pmax, M, 4], got {bank.shape}")
        periods = spec.pop("periods", None)
        periods = np.full(bank.shape[0], bank.shape[1], dtype=np.int32) if periods is None else np.asarray(periods, dtype=np.int32)
        if periods.shape != (bank.shape[0],) or periods.min() < 1 or periods.max() > bank.shape[1]:
            raise ValueError(f"movers: periods must be {bank.shape[0]} integers in [1, {bank.shape[1]}]")
        out = MoverBank(bank, periods, spec.pop("rects", None), spec.pop("assign", "random"))
    elif isinstance(name, str) and name.startswith("random:"):
        spec.pop("name")
        try:
            K = int(name[len("random:"):])
        except ValueError:
            K = 0
        if K < 1:
            raise ValueError(f"movers: {name!r} is not 'random:K' with K >= 1")
        out = MoverBank(*random_mover_bank(K, seed=int(spec.pop("seed", 0))), spec.pop("assign", "random"))
    elif isinstance(name, str) and name.startswith("bank:"):
        spec.pop("name")
        scenes = [n for n in name[len("bank:"):].split(",") if n]
        if not scenes:
            raise ValueError(f"movers: {name!r} lists no scene; have {sorted(_SCENES)}")
        P = spec.pop("period", None)
        out = MoverBank(*mover_bank([movers_by_name(n, P) for n in scenes], [_SCENES[n][1] if _SCENES[n][1] is not None else [] for n in scenes]),
                        spec.pop("assign", "random"))
    elif "tape" in spec:
        out = spec.pop("tape")
    else:
        out = movers_by_name(spec.pop("name"), spec.pop("period", None))
    if isinstance(out, MoverBank) and isinstance(out.assign, str) and out.assign not in ("random", "cycle"):
        raise ValueError(f"movers: assign must be 'random', 'cycle' or an array of tape ids, got {out.assign!r}")
    if spec:
        raise ValueError(f"movers: unknown entries {sorted(spec)}")
    return out, phase


def _env_hash(n_envs, map_seed, env_id_base, salt):
    """the splitmix64 finaliser of (map_seed, global env id) and of nothing else, one uint64 per env"""
    g = np.arange(int(env_id_base), int(env_id_base) + int(n_envs), dtype=np.uint64)
    z = g * np.uint64(0x9E3779B97F4A7C15) + np.uint64((int(map_seed) * 0xD1B54A32D192ED03 + salt) & 0xFFFFFFFFFFFFFFFF)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mover_phases(period, n_envs, map_seed=0, env_id_base=0):
    """phase0[i] in [0, period) for envs env_id_base .. env_id_base + n_envs - 1: a hash (the splitmix64 finaliser) of
    (map_seed, global env id) and of nothing else, so every shard of a run draws the phases the single-GPU run draws."""
    return (_env_hash(n_envs, map_seed, env_id_base, 0x2545F4914F6CDD1D) % np.uint64(int(period))).astype(np.int32)


def mover_tape_ids(K, n_envs, map_seed=0, env_id_base=0):
    """tape_id[i] in [0, K): mover_phases' counterpart for the tape of a bank, with a constant of its own (so that an env's tape and
    its phase are independent).  Every shard of a run gives a global env the tape the single-GPU run gives it."""
    return (_env_hash(n_envs, map_seed, env_id_base, 0x6A09E667F3BCC909) % np.uint64(int(K))).astype(np.int32)


def mover_bank_phases(periods_of_env, map_seed=0, env_id_base=0):
    """phase0[i] in [0, periods_of_env[i]): the hash of mover_phases reduced by each env's own period (K = 1: mover_phases)."""
    per = np.asarray(periods_of_env).astype(np.uint64).reshape(-1)
    return (_env_hash(per.size, map_seed, env_id_base, 0x2545F4914F6CDD1D) % per).astype(np.int32)


def by_name(name):
    table = {"stage_1": stage_1, "stage_2": stage_2, "stage_4": stage_4, "house": house, "house_base": house_base}
    if name not in table:
        raise KeyError(f"unknown map {name!r}; have {sorted(table)}")
    return table[name]()


def goal_rects(name):
    """(reset_rects, respawn_rects) for a named map."""
    if name == "stage_1":
        return RESET_RECTS_STAGE1, RESPAWN_RECTS_STAGE1
    if name == "stage_2":
        return (np.concatenate([RESET_RECTS_STAGE1, STAGE2_EXTRA_RECTS]),
                np.concatenate([RESPAWN_RECTS_STAGE1, STAGE2_EXTRA_RECTS]))
    if name == "stage_4":
        return (np.concatenate([RESET_RECTS_STAGE1, STAGE4_EXTRA_RECTS]),
                np.concatenate([RESPAWN_RECTS_STAGE1, STAGE4_EXTRA_RECTS]))
    if name in ("house", "house_base"):  # goals come from the curated tables (sampler), not from the uniform box
        return np.zeros((0, 4)), np.zeros((0, 4))
    raise KeyError(name)


def replicate_per_env(seg, n_envs, seed=0, jitter=0.02, shuffle=True):
    """Per-env segment buffers ``[N, S, 4]`` (BASELINE cfg 3: "per-env pose/segment buffers").

    Every env gets its own copy of the map with a small random rigid offset (|d| <= jitter
    metres, so the spawn pose and goal box stay valid) and, optionally, its own segment order,
    so that per-env loads are real and no two envs read identical bytes.
    """
    rng = np.random.default_rng(seed)
    seg = np.asarray(seg, dtype=np.float32).reshape(-1, 4)
    S = seg.shape[0]
    out = np.empty((n_envs, S, 4), dtype=np.float32)
    off = rng.uniform(-jitter, jitter, size=(n_envs, 2))
    for i in range(n_envs):
        order = rng.permutation(S) if shuffle else np.arange(S)
        s64 = seg[order].astype(np.float64)
        s64[:, [0, 2]] += off[i, 0]
        s64[:, [1, 3]] += off[i, 1]
        out[i] = s64.astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------
# Curated start poses (x, y, yaw) and goal points of the reference's GoalSpawnSampler
# (project_ppo/src/spawn_goal_sampler.py:5-35).  These are scenario DATA of the reference (hand-picked free-space
# coordinates for its two worlds), reproduced so that `--use_external_sampler` runs are drop-in; the sampling rule
# itself is re-implemented in the step/reset kernels (navsim_set_spawn_sampler).
_STAGE1_STARTS = [(0.0, 0.0, 0.0), (0.5, 0.5, 0.785), (-0.5, 0.5, 2.356), (0.5, -0.5, -0.785), (-0.5, -0.5, -2.356),
                  (1.0, 0.0, 0.0), (0.0, 1.0, 1.57), (-1.0, 0.0, 3.14), (0.0, -1.0, -1.57), (1.0, 1.0, 0.785)]
_STAGE1_GOALS = [(3.0, 3.0), (3.5, 2.5), (2.5, 3.5), (4.0, 3.0), (-3.0, 3.0), (-3.5, 2.5), (-2.5, 3.5), (-4.0, 3.0),
                 (3.0, -3.0), (3.5, -2.5), (2.5, -3.5), (4.0, -3.0), (-3.0, -3.0), (-3.5, -2.5), (-2.5, -3.5), (-4.0, -3.0),
                 (4.0, 0.0), (-4.0, 0.0), (0.0, 4.0), (0.0, -4.0), (3.0, 0.0), (-3.0, 0.0), (0.0, 3.0), (0.0, -3.0),
                 (2.0, 2.0), (-2.0, 2.0), (2.0, -2.0), (-2.0, -2.0)]
_HOUSE_STARTS = [(-3.5, 1.0, 0.0), (-3.0, 0.5, 1.57), (-2.5, 1.5, -1.57), (-3.0, 2.0, 0.0), (-1.0, 0.0, 0.0), (-0.5, 0.5, 1.57),
                 (0.0, 0.0, -1.57), (2.0, 1.5, 3.14), (2.5, 0.5, -1.57), (3.0, 1.0, 0.0), (1.0, -2.0, 1.57), (0.5, -2.5, 0.0),
                 (1.5, -2.0, -1.57), (-1.5, 2.5, 0.0), (-2.0, 3.0, 1.57), (0.0, 1.0, 0.0), (-1.0, 1.5, 1.57), (1.0, 1.0, -1.57)]
_HOUSE_GOALS = [(-3.5, 0.5), (-3.0, 1.5), (-2.5, 2.0), (-3.5, 2.5), (-4.0, 1.0), (-2.0, 1.0), (-3.0, 0.0), (-1.0, 0.5),
                (-0.5, 0.0), (0.0, 0.5), (-1.5, 0.0), (0.5, 0.0), (-1.0, -0.5), (2.0, 0.5), (2.5, 1.0), (3.0, 1.5), (2.0, 2.0),
                (3.5, 1.0), (2.5, 0.0), (3.0, 0.5), (1.0, -2.5), (0.5, -2.0), (1.5, -2.5), (1.0, -3.0), (0.0, -2.5), (1.5, -1.5),
                (-1.5, 2.0), (-2.0, 2.5), (-1.0, 3.0), (-2.5, 2.5), (-1.5, 3.5), (0.0, 1.5), (-1.0, 1.0), (1.0, 0.5), (0.5, 1.5),
                (-0.5, 1.0), (0.0, 2.0), (1.0, 1.5), (-4.0, 3.0), (3.5, 2.0), (2.0, -3.0), (-2.0, -1.0)]


def spawn_tables(world_type, min_dist=1.5, max_dist=6.0):
    """(starts [K,3], goals [G,2], min_dist, max_dist) as GoalSpawnSampler(world_type) holds them
    (spawn_goal_sampler.py:38-50; defaults min_dist=1.5, max_dist=6.0 at :38)."""
    if world_type == "stage1":
        st, g = _STAGE1_STARTS, _STAGE1_GOALS
    elif world_type == "small_house":
        st, g = _HOUSE_STARTS, _HOUSE_GOALS
    else:
        raise ValueError(f"Unknown world_type: {world_type}")  # same error as spawn_goal_sampler.py:49
    return np.array(st, dtype=np.float64), np.array(g, dtype=np.float64), float(min_dist), float(max_dist)


def validate_open_space(ranges, range_min=0.12, range_max=3.5, open_thresh=0.4):
    """GoalSpawnSampler.validate_open_space (spawn_goal_sampler.py:64-72) on a raw scan array [..., B]: the smallest
    range strictly inside (range_min, range_max) must exceed open_thresh; no valid range -> False."""
    r = np.asarray(ranges, dtype=np.float64)
    valid = (r > range_min) & (r < range_max)
    mn = np.where(valid, r, np.inf).min(axis=-1)
    return valid.any(axis=-1) & (mn > open_thresh)
