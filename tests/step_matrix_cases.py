"""Constructed cases for the per-shape, per-variant matrix of the fused step (tests/test_step_matrix_gpu.py on the
device, tests/test_step_matrix_host.py on the oracle alone), and for the same matrix on the size-generic kernels
(tests/test_step_generic_gpu.py, tests/test_step_generic_host.py: rectangular boards, `Case(H, cfg, W=..., family="generic")`).

Nothing here is random: a case is a function of (shape, configuration, batch) only.  A pool holds eight levels whose
agents start on the cells where the row kernels change code path -- the four corners, both sides of the seam of the
split-halves row layout (columns WS-1 and WS, WS = ceil(W/2)) and one interior cell -- plus one level without an agent;
the life patterns, crates, exits and spawners sit on the same seams, and every level has a short action script that
walks, creates, destroys and pushes across them.  Seven start cells and an agent-less level make eight levels; eight
divides every workgroup size, so env e starts on level (e + e // NB) % 8 -- a level then sits at another position of the
wave and of the workgroup in every workgroup.

The actions of an env are scripted per LEVEL, so the builder has to know which level an env plays at every step.  It
does, without running anything: an episode's length depends on the level alone (the time limit; two steps on the level
whose exit is open next to the agent; one step on the agent-less level), so `Case.schedule` is plain arithmetic -- and
the host test asserts at every step that the oracle is where the schedule says.
"""
import numpy as np

from safelife_amd.cell_types import CellTypes as CT, DEFAULT_POINTS_TABLE
from safelife_amd.levels import Level, LevelPool

# The fourteen shapes with row kernels (SL_ROWLANE_SHAPES of sl_rowlane.hip).
SHAPES = (25, 26, 64, 24, 15, 20, 10, 8, 12, 16, 30, 32, 40, 48)
N_LEVELS = 8
T_SINGLE, T_ROLLOUT = 24, 6
WAVES = 4               # wavefronts per workgroup of the row kernels


def geometry(H, W):
    """The rule of `struct Geom` (sl_rowlane.hip), restated: a board's rows sit in consecutive lanes of a wavefront.
    VERT, how a lane reaches the rows above and below: "rotate" if H == 64 (the board fills the wave); "shift" if
    64 // (H + 2) == 64 // H (a halo lane either side of the board costs no board per wave); else "bpermute".
    GL = H + 2 for shift, else H (lanes per board); G = 64 // GL (boards per wave); NB = 4 * G (boards per workgroup).
    The goal-word cache exists only where a 64-env slice boundary is also a workgroup boundary (64 % NB == 0); rows
    wider than 32 cells (WS > 16) run at two waves per SIMD, and their plain kernels also serve a finished-episode
    queue (rowlane_lean_takes_queue)."""
    vert = "rotate" if H == 64 else ("shift" if 64 // (H + 2) == 64 // H else "bpermute")
    GL = H + 2 if vert == "shift" else H
    G = 64 // GL
    WS = (W + 1) // 2
    return dict(VERT=vert, GL=GL, G=G, NB=WAVES * G, WS=WS, cache=64 % (WAVES * G) == 0, lean_takes_queue=WS > 16)


def generic_threads(HW):
    """The workgroup size of the size-generic kernels (generic_threads of sl_generic.hip), restated: one wavefront for
    boards of up to 256 cells, two up to 1024, else four."""
    return 64 if HW <= 256 else 128 if HW <= 1024 else 256


# The side-effect pass (what a flush of the finished-episode queue runs) takes boards of up to 4096 cells on the
# size-generic kernels: the queue of a larger generic case is read as the step kernels left it, without the pass
# (Case.queue_raw).
GENERIC_QUEUE_MAX_CELLS = 4096


def generic_geometry(H, W):
    """The size-generic family: one board per workgroup (NB = 1) of generic_threads(H * W) threads, each thread a cell
    per pass.  WS = ceil(W/2) means nothing to these kernels; it stays the place where the constructed items sit.  The
    levels are dealt in groups of eight (`deal`), as on the 8-board workgroups of the row kernels."""
    threads = generic_threads(H * W)
    return dict(VERT=None, GL=None, G=None, NB=1, WS=(W + 1) // 2, cache=False, lean_takes_queue=False, threads=threads,
                passes=-(-H * W // threads), deal=N_LEVELS)


def goal_cache_expected(H, W, spawn):
    """Whether a plain batch of this shape keeps a goal-word cache (rowlane_goal_cache_bytes, restated): workgroups that
    tile a 64-env slice, and a plain single-step kernel whose goal words live in registers -- every spawner-free one,
    and with spawners the rows of at most 25 or more than 32 cells (gsh_in_registers)."""
    g = geometry(H, W)
    return g["cache"] and (spawn == "still" or g["WS"] > 16 or W <= 25)


# (shape, pool) whose step kernels the library's own queues cannot dispatch: every single-step kernel of 32x32 spawner pools
# spills (40 to 80 bytes of private memory per lane), and the queues' packets set up no private memory.  queues_open()
# refuses such a batch; the device test asserts the refusal, its reason, and that no other batch is refused.
QUEUES_CANNOT_DISPATCH = {(32, "spawn")}

EXPECTED_NB = {25: 8, 26: 8, 24: 8, 30: 8, 32: 8, 15: 16, 16: 16, 20: 12, 12: 20, 10: 24, 8: 32, 40: 4, 48: 4, 64: 4}

TRAINING_WRAPPERS = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4,
                         as_penalty=True, exit_bonus=0.5, penalty_coef=0.3, ignore_reward_cells=False)
OTHER_WRAPPERS = dict(movement_bonus=0.25, movement_bonus_power=0.5, movement_bonus_period=3,
                      as_penalty=False, exit_bonus=1.5, penalty_coef=0.125, ignore_reward_cells=True)
CHANNELS_15 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 25, 26, 27)

# (tables, spawners, front end): twelve configurations per shape
CONFIGS = tuple((tables, spawn, front) for front in ("plain", "obs", "wrap")
                for tables in ("one", "many") for spawn in ("still", "spawn"))


def config_id(cfg):
    return "-".join(cfg)


def kernel_slots(n_tables, spawner_free, wrapped, lean):
    """The slot rule of pick_rollout_t (sl_rowlane.hip), restated: bit 0 = one points table, bit 1 = spawner-free pool,
    then 4 = wrappers, 8 = lean (no wrappers, no observation of either layout, and no finished-episode queue unless the
    shape's lean kernels take one), 0 = neither; single-step launches use the twelve slots behind the T-step ones."""
    variant = (1 if n_tables == 1 else 0) | (2 if spawner_free else 0) | (4 if wrapped else (8 if lean else 0))
    return {variant, variant + 12}          # the T-step launch and the single-step one


# ---------------------------------------------------------------------------------------------- levels

GREEN = CT.color_g
AGENT = CT.player | GREEN
LIFE = CT.life | GREEN
RED_LIFE = CT.life | CT.color_r

# per level: the action scripts (two variants; an episode plays the first `time_limit` actions of one).  Moves are 1-4
# (up, right, down, left), create / destroy / shove 5-8 in the same directions.
SCRIPTS = (
    ((4, 1, 2, 3, 8, 5, 6, 7, 0), (8, 5, 4, 7, 2, 6, 1, 3, 0)),         # 0: from (0, 0) round the four corners
    ((2, 1, 4, 3, 6, 7, 5, 8, 0), (6, 7, 2, 5, 4, 8, 3, 1, 0)),         # 1: from (0, W-1), the other way round
    ((3, 4, 1, 2, 7, 8, 5, 6, 0), (5, 8, 3, 6, 4, 7, 1, 2, 0)),         # 2: from (H-1, 0)
    ((8, 3), (5, 3)),                                                   # 3: from (H-1, W-1): an edit, then out of the exit
    ((2, 2, 5, 7, 6, 4, 4, 8, 0), (6, 2, 5, 2, 7, 8, 4, 1, 3)),         # 4: interior: the crate over the row seam
    ((3, 3, 3, 1, 1, 8, 6, 4, 2), (7, 3, 3, 6, 8, 1, 1, 2, 4)),         # 5: from (H-2, WS-1): the crate over row H-1 -> 0
    ((4, 2, 8, 6, 5, 7, 1, 3, 0), (8, 4, 6, 2, 7, 5, 3, 1, 0)),         # 6: from (2, WS): both sides of the seam
    ((0,), (0,)),                                                       # 7: no agent
)
SUCCESS_LEVEL, CRATE_ROW_LEVEL, CRATE_TORUS_LEVEL, EVOLVING_LEVEL, AGENTLESS_LEVEL = 3, 4, 5, 6, 7


def small_table(k):
    """A points table of small integers (-3..3; they fit int8, so the row kernels still run)."""
    return ((np.arange(72).reshape(8, 9) * 7 + 3 * k + np.arange(72).reshape(8, 9) // 5) % 7 - 3).astype(np.int64)


def build_levels(H, W, tables, spawn):
    """The eight levels of a pool.  tables: "one" (every level the default table) or "many" (levels 2 and 5 their own);
    spawn: "still" or "spawn" (spawners on rows 0 and H-1 at columns WS-1 and WS, spawn_prob 0.05 / 0.9)."""
    WS = (W + 1) // 2
    r = H // 2
    levels = []

    def level(board, goals, loc, min_performance, k, exits=()):
        for y, x in exits:
            board[y, x] = CT.level_exit
        if loc is not None:
            board[loc] = AGENT
        if spawn == "spawn" and k in (0, 1, 2, 4, 6):
            a, b = ((0, WS - 1), (H - 1, WS)) if k in (0, 2, 6) else ((0, WS), (H - 1, WS - 1))
            board[a] = CT.spawner | GREEN
            board[b] = CT.spawner | CT.color_r
        table = small_table(k)[None] if tables == "many" and k in (2, 5) else DEFAULT_POINTS_TABLE[None]
        levels.append(Level(board, goals, None if loc is None else [loc], spawn_prob=0.05 if k in (1, 4) else 0.9,
                            min_performance=min_performance, points_table=table,
                            rng_words=[0x9E3779B97F4A7C15 ^ (k * 0x1234567), 0xD1B54A32D192ED03 + k, 0, 2 * (H * 131 + k) + 1]))

    def blank():
        goals = np.zeros((H, W), np.uint16)
        # goal cells where the scripts create life (points on a create, and required points > 0: the exits stay shut)
        for y, x in ((0, W - 1), (H - 1, 0), (0, 0), (H - 1, W - 1), (r - 2, WS), (r, WS), (2, WS - 1), (0, WS)):
            goals[y, x] = GREEN
        goals[r, 0] = goals[r, W - 1] = CT.color_r
        goals[1, 2] = CT.color_b
        return np.zeros((H, W), np.uint16), goals

    # 0: agent on corner (0, 0); a blinker across columns W-1 | 0; one exit, on a seam cell
    b, g = blank()
    b[r, W - 1] = b[r, 0] = b[r, 1] = RED_LIFE
    level(b, g, (0, 0), 0.5, 0, exits=[(2, WS - 1)])
    # 1: agent on corner (0, W-1); a blinker across rows H-1 | 0; three exits
    b, g = blank()
    b[H - 1, 2] = b[0, 2] = b[1, 2] = LIFE
    level(b, g, (0, W - 1), 0.5, 1, exits=[(r, WS - 1), (r, WS), (r + 1, 0)])
    # 2: agent on corner (H-1, 0); eight exits, all on seam columns
    b, g = blank()
    level(b, g, (H - 1, 0), 0.5, 2, exits=[(y, x) for y in (r, r + 1) for x in (0, WS - 1, WS, W - 1)])
    # 3: agent on corner (H-1, W-1); its exit is open from the reset and lies across the torus seam, on (0, W-1)
    b, g = blank()
    level(b, g, (H - 1, W - 1), -1.0, 3, exits=[(0, W - 1)])
    # 4: agent on an interior cell with a crate between it and the row seam; a block on the four corners of the array;
    #    no exit (episodes end by the time limit)
    b, g = blank()
    b[0, 0] = b[0, W - 1] = b[H - 1, 0] = b[H - 1, W - 1] = LIFE
    b[r - 1, WS - 1] = CT.crate
    level(b, g, (r - 1, WS - 2), 0.5, 4)
    # 5: agent on (H-2, WS-1) with a crate below it, on the last row; no exit
    b, g = blank()
    b[H - 1, WS - 1] = CT.crate
    level(b, g, (H - 2, WS - 1), 0.5, 5)
    # 6: agent on (2, WS); a glider that leaves through the bottom-right corner; living goal cells (a blinker in the
    #    goals: goals_static never becomes 1); one exit
    b, g = blank()
    for y, x in ((H - 3, W - 2), (H - 2, W - 1), (H - 1, W - 3), (H - 1, W - 2), (H - 1, W - 1)):
        b[y, x] = LIFE
    g[H - 3, 1] = g[H - 3, 2] = g[H - 3, 3] = CT.life | CT.color_b
    level(b, g, (2, WS), 0.5, 6, exits=[(r + 1, W - 1)])
    # 7: no agent (such an env is done at every step); three exits
    b, g = blank()
    b[r - 1, WS - 2] = b[r - 1, WS - 1] = b[r - 1, WS] = LIFE
    level(b, g, None, 0.5, 7, exits=[(0, 0), (r, WS), (H - 1, W - 1)])
    return levels


# ---------------------------------------------------------------------------------------------- cases

class Case(object):
    """One (shape, configuration, batch): the pool's levels, the env keywords and the scripted actions."""

    def __init__(self, H, cfg, batch="main", B=None, n_steps=T_SINGLE + T_ROLLOUT + 1, queue=None, W=None, family="row",
                 big_view=False):
        """family: "row" (a square row-kernel shape; W is H) or "generic" (any H x W; 17 envs in the main batch, dealt in
        groups of eight).  big_view: an "obs" case takes the raw view larger than the board whatever its tables and
        spawners say (and keeps its queue)."""
        tables, spawn, front = cfg
        assert family in ("row", "generic") and (family == "generic" or W in (None, H))
        W = H if W is None else W
        self.H, self.W, self.cfg, self.batch, self.family = H, W, cfg, batch, family
        self.big_view = big_view
        self.tables, self.spawn, self.front = tables, spawn, front
        if family == "row":
            self.geom = geometry(H, W)
            NB = deal = self.geom["NB"]
            self.B = B if B is not None else (2 * NB + 1 if batch == "main" else NB - 1)
        else:
            self.geom = generic_geometry(H, W)
            deal = self.geom["deal"]
            self.B = B if B is not None else 2 * deal + 1
        idx = CONFIGS.index(cfg)
        self.time_limit = 5 + idx % 5
        self.levels = build_levels(H, W, tables, spawn)
        e = np.arange(self.B)
        self.first_level = ((e + e // deal) % N_LEVELS).astype(np.int32)    # (shifted by one level per workgroup)
        self.kw = dict(auto_reset=True, level_stride=1, time_limit=self.time_limit, view_shape=(5, 7))
        self.policy_layout, self.queue_capacity, self.reset_at = None, 0, None
        combo = (tables == "many") * 2 + (spawn == "spawn")          # 0..3: the four (table, spawn) combinations
        if front == "plain":
            self.kw["with_obs"] = False
            self.reset_at = 9                               # a masked reset after this single step
            if queue:       # (only the wide shapes' plain kernels serve a queue: elsewhere this leaves the lean slots)
                self.queue_capacity = max(2, self.B // 4)
        elif front == "obs":
            # raw view larger than the board; channel list on a view equal to it; the two policy layouts on small views
            self.kw.update([dict(view_shape=(H + 2, W + 1), output_channels=None),
                            dict(view_shape=(H, W), output_channels=CHANNELS_15),
                            dict(view_shape=(5, 7), output_channels=CHANNELS_15),
                            dict(view_shape=(9, 15), output_channels=CHANNELS_15, remove_white_goals=False)][combo])
            self.policy_layout = (None, None, "uint8", "float32")[combo]
            if big_view:
                self.kw.update(view_shape=(H + 2, W + 1), output_channels=None)
                self.policy_layout = None
            if combo in (1, 2) if queue is None else queue:
                self.queue_capacity = max(2, self.B // 4)
        else:
            w = dict(TRAINING_WRAPPERS if tables == "one" else OTHER_WRAPPERS)
            if spawn == "spawn":                                            # the "inaction" baseline, a generator per env
                words = (np.arange(self.B * 4, dtype=np.uint64).reshape(self.B, 4) + np.uint64(17)) * np.uint64(0x9E3779B97F4A7C15)
                words[:, 3] |= np.uint64(1)                                 # a PCG64 increment is odd
                w.update(baseline="inaction", inaction_rng=words)
            self.kw["wrappers"] = w
        self.queue_raw = family == "generic" and H * W > GENERIC_QUEUE_MAX_CELLS
        self.wrapped = front == "wrap"
        self.inaction = self.wrapped and spawn == "spawn"
        self.with_obs = front != "plain"
        self.n_steps = n_steps
        self.reset_mask = (np.arange(self.B) % 3 == 0).astype(np.uint8)
        self.schedule, self.actions = self._script(n_steps)

    # the kernel slots this case launches (kernel_slots above)
    def slots(self):
        lean = self.front == "plain" and (self.queue_capacity == 0 or self.geom["lean_takes_queue"])
        return kernel_slots(1 if self.tables == "one" else 2, self.spawn == "still", self.wrapped, lean)

    def episode_steps(self, level):
        return 2 if level == SUCCESS_LEVEL else 1 if level == AGENTLESS_LEVEL else self.time_limit

    def _script(self, n_steps):
        """schedule int32 [n_steps, B, 2]: (level, steps played in the episode) of every env BEFORE step t;
        actions int32 [n_steps, B]."""
        sched = np.zeros((n_steps, self.B, 2), np.int32)
        acts = np.zeros((n_steps, self.B), np.int32)
        for e in range(self.B):
            level, s, episode = int(self.first_level[e]), 0, 0
            for t in range(n_steps):
                sched[t, e] = level, s
                script = SCRIPTS[level][(episode + e // N_LEVELS) % 2]
                acts[t, e] = script[s % len(script)]
                s += 1
                if s == self.episode_steps(level):
                    level, s, episode = (level + 1) % N_LEVELS, 0, episode + 1
                if t == self.reset_at and self.reset_mask[e]:       # the masked reset behind this step: on to the next level
                    level, s, episode = (level + 1) % N_LEVELS, 0, episode + 1
        return sched, acts

    def pool(self, counts_fn):
        return LevelPool(self.levels, counts_fn=counts_fn, min_performance_fraction=1.0)

    def backend_kw(self, device):
        """Keywords of util.DeviceBackend (device=True) or util.OracleBackend for this case."""
        kw = dict(self.kw, first_level=self.first_level)
        if device:
            if self.policy_layout:
                kw["policy_layout"] = self.policy_layout
            if self.queue_capacity:
                kw["side_effects"] = dict(capacity=self.queue_capacity, num_samples=2)
        return kw


def all_cases():
    return [(H, cfg) for H in SHAPES for cfg in CONFIGS]


def case_id(H, cfg, W=None):
    return "%dx%d-%s" % (H, H if W is None else W, config_id(cfg))


# ---------------------------------------------------------------------------------------------- the oracle's side

ENV_STATE = ("board", "goals", "agent_loc", "exit_locs", "rng", "num_steps", "old_value",
             "required_points", "initial_points", "goals_static", "is_active", "episode_reward",
             "episode_length", "level_idx", "episode_idx", "success", "times_up")


class OracleRun(object):
    """Steps a util.OracleBackend through a case's actions.  With `finished=True` the auto-reset is made by hand, so
    that the boards as the agents left them can be looked at first (what the device's finished-episode queue holds):
    `self.finished` is then the step's list of (env, episode_idx, level, num_steps, board, success, times_up,
    episode_reward, episode_length), in env order.  (Not with wrappers: a reset by hand clears the shaped reward.)"""

    def __init__(self, case, cpu, finished=False):
        assert not (finished and case.wrapped)
        self.case, self.cpu, self.by_hand = case, cpu, finished
        self.finished = []
        self.t = 0

    def step(self, actions=None):
        cpu, env = self.cpu, self.cpu.env
        a = self.case.actions[self.t] if actions is None else actions
        self.t += 1
        if not self.by_hand:
            obs, r, d = env.step(a)
            return None if obs is None else obs.copy(), r.copy(), d.copy()
        before = {k: cpu.get(k) for k in ("level_idx", "episode_idx")}
        env.s.auto_reset = 0
        _, r, d = env.step(a)
        r, d = r.copy(), d.copy()
        env.s.auto_reset = 1
        board, get = cpu.get("board"), cpu.get
        cols = {k: get(k) for k in ("num_steps", "success", "times_up", "episode_reward", "episode_length")}
        self.finished = [(int(e), int(before["episode_idx"][e]), int(before["level_idx"][e]), int(cols["num_steps"][e]),
                          board[e].copy(), int(cols["success"][e]), int(cols["times_up"][e]),
                          float(cols["episode_reward"][e]), int(cols["episode_length"][e])) for e in np.nonzero(d)[0]]
        if d.any():
            env.reset(d.astype(np.uint8))           # (a loaded env moves on to its next level, as the auto-reset does)
        obs = None if env.obs is None else env.obs.copy()
        return obs, r, d
