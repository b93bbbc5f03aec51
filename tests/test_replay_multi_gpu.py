"""Multi-agent DQN replay on the device: slhip_replay_add_masked against what the reference's DQN left in its replay buffer
when driven with multi-agent envs (tests/golden/replay_multi_cases.npz), with inactive columns poisoned, and against
slhip_replay_add when everybody is active; the masked epsilon-greedy draw against its exact host model; sample and gather
on a multi-agent ring; MultiAgentDQNRunner.collect end to end against the numpy restatement (tests/replay_multi_ref.py) fed
the same step stream.  Everything is compared for equality."""
import collections
import ctypes as C

import numpy as np
import pytest

from safelife_amd import _hip
from tests import replay_multi_ref as mr
from tests import replay_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

CASES = mr.load_cases()
SINGLE = [c for c in rr.load_cases() if c["B"] in (65, 257)]
ROW_BYTES = (16, 48, 6250, 6256)        # 16-byte lanes, 16-byte lanes with a tail wave, 2-byte lanes, 16-byte lanes
Step = collections.namedtuple("Step", "obs actions rewards done next_obs active")
STATE = ("obs", "next_obs", "action", "reward", "done", "win_obs", "win_action", "win_reward", "fill", "head", "idx",
         "status")


def _device_counts(boards, goals):
    from safelife_amd.levels import _device_counts as f
    return f(boards, goals)


def rows_of(c, t, nbytes):
    """The observation of column c at time t as a real row: uint8 [len(c), nbytes], every (c, t) a different row, no row
    all 0 or all 0xFF."""
    c, t = np.asarray(c, np.int64).reshape(-1, 1), np.asarray(t, np.int64).reshape(-1, 1)
    col = np.arange(nbytes, dtype=np.int64).reshape(1, -1)
    return ((c * 131 + t * 29 + col * 7 + (c * t + col // 251) % 13) % 251).astype(np.uint8)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bytes(a, b):
    """Two tensors hold the same bytes (NaN rewards included)."""
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _buffer(case, nbytes):
    import torch
    from safelife_amd.replay import MultiAgentReplayBuffer
    rdt = torch.float64 if case["R"].dtype == np.float64 else torch.float32
    return MultiAgentReplayBuffer(case["capacity"], case["B"], case["A"], multi_step=case["n"], gamma=case["gamma"],
                                  obs_shape=(nbytes,), obs_dtype=torch.uint8, reward_dtype=rdt, device=_hip.device())


def _steps(case, nbytes, poisoned=False):
    """The case's step stream as device tensors shaped [B, A, ...].  ``poisoned``: what an inactive column holds is what
    must never be read -- NaN rewards, actions -1 and 2^31 - 1, rows of 0xFF, done = 1 (as the real env reports it)."""
    import torch
    dev = _hip.device()
    B, A, N = case["B"], case["A"], case["columns"]
    cols = np.arange(N)
    for t in range(case["T"]):
        on = case["active"][t].reshape(N) != 0
        obs, nxt = rows_of(cols, t, nbytes), rows_of(cols, t + 1, nbytes)
        act, rew, done = case["ACT"][t].reshape(N).copy(), case["R"][t].reshape(N).copy(), case["D"][t].reshape(N).copy()
        if poisoned:
            obs[~on], nxt[~on], rew[~on], done[~on] = 0xFF, 0xFF, np.nan, 1
            act[~on] = np.where(cols[~on] % 2 == 0, -1, 2 ** 31 - 1)
        yield Step(torch.from_numpy(obs).to(dev).view(B, A, nbytes), torch.from_numpy(act).to(dev).view(B, A),
                   torch.from_numpy(rew).to(dev).view(B, A), torch.from_numpy(done).to(dev).view(B, A),
                   torch.from_numpy(nxt).to(dev).view(B, A, nbytes), torch.from_numpy(case["active"][t].copy()).to(dev))


def _check_against_dump(buf, case, dump, steps, nbytes):
    n, N = case["n"], case["columns"]
    size = len(dump["done"])
    assert int(buf.idx.item()) == dump["idx"] and len(buf) == size
    assert np.array_equal(buf.action.cpu().numpy()[:size], dump["action"])
    assert np.array_equal(bits64(buf.reward.cpu().numpy()[:size]), bits64(dump["reward"]))
    assert np.array_equal(buf.done.cpu().numpy()[:size], dump["done"])
    obs, nxt = buf.obs.cpu().numpy(), buf.next_obs.cpu().numpy()
    assert np.array_equal(obs[:size], rows_of(dump["obs_c"], dump["obs_t"], nbytes))
    assert np.array_equal(nxt[:size], rows_of(dump["next_c"], dump["next_t"], nbytes))
    assert not obs[size:].any() and not nxt[size:].any()           # slots never pushed stay as they were
    fill = buf.fill.cpu().numpy()
    assert np.array_equal(fill, dump["fill"])
    assert int(buf.head.item()) == steps % n
    # the device window is a ring over t mod n: a column with fill > k took part in the last k + 1 steps (it is only ever
    # away after a done, which empties it), so its step k steps back sits in slot (steps - 1 - k) mod n
    wr, wa, wo = buf.win_reward.cpu().numpy(), buf.win_action.cpu().numpy(), buf.win_obs.cpu().numpy()
    for k in range(n):
        slot, live = (steps - 1 - k) % n, fill > k
        assert np.array_equal(bits64(wr[slot][live]), bits64(dump["w_reward"][k][live]))
        assert np.array_equal(wa[slot][live], dump["w_action"][k][live])
        assert np.array_equal(wo[slot][live], rows_of(np.arange(N)[live], dump["w_obs_t"][k][live], nbytes))
    assert int(buf.status.item()) == 0
    assert buf.min_len() <= size


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_add_masked_equals_the_reference(case):
    """Ring, idx, fill and the windows equal the reference's at the three dumps, with real rows built from the tags: a
    small row size and a large one per case, all four sizes over the cases of every n."""
    i = case["index"]
    # (the widest windows take the two small sizes: what they are here for is the plan's scan and the copy grid)
    for nbytes in (ROW_BYTES[i % 2], ROW_BYTES[2 + (i // 2) % 2]) if case["columns"] < 1000 else ROW_BYTES[:2]:
        buf = _buffer(case, nbytes)
        for t, step in enumerate(_steps(case, nbytes)):
            buf.add(step)
            for j, s in enumerate(case["dump_steps"]):
                if s == t + 1:
                    _check_against_dump(buf, case, case["dumps"][j], t + 1, nbytes)
        assert buf.steps_added == case["T"]


N5 = [c for c in CASES if c["n"] == 5]


@pytest.mark.parametrize("case", N5, ids=[c["id"] for c in N5])
def test_nothing_of_an_inactive_column_is_read(case):
    """The n = 5 cases once more with every input of the inactive columns poisoned: ring, windows, fill, idx, head and
    status are byte for byte those of the clean run, and ring slots never pushed are still zero."""
    import torch
    nbytes = ROW_BYTES[(case["index"] // 2) % (4 if case["columns"] < 1000 else 2)]
    clean, dirty = _buffer(case, nbytes), _buffer(case, nbytes)
    for a, b in zip(_steps(case, nbytes), _steps(case, nbytes, poisoned=True)):
        clean.add(a), dirty.add(b)
    for name in STATE:
        assert same_bytes(getattr(clean, name), getattr(dirty, name)), name
    size = len(dirty)
    assert int(dirty.idx.item()) == case["dumps"][2]["idx"] and int(dirty.status.item()) == 0
    assert not dirty.obs[size:].any() and not dirty.next_obs[size:].any()
    assert not dirty.action[size:].any() and not dirty.done[size:].any() and not dirty.reward[size:].view(torch.uint8).any()
    if case["A"] >= 2 and case["T"] > 1:
        assert not case["active"].all()                 # (there was something to poison)


@pytest.mark.parametrize("case", SINGLE, ids=[c["id"] for c in SINGLE])
def test_null_and_all_ones_masks_equal_the_unmasked_add(case):
    """The single-agent fixture through slhip_replay_add, slhip_replay_add_masked(active = NULL) and an all-ones mask: every
    array of the three buffers holds the same bytes after every step -- and they are the reference's."""
    import torch
    from safelife_amd.replay import ReplayBuffer
    dev, lib = _hip.device(), _hip.lib()
    B, T, n = case["B"], case["T"], case["n"]
    nbytes = ROW_BYTES[case["index"] % 4]
    rdt = torch.float64 if case["R"].dtype == np.float64 else torch.float32
    bufs = [ReplayBuffer(case["capacity"], B, multi_step=n, gamma=case["gamma"], obs_shape=(nbytes,), obs_dtype=torch.uint8,
                         reward_dtype=rdt, device=dev) for _ in range(3)]
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    envs = np.arange(B)
    for t in range(T):
        obs, nxt = (torch.from_numpy(rows_of(envs, t + k, nbytes)).to(dev) for k in (0, 1))
        act, rew, done = (torch.from_numpy(case[k][t].copy()).to(dev) for k in ("A", "R", "D"))
        args = [_hip.ptr(x) for x in (obs, act, rew, done, nxt)]
        st = _hip.current_stream_ptr()
        _hip.check(lib.slhip_replay_add(C.byref(bufs[0].struct), *args, st))
        _hip.check(lib.slhip_replay_add_masked(C.byref(bufs[1].struct), *args, None, st))
        _hip.check(lib.slhip_replay_add_masked(C.byref(bufs[2].struct), *args, _hip.ptr(ones), st))
        for name in STATE + ("plan_base", "plan_code"):
            assert same_bytes(getattr(bufs[0], name), getattr(bufs[1], name)), (t, name)
            assert same_bytes(getattr(bufs[0], name), getattr(bufs[2], name)), (t, name)
    dump = case["dumps"][2]
    size = len(dump["done"])
    assert int(bufs[2].idx.item()) == dump["idx"]
    assert np.array_equal(bits64(bufs[2].reward.cpu().numpy()[:size]), bits64(dump["reward"]))
    assert np.array_equal(bufs[2].obs.cpu().numpy()[:size], rows_of(dump["obs_b"], dump["obs_t"], nbytes))
    assert np.array_equal(bufs[2].fill.cpu().numpy(), dump["fill"])


# ----------------------------------------------------------------------------------------------- the masked epsilon draw

@pytest.mark.parametrize("B", [1, 255, 256, 257, 1032])
def test_masked_eps_draw_equals_the_model(B):
    import torch
    dev, lib = _hip.device(), _hip.lib()
    NA = 9
    rng = np.random.default_rng(B)
    q = rng.standard_normal((B, NA)).astype(np.float32)
    q[1::7, 2] = q[1::7, 6] = 5.0                       # two maxima: the first
    active = (rng.random(B) < 0.6).astype(np.uint8)
    if B > 1:
        active[:3] = (1, 0, 1)
    q[active == 0] = np.nan                             # rows under the mask are not read
    qd, ad = torch.from_numpy(q).to(dev), torch.from_numpy(active).to(dev)

    def draw(rows, mask, eps, seed, counter, masked=True):
        out = torch.full((rows.shape[0] + 1,), -3, dtype=torch.int32, device=dev)
        if masked:
            rc = lib.slhip_sample_actions_eps_masked(_hip.ptr(rows), _hip.ptr(mask), rows.shape[0], NA, eps, seed % 2 ** 64,
                                                     counter, _hip.ptr(out), _hip.current_stream_ptr())
        else:
            rc = lib.slhip_sample_actions_eps(_hip.ptr(rows), rows.shape[0], NA, eps, seed % 2 ** 64, counter, _hip.ptr(out),
                                              _hip.current_stream_ptr())
        _hip.check(rc)
        out = out.cpu().numpy()
        assert out[-1] == -3
        return out[:-1]

    on = active != 0
    for eps in (0.0, 0.3, 1.0):
        for seed, counter in ((0, 0), (5, 17), (2 ** 64 - 1, 2 ** 64 - 1)):
            got = draw(qd, ad, eps, seed, counter)
            assert np.array_equal(got, mr.eps_model_masked(q, active, eps, seed, counter)), (eps, seed, counter)
            assert not got[~on].any()
            # a null mask is the plain draw (NaN rows included: the first NaN wins), and active rows draw what it draws
            plain = draw(qd, None, eps, seed, counter, masked=False)
            assert np.array_equal(draw(qd, None, eps, seed, counter), plain)
            assert np.array_equal(got[on], plain[on])
    if B > 1:       # two shards of one run reproduce the whole: envs [0, lo) and [lo, B / A) of A agents each
        A = 3 if B % 3 == 0 else (8 if B % 8 == 0 else 1)
        lo = (B // A) // 3 * A                          # the first row of the second shard
        whole = draw(qd, ad, 0.3, 77, 3)
        first = draw(qd[:lo].contiguous(), ad[:lo].contiguous(), 0.3, 77, 3)
        second = draw(qd[lo:].contiguous(), ad[lo:].contiguous(), 0.3, 77 + rr.policy_ref.G * lo, 3)
        assert np.array_equal(np.concatenate([first, second]), whole)


# ------------------------------------------------------------------------------------------------------ sample and gather

def test_sample_and_gather_on_a_multi_agent_ring():
    """An unchanged pair of kernels on a ring filled through the masked add: the sampler's model over the rows held, and
    numpy indexing of the ring."""
    import torch
    case = next(c for c in CASES if (c["B"], c["A"], c["n"], c["T"]) == (21, 3, 5, 17))
    nbytes = 48
    buf = _buffer(case, nbytes)
    buf.seed = 11
    for step in _steps(case, nbytes):
        buf.add(step)
    size = len(buf)
    assert size == min(case["dumps"][2]["idx"], case["capacity"])
    index = buf.sample_indices(32)
    want = rr.sample_model(size, 32, 11, 0)
    assert np.array_equal(index.cpu().numpy(), want)
    ring = {name: getattr(buf, name).cpu().numpy() for name in ("obs", "next_obs", "action", "reward", "done")}
    for widen in (True, False):
        got = buf.gather(index, obs_float32=widen)
        dt = np.float32 if widen else np.uint8
        assert np.array_equal(got.obs.cpu().numpy(), ring["obs"][want].astype(dt))
        assert np.array_equal(got.next_obs.cpu().numpy(), ring["next_obs"][want].astype(dt))
        assert np.array_equal(got.action.cpu().numpy(), ring["action"][want].astype(np.int64))
        assert np.array_equal(got.reward.cpu().numpy().view(np.uint32), ring["reward"][want].astype(np.float32).view(np.uint32))
        assert np.array_equal(got.done.cpu().numpy(), ring["done"][want].astype(np.float32))
    batch = buf.sample(32)
    assert buf.draws == 2 and batch.obs.shape == (32, nbytes) and batch.obs.dtype == torch.float32
    buf.check_status()


# ------------------------------------------------------------------------------------------------------------ end to end

TRAIN = dict(movement_bonus=0.1, movement_bonus_power=1e-100, movement_bonus_period=4, as_penalty=True, exit_bonus=0.5,
             penalty_coef=0.3, ignore_reward_cells=False)
# (min_performance_fraction 0: the exits are open from the start, so an agent that walks to one leaves before the time limit)
E2E = dict(B=65, A=2, T=30, n=5, time_limit=9, view_shape=(7, 11), seed=12345, eps=0.3)


class _QModel(object):
    """Q-values with exact arithmetic (integer weights on a 0 / 1 observation, sums far below 2^24), the same on any device
    and in any summation order: obs [N,C,W,H] -> qvals [N,9].  An agent that sees an exit (channel 8 without the agent bit,
    channel 1) values the move towards the nearest one most, so that some agents leave their level while their partners
    stay; everybody else an action hashed from the observation.  Remembers what it returned."""

    def __init__(self, torch, obs_shape, device):
        g = torch.Generator(device="cpu").manual_seed(7)
        self.torch, self.seen = torch, []
        Cn, W, H = obs_shape
        self.w = torch.randint(-3, 4, (Cn * W * H,), generator=g).to(torch.float32).to(device)
        x = torch.arange(W, dtype=torch.int64).view(W, 1).expand(W, H) - W // 2
        y = torch.arange(H, dtype=torch.int64).view(1, H).expand(W, H) - H // 2
        flat = torch.arange(W * H, dtype=torch.int64).view(W, H)
        self.key = ((x.abs() + y.abs()) * 4096 + flat).to(device)       # nearest first, no ties
        self.dx, self.dy = x.reshape(-1).to(device), y.reshape(-1).to(device)

    def __call__(self, obs):
        torch = self.torch
        N = obs.shape[0]
        h = (obs.reshape(N, -1).to(torch.float32) * self.w).sum(dim=1)
        hashed = torch.remainder(h, 9.0).to(torch.int64)
        exits = (obs[:, 8] != 0) & (obs[:, 1] == 0)
        far = 1 << 40
        key = torch.where(exits, self.key, torch.full_like(self.key, far)).view(N, -1).min(dim=1).values
        seen = key < far
        cell = torch.where(seen, key % 4096, torch.zeros_like(key))
        dx, dy = self.dx[cell], self.dy[cell]
        sideways = (dy == 0) | ((dx != 0) & (hashed % 2 == 0))
        move = torch.where(sideways, torch.where(dx > 0, 2, 4), torch.where(dy > 0, 3, 1))
        q = torch.zeros((N, 9), dtype=torch.float32, device=obs.device)
        q[torch.arange(N, device=obs.device), torch.where(seen, move, hashed)] = 1.0
        self.seen.append(q.cpu().numpy())
        return q


class _Recorder(object):
    """Hands every step on to the buffer and keeps a host copy of it and of the runner's carried state after it."""

    def __init__(self, buf, runner, widen):
        self.buf, self.runner, self.widen, self.steps, self.state = buf, runner, widen, [], []

    def add(self, step):
        if self.widen:
            step = step._replace(rewards=step.rewards.double())
        self.steps.append(Step(*(getattr(step, f).cpu().numpy().copy() for f in Step._fields)))
        self.state.append((self.runner.active.cpu().numpy().copy(), self.runner.num_resets.cpu().numpy().copy(),
                           step.agent_ids[1].cpu().numpy().copy()))
        self.buf.add(step)


@pytest.mark.parametrize("wrapped", [False, True], ids=["game reward float32", "wrapped reward as float64"])
def test_multi_agent_dqn_runner_end_to_end(wrapped):
    """MultiAgentDQNRunner.collect on 65 envs x 2 agents of the 26x26 multi-agent levels, time limit 9, the uint8 policy
    row, n = 5, a ring of exactly 65 * 2 * 6 slots: ring, idx and fill equal the numpy restatement fed the recorded step
    stream; ``active`` / ``num_resets`` equal the restated carried state after every step; every action equals the masked
    draw's model on the Q-values the model returned, and the env was handed 0 for every agent that was gone.  (The
    multi-agent env's wrapped reward is float32 as well; the second run widens it, so that a float64 buffer is fed.)"""
    import torch
    from safelife_amd.levels import LevelPool
    from safelife_amd.multi_env import SafeLifeMultiAgentVectorEnv
    from safelife_amd.replay import MultiAgentReplayBuffer
    from safelife_amd.runner import MultiAgentDQNRunner
    B, A, T, n, eps, seed = (E2E[k] for k in ("B", "A", "T", "n", "eps", "seed"))
    levels = []
    for name in ("multi_asym1", "multi_build_coop", "multi_build_compete"):
        levels += util.levels_from_trace(util.load_trace(name))
    assert all(lv.board.shape == (26, 26) for lv in levels)
    pool = LevelPool(levels, counts_fn=_device_counts, n_agents=A, min_performance_fraction=0.0)
    env = SafeLifeMultiAgentVectorEnv(pool, B, first_level=np.arange(B) % len(levels), auto_reset=True,
                                      time_limit=E2E["time_limit"], view_shape=E2E["view_shape"],
                                      output_channels=tuple(range(12)) + (25, 26, 27), policy_layout="uint8", with_obs=False,
                                      **(dict(wrappers=TRAIN) if wrapped else {}))
    assert env.policy_tensor.dtype == torch.uint8
    obs_shape = tuple(env.policy_tensor.shape[2:])
    model = _QModel(torch, obs_shape, env.device)
    runner = MultiAgentDQNRunner(env, model, seed=seed, cast_obs=False)
    handed, env_step = [], env.step

    def logging_step(actions):
        handed.append(actions.cpu().numpy().copy())
        return env_step(actions)

    env.step = logging_step
    cap = B * A * (n + 1)
    buf = MultiAgentReplayBuffer(cap, B, A, multi_step=n, gamma=0.97, obs_shape=obs_shape, obs_dtype=torch.uint8,
                                 reward_dtype=torch.float64 if wrapped else torch.float32, device=env.device, seed=3)
    rec = _Recorder(buf, runner, wrapped)
    last = runner.collect(T, eps, rec)
    assert runner.num_steps == T * B and runner.draws == T and buf.steps_added == T and len(rec.steps) == len(handed) == T
    assert last.rewards.dtype == torch.float32 and last.actions.dtype == torch.int32 and last.active.dtype == torch.uint8
    assert last.obs.shape == (B, A) + obs_shape and last.next_obs is env.policy_tensor
    # the carried state, the draws, what the env was handed
    active, resets = np.ones((B, A), bool), np.zeros(B, np.int64)
    rep = mr.MultiReplay(cap, B, A, n, 0.97)
    gaps = reloads = agent_steps = 0
    for t, s in enumerate(rec.steps):
        on = s.active != 0
        assert np.array_equal(on, active), t
        assert np.array_equal(rec.state[t][2], resets), t               # agent ids: resets so far, before the step
        want = mr.eps_model_masked(model.seen[t], on, eps, seed, t).reshape(B, A)
        assert np.array_equal(s.actions, want) and np.array_equal(handed[t], want), t
        assert not handed[t][~on].any()
        assert s.done[~on].all()                                        # the env keeps reporting done for whoever left
        if t:
            assert np.array_equal(s.obs, rec.steps[t - 1].next_obs)
        flat, nxt = s.obs.reshape(B * A, -1), s.next_obs.reshape(B * A, -1)
        rep.add([r.tobytes() for r in flat], s.actions, s.rewards, s.done, [r.tobytes() for r in nxt], on)
        active, resets = mr.carried_state(active, resets, s.done)
        assert np.array_equal(rec.state[t][0] != 0, active) and np.array_equal(rec.state[t][1], resets), t
        gaps += int((~on).sum())
        reloads += int(s.done.astype(bool).all(axis=1).sum())
        agent_steps += int(on.sum())
    assert gaps >= 10 and reloads >= 10             # agents finished apart, envs reloaded
    assert (resets > 0).sum() >= 5
    assert int(runner.num_agent_steps.item()) == agent_steps
    assert s.rewards.dtype == (np.float64 if wrapped else np.float32)
    # the ring
    size = len(rep)
    assert int(buf.idx.item()) == rep.idx == agent_steps - rep.pending() and len(buf) == size
    assert rep.idx > cap                            # it wrapped
    assert buf.min_len() <= size
    assert np.array_equal(buf.fill.cpu().numpy(), rep.fill())
    obs = buf.obs.cpu().numpy().reshape(cap, -1)
    nxt = buf.next_obs.cpu().numpy().reshape(cap, -1)
    act, rew, done = buf.action.cpu().numpy(), buf.reward.cpu().numpy(), buf.done.cpu().numpy()
    for slot in range(size):
        o, a, r, no, d = rep.ring[slot]
        assert obs[slot].tobytes() == o and nxt[slot].tobytes() == no and act[slot] == a and done[slot] == d, slot
        assert bits64(rew[slot]) == bits64(r), slot
    assert int(buf.status.item()) == 0
    batch = buf.sample(32)
    buf.check_status()
    index = rr.sample_model(size, 32, 3, 0)
    assert np.array_equal(batch.obs.cpu().numpy().astype(np.uint8).reshape(32, -1), obs[index])
    assert np.array_equal(batch.action.cpu().numpy(), act[index].astype(np.int64))
