"""
Multi-agent DQN replay restated in numpy: the masked rule of slhip_replay_add_masked written column by column the way the
reference's add_to_replay reads when it is handed the active agents only (training/dqn.py:110-134 over
training/base_algo.py:152-244), the carried state (who is active, how often an env has reloaded), and the EXACT host model
of the masked epsilon-greedy draw (slhip_sample_actions_eps_masked).  It builds on tests/replay_ref.py (the ring, the
window entries, the unmasked draw's model) and shares nothing with the kernels.  numpy only; nothing here loads the library.

    MultiReplay(capacity, B, A, n, gamma).add(obs, actions, rewards, done, next_obs, active)

takes the fields over the B * A COLUMNS (column b * A + a is agent a of env b), flat or shaped [B, A]; a column with
``active == 0`` is skipped: nothing it holds is looked at.
"""
import os

import numpy as np

from tests import replay_ref as rr


class MultiReplay(rr.Replay):
    def __init__(self, capacity, B, A, n, gamma):
        super().__init__(capacity, int(B) * int(A), n, gamma)
        self.num_envs, self.n_agents = int(B), int(A)

    def add(self, obs, actions, rewards, done, next_obs, active):
        rewards = np.asarray(rewards)
        assert rewards.dtype in (np.dtype(np.float32), np.dtype(np.float64))
        rewards, actions = rewards.reshape(-1), np.asarray(actions).reshape(-1)
        done, active = np.asarray(done).reshape(-1), np.asarray(active).reshape(-1)
        assert len(obs) == len(next_obs) == len(rewards) == len(actions) == len(done) == len(active) == self.B
        for c in range(self.B):
            if not active[c]:
                continue                                # the agent sat this step out: its window waits as it is
            win = self.windows[c]
            r = np.float64(rewards[c])
            d = bool(done[c])
            oldest = win.pop() if len(win) == self.n else None
            for k, entry in enumerate(win):
                entry[2] = np.float64(entry[2] + np.float64(r * self.G[k]))
            win.insert(0, [obs[c], int(actions[c]), r])
            if oldest is not None:
                self.push(oldest[0], oldest[1], oldest[2], obs[c], d)
            if d:
                for o, a, rew in win:
                    self.push(o, a, rew, next_obs[c], d)
                self.windows[c] = []
        self.steps += 1


def carried_state(active, resets, done):
    """The state after a step: ``active`` bool [B,A] and ``resets`` int64 [B] before it, ``done`` [B,A] the ENV's flags
    (1 for an agent that is gone).  Whoever is done leaves; an env with nobody left has reloaded: all its agents are back
    and its reset count goes up by one.  Returns new arrays."""
    now = np.array(active, bool) & ~np.asarray(done).astype(bool)
    over = ~now.any(axis=1)
    now[over] = True
    return now, np.array(resets, np.int64) + over


def min_len(capacity, B, A, n, steps_added):
    """MultiAgentReplayBuffer.min_len's bound."""
    return min(capacity, max(0, B * steps_added - B * A * n))


def eps_model_masked(qvals, active, epsilon, seed, counter, first_row=0):
    """What slhip_sample_actions_eps_masked writes, row e drawing as row first_row + e of the whole run: int32 [B].  Rows
    with active == 0 get 0 and their Q-values do not matter."""
    q = np.array(qvals, np.float32)
    on = np.asarray(active).reshape(-1) != 0
    q[~on] = 0.0
    actions, _ = rr.eps_model(q, epsilon, seed, counter, first_env=first_row)
    return np.where(on, actions, 0).astype(np.int32)


# ------------------------------------------------------------------------------------------------------ the fixture

_cases = None


def load_cases():
    """tests/golden/replay_multi_cases.npz (make_golden_replay_multi.py) as a list of dicts: n, B, A, T, columns,
    capacity, gamma, R / D / ACT / active [T,B,A], dump_steps and ``dumps`` -- three dicts with idx, the ring's columns
    (obs_c, obs_t, action, reward, next_c, next_t, done), the windows (fill [B*A]; w_reward, w_action, w_obs_t [n,B*A]) and
    resets [B].  Loaded once; nobody writes into it."""
    global _cases
    if _cases is None:
        out = []
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_multi_cases.npz")) as d:
            z = {k: d[k] for k in d.files}
        for i in range(len(z["n"])):
            n, B, A, T = int(z["n"][i]), int(z["B"][i]), int(z["A"][i]), int(z["T"][i])
            N = B * A
            so, ro = int(z["step_offsets"][i]), int(z["r_offsets"][i])
            c = dict(index=i, n=n, B=B, A=A, T=T, columns=N, capacity=int(z["capacity"][i]), gamma=float(z["gamma"][i]),
                     R=z["R64" if z["reward_f64"][i] else "R32"][ro:ro + T * N].reshape(T, B, A),
                     D=z["D"][so:so + T * N].reshape(T, B, A), ACT=z["ACT"][so:so + T * N].reshape(T, B, A),
                     active=z["active"][so:so + T * N].reshape(T, B, A),
                     dump_steps=[int(s) for s in z["dump_steps"][i]], dumps=[])
            for j in range(3):
                q = 3 * i + j
                e0, e1 = int(z["entry_offsets"][q]), int(z["entry_offsets"][q + 1])
                w0, wn0, r0 = int(z["win_offsets"][q]), int(z["winn_offsets"][q]), int(z["res_offsets"][q])
                dump = dict(idx=int(z["idx"][q]), fill=z["w_fill"][w0:w0 + N].astype(np.int32), resets=z["resets"][r0:r0 + B])
                for name in ("obs_c", "obs_t", "action", "reward", "next_c", "next_t", "done"):
                    dump[name] = z["e_" + name][e0:e1]
                for name in ("w_reward", "w_action", "w_obs_t"):
                    dump[name] = z[name][wn0:wn0 + n * N].reshape(n, N)
                c["dumps"].append(dump)
            for a in [c["R"], c["D"], c["ACT"], c["active"]] + [v for dmp in c["dumps"] for v in dmp.values()
                                                                if isinstance(v, np.ndarray)]:
                a.setflags(write=False)
            c["id"] = "n%d-T%d-B%dx%d-%s-g%g-cap%d" % (n, T, B, A, c["R"].dtype.name, c["gamma"], c["capacity"])
            out.append(c)
        _cases = out
    return _cases


def replay_case(case, make_obs=None):
    """Feed a golden case's step stream to ``MultiReplay``; yields (steps done, MultiReplay, active bool [B,A] for the NEXT
    step, resets [B]) after every step.  Observations are the tags (column, t) unless ``make_obs(column, t)`` builds
    something else.  The active mask handed over is the carried state restated here, not the fixture's."""
    n, B, A, T, N = case["n"], case["B"], case["A"], case["T"], case["columns"]
    make_obs = make_obs or (lambda c, t: (c, t))
    rep = MultiReplay(case["capacity"], B, A, n, case["gamma"])
    active, resets = np.ones((B, A), bool), np.zeros(B, np.int64)
    for t in range(T):
        obs = [make_obs(c, t) for c in range(N)]
        nxt = [make_obs(c, t + 1) for c in range(N)]
        rep.add(obs, case["ACT"][t], case["R"][t], case["D"][t], nxt, active)
        active, resets = carried_state(active, resets, case["D"][t])
        yield t + 1, rep, active, resets


def ring_columns(rep):
    """The ring of a tag-fed ``MultiReplay`` as the fixture's columns (slots [0, len))."""
    rows = rep.ring[:len(rep)]
    return dict(obs_c=np.array([r[0][0] for r in rows], np.int16), obs_t=np.array([r[0][1] for r in rows], np.int16),
                action=np.array([r[1] for r in rows], np.int32), reward=np.array([r[2] for r in rows], np.float64),
                next_c=np.array([r[3][0] for r in rows], np.int16), next_t=np.array([r[3][1] for r in rows], np.int16),
                done=np.array([r[4] for r in rows], np.uint8))
