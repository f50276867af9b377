"""Early episode ending (include/mcr.h: mcr_set_end_rules; csrc/k_endrules.h) restated on the CPU oracle: the counters as plain Python on the
oracle's state, and a wrapper round `OracleEnv` — TimeLimit(env) with the end rules on top — whose every output the device must reproduce bit
for bit, the ONE ENV STEP OF LAG between "the rule is met" and "the episode ends" included.  No GPU, no package import."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
END_IDLE, END_OFFROAD = 1, 2
MODES = ("all", "any")


def _sat_inc(v):
    return v if v == INT32_MAX else v + 1


class EndRules:
    """One env's counters: `counters` = [idle, offroad, tvc_sum, 0] (int32), `armed` (0..3).  The state it reads off an oracle `o`: the sum
    of the counted cars' tile_visited_count and, per counted car, "no wheel has a tile under it" (every on_road bit 0)."""

    def __init__(self, N, patience=0, offroad=0, mode="all", agents=None, end_reward=0.0):
        assert mode in MODES and patience >= 0 and offroad >= 0
        self.N, self.P, self.G, self.mode, self.end_reward = N, int(patience), int(offroad), mode, float(end_reward)
        self.agents = tuple(range(N)) if agents is None else tuple(sorted(set(int(a) for a in agents)))
        assert self.agents and 0 <= self.agents[0] and self.agents[-1] < N
        self.counters = np.zeros(4, np.int32)
        self.armed = 0

    # ---- what the rules read
    def read(self, o):
        """(s, cond) of oracle env `o`"""
        tvc = o.env_state()["tile_visited_count"]
        on = o.state()["on_road"]
        return self.read_arrays(tvc, on)

    def read_arrays(self, tvc, on_road):
        """the same from tile_visited_count [N] and on_road [N, 4]"""
        s = int(np.array([sum(int(tvc[a]) for a in self.agents) & 0xffffffff], np.uint32).view(np.int32)[0])      # (u32 wrapping, read as int32)
        off = [not np.asarray(on_road[a]).any() for a in self.agents]
        return s, (all(off) if self.mode == "all" else any(off))

    def armed_of(self, idle, offroad):
        return (END_IDLE if self.P > 0 and idle >= self.P else 0) | (END_OFFROAD if self.G > 0 and offroad >= self.G else 0)

    # ---- the three transitions of a LIVE env (an env that is not live keeps its counters; its armed word is 0)
    def first_state(self, s):
        """the first state of an episode (the env record's steps == 0)"""
        self.counters[:] = (0, 0, s, 0)
        self.armed = 0

    def advance(self, s, cond):
        """behind an env step taken with actions that did not start a new episode"""
        idle, offroad, tvc_sum, _ = (int(v) for v in self.counters)
        idle = 0 if s != tvc_sum else _sat_inc(idle)
        offroad = _sat_inc(offroad) if cond else 0
        self.counters[:] = (idle, offroad, s, 0)
        self.armed = self.armed_of(idle, offroad)

    def settle(self, steps, s):
        """behind a reset / restore / clone: a first state starts over, any other keeps its counters and has `armed` recomputed"""
        if steps == 0:
            self.first_state(s)
        else:
            self.armed = self.armed_of(int(self.counters[0]), int(self.counters[1]))

    def not_live(self):
        self.armed = 0

    # ---- the armed step
    def end(self, rew, done, trunc):
        """what the env step an env ENTERED with `self.armed` makes of the reference's (rew [N] f64, done, truncated — TimeLimit applied):
        (rew, done, truncated, end_reason)"""
        reason = self.armed
        if reason:
            trunc = not done
            done = True
            rew = rew + np.float64(self.end_reward)          # one f64 add per car
        return rew, done, trunc, reason


class EndRulesEnv:
    """EndRules(TimeLimit(OracleEnv)): reset(ep) / step(action) -> (obs, reward [N], done, info) with info = truncated, end_reason and — at
    done — episode_return [N], episode_length.  It does not reset itself: stepping past an ending goes on counting (auto_reset=False)."""

    def __init__(self, o, max_steps=0, **rules):
        self.o, self.max_steps = o, int(max_steps)
        self.rules = EndRules(o.N, **rules)
        self.steps = 0
        self.ret = np.zeros(o.N)

    def reset(self, ep=None, render=False):
        obs = self.o.reset(ep, render=render)
        self.steps = 0
        self.ret = np.zeros(self.o.N)
        self.rules.first_state(self.rules.read(self.o)[0])
        return obs

    def step(self, action, render=False):
        assert action is not None, "the action-less step counts nothing and ends nothing: step the oracle itself"
        obs, rew, done, _ = self.o.step(action, render=render)
        self.steps += 1
        trunc = False
        if self.max_steps > 0 and self.steps >= self.max_steps:
            trunc = not done
            done = True
        rew, done, trunc, reason = self.rules.end(rew, done, trunc)
        self.ret = self.ret + rew
        self.rules.advance(*self.rules.read(self.o))
        info = dict(truncated=trunc, end_reason=reason)
        if done:
            info.update(episode_return=self.ret.copy(), episode_length=self.steps)
        return obs, rew, done, info
