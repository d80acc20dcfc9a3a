"""Numpy twin of the servo surrogate's command process (csrc/servo_sim.hip: the commands-on instances, include/catppo.h
catppo_servo_commands; DESIGN section 9, "Commands").

``ServoCommandsTwin`` sits on top of the events twin and touches none of its parents.  The parents ask ``command(ep, k)``
for the command of a step and, with a scalar ``k``, for the first command of the next episode; this class answers both
from the stateful process of the header - the command and the time left of the input row, updated statement by statement
- and keeps the parents' answer when a fixed-command table or a schedule is attached.  The row gets the field
``cmd_state`` (four floats: time left | 0 0 0) behind everything else; float 15 of a trace row is the update's mark.  One
``np.float32`` operation per rounded kernel operation.  ``stats`` counts how often every rule fired.  Test infrastructure.
"""
from __future__ import annotations

import numpy as np

import servo_events_twin as ET
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T

F32 = np.float32
TAG_DRAW, TAG_TIME = 0x434D4444, 0x434D4454                # "CMDD" "CMDT"
DEADZONE, RANDOM_RESAMPLE, YAW_FLIP, STANDING = 1, 2, 4, 8
FLOATS = 16
#: word offsets of the block, restated here; the tests compare them with native.SERVO_COMMAND_WORDS
WORDS = {"flags": 0, "dz": 1, "p_still": 2, "p_move": 3, "ranges": 4, "rel_standing": 10, "T_lo": 11, "T_width": 12}
TRACE_COMMAND = 15
COUNTS = ("timed", "random_moving", "random_still", "deadzone", "yaw_flips", "episode_ends")


def block(flags, ranges, time, dz=0.0, p_still=0.0, p_move=0.0, rel_standing=0.0):
    """the 16 words from (a, b) pairs: ``ranges`` = three of x y wz, ``time`` = one; lo = f32(a), width = f32(b - a)"""
    w = np.zeros(FLOATS, F32)
    w.view(np.int32)[WORDS["flags"]] = int(flags)
    w[WORDS["dz"]], w[WORDS["p_still"]], w[WORDS["p_move"]], w[WORDS["rel_standing"]] = dz, p_still, p_move, rel_standing
    for i, (a, b) in enumerate(ranges):
        w[WORDS["ranges"] + 2 * i], w[WORDS["ranges"] + 2 * i + 1] = F32(a), F32(float(b) - float(a))
    w[WORDS["T_lo"]], w[WORDS["T_width"]] = F32(time[0]), F32(float(time[1]) - float(time[0]))
    return w


class ServoCommandsTwin(ET.ServoEventsTwin):
    def __init__(self, *args, commands=None, **kw):
        super().__init__(*args, **kw)
        self.off = dict(self.off)
        self.off["cmd_state"] = (self.F, 4)
        self.F += 4
        self.set_commands(commands)
        self.stats = dict(self.stats, **{k: 0 for k in COUNTS})
        self._now = None                                    # (command, time left, mark) of the call in flight
        self.mark = np.zeros(self.N, F32)

    def set_commands(self, words):
        w = np.ascontiguousarray(words, F32).copy()
        assert w.shape == (FLOATS,)
        self.cm = w
        self.cflags = int(w.view(np.int32)[WORDS["flags"]])

    def _generated(self):
        return self.fixed is None and self.schedule is None

    # ------------------------------------------------------------------ the header's draw / time / rules
    def _range(self, i):
        return self.cm[WORDS["ranges"] + 2 * i], self.cm[WORDS["ranges"] + 2 * i + 1]

    def draw(self, ep, third):
        """(c [N, 3], standing [N]) of counter {gid, ep, third, "CMDD"}"""
        u = self._uniform(self.gid, ep, third, TAG_DRAW)
        c = np.stack([self._sample(u[:, i], self._range(i)) for i in range(3)], 1)
        return c, u[:, 3] <= self.cm[WORDS["rel_standing"]]

    def time_block(self, ep, third):
        """(time sample [N], u word 2 [N], u word 3 [N]) of counter {gid, ep, third, "CMDT"}"""
        u = self._uniform(self.gid, ep, third, TAG_TIME)
        return self._sample(u[:, 0], (self.cm[WORDS["T_lo"]], self.cm[WORDS["T_width"]])), u[:, 2], u[:, 3]

    def deadzone(self, c):
        """(c after the rule, which envs it zeroed)"""
        if not self.cflags & DEADZONE:
            return c, np.zeros(self.N, bool)
        none = ~(np.abs(c) > self.cm[WORDS["dz"]]).any(1)
        return np.where(none[:, None], F32(0), c).astype(F32), none

    def first_command(self, ep):
        c, standing = self.draw(ep, 0)
        c, _ = self.deadzone(c)
        if self.cflags & STANDING:
            c = np.where(standing[:, None], F32(0), c).astype(F32)
        return c

    def first_time(self, ep):
        return self.time_block(ep, 0)[0]

    def update(self, c, tl, ep, t, live):
        """one update of the envs ``live`` (the others keep c, tl): (c, tl, mark); counts what fired"""
        cm, st = self.cm, self.stats
        assert (t >= 0).all() and (t < 2 ** 27).all()
        third = (t + 1) << 1
        sample, u_rs, u_yaw = self.time_block(ep, third)
        mark = np.zeros(self.N, F32)
        # 1. the timed resample
        tl = (tl - self.step_dt).astype(F32)
        timed = tl <= F32(0)
        c0, standing = self.draw(ep, third)
        if self.cflags & STANDING:
            c0 = np.where(standing[:, None], F32(0), c0).astype(F32)
        c = np.where(timed[:, None], c0, c).astype(F32)
        tl = np.where(timed, sample, tl).astype(F32)
        mark = np.where(timed, F32(1), mark)
        st["timed"] += int((timed & live).sum())
        # 2. the dead zone
        before = c
        c, zeroed = self.deadzone(c)
        st["deadzone"] += int((zeroed & live & (before != 0).any(1)).sum())
        # 3. the random resample
        if self.cflags & RANDOM_RESAMPLE:
            still = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) < cm[WORDS["dz"]]
            p = np.where(still, cm[WORDS["p_still"]], cm[WORDS["p_move"]]).astype(F32)
            hit = u_rs < p
            c1, _ = self.draw(ep, third | 1)
            c = np.where(hit[:, None], c1, c).astype(F32)
            tl = np.where(hit, self.time_block(ep, third | 1)[0], tl).astype(F32)
            mark = np.where(hit, F32(1), mark)
            st["random_still"] += int((hit & still & live).sum())
            st["random_moving"] += int((hit & ~still & live).sum())
        # 4. the yaw flip
        if self.cflags & YAW_FLIP:
            flip = u_yaw < cm[WORDS["p_move"]]
            c[:, 2] = np.where(flip, -c[:, 2], c[:, 2])
            mark = np.where(flip, mark + F32(2), mark).astype(F32)
            st["yaw_flips"] += int((flip & live).sum())
        return c, tl, mark

    # ------------------------------------------------------------------ what the parents ask
    def command(self, ep, k):
        if not self._generated():
            return super().command(ep, k)
        if np.isscalar(k):                                  # the post-reset observation: the next episode's first command
            return self.first_command(ep)
        return self._now[0].copy()

    def _write_state(self, out, tl):
        s = self._f(out, "cmd_state")
        s[:] = 0
        if self._generated():
            s[:, 0] = tl
        return out

    def initial(self, episode_length):
        zero = np.zeros(self.N, np.uint32)
        tl = np.zeros(self.N, F32)
        if self._generated():
            self._now, tl = (self.first_command(zero),), self.first_time(zero)
        return self._write_state(super().initial(episode_length), tl)

    def step(self, slab, action, reset, episode_length):
        f, n = self._f, self.N
        rst = np.asarray(reset).astype(bool)
        t = np.asarray(episode_length, np.int64)
        tl, mark = np.zeros(n, F32), np.zeros(n, F32)
        if self._generated():
            ep = f(slab, "servo")[:, 13].astype(np.uint32)
            c, tl, mark = self.update(f(slab, "command").astype(F32), f(slab, "cmd_state")[:, 0].astype(F32), ep, t, ~rst)
            # a step whose reset flag is set takes the first command as it stands and runs no update
            c = np.where(rst[:, None], self.first_command(ep), c).astype(F32)
            tl = np.where(rst, self.first_time(ep), tl).astype(F32)
            mark = np.where(rst, F32(0), mark).astype(F32)
            self._now = (c,)
        self.mark = mark
        slot = self.record[:, 0].astype(np.int64)
        out = super().step(slab, action, reset, episode_length)
        self.stats["episode_ends"] += int(((t + 1 >= self.max_len) | (f(out, "hard_reset")[:, 0] > 0)).sum())
        if self.trace is not None:
            for i in range(self.K):
                if 0 <= slot[i] < self.T:
                    self.trace[slot[i], i, TRACE_COMMAND] = mark[i]
        return self._write_state(out, tl)


def make_twin(cfg, n, commands, events=None, obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=25, **kw):
    return ServoCommandsTwin(n, OT.RAW, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, env_offset,
                             table=table, obs_table=obs_table, events=events, commands=commands, **kw)


def run_commands_twin(twin, actions, episode_length0, switch=None):
    """(slabs [steps + 1, N, F], marks [steps, N]); ``switch`` = (step index, words): the block is replaced before that step"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, marks = [slab], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_commands(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        marks.append(twin.mark.copy())
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs), np.stack(marks) if marks else np.zeros((0, twin.N), F32)
