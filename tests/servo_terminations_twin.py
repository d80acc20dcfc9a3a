"""Numpy twin of the servo surrogate's termination terms (csrc/servo_sim.hip: the terminations-on instances,
include/catppo.h catppo_servo_terminations; DESIGN section 9, "Terminations").

``ServoTerminationsTwin`` sits on top of the commands twin, ``ServoTerminationsPlainTwin`` on top of the events twin (a
simulator without a command block); both touch none of their parents.  The parents decide "did this step end its episode"
with one expression, ``tilt2 > tilt_max * tilt_max``, and read it back from the row's ``hard_reset`` everywhere else, so
the block is restated in two passes over the parents' step:

1. a throw-away copy of the twin steps once; the state it writes (joints, tilt, height, forces and their history) does not
   depend on how the episode ends, and the termination terms are evaluated on it, statement by statement as in the header;
2. the twin itself steps with ``tilt_max`` replaced by a stand-in whose square is below every ``tilt2`` for the envs the
   table terminates and above every ``tilt2`` for the others: the parents' flag *is* ``terminated`` in this pass, in
   ``ends``, ``hard_reset``, reward kinds 15 / 16, the evaluation record and the trace.

What the parents then get wrong is the written projected gravity, whose roll-over override stays tied to the model's own
flag: it is put right on the row and in the raw observation (before the reward terms read it), and the policy observation
is recomputed.  The row gets the field ``term_state`` (fired terms | 0 0 0) behind everything else, and the twin keeps the
``[N, 16]`` record.  One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import copy

import numpy as np

import servo_commands_twin as CT
import servo_events_twin as ET
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T

F32 = np.float32
REC_FLOATS, MAX_TERMS = 16, 15
KINDS = {"time_out": 1, "illegal_contact": 2, "upside_down": 3, "bad_orientation": 4, "root_height_below_minimum": 5,
         "joint_pos_out_of_manual_limit": 6, "joint_vel_out_of_manual_limit": 7, "rolled_over": 8}


class _Verdict:
    """stands where ``tilt_max`` stands in the parents' ``tilt2 > tilt_max * tilt_max``: its square is -1 for the envs that
    terminate (every tilt2 >= 0 is above it) and +inf for the others"""

    def __init__(self, terminated):
        self.square = np.where(terminated, F32(-1), F32(np.inf)).astype(F32)

    def __mul__(self, other):
        assert other is self
        return self.square


class _Terminations:
    def __init__(self, *args, terminations=(), **kw):
        super().__init__(*args, **kw)
        self.off = dict(self.off)
        self.off["term_state"] = (self.F, 4)
        self.F += 4
        self.set_terminations(terminations)
        self.term_record = np.zeros((self.N, REC_FLOATS), F32)
        self.bits = np.zeros(self.N, np.uint32)              # the fired terms of the last step
        self.stats = dict(self.stats, ended_by_time_out=0, ended_by_termination=0)
        self._fix = None

    def set_terminations(self, entries):
        self.terms = [(int(k), int(m), F32(p0), F32(p1)) for k, m, p0, p1 in entries]
        assert 1 <= len(self.terms) <= MAX_TERMS

    # ------------------------------------------------------------------ the header's rules
    def fired(self, out, t):
        """(bits [N] uint32, terminated [N], model's flag [N], g before the override [N, 3]) from the written state"""
        f, p = self._f, self.p
        q, qd, z = f(out, "joint_pos"), f(out, "joint_vel"), f(out, "root_pos_w")[:, 2]
        roll, pitch = f(out, "servo")[:, 3], f(out, "servo")[:, 4]
        tilt2 = roll * roll + pitch * pitch
        rolled = tilt2 > p["tilt_max"] * p["tilt_max"]
        nrm = np.sqrt(tilt2 + F32(1))
        g = np.stack([(F32(0) - pitch) / nrm, roll / nrm, F32(-1) / nrm], 1).astype(F32)
        force = f(out, "forces").reshape(self.N, T.H, T.B, 3)          # slot 0: this step; slot h: the input row's slot h - 1
        norm = np.sqrt((force[..., 0] * force[..., 0] + force[..., 1] * force[..., 1]) + force[..., 2] * force[..., 2])
        bits = np.zeros(self.N, np.uint32)
        terminated = np.zeros(self.N, bool)
        for k, (kind, mask, p0, p1) in enumerate(self.terms):
            joints = ((mask >> np.arange(T.J)) & 1).astype(bool)
            bodies = ((mask >> np.arange(T.B)) & 1).astype(bool)
            if kind == 1:
                fire = t + 1 >= self.max_len
            elif kind == 2:
                fire = (norm[:, :, bodies] > p0).any((1, 2))
            elif kind == 3:
                fire = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) > p0
            elif kind == 4:
                fire = (F32(0) - g[:, 2]) < p0
            elif kind == 5:
                fire = z < p0
            elif kind == 6:
                fire = ((q < p0) | (q > p1))[:, joints].any(1)
            elif kind == 7:
                fire = (np.abs(qd) > p0)[:, joints].any(1)
            elif kind == 8:
                fire = rolled
            else:
                fire = np.zeros(self.N, bool)                # an unknown kind never fires
            bits |= (fire.astype(np.uint32) << np.uint32(k))
            if kind != 1:
                terminated |= fire
        return bits, terminated, rolled, g

    # ------------------------------------------------------------------ rows
    def _put_gravity(self, out):
        if self._fix is None:                               # pass 1: the probe's gravity is not looked at
            return
        grav, ends = self._fix
        self._f(out, "projected_gravity_b")[:] = grav
        obs = self._f(out, "obs")
        obs[:, 3:6] = np.where(ends[:, None], np.array([0, 0, -1], F32), grav)

    def raw_terms(self, slab, out, action, reset, episode_length):
        """the reward terms read the written gravity: put it right before they do"""
        self._put_gravity(out)
        return super().raw_terms(slab, out, action, reset, episode_length)

    def initial(self, episode_length):
        self.term_record = np.zeros((self.N, REC_FLOATS), F32)          # an init launch zeroes the record
        self.bits = np.zeros(self.N, np.uint32)
        slab = super().initial(episode_length)
        self._f(slab, "term_state")[:] = 0
        return slab

    def step(self, slab, action, reset, episode_length):
        t = np.asarray(episode_length, np.int64)
        # ---- pass 1: the state this step writes, on a copy; the terms on it
        probe = copy.deepcopy(self)
        probe._fix = None
        state = super(_Terminations, probe).step(np.array(slab, F32, copy=True), action, reset, t.copy())
        bits, terminated, rolled, g = self.fired(state, t)
        ends = (t + 1 >= self.max_len) | terminated
        self._fix = (np.where(rolled[:, None], np.array([0, 0, 1], F32), g).astype(F32), ends)
        # ---- pass 2: the parents with `terminated` where their flag stands
        tilt_max = self.p["tilt_max"]
        self.p["tilt_max"] = _Verdict(terminated)
        try:
            out = super().step(slab, action, reset, episode_length)
        finally:
            self.p["tilt_max"] = tilt_max
        assert ((self._f(out, "hard_reset")[:, 0] > 0) == terminated).all()
        self._put_gravity(out)
        if getattr(self, "has_policy", False):
            self._finish(out, *self.key_of(out, t))
        # ---- term_state and the record
        s = self._f(out, "term_state")
        s[:] = 0
        s[:, 0] = bits.astype(F32)
        lanes = np.arange(REC_FLOATS)
        add = ((bits[:, None] >> lanes[None, :].astype(np.uint32)) & 1).astype(F32)
        add[:, 15] = F32(1)
        self.term_record = np.where(ends[:, None], self.term_record + add, self.term_record).astype(F32)
        self.bits = bits
        self.stats["ended_by_termination"] += int(terminated.sum())
        self.stats["ended_by_time_out"] += int((ends & ~terminated).sum())
        return out


class ServoTerminationsTwin(_Terminations, CT.ServoCommandsTwin):
    """terminations on top of the commands twin"""


class ServoTerminationsPlainTwin(_Terminations, ET.ServoEventsTwin):
    """terminations on top of the events twin: a simulator without a command block"""


def make_twin(cfg, n, terminations, commands=None, events=None, obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=25,
              **kw):
    """``commands`` None: the twin of a simulator built without the command descriptor"""
    args = (n, OT.RAW, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if commands is None:
        return ServoTerminationsPlainTwin(*args, table=table, obs_table=obs_table, events=events, terminations=terminations, **kw)
    return ServoTerminationsTwin(*args, table=table, obs_table=obs_table, events=events, commands=commands,
                                 terminations=terminations, **kw)


def run_terminations_twin(twin, actions, episode_length0, switch=None):
    """(slabs [steps + 1, N, F], bits [steps, N]); ``switch`` = (step index, entries): the table is replaced before that step"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, bits = [slab], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_terminations(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        bits.append(twin.bits.copy())
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs), np.stack(bits) if bits else np.zeros((0, twin.N), np.uint32)
