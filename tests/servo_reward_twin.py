"""Numpy twin of the servo surrogate's reward terms (csrc/servo_sim.hip: ``reward_terms``, ``reward_rec``,
``reward_table``; DESIGN section 9, "Rewards").

``ServoRewardTwin`` sits on top of the trace / eval twin.  After the parent's ``step`` it recomputes the terms of the
table from the row the step just wrote, the input row and the action - every operand is a field of one of them, or one
kernel expression away from fields with the same fp32 operands (``ang`` from roll and pitch of both rows, ``a_prev`` from
the input row's observation) - and then overwrites the row's ``reward``.  The parents have read the built-in reward
before that, so the evaluation record and the trace keep it.  fp32 with the kernel's orders; the two exp kinds use an fp64
``exp`` rounded to fp32 (the correctly rounded value, against which the device's ``expf`` is allowed its error).  It keeps
the ``[N, 32]`` record.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_trace_twin as ST
import servo_twin as T

F32 = np.float32
REC_FLOATS = 32
KINDS = {"track_lin_vel_xy_exp": 1, "track_ang_vel_z_exp": 2, "track_lin_vel_xy_rational": 3, "track_ang_vel_z_rational": 4,
         "ang_vel_xy_l2": 5, "flat_orientation_l2": 6, "joint_torques_l2": 7, "joint_acc_l2": 8, "joint_vel_l2": 9,
         "joint_deviation_l1": 10, "action_rate_l2": 11, "action_l2": 12, "feet_air_time": 13, "base_height_l2": 14,
         "is_terminated": 15, "is_alive": 16}
HAA_MASK = 0b001001001001                                   # bits 0, 3, 6, 9

#: every kind but the two exp ones, distinct weights (some negative), an HAA-only mask on kind 10: (kind, mask, weight, param)
ALL_NON_EXP = [(3, 0, 1.0, 0.25), (4, 0, 0.5, 0.3), (5, 0, -0.05, 0.0), (6, 0, -1.25, 0.0), (7, 0xFFF, -1.0e-3, 0.0),
               (8, 0x0F0, -2.5e-7, 0.0), (9, 0xFFF, -2.0e-3, 0.0), (10, HAA_MASK, -0.1, 0.0), (11, 0, -0.01, 0.0),
               (12, 0, -0.005, 0.0), (13, 0, 0.75, 0.01), (14, 0, -3.0, 0.2), (15, 0, -20.0, 0.0), (16, 0, 0.125, 0.0)]

SEED, MAX_LEN, STEPS = 1276, 7, 50


def recipe(n):
    """the input recipe of the reward tests: (actions [50, n, 12] fp32, first episode lengths [n])"""
    rs = np.random.RandomState(3)
    actions = (rs.standard_normal((STEPS, n, 12)) * 2).astype(F32)
    ep0 = rs.randint(0, 7, n)
    return actions, ep0


def _pad16(x):
    out = np.zeros((x.shape[0], 16), F32)
    out[:, :x.shape[1]] = x
    return out


class ServoRewardTwin(ST.ServoTraceTwin):
    def __init__(self, *args, table=(), **kw):
        super().__init__(*args, **kw)
        self.table = [(int(k), int(m), F32(w), F32(p)) for k, m, w, p in table]
        assert len(self.table) <= 15
        self.reward_record = np.zeros((self.N, REC_FLOATS), F32)
        self.values = None                                  # [N, T] fp32: value_k of the last step
        self.stats = dict(falls=0, timeouts=0, touch_air=0)

    def initial(self, episode_length):
        self.reward_record = np.zeros((self.N, REC_FLOATS), F32)        # an init launch zeroes the whole record
        return super().initial(episode_length)

    def raw_terms(self, slab, out, action, reset, episode_length):
        """[N, T] fp32: raw_k of every table entry, from the written row, the input row and the action"""
        f, n, p = self._f, self.N, self.p
        rst = np.asarray(reset).astype(bool)
        xin, x = f(slab, "servo"), f(out, "servo")
        cmd, v = f(out, "command"), x[:, 0:3]
        ex, ey, ew = cmd[:, 0] - v[:, 0], cmd[:, 1] - v[:, 1], cmd[:, 2] - v[:, 2]
        roll0, pitch0 = np.where(rst, F32(0), xin[:, 3]).astype(F32), np.where(rst, F32(0), xin[:, 4]).astype(F32)
        ang0, ang1 = (x[:, 3] - roll0) / self.step_dt, (x[:, 4] - pitch0) / self.step_dt
        g = f(out, "projected_gravity_b")
        tau_w, acc, qd = _pad16(f(out, "applied_torque")), _pad16(f(out, "joint_acc")), _pad16(f(out, "joint_vel"))
        dq = _pad16((f(out, "joint_pos") - T.DEFAULT_JOINT_POS).astype(F32))
        a = _pad16(np.asarray(action, F32))
        a_prev = np.zeros((n, 16), F32)
        if self.D >= 45:
            a_prev[:, :12] = np.where(rst[:, None], F32(0), f(slab, "obs")[:, 33:45])
        da = a - a_prev
        last_air = f(out, "last_air_time")[:, T.FOOT_BODY]
        touch = (f(out, "first_contact")[:, T.FOOT_BODY] > 0).astype(F32)
        z = f(out, "root_pos_w")[:, 2]
        fallen = f(out, "hard_reset")[:, 0] > 0
        moving = (np.sqrt(cmd[:, 0] * cmd[:, 0] + cmd[:, 1] * cmd[:, 1]) > F32(0.1)).astype(F32)
        one, zero = F32(1), F32(0)
        lanes = np.arange(16)
        raws = []
        for kind, mask, _, param in self.table:
            m = ((mask >> lanes) & 1).astype(F32)[None, :]
            if kind == 1:
                raw = np.exp((zero - (ex * ex + ey * ey) / param).astype(np.float64)).astype(F32)
            elif kind == 2:
                raw = np.exp((zero - (ew * ew) / param).astype(np.float64)).astype(F32)
            elif kind == 3:
                raw = one / (one + (ex * ex + ey * ey) / param)
            elif kind == 4:
                raw = one / (one + (ew * ew) / param)
            elif kind == 5:
                raw = ang0 * ang0 + ang1 * ang1
            elif kind == 6:
                raw = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]
            elif kind == 7:
                raw = T.tree16(m * (tau_w * tau_w))
            elif kind == 8:
                raw = T.tree16(m * (acc * acc))
            elif kind == 9:
                raw = T.tree16(m * (qd * qd))
            elif kind == 10:
                raw = T.tree16(m * np.abs(dq))
            elif kind == 11:
                raw = T.tree16(da * da)
            elif kind == 12:
                raw = T.tree16(a * a)
            elif kind == 13:
                raw = T.tree4((last_air - param) * touch) * moving
            elif kind == 14:
                raw = (z - param) * (z - param)
            elif kind == 15:
                raw = np.where(fallen, one, zero)
            elif kind == 16:
                raw = np.where(fallen, zero, one)
            else:
                raise ValueError(kind)
            raws.append(np.asarray(raw, F32))
        t = np.asarray(episode_length, np.int64)
        timeout = (t + 1 >= self.max_len) & ~fallen
        self.stats["falls"] += int(fallen.sum())
        self.stats["timeouts"] += int(timeout.sum())
        self.stats["touch_air"] += int(((touch > 0) & (last_air > 0)).sum())
        return np.stack(raws, 1) if raws else np.zeros((n, 0), F32), (t + 1 >= self.max_len) | fallen

    def step(self, slab, action, reset, episode_length):
        out = super().step(slab, action, reset, episode_length)
        if not self.table:
            return out
        raw, ends = self.raw_terms(slab, out, action, reset, episode_length)
        n, nt = self.N, len(self.table)
        reward = np.zeros(n, F32)
        values = np.zeros((n, nt), F32)
        for k, (_, _, weight, _) in enumerate(self.table):
            values[:, k] = (raw[:, k] * weight) * self.step_dt           # two rounded fp32 multiplies
            reward = reward + values[:, k]                               # from 0.f, table order, unfused
        self.values = values
        rec = self.reward_record
        v16 = np.zeros((n, 16), F32)
        v16[:, :nt] = values
        s = rec[:, :16] + v16                                            # lane 15: 0 + 0
        add = s.copy()
        add[:, 15] = F32(1)                                              # float 31 counts the ended episodes
        new = rec.copy()
        new[:, :16] = np.where(ends[:, None], F32(0), s)
        new[:, 16:] = np.where(ends[:, None], rec[:, 16:] + add, rec[:, 16:])
        self.reward_record = new.astype(F32)
        self._f(out, "reward")[:, 0] = reward
        return out


def make_twin(cfg, n, table, env_offset=0, obs_dim=None, seed=SEED, max_len=MAX_LEN, **kw):
    """the twin of a device simulator built from env cfg ``cfg`` (its servo constants, dt, decimation)"""
    return ServoRewardTwin(n, int(cfg.synthetic.obs_dim if obs_dim is None else obs_dim), T.params_from_cfg(cfg.synthetic),
                           seed, max_len, cfg.sim.dt, cfg.decimation, env_offset, table=table, **kw)


def run_reward_twin(twin: ServoRewardTwin, actions, episode_length0):
    """(slabs [steps + 1, N, F], reward record [N, 32] after the last step, per-step values [steps, N, T])"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, values = [slab], []
    for a in actions:
        slab = twin.step(slab, a, reset, ep_len)
        values.append(twin.values.copy() if twin.values is not None else np.zeros((twin.N, 0), F32))
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs), twin.reward_record.copy(), np.stack(values)


def recount_record(twin, slabs, values, episode_length0):
    """the record by a plain per-env loop over the slabs and the per-step values: running sums, ended sums, count"""
    n, nt = twin.N, values.shape[2]
    o = twin.off["hard_reset"][0]
    rec = np.zeros((n, REC_FLOATS), F32)
    for i in range(n):
        t = int(episode_length0[i])
        run = [F32(0)] * nt
        done = [F32(0)] * nt
        count = F32(0)
        for s in range(1, len(slabs)):
            run = [F32(run[k] + values[s - 1, i, k]) for k in range(nt)]
            t += 1
            if slabs[s, i, o] > 0.5 or t >= twin.max_len:
                done = [F32(done[k] + run[k]) for k in range(nt)]
                run = [F32(0)] * nt
                count = F32(count + F32(1))
                t = 0
        rec[i, :nt], rec[i, 16:16 + nt], rec[i, 31] = run, done, count
    return rec
