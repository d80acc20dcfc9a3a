"""Numpy twin of the servo surrogate's joint action terms (csrc/servo_sim_kernel.h: the actions-on instances,
include/catppo.h catppo_servo_actions; DESIGN section 9, "Actions").

The only place the action enters the model is the substep loop of ``servo_twin.ServoTwin.step``, which is one monolithic
function, so ``_ServoLoop`` restates that function with the loop's torque taken from the action table and nothing else
changed.  It subclasses ``ServoTwin`` and is listed last among the bases of the twins below, so that it lies right before
``ServoTwin`` in their method resolution order: every parent (terminations, commands, events, observations, rewards,
trace, evaluation record) runs as it is and ends up in the restated step.  None of the parents is edited.

The parents know the action as twelve columns (the last-action block of the observation, the trace's floats 60..71, reward
kinds 11 and 12); the twins below hand them the raw action by column, zero past the width A, which is what the header says
those places hold.  One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T

F32 = np.float32
KINDS = {"none": 0, "joint_position": 1, "relative_joint_position": 2, "joint_velocity": 3, "joint_effort": 4}


def identity_entries(action_scale):
    """the block that must change nothing: column j drives joint j as a position target def + scale * a, no clip"""
    return [(j, 1, F32(action_scale), T.DEFAULT_JOINT_POS[j], None) for j in range(T.J)]


class _ServoLoop(T.ServoTwin):
    """``ServoTwin.step`` with the servo torque of the action table; ``action`` is the raw action by column, [N, 12]"""

    def set_actions(self, entries, width):
        """``entries``: 12 ``(col, kind, scale, offset, clip or None)``, one per simulator joint"""
        assert len(entries) == T.J and 1 <= int(width) <= T.J
        self.A = int(width)
        self.act_col = np.array([e[0] for e in entries], np.int64)
        self.act_kind = np.array([e[1] for e in entries], np.int64)
        self.act_scale = np.array([e[2] for e in entries], F32)
        self.act_offset = np.array([e[3] for e in entries], F32)
        self.act_clip = np.array([e[4] is not None for e in entries], bool)
        self.act_lo = np.array([0 if e[4] is None else e[4][0] for e in entries], F32)
        self.act_hi = np.array([0 if e[4] is None else e[4][1] for e in entries], F32)
        self.act_stats = None

    def processed(self, action):
        """[N, 12] fp32: the processed action of every joint (whatever its kind; kind 0 does not read it)"""
        col = np.clip(self.act_col, 0, self.A - 1)                       # the kernel's clamp
        raw = np.asarray(action, F32)[:, col]
        p = raw * self.act_scale + self.act_offset                       # a rounded product, then a rounded sum
        lo = np.where(p < self.act_lo, self.act_lo, p)
        hi = np.where(lo > self.act_hi, self.act_hi, lo)
        return np.where(self.act_clip, hi, p).astype(F32), p.astype(F32)

    def step(self, slab, action, reset, episode_length):
        n, p, f = self.N, self.p, self._f
        J, H, B, FOOT_BODY, DEFAULT_JOINT_POS = T.J, T.H, T.B, T.FOOT_BODY, T.DEFAULT_JOINT_POS
        action = np.asarray(action, F32)
        assert action.shape == (n, J) and not action[:, self.A:].any()
        reset = np.asarray(reset).astype(bool)
        t = np.asarray(episode_length, np.int64)
        x_in = f(slab, "servo")
        ep = x_in[:, 13].astype(np.uint32)
        r1 = reset[:, None]
        # ---- the state this step starts from: the row, or the first state of episode `ep` re-derived from the counter
        q = np.where(r1, self.init_q(ep), f(slab, "joint_pos")).astype(F32)
        qd = np.where(r1, F32(0), f(slab, "joint_vel")).astype(F32)
        v = np.where(r1, F32(0), x_in[:, 0:3]).astype(F32)
        tilt = np.where(r1, F32(0), x_in[:, 3:5]).astype(F32)
        air = np.where(r1, F32(0), x_in[:, 5:9]).astype(F32)
        con_prev = np.where(r1, F32(1), x_in[:, 9:13]).astype(F32)
        root = np.where(r1, np.array([0, 0, p["stand_height"]], F32), f(slab, "root_pos_w")).astype(F32)
        last_air = np.where(r1, F32(0), f(slab, "last_air_time")[:, FOOT_BODY]).astype(F32)
        hist = np.where(r1, F32(0), f(slab, "forces")).astype(F32).reshape(n, H, B, 3)
        cmd = self.command(ep, t // p["resample_steps"])
        # ---- joints: `decimation` substeps of the clamped servo of the joint's action term, semi-implicit Euler
        pa, unclipped = self.processed(action)
        kind = self.act_kind[None, :]
        tau_w = np.zeros((n, J), F32)
        clamped = np.zeros((n, J), bool)
        free = np.zeros((n, J), bool)
        for _ in range(self.dec):
            tgt = np.where(kind == 1, pa, np.where(kind == 2, pa + q, DEFAULT_JOINT_POS)).astype(F32)
            pd = p["kp"] * (tgt - q) - p["kd"] * qd
            vel = p["kd"] * (pa - qd)
            tau0 = np.where(kind == 3, vel, np.where(kind == 4, pa, pd)).astype(F32)
            tau = np.minimum(np.maximum(tau0, -p["tau_max"]), p["tau_max"])
            clamped |= tau != tau0
            free |= tau == tau0
            qdd = tau / p["inertia"]
            qd = qd + qdd * self.dt
            q = q + qd * self.dt
            tau_w = np.where(np.abs(tau) > np.abs(tau_w), tau, tau_w)       # the substep of largest |tau| is reported
        # what the liveness recipe counts: per joint, the joint-steps whose clip bounds bound and whose torque clamp was reached
        self.act_stats = dict(below=(unclipped < self.act_lo) & self.act_clip, above=(unclipped > self.act_hi) & self.act_clip,
                              clamped=clamped, free=free)
        acc_w = tau_w / p["inertia"]
        dq = (q - DEFAULT_JOINT_POS).astype(F32)
        # ---- base: five fixed-order joint reductions, first-order lags
        dq16 = np.zeros((n, 16), F32)
        dq16[:, :J] = dq
        red = [T.tree16(self.G[k] * dq16) for k in range(5)]
        v_new = np.stack([v[:, k] + p["vel_alpha"] * (red[k] - v[:, k]) for k in range(3)], 1).astype(F32)
        roll = tilt[:, 0] + p["tilt_beta"] * (red[3] - tilt[:, 0])
        pitch = tilt[:, 1] + p["tilt_beta"] * (red[4] - tilt[:, 1])
        ang = np.stack([(roll - tilt[:, 0]) / self.step_dt, (pitch - tilt[:, 1]) / self.step_dt, v_new[:, 2]], 1)
        tilt2 = roll * roll + pitch * pitch
        fallen = tilt2 > p["tilt_max"] * p["tilt_max"]
        nrm = np.sqrt(tilt2 + F32(1))
        grav = np.stack([(F32(0) - pitch) / nrm, roll / nrm, F32(-1) / nrm], 1)
        grav = np.where(fallen[:, None], np.array([0, 0, 1], F32), grav).astype(F32)
        # ---- feet, height, contact forces
        knee, knee_v, hfe = dq[:, 2::3], qd[:, 2::3], dq[:, 1::3]
        con = ((F32(0) - p["foot_clearance"] * knee) < p["contact_threshold"]).astype(F32)
        ncon = T.tree4(con)
        zleg = p["stand_height"] - p["height_drop"] * np.abs(hfe)
        nsafe = np.maximum(ncon, F32(1))
        z = np.where(ncon > 0, T.tree4(con * zleg) / nsafe, p["floor_height"]).astype(F32)
        touch = (con > 0) & ~(con_prev > 0)
        fz = np.where(con > 0, (p["weight"] / nsafe)[:, None] + np.where(touch, p["impact_gain"] * np.abs(knee_v), F32(0)),
                      F32(0)).astype(F32)
        last_air = np.where(touch, air, last_air).astype(F32)
        air = np.where(con > 0, F32(0), air + self.step_dt).astype(F32)
        fbase = np.where(z < p["min_height"], p["base_stiffness"] * (p["min_height"] - z), F32(0)).astype(F32)
        root = np.stack([root[:, 0] + v_new[:, 0] * self.step_dt, root[:, 1] + v_new[:, 1] * self.step_dt, z], 1)
        # ---- reward: rational stand-ins for the two exp tracking rewards
        ex, ey, ew = cmd[:, 0] - v_new[:, 0], cmd[:, 1] - v_new[:, 1], cmd[:, 2] - v_new[:, 2]
        s = p["reward_scale"]
        reward = F32(1) / (F32(1) + (ex * ex + ey * ey) / s) + F32(0.5) / (F32(1) + (ew * ew) / s)
        # ---- does this step end the episode?  Then `obs` already shows the first state of the next one.
        ends = (t + 1 >= self.max_len) | fallen
        ep_out = (ep + ends.astype(np.uint32)).astype(np.uint32)
        q_next = self.init_q(ep_out)
        cmd_next = self.command(ep_out, 0)
        z3, z12 = np.zeros((n, 3), F32), np.zeros((n, 12), F32)
        obs_run = self._obs(ang, grav, cmd, dq, qd, action)
        obs_new = self._obs(z3, np.tile(np.array([0, 0, -1], F32), (n, 1)), cmd_next, q_next - DEFAULT_JOINT_POS, z12, z12)
        # ---- the next row
        out = np.zeros((n, self.F), F32)
        f(out, "joint_pos")[:], f(out, "joint_vel")[:] = q, qd
        f(out, "joint_acc")[:], f(out, "applied_torque")[:] = acc_w, tau_w
        f(out, "projected_gravity_b")[:], f(out, "root_pos_w")[:], f(out, "command")[:] = grav, root, cmd
        f(out, "last_air_time")[:, FOOT_BODY] = last_air
        f(out, "first_contact")[:, FOOT_BODY] = touch.astype(F32)
        hist_out = np.zeros((n, H, B, 3), F32)
        hist_out[:, 1:] = hist[:, :-1]
        hist_out[:, 0, FOOT_BODY, 2] = fz
        hist_out[:, 0, 0, 2] = fbase
        f(out, "forces")[:] = hist_out.reshape(n, -1)
        f(out, "reward")[:, 0] = reward
        f(out, "hard_reset")[:, 0] = fallen.astype(F32)
        f(out, "obs")[:] = np.where(ends[:, None], obs_new, obs_run)
        x = f(out, "servo")
        x[:, 0:3], x[:, 3], x[:, 4], x[:, 5:9], x[:, 9:13], x[:, 13] = v_new, roll, pitch, air, con, ep_out.astype(F32)
        return out


class _Actions:
    """the top of the chain: takes the action [N, A] and hands the parents the raw action by column, zero past A"""

    def __init__(self, *args, actions=None, width=T.J, **kw):
        super().__init__(*args, **kw)
        self.set_actions(actions if actions is not None else identity_entries(self.p["action_scale"]), width)
        self.live = None

    def step(self, slab, action, reset, episode_length):
        action = np.asarray(action, F32)
        assert action.shape == (self.N, self.A)
        a12 = np.zeros((self.N, T.J), F32)
        a12[:, :self.A] = action
        out = super().step(slab, a12, reset, episode_length)
        self.live = self.act_stats
        return out


class ServoActionsTwin(_Actions, RT.ServoRewardTwin, _ServoLoop):
    """actions on the simulator without further descriptors (evaluation record, trace and reward table as the parents take them)"""


class ServoActionsTerminationsTwin(_Actions, TT.ServoTerminationsTwin, _ServoLoop):
    """actions on top of the whole chain: observations, events, commands, terminations"""


class ServoActionsTerminationsPlainTwin(_Actions, TT.ServoTerminationsPlainTwin, _ServoLoop):
    """... without a command block"""


def make_twin(cfg, n, actions=None, width=T.J, terminations=None, commands=None, events=None, obs_table=None, table=(),
              env_offset=0, seed=RT.SEED, max_len=25, obs_dim=None, **kw):
    """``terminations`` None: the twin of a simulator that carries the action descriptor (and, through ``table``, rewards)
    and nothing else; otherwise the chain of ``servo_terminations_twin.make_twin``"""
    params = T.params_from_cfg(cfg.synthetic)
    if terminations is None:
        assert commands is None and events is None and obs_table is None
        d = int(cfg.synthetic.obs_dim if obs_dim is None else obs_dim)
        return ServoActionsTwin(n, d, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset, table=table,
                                actions=actions, width=width, **kw)
    args = (n, OT.RAW, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if commands is None:
        return ServoActionsTerminationsPlainTwin(*args, table=table, obs_table=obs_table, events=events,
                                                 terminations=terminations, actions=actions, width=width, **kw)
    return ServoActionsTerminationsTwin(*args, table=table, obs_table=obs_table, events=events, commands=commands,
                                        terminations=terminations, actions=actions, width=width, **kw)


def run_actions_twin(twin, actions, episode_length0, switch=None):
    """slabs [steps + 1, N, F]; ``switch`` = (step index, entries): the table is replaced before that step.  The
    bookkeeping around the twin is ``servo_twin.run_twin``'s"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs = [slab]
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_actions(switch[1], twin.A)
        slab = twin.step(slab, a, reset, ep_len)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs)
