"""Numpy twin of the servo surrogate's actuator table (csrc/servo_sim_kernel.h: the actuators-on instances,
include/catppo.h catppo_servo_actuators; DESIGN section 9, "Actuators").

The gains, the inertia, the torque clamp and the delayed target all live in the substep loop of the monolithic step, so
``_ActuatorLoop`` restates ``servo_actions_twin._ServoLoop.step`` with the loop taken from the actuator table and the row's
history field, and nothing else changed.  It subclasses ``_ServoLoop`` and is listed last among the bases of the twins below,
so that it lies right before ``_ServoLoop`` in their method resolution order: every parent (actions, terminations, commands,
events, observations, rewards, trace, evaluation record) runs as it is and ends up in the restated step.  None of the
parents is edited.

An entry is a dict with ``kp``, ``kd``, ``inertia``, ``effort_limit`` and optionally ``saturation_effort``,
``velocity_limit``, ``dc_motor``, ``min_delay``, ``max_delay``, ``group`` - what ``Solo12ServoSim.set_actuator_table`` takes.
One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_actions_twin as AT
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T

F32 = np.float32
TAG_ACT_DELAY = 0x41444C59                                 # "ADLY": fourth counter word of the lag's Philox block
HIST_FLOATS, SLOTS = 48, 3


def identity_entries(params):
    """the table that must change nothing: the simulator's own scalars on every joint, ideal PD, no delay"""
    return [dict(kp=params["kp"], kd=params["kd"], inertia=params["inertia"], effort_limit=params["tau_max"])] * T.J


class _ActuatorLoop(AT._ServoLoop):
    """``_ServoLoop.step`` with per-joint gains, inertia and clamp, and the delayed processed action"""

    def set_actuators(self, entries):
        assert len(entries) == T.J
        col = lambda k, d=0.0: np.array([e.get(k, d) or d for e in entries], F32)   # noqa: E731
        self.u_kp, self.u_kd, self.u_inertia, self.u_eff = col("kp"), col("kd"), col("inertia"), col("effort_limit")
        self.u_sat, self.u_vlim = col("saturation_effort"), col("velocity_limit")
        self.u_dc = np.array([bool(e.get("dc_motor", False)) for e in entries], bool)
        self.u_min = np.array([int(e.get("min_delay", 0)) for e in entries], np.int64)
        self.u_max = np.array([int(e.get("max_delay", 0)) for e in entries], np.int64)
        self.u_group = np.array([int(e.get("group", 0)) for e in entries], np.int64)
        self.actu_stats = None

    def lag(self, ep):
        """[N, 12] int: the lag of every joint's group in physics steps, of episode ``ep``"""
        L = np.tile(self.u_min, (self.N, 1))
        for j in range(T.J):
            mn, mx = int(self.u_min[j]), int(self.u_max[j])
            if mx > mn:
                u = self._philox(ep, int(self.u_group[j]), TAG_ACT_DELAY)[:, 0]
                l = mn + (u * F32(mx - mn + 1)).astype(np.int64)          # a rounded product, truncated
                L[:, j] = np.minimum(l, mx)
        return L

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
        # ---- actuators: the history of the input row (all three slots count as this step's p after a reset or behind an
        # init launch) and the lag of every joint's group
        pa, unclipped = self.processed(action)
        kind = self.act_kind[None, :]
        hin = f(slab, "act_hist").reshape(n, SLOTS, 16)
        fresh = (reset | (hin[:, 0, 12] == 0))[:, None]
        h = [np.where(fresh, pa, hin[:, k, :J]).astype(F32) for k in range(SLOTS)]
        L = self.lag(ep)
        vl = np.where(self.u_dc, self.u_vlim, F32(1)).astype(F32)
        kp, kd, eff, sat = self.u_kp, self.u_kd, self.u_eff, self.u_sat
        # ---- joints: `decimation` substeps of the clamped servo of the joint's action term, semi-implicit Euler
        tau_w = np.zeros((n, J), F32)
        clamped = np.zeros((n, J), bool)
        free = np.zeros((n, J), bool)
        stats = dict(slot=np.zeros((n, J), np.int64), late=np.zeros((n, J), bool), same=np.zeros((n, J), bool),
                     hi_binds=np.zeros((n, J), bool), hi_free=np.zeros((n, J), bool), lo_binds=np.zeros((n, J), bool),
                     lo_free=np.zeros((n, J), bool), lag=L.copy())
        for s in range(self.dec):
            k = np.where(s >= L, 0, (L - s + self.dec - 1) // self.dec)
            k = np.minimum(k, 3)
            pt = np.where(k == 0, pa, np.where(k == 1, h[0], np.where(k == 2, h[1], h[2]))).astype(F32)
            tgt = np.where(kind == 1, pt, np.where(kind == 2, pt + q, DEFAULT_JOINT_POS)).astype(F32)
            pd = kp * (tgt - q) - kd * qd
            vel = kd * (pt - qd)
            tau0 = np.where(kind == 3, vel, np.where(kind == 4, pt, pd)).astype(F32)
            ideal = np.minimum(np.maximum(tau0, -eff), eff)
            r = qd / vl
            hi = sat * (F32(1) - r)
            hi = np.minimum(np.maximum(hi, F32(0)), eff)
            lo = sat * (F32(-1) - r)
            lo = np.minimum(np.maximum(lo, -eff), F32(0))
            dc = np.minimum(np.maximum(tau0, lo), hi)
            tau = np.where(self.u_dc, dc, ideal).astype(F32)
            clamped |= tau != tau0
            free |= tau == tau0
            stats["slot"] = np.maximum(stats["slot"], k)
            stats["late"] |= (k > 0) & (pt != pa)
            stats["same"] |= (k > 0) & (pt == pa)
            stats["hi_binds"] |= self.u_dc & (tau0 > hi)
            stats["hi_free"] |= self.u_dc & ~(tau0 > hi)
            stats["lo_binds"] |= self.u_dc & (tau0 < lo)
            stats["lo_free"] |= self.u_dc & ~(tau0 < lo)
            qdd = tau / self.u_inertia
            qd = qd + qdd * self.dt
            q = q + qd * self.dt
            tau_w = np.where(np.abs(tau) > np.abs(tau_w), tau, tau_w)       # the substep of largest |tau| is reported
        self.act_stats = dict(below=(unclipped < self.act_lo) & self.act_clip, above=(unclipped > self.act_hi) & self.act_clip,
                              clamped=clamped, free=free)
        self.actu_stats = dict(stats, clamped=clamped, free=free, fresh=np.broadcast_to(fresh, (n, J)).copy())
        acc_w = tau_w / self.u_inertia
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
        # the history moves one slot back: p | old slot 0 | old slot 1; float 12 of slot 0 says that a step wrote the row
        hout = np.zeros((n, SLOTS, 16), F32)
        hout[:, 0, :J], hout[:, 1, :J], hout[:, 2, :J] = pa, h[0], h[1]
        hout[:, 0, 12] = 1
        f(out, "act_hist")[:] = hout.reshape(n, -1)
        return out


class _Actuators:
    """the top of the chain: the row's ``act_hist`` field behind everything else, and the table"""

    def __init__(self, *args, actuators=None, **kw):
        super().__init__(*args, **kw)
        self.off = dict(self.off)
        self.off["act_hist"] = (self.F, HIST_FLOATS)
        self.F += HIST_FLOATS
        self.set_actuators(actuators if actuators is not None else identity_entries(self.p))
        self.actu_live = None

    def initial(self, episode_length):
        slab = super().initial(episode_length)
        self._f(slab, "act_hist")[:] = 0                    # the init launch leaves the field zero
        return slab

    def step(self, slab, action, reset, episode_length):
        out = super().step(slab, action, reset, episode_length)
        self.actu_live = self.actu_stats
        return out


class ServoActuatorsTwin(_Actuators, AT._Actions, RT.ServoRewardTwin, _ActuatorLoop):
    """actuators (behind an action table) on the simulator without further descriptors"""


class ServoActuatorsTerminationsTwin(_Actuators, AT._Actions, TT.ServoTerminationsTwin, _ActuatorLoop):
    """actuators on top of the whole chain: observations, events, commands, terminations, actions"""


class ServoActuatorsTerminationsPlainTwin(_Actuators, AT._Actions, TT.ServoTerminationsPlainTwin, _ActuatorLoop):
    """... without a command block"""


def make_twin(cfg, n, actuators=None, actions=None, width=T.J, terminations=None, commands=None, events=None, obs_table=None,
              table=(), env_offset=0, seed=RT.SEED, max_len=25, obs_dim=None, **kw):
    """as ``servo_actions_twin.make_twin``, with the actuator table (None: the identity table)"""
    params = T.params_from_cfg(cfg.synthetic)
    if terminations is None:
        assert commands is None and events is None and obs_table is None
        d = int(cfg.synthetic.obs_dim if obs_dim is None else obs_dim)
        return ServoActuatorsTwin(n, d, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset, table=table,
                                  actions=actions, width=width, actuators=actuators, **kw)
    args = (n, OT.RAW, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if commands is None:
        return ServoActuatorsTerminationsPlainTwin(*args, table=table, obs_table=obs_table, events=events,
                                                   terminations=terminations, actions=actions, width=width,
                                                   actuators=actuators, **kw)
    return ServoActuatorsTerminationsTwin(*args, table=table, obs_table=obs_table, events=events, commands=commands,
                                          terminations=terminations, actions=actions, width=width, actuators=actuators, **kw)


def run_actuators_twin(twin, actions, episode_length0, switch=None):
    """slabs [steps + 1, N, F]; ``switch`` = (step index, entries): the actuator table is replaced before that step.  The
    bookkeeping around the twin is ``servo_twin.run_twin``'s"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, live = [slab], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_actuators(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        live.append(twin.actu_live)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    twin.live_steps = live
    return np.stack(slabs)
