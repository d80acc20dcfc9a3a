"""Numpy twin of the servo surrogate's disturbances (csrc/servo_sim_kernel.h: the events-on instances with an extended block,
include/catppo.h "Disturbances"; DESIGN section 9, "Disturbances").

``_Disturb`` sits on top of a chain that holds the events twin and touches none of its parents:

* the timed push is an event like the push: ``push()`` is overridden to say which envs fire (the timer of the input row's
  ``ev_state``, updated statement by statement) and to ADD the samples to the velocities the step starts from; the updated
  timer is written into the output row, trace float 14 is the fire mask;
* the wrench acts inside the base model - after the five joint reductions and in the load the stance feet share - so the two
  loops it can sit on are restated with it, in the way every loop of the chain restates its parent's: ``_WrenchBaseLoop`` is
  ``servo_twin.ServoTwin.step``, ``_WrenchRobotLoop`` is ``servo_randomize_twin._RandomizeLoop.step`` (under the plant twin's
  ``robot`` and ``lag``), each with the lines marked ``wrench`` added and nothing else changed.

One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_actions_twin as AT
import servo_actuators_twin as UT
import servo_events_twin as ET
import servo_obs_twin as OT
import servo_plant_twin as PT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T

F32 = np.float32
TAG_PUSH_TIME, TAG_WRENCH = 0x50534854, 0x57524E43                       # "PSHT" "WRNC"
PUSH_TIMED, WRENCH, WRENCH_RESET = 32, 64, 128
FLOATS_EXT = 64
#: word offsets of the extended block's new words, restated here; the tests compare them with native.SERVO_EVENT_WORDS_EXT
WORDS_EXT = {"T_lo": 32, "T_width": 33, "force": 34, "torque": 36}
FIRE_BELOW = F32(1e-6)


def block(flags=0, interval=None, force=None, torque=None, **base):
    """the 64 words: ``servo_events_twin.block``'s 32 (``flags`` may carry the three new bits), then ``interval=(a, b)`` seconds,
    ``force=(a, b)``, ``torque=(a, b)``; lo = f32(a), width = f32(b - a)"""
    w = np.zeros(FLOATS_EXT, F32)
    w[:ET.FLOATS] = ET.block(flags=flags, **base)
    for name, rng in (("T_lo", interval), ("force", force), ("torque", torque)):
        if rng is not None:
            w[WORDS_EXT[name]], w[WORDS_EXT[name] + 1] = F32(rng[0]), F32(float(rng[1]) - float(rng[0]))
    return w


class _WrenchMixin:
    """the wrench of (env, episode) - or of the env - and what it does to the reductions and the load"""
    xflags = 0
    evx = np.zeros(FLOATS_EXT, F32)

    def wrench(self, ep, W):
        """None with the flag clear; else (the five addends of red[0..4], the load the stance feet share); ``W`` [N]"""
        if not self.xflags & WRENCH:
            return None
        e = ep if self.xflags & WRENCH_RESET else np.zeros(self.N, np.uint32)
        a, b = self._uniform(self.gid, e, 0, TAG_WRENCH), self._uniform(self.gid, e, 1, TAG_WRENCH)
        fr = (self.evx[WORDS_EXT["force"]], self.evx[WORDS_EXT["force"] + 1])
        tq = (self.evx[WORDS_EXT["torque"]], self.evx[WORDS_EXT["torque"] + 1])
        F = [self._sample(a[:, i], fr) for i in range(3)]
        Tq = [self._sample(b[:, i], tq) for i in range(3)]
        L = (W * self.p["stand_height"]).astype(F32)
        load = np.maximum(W - F[2], F32(0)).astype(F32)
        self.wrench_stats = dict(F=np.stack(F, 1), T=np.stack(Tq, 1), W=W.copy(), clamped=(W - F[2]) < F32(0))
        return [F[0] / W, F[1] / W, Tq[2] / L, Tq[0] / L, Tq[1] / L], load


class _WrenchBaseLoop(_WrenchMixin, T.ServoTwin):
    """``servo_twin.ServoTwin.step`` with the wrench"""

    def step(self, slab, action, reset, episode_length):
        """(state row block, action, reset mask of the previous step, episode lengths before this step) -> next block"""
        n, p, f = self.N, self.p, self._f
        J, H, B, FOOT_BODY, DEFAULT_JOINT_POS = T.J, T.H, T.B, T.FOOT_BODY, T.DEFAULT_JOINT_POS
        action = np.asarray(action, F32)
        reset = np.asarray(reset).astype(bool)
        t = np.asarray(episode_length, np.int64)
        x_in = f(slab, "servo")
        ep = x_in[:, 13].astype(np.uint32)
        r1, r0 = reset[:, None], reset
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
        # ---- joints: `decimation` substeps of the clamped PD servo, semi-implicit Euler
        q_des = DEFAULT_JOINT_POS + p["action_scale"] * action
        tau_w = np.zeros((n, J), F32)
        for _ in range(self.dec):
            tau = p["kp"] * (q_des - q) - p["kd"] * qd
            tau = np.minimum(np.maximum(tau, -p["tau_max"]), p["tau_max"])
            qdd = tau / p["inertia"]
            qd = qd + qdd * self.dt
            q = q + qd * self.dt
            tau_w = np.where(np.abs(tau) > np.abs(tau_w), tau, tau_w)       # the substep of largest |tau| is reported
        acc_w = tau_w / p["inertia"]
        dq = (q - DEFAULT_JOINT_POS).astype(F32)
        # ---- base: five fixed-order joint reductions, first-order lags
        dq16 = np.zeros((n, 16), F32)
        dq16[:, :J] = dq
        red = [T.tree16(self.G[k] * dq16) for k in range(5)]
        W = np.full(n, p["weight"], F32)                                                            # wrench
        wr, load = self.wrench(ep, W), W                                                            # wrench
        if wr is not None:                                                                          # wrench
            red, load = [(red[k] + wr[0][k]).astype(F32) for k in range(5)], wr[1]                  # wrench
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
        fz = np.where(con > 0, (load / nsafe)[:, None] + np.where(touch, p["impact_gain"] * np.abs(knee_v), F32(0)),
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


class _WrenchRobotLoop(_WrenchMixin, PT._PlantLoop):
    """``servo_randomize_twin._RandomizeLoop.step`` with the wrench; ``robot`` and ``lag`` are the plant twin's"""

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
        # ---- actuators: the history of the input row and the lag of every joint's group
        pa, unclipped = self.processed(action)
        kind = self.act_kind[None, :]
        hin = f(slab, "act_hist").reshape(n, UT.SLOTS, 16)
        fresh = (reset | (hin[:, 0, 12] == 0))[:, None]
        h = [np.where(fresh, pa, hin[:, k, :J]).astype(F32) for k in range(UT.SLOTS)]
        L = self.lag(ep)
        vl = np.where(self.u_dc, self.u_vlim, F32(1)).astype(F32)
        eff, sat = self.u_eff, self.u_sat
        # ---- randomisation: the robot of this env and episode
        rb = self.robot(ep)
        kp, kd, inertia, fr, df = rb["kp"], rb["kd"], rb["inertia"], rb["fr"], rb["df"]
        # ---- joints: `decimation` substeps of the clamped servo, semi-implicit Euler, joint friction as an impulse
        tau_w = np.zeros((n, J), F32)
        clamped, free = np.zeros((n, J), bool), np.zeros((n, J), bool)
        stick, slip = np.zeros((n, J), bool), np.zeros((n, J), bool)
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
            qdd = tau / inertia
            qd_free = (qd + qdd * self.dt).astype(F32)
            stick |= (fr > 0) & (np.abs(qd_free) <= df)
            slip |= (fr > 0) & (np.abs(qd_free) > df)
            qd = np.where(fr > 0, qd_free - np.minimum(np.maximum(qd_free, -df), df), qd_free).astype(F32)
            q = (q + qd * self.dt).astype(F32)
            tau_w = np.where(np.abs(tau) > np.abs(tau_w), tau, tau_w)       # the torque before friction is reported
        self.act_stats = dict(below=(unclipped < self.act_lo) & self.act_clip, above=(unclipped > self.act_hi) & self.act_clip,
                              clamped=clamped, free=free)
        self.actu_stats = dict(clamped=clamped, free=free, fresh=np.broadcast_to(fresh, (n, J)).copy(), lag=L.copy())
        self.rnd_stats = dict(stick=stick, slip=slip, clamped=clamped, free=free, fresh=np.broadcast_to(fresh, (n, J)).copy(),
                              capped=np.broadcast_to((p["vel_alpha"] / rb["rho"] > F32(1))[:, None], (n, J)).copy(),
                              kp=kp, kd=kd, inertia=inertia, fr=fr, m=np.broadcast_to(rb["m"][:, None], (n, J)).copy(),
                              ep=np.broadcast_to(ep[:, None], (n, J)).copy())
        self.rnd_samples = rb["samples"]
        acc_w = tau_w / inertia
        dq = (q - DEFAULT_JOINT_POS).astype(F32)
        # ---- base: five fixed-order joint reductions, first-order lags; the velocity lags follow the env's mass
        dq16 = np.zeros((n, 16), F32)
        dq16[:, :J] = dq
        red = [T.tree16(self.G[k] * dq16) for k in range(5)]
        W = rb["weight"]                                                                            # wrench
        wr, load = self.wrench(ep, W), W                                                            # wrench
        if wr is not None:                                                                          # wrench
            red, load = [(red[k] + wr[0][k]).astype(F32) for k in range(5)], wr[1]                  # wrench
        v_new = np.stack([v[:, k] + rb["av"] * (red[k] - v[:, k]) for k in range(3)], 1).astype(F32)
        roll = tilt[:, 0] + p["tilt_beta"] * (red[3] - tilt[:, 0])
        pitch = tilt[:, 1] + p["tilt_beta"] * (red[4] - tilt[:, 1])
        ang = np.stack([(roll - tilt[:, 0]) / self.step_dt, (pitch - tilt[:, 1]) / self.step_dt, v_new[:, 2]], 1)
        tilt2 = roll * roll + pitch * pitch
        fallen = tilt2 > p["tilt_max"] * p["tilt_max"]
        nrm = np.sqrt(tilt2 + F32(1))
        grav = np.stack([(F32(0) - pitch) / nrm, roll / nrm, F32(-1) / nrm], 1)
        grav = np.where(fallen[:, None], np.array([0, 0, 1], F32), grav).astype(F32)
        # ---- feet, height, contact forces: the stance feet share the env's own weight
        knee, knee_v, hfe = dq[:, 2::3], qd[:, 2::3], dq[:, 1::3]
        con = ((F32(0) - p["foot_clearance"] * knee) < p["contact_threshold"]).astype(F32)
        ncon = T.tree4(con)
        zleg = p["stand_height"] - p["height_drop"] * np.abs(hfe)
        nsafe = np.maximum(ncon, F32(1))
        z = np.where(ncon > 0, T.tree4(con * zleg) / nsafe, p["floor_height"]).astype(F32)
        touch = (con > 0) & ~(con_prev > 0)
        fz = np.where(con > 0, (load / nsafe)[:, None] + np.where(touch, p["impact_gain"] * np.abs(knee_v), F32(0)),
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
        hout = np.zeros((n, UT.SLOTS, 16), F32)
        hout[:, 0, :J], hout[:, 1, :J], hout[:, 2, :J] = pa, h[0], h[1]
        hout[:, 0, 12] = 1
        f(out, "act_hist")[:] = hout.reshape(n, -1)
        return out


class _Disturb:
    """the top of the chain: the extended block, the timer field and the timed push"""

    def __init__(self, *args, ev_state=True, **kw):
        self.has_state = bool(ev_state)                     # before the parents' constructor: it calls set_events
        super().__init__(*args, **kw)
        if self.has_state:                                  # behind everything else, like the simulator's row
            self.off = dict(self.off)
            self.off["ev_state"] = (self.F, 4)
            self.F += 4
        self.timer_fired = np.zeros(self.N, bool)

    def set_events(self, words):
        """32 words (the new bits are ignored, as the kernel ignores them) or 64"""
        w = np.ascontiguousarray(words, F32).copy()
        assert w.shape in ((ET.FLOATS,), (FLOATS_EXT,))
        ext = w.shape == (FLOATS_EXT,)
        flags = int(w.view(np.int32)[0])
        base = w[:ET.FLOATS].copy()
        base.view(np.int32)[0] = flags & 31
        super().set_events(base)
        self.evx = np.zeros(FLOATS_EXT, F32)
        self.evx[:len(w)] = w
        self.xflags = flags & (PUSH_TIMED | WRENCH | WRENCH_RESET) if ext else 0
        if not self.has_state:                              # off_ev_state == 0: the kernel ignores the timed bit
            self.xflags &= ~PUSH_TIMED

    def push_time(self, ep, third):
        """the time until the next timed push from counter {gid, ep, third, "PSHT"} word 0"""
        u = self._uniform(self.gid, ep, third, TAG_PUSH_TIME)[:, 0]
        return self._sample(u, (self.evx[WORDS_EXT["T_lo"]], self.evx[WORDS_EXT["T_width"]]))

    def push(self, ep, t):
        """the per-step push, or - the timer of this step having run out - the timed one: the same samples, ADDED to the
        velocities the step starts from (``_raw_slab``: the input row; a fired step is no reset step)"""
        if self.flags & ET.PUSH or not self.xflags & PUSH_TIMED:
            return super().push(ep, t)
        t = np.asarray(t, np.int64)
        u0 = self._uniform(self.gid, ep, (t << 1), ET.TAG_PUSH)
        u1 = self._uniform(self.gid, ep, (t << 1) | 1, ET.TAG_PUSH)
        x = self._f(self._raw_slab, "servo")
        v = np.stack([(x[:, k] + self._sample(u0[:, 1 + k], self._pair("push", k))).astype(F32) for k in range(3)], 1)
        kick = np.stack([(self._sample(u1[:, k], self._pair("push", 3 + k)) * self.step_dt).astype(F32) for k in range(2)], 1)
        return self.timer_fired.copy(), v, kick

    def _write_ev_state(self, out, tl):
        if self.has_state:
            s = self._f(out, "ev_state")
            s[:] = 0
            s[:, 0] = tl
        return out

    def initial(self, episode_length):
        tl = np.zeros(self.N, F32)
        if self.xflags & PUSH_TIMED:
            tl = self.push_time(np.zeros(self.N, np.uint32), 0)
        return self._write_ev_state(super().initial(episode_length), tl)

    def step(self, slab, action, reset, episode_length):
        f, n = self._f, self.N
        rst = np.asarray(reset).astype(bool)
        t = np.asarray(episode_length, np.int64)
        ep = f(slab, "servo")[:, 13].astype(np.uint32)
        tl = f(slab, "ev_state")[:, 0].astype(F32) if self.has_state else np.zeros(n, F32)
        fire = np.zeros(n, bool)
        if self.xflags & PUSH_TIMED:
            assert (t >= 0).all() and (t < 2 ** 27).all()
            tl = (tl - self.step_dt).astype(F32)
            fire = (tl < FIRE_BELOW) & ~rst
            tl = np.where(fire, self.push_time(ep, t + 1), tl).astype(F32)
            # a step whose reset flag is set draws the timer of its episode and runs no update
            tl = np.where(rst, self.push_time(ep, 0), tl).astype(F32)
        self.timer_fired = fire
        slot = self.record[:, 0].astype(np.int64)
        out = super().step(slab, action, reset, episode_length)
        if self.trace is not None and self.xflags & PUSH_TIMED and not self.flags & ET.PUSH:
            for i in range(self.K):
                if 0 <= slot[i] < self.T:
                    self.trace[slot[i], i, ET.TRACE_PUSHED] = F32(self.pushed[i])
        return self._write_ev_state(out, tl)


class ServoDisturbTwin(_Disturb, ET.ServoEventsTwin, _WrenchBaseLoop):
    """disturbances on the simulator with an event block (and, with ``obs_table``, an observation table) alone"""


class ServoDisturbRobotTwin(_Disturb, PT._Plant, ZT._Randomize, UT._Actuators, AT._Actions, TT.ServoTerminationsTwin,
                            _WrenchRobotLoop):
    """disturbances on top of the whole chain: observations, events, commands, terminations, actions, actuators, randomisation,
    pinned plants"""


def make_twin(cfg, n, events, obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=12, ev_state=True, robot=None, **kw):
    """``events``: 32 or 64 words.  ``robot`` None: the event pack alone; else a dict with ``commands``, ``terminations`` and
    optionally ``actions``, ``width``, ``actuators``, ``randomize``, ``plant`` (as ``servo_plant_twin.make_twin``)"""
    args = (n, OT.RAW, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if robot is None:
        return ServoDisturbTwin(*args, table=table, obs_table=obs_table, events=events, ev_state=ev_state, **kw)
    return ServoDisturbRobotTwin(*args, table=table, obs_table=obs_table, events=events, ev_state=ev_state, **robot, **kw)


def run_disturb_twin(twin, actions, episode_length0, switch=None):
    """(slabs [steps + 1, N, F], fire / push masks [steps, N], reset masks [steps, N], clamp masks [steps, N]); ``switch`` =
    (step index, words): the block is replaced before that step.  The bookkeeping around the twin is ``servo_twin.run_twin``'s"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, masks, resets, clamps = [slab], [], [], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_events(switch[1])
        twin.wrench_stats = None
        resets.append(reset.copy())
        slab = twin.step(slab, a, reset, ep_len)
        masks.append(twin.pushed.copy())
        clamps.append(np.zeros(twin.N, bool) if twin.wrench_stats is None else twin.wrench_stats["clamped"].copy())
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs), np.stack(masks), np.stack(resets), np.stack(clamps)
