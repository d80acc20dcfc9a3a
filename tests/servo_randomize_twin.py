"""Numpy twin of the servo surrogate's randomisation block (csrc/servo_sim_kernel.h: the randomisation-on instances,
include/catppo.h catppo_servo_randomize; DESIGN section 9, "Randomisation").

The env's own gains, inertia and joint friction live in the substep loop of the monolithic step, its foot load and the gain
of its velocity lags right behind it, so ``_RandomizeLoop`` restates ``servo_actuators_twin._ActuatorLoop.step`` with those
five taken from the draws of the block, and nothing else changed.  It subclasses ``_ActuatorLoop`` and is listed last among
the bases of the twins below, so that it lies right before ``_ActuatorLoop`` in their method resolution order: every parent
(actuators' row field, actions, terminations, commands, events, observations, rewards, trace, evaluation record) runs as it is
and ends up in the restated step.  None of the parents is edited.

The block is the 32 fp32 words the device reads (``block(...)`` below builds them from ranges; the tests compare the layout
with ``native.SERVO_RANDOMIZE_WORDS``).  One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_actions_twin as AT
import servo_actuators_twin as UT
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T

F32 = np.float32
TAG_GAINS, TAG_JOINT, TAG_MASS = 0x4147414E, 0x4A504152, 0x4D415353       # "AGAN" "JPAR" "MASS"
FLOATS = 32
ENABLE, KP, KD, FRICTION, ARMATURE, MASS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
GAINS_RESET, JOINT_RESET, MASS_RESET = 0x100, 0x200, 0x400
OPS = {"scale": 0, "add": 1, "abs": 2}
#: word offsets of the block, restated here
WORDS = {"flags": 0, "ops": 1, "gains_mask": 2, "joint_mask": 3, "body_mask": 4, "stiffness": 6, "damping": 8, "friction": 10,
         "armature": 12, "mass": 14, "m0": 16, "g": 17, "servo_inertia": 18, "armatures": 20}
QUANTITY = {"stiffness": KP, "damping": KD, "friction": FRICTION, "armature": ARMATURE, "mass": MASS}
ALL_JOINTS = (1 << T.J) - 1


def block(params, enabled=True, stiffness=None, damping=None, friction=None, armature=None, mass=None, gains_op="scale",
          joint_op="abs", mass_op="add", gains_mask=ALL_JOINTS, joint_mask=ALL_JOINTS, gains_reset=False, joint_reset=False,
          mass_reset=False, armatures=None):
    """the 32 words from (a, b) ranges (None: the quantity is off); lo = f32(a), width = f32(b - a); ``params`` gives
    ``weight`` and ``inertia`` of the simulator (m0 = f32(weight / 9.81), servo_inertia), ``armatures`` the twelve nominal ones"""
    w = np.zeros(FLOATS, F32)
    ints = w.view(np.int32)
    flags = ENABLE if enabled else 0
    for name, r in (("stiffness", stiffness), ("damping", damping), ("friction", friction), ("armature", armature), ("mass", mass)):
        if r is not None:
            flags |= QUANTITY[name]
            w[WORDS[name]], w[WORDS[name] + 1] = F32(r[0]), F32(float(r[1]) - float(r[0]))
    flags |= (GAINS_RESET if gains_reset else 0) | (JOINT_RESET if joint_reset else 0) | (MASS_RESET if mass_reset else 0)
    ints[WORDS["flags"]] = flags
    ints[WORDS["ops"]] = OPS[gains_op] | OPS[joint_op] << 8 | OPS[mass_op] << 16
    ints[WORDS["gains_mask"]], ints[WORDS["joint_mask"]], ints[WORDS["body_mask"]] = gains_mask, joint_mask, 1
    w[WORDS["m0"]], w[WORDS["g"]] = F32(float(params["weight"]) / 9.81), F32(9.81)
    w[WORDS["servo_inertia"]] = params["inertia"]
    w[WORDS["armatures"]:] = 0 if armatures is None else np.asarray(armatures, F32)
    return w


def _op(op, x, s):
    """one rounded operation on the nominal value"""
    assert x.shape == s.shape and x.dtype == s.dtype == F32
    return x * s if op == 0 else x + s if op == 1 else s.copy()


class _RandomizeLoop(UT._ActuatorLoop):
    """``_ActuatorLoop.step`` with the env's own gains, inertia, joint friction, foot load and velocity-lag gain"""

    def set_randomize(self, words):
        w = np.ascontiguousarray(words, F32).copy()
        assert w.shape == (FLOATS,)
        self.rnd = w
        self.rnd_stats = None

    def robot(self, ep):
        """dict of [N, 12] ``kp kd inertia fr df`` and [N] ``weight av m rho`` of episode ``ep``: the actuator table's and the
        simulator's values, or what the block's terms make of them"""
        n, w, p = self.N, self.rnd, self.p
        ints = w.view(np.int32)
        flags, ops = int(ints[WORDS["flags"]]), int(ints[WORDS["ops"]])
        tile = lambda x: np.tile(np.asarray(x, F32), (n, 1))                  # noqa: E731
        kp, kd, inertia = tile(self.u_kp), tile(self.u_kd), tile(self.u_inertia)
        fr, df = np.zeros((n, T.J), F32), np.zeros((n, T.J), F32)
        weight, av = np.full(n, p["weight"], F32), np.full(n, p["vel_alpha"], F32)
        m, rho = np.full(n, w[WORDS["m0"]], F32), np.ones(n, F32)
        zero = np.zeros(n, np.uint32)
        pair = lambda name: (w[WORDS[name]], w[WORDS[name] + 1])              # noqa: E731
        sample = lambda u, pr: (pr[0] + u * pr[1]).astype(F32)               # noqa: E731
        sel = lambda name: np.array([(int(ints[WORDS[name]]) >> j) & 1 for j in range(T.J)], bool)[None, :]   # noqa: E731
        samples = {}
        if flags & ENABLE:
            if flags & (KP | KD):
                e = ep if flags & GAINS_RESET else zero
                u = np.stack([self._philox(e, j, TAG_GAINS) for j in range(T.J)], 1)        # [N, 12, 4]
                s0, s1 = sample(u[:, :, 0], pair("stiffness")), sample(u[:, :, 1], pair("damping"))
                if flags & KP:
                    kp = np.where(sel("gains_mask"), _op(ops & 0xFF, kp, s0), kp).astype(F32)
                    samples["stiffness"] = s0
                if flags & KD:
                    kd = np.where(sel("gains_mask"), _op(ops & 0xFF, kd, s1), kd).astype(F32)
                    samples["damping"] = s1
            if flags & (FRICTION | ARMATURE):
                e = ep if flags & JOINT_RESET else zero
                u = np.stack([self._philox(e, j, TAG_JOINT) for j in range(T.J)], 1)
                s0, s1 = sample(u[:, :, 0], pair("friction")), sample(u[:, :, 1], pair("armature"))
                op = (ops >> 8) & 0xFF
                if flags & FRICTION:
                    fr = np.where(sel("joint_mask"), _op(op, np.zeros((n, T.J), F32), s0), fr).astype(F32)
                    samples["friction"] = s0
                if flags & ARMATURE:
                    arm = _op(op, tile(w[WORDS["armatures"]:]), s1)
                    inertia = np.where(sel("joint_mask"), w[WORDS["servo_inertia"]] + arm, inertia).astype(F32)
                    samples["armature"] = s1
                df = ((fr / inertia) * self.dt).astype(F32)
            if flags & MASS:
                e = ep if flags & MASS_RESET else zero
                s = sample(self._philox(e, 0, TAG_MASS)[:, 0], pair("mass"))
                m = _op((ops >> 16) & 0xFF, np.full(n, w[WORDS["m0"]], F32), s)
                weight = (m * w[WORDS["g"]]).astype(F32)
                rho = (m / w[WORDS["m0"]]).astype(F32)
                av = np.minimum(p["vel_alpha"] / rho, F32(1)).astype(F32)
                samples["mass"] = s
        return dict(kp=kp, kd=kd, inertia=inertia, fr=fr, df=df, weight=weight, av=av, m=m, rho=rho, samples=samples)

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
        fz = np.where(con > 0, (rb["weight"] / nsafe)[:, None] + np.where(touch, p["impact_gain"] * np.abs(knee_v), F32(0)),
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


class _Randomize:
    """the top of the chain: the block (None: all zero, which is the switch off)"""

    def __init__(self, *args, randomize=None, **kw):
        super().__init__(*args, **kw)
        self.set_randomize(np.zeros(FLOATS, F32) if randomize is None else randomize)
        self.rnd_live = None

    def step(self, slab, action, reset, episode_length):
        out = super().step(slab, action, reset, episode_length)
        self.rnd_live = self.rnd_stats
        return out


class ServoRandomizeTwin(_Randomize, UT._Actuators, AT._Actions, RT.ServoRewardTwin, _RandomizeLoop):
    """randomisation (behind an actuator and an action table) on the simulator without further descriptors"""


class ServoRandomizeTerminationsTwin(_Randomize, UT._Actuators, AT._Actions, TT.ServoTerminationsTwin, _RandomizeLoop):
    """randomisation on top of the whole chain: observations, events, commands, terminations, actions, actuators"""


class ServoRandomizeTerminationsPlainTwin(_Randomize, UT._Actuators, AT._Actions, TT.ServoTerminationsPlainTwin, _RandomizeLoop):
    """... without a command block"""


def make_twin(cfg, n, randomize=None, actuators=None, actions=None, width=T.J, terminations=None, commands=None, events=None,
              obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=25, obs_dim=None, **kw):
    """as ``servo_actuators_twin.make_twin``, with the randomisation block (None: all zero)"""
    params = T.params_from_cfg(cfg.synthetic)
    if terminations is None:
        assert commands is None and events is None and obs_table is None
        d = int(cfg.synthetic.obs_dim if obs_dim is None else obs_dim)
        return ServoRandomizeTwin(n, d, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset, table=table,
                                  actions=actions, width=width, actuators=actuators, randomize=randomize, **kw)
    args = (n, OT.RAW, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if commands is None:
        return ServoRandomizeTerminationsPlainTwin(*args, table=table, obs_table=obs_table, events=events,
                                                   terminations=terminations, actions=actions, width=width,
                                                   actuators=actuators, randomize=randomize, **kw)
    return ServoRandomizeTerminationsTwin(*args, table=table, obs_table=obs_table, events=events, commands=commands,
                                          terminations=terminations, actions=actions, width=width, actuators=actuators,
                                          randomize=randomize, **kw)


def run_randomize_twin(twin, actions, episode_length0, switch=None, gains=None):
    """slabs [steps + 1, N, F]; ``switch`` = (step index, words): the block is replaced before that step; ``gains`` = (step
    index, entries): the actuator table likewise.  The bookkeeping around the twin is ``servo_twin.run_twin``'s"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, live = [slab], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_randomize(switch[1])
        if gains is not None and s == gains[0]:
            twin.set_actuators(gains[1])
        slab = twin.step(slab, a, reset, ep_len)
        live.append(twin.rnd_live)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    twin.live_steps = live
    return np.stack(slabs)
