"""Numpy twin of the Solo12 servo surrogate (csrc/servo_sim.hip) and a closed-loop CPU oracle env.

The twin restates the kernel statement by statement in fp32: every product, sum, quotient and square root is rounded
on its own (numpy float32 arithmetic never fuses), every reduction runs in the kernel's documented order (``tree16``:
the 16-lane butterfly with masks 8, 4, 2, 1; ``tree4``: masks 1, 2), and the randomness is the kernel's Philox4x32-10
counters (oracle/rng_oracle.py).  A slab computed here equals the kernel's slab bit for bit.

``ServoEnvOracle`` is ``CaTEnvOracle`` with a one-slab stream that the twin overwrites before every step: the CPU side
of the closed loop action -> state -> observation -> action.  Test infrastructure only.
"""
from __future__ import annotations

import re

import numpy as np

from oracle import env_oracle
from oracle import rng_oracle as R

F32 = np.float32
J, B, H = 12, 17, 3
JOINTS = ["FL_HAA", "FL_HFE", "FL_KFE", "FR_HAA", "FR_HFE", "FR_KFE",
          "HL_HAA", "HL_HFE", "HL_KFE", "HR_HAA", "HR_HFE", "HR_KFE"]
BODIES = ["base_link"] + [f"{leg}_{part}" for leg in ("FL", "FR", "HL", "HR")
                          for part in ("SHOULDER", "UPPER_LEG", "LOWER_LEG", "FOOT")]
DEFAULT_JOINT_POS = np.array([0.05, 0.4, -0.8, -0.05, 0.4, -0.8, 0.05, 0.4, -0.8, -0.05, 0.4, -0.8], F32)
FOOT_BODY = [4, 8, 12, 16]
TAG_COMMAND, TAG_INIT = 0x434D4453, 0x494E4954            # "CMDS", "INIT": fourth counter word
CMD_LO = np.array([-0.3, -0.7, -0.78], F32)
CMD_RANGE = np.array([1.3, 1.4, 1.56], F32)
NX = 14                                                    # private state: v 3 | roll pitch | air 4 | contact 4 | episode


def gains() -> np.ndarray:
    """G[5][16]: rows vx, vy, wz, roll, pitch over the 12 joint lanes (lanes 12..15 are zero)"""
    G = np.zeros((5, 16), F32)
    for leg in range(4):
        left, front = (leg % 2 == 0), (leg < 2)
        G[0, 3 * leg + 1] = 0.5                            # vx: the four HFE offsets
        G[1, 3 * leg] = 0.5                                # vy: the four HAA offsets
        G[2, 3 * leg] = 0.5 if front else -0.5             # wz: front against hind HAA
        G[3, 3 * leg + 1] = 0.3 if left else -0.3          # roll: left against right HFE
        G[4, 3 * leg + 2] = 0.3 if front else -0.3         # pitch: front against hind KFE
    return G


def layout(obs_dim: int):
    fields = [("joint_pos", J), ("joint_vel", J), ("joint_acc", J), ("applied_torque", J),
              ("projected_gravity_b", 3), ("root_pos_w", 3), ("command", 3), ("last_air_time", B),
              ("first_contact", B), ("forces", H * B * 3), ("reward", 1), ("hard_reset", 1), ("obs", obs_dim),
              ("servo", NX)]
    off, o = {}, 0
    for name, w in fields:
        off[name] = (o, w)
        o += w
    return off, (o + 3) // 4 * 4


PARAM_NAMES = ("kp", "kd", "inertia", "tau_max", "action_scale", "vel_alpha", "tilt_beta", "tilt_max", "reward_scale",
               "foot_clearance", "contact_threshold", "stand_height", "height_drop", "floor_height", "min_height",
               "base_stiffness", "weight", "impact_gain", "init_noise", "standing_fraction", "command_deadzone")


def params_from_cfg(syn) -> dict:
    p = {k: F32(getattr(syn, "servo_" + k)) for k in PARAM_NAMES}
    p["resample_steps"] = int(syn.servo_resample_steps)
    return p


def tree16(x):
    """sum over 16 lanes in the order of the xor butterfly 8, 4, 2, 1"""
    y = x[:, :8] + x[:, 8:]
    z = y[:, :4] + y[:, 4:]
    w = z[:, :2] + z[:, 2:]
    return w[:, 0] + w[:, 1]


def tree4(x):
    """sum over the four feet in the order of the xor butterfly 1, 2"""
    return (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])


class ServoTwin:
    def __init__(self, num_envs, obs_dim, params, seed, max_episode_length, dt, decimation, env_offset=0):
        self.N, self.D, self.p = int(num_envs), int(obs_dim), dict(params)
        self.off, self.F = layout(obs_dim)
        self.seed, self.max_len = int(seed) & (2 ** 64 - 1), int(max_episode_length)
        self.dt, self.dec = F32(dt), int(decimation)
        self.step_dt = F32(self.dt * F32(self.dec))
        self.gid = (np.arange(self.N, dtype=np.int64) + int(env_offset)).astype(np.uint32)
        self.G = gains()

    # ------------------------------------------------------------------ randomness
    def _philox(self, ep, third, tag):
        n = self.N
        ctr = np.stack([self.gid, ep.astype(np.uint32), np.full(n, third, np.uint32) if np.isscalar(third)
                        else third.astype(np.uint32), np.full(n, tag, np.uint32)], -1)
        key = np.broadcast_to(np.array([self.seed & 0xFFFFFFFF, self.seed >> 32], np.uint32), (n, 2))
        return R.uniform_open(R.philox4x32_10(ctr, key))

    def command(self, ep, k):
        p = self.p
        u = self._philox(ep, k, TAG_COMMAND)
        c = CMD_LO + u[:, :3] * CMD_RANGE
        n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        keep = (n2 > p["command_deadzone"] * p["command_deadzone"]) & ~(u[:, 3] < p["standing_fraction"])
        return np.where(keep[:, None], c, F32(0)).astype(F32)

    def init_q(self, ep):
        u = np.concatenate([self._philox(ep, blk, TAG_INIT) for blk in range(3)], 1)       # joint j: block j/4, word j%4
        return (DEFAULT_JOINT_POS + (u - F32(0.5)) * self.p["init_noise"]).astype(F32)

    # ------------------------------------------------------------------ rows
    def _f(self, slab, name):
        a, w = self.off[name]
        return slab[:, a:a + w]

    def _obs(self, ang, grav, cmd, dq, qd, act):
        full = np.concatenate([ang, grav, cmd, dq, qd, act], 1).astype(F32)
        out = np.zeros((self.N, self.D), F32)
        w = min(self.D, full.shape[1])
        out[:, :w] = full[:, :w]
        return out

    def initial(self, episode_length):
        """the slab of episode 0's first state (what the kernel writes in init mode)"""
        n, p = self.N, self.p
        slab = np.zeros((n, self.F), F32)
        ep = np.zeros(n, np.uint32)
        q = self.init_q(ep)
        cmd = self.command(ep, np.asarray(episode_length, np.int64) // p["resample_steps"])
        self._f(slab, "joint_pos")[:] = q
        self._f(slab, "projected_gravity_b")[:] = np.array([0, 0, -1], F32)
        self._f(slab, "root_pos_w")[:, 2] = p["stand_height"]
        self._f(slab, "command")[:] = cmd
        z3, z12 = np.zeros((n, 3), F32), np.zeros((n, 12), F32)
        self._f(slab, "obs")[:] = self._obs(z3, self._f(slab, "projected_gravity_b"), cmd, q - DEFAULT_JOINT_POS, z12, z12)
        x = self._f(slab, "servo")
        x[:, 9:13] = 1.0                                   # the four feet stand
        return slab

    def step(self, slab, action, reset, episode_length):
        """(state row block, action, reset mask of the previous step, episode lengths before this step) -> next block"""
        n, p, f = self.N, self.p, self._f
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
        red = [tree16(self.G[k] * dq16) for k in range(5)]
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
        ncon = tree4(con)
        zleg = p["stand_height"] - p["height_drop"] * np.abs(hfe)
        nsafe = np.maximum(ncon, F32(1))
        z = np.where(ncon > 0, tree4(con * zleg) / nsafe, p["floor_height"]).astype(F32)
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


def run_twin(twin: ServoTwin, actions, episode_length0):
    """the env's bookkeeping around the twin (counters, time-outs, hard resets): the slabs [steps + 1, N, F], first state first"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs = [slab]
    for a in actions:
        slab = twin.step(slab, a, reset, ep_len)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs)


# ---------------------------------------------------------------------------------------------- closed-loop oracle env
def oracle_terms(constraints_cfg):
    """the term list CaTEnvOracle wants, resolved from a ConstraintsCfg without a device env"""
    items = constraints_cfg.items() if isinstance(constraints_cfg, dict) else constraints_cfg.__dict__.items()
    terms = []

    def ids(patterns, names):
        if patterns is None:
            return None
        patterns = [patterns] if isinstance(patterns, str) else patterns
        got = [i for i, nm in enumerate(names) if any(re.fullmatch(p, nm) for p in patterns)]
        return None if got == list(range(len(names))) else got
    for name, cfg in items:
        if cfg is None:
            continue
        asset = cfg.params.get("asset_cfg")
        terms.append({"name": name, "func": cfg.func.__name__, "max_p": cfg.max_p,
                      "params": {k: v for k, v in cfg.params.items() if k != "asset_cfg"},
                      "joints": ids(getattr(asset, "joint_names", None), JOINTS),
                      "bodies": ids(getattr(asset, "body_names", None), BODIES)})
    return terms


def oracle_curriculum(curriculum_cfg):
    if curriculum_cfg is None:
        return []
    items = curriculum_cfg.items() if isinstance(curriculum_cfg, dict) else curriculum_cfg.__dict__.items()
    return [dict(term_name=t.params["term_name"], num_steps=t.params["num_steps"], init_max_p=t.params["init_max_p"])
            for _, t in items if t is not None]


class ServoEnvOracle(env_oracle.CaTEnvOracle):
    """closed-loop CPU env: a one-slab stream that the twin advances with the action before every CaT step"""

    def __init__(self, twin: ServoTwin, terms, curriculum, episode_length0, step_dt, tau=0.95, min_p=0.0):
        ep0 = np.asarray(episode_length0).astype(np.int64)
        stream = twin.initial(ep0)[None].copy()
        super().__init__(stream, twin.off, B, H, np.tile(DEFAULT_JOINT_POS, (twin.N, 1)), terms, curriculum, ep0,
                         twin.max_len, step_dt, tau=tau, min_p=min_p)
        self.twin = twin
        self._reset = np.zeros(twin.N, bool)
        self.violated = None

    def step(self, action):
        a = np.asarray(action.detach().cpu().numpy(), F32)
        self.stream[0] = self.twin.step(self.stream[0], a, self._reset, self.episode_length)
        out = super().step(action)
        self._reset = self.episode_length == 0           # incremented to >= 1 above unless the step ended in a reset
        self.violated = self.mgr.cat.get_probs() > 0     # some constraint is violated in this env step
        return out


def env_oracle_from_cfg(env_cfg, num_envs, episode_length0, env_offset=0, tau=0.95, min_p=0.0):
    import math
    syn = env_cfg.synthetic
    step_dt = env_cfg.sim.dt * env_cfg.decimation
    max_len = math.ceil(env_cfg.episode_length_s / step_dt)
    seed = int(getattr(env_cfg, "seed", 0) or 0) + int(syn.seed_offset)
    twin = ServoTwin(num_envs, int(syn.obs_dim), params_from_cfg(syn), seed, max_len, env_cfg.sim.dt, env_cfg.decimation,
                     env_offset)
    return ServoEnvOracle(twin, oracle_terms(env_cfg.constraints), oracle_curriculum(getattr(env_cfg, "curriculum", None)),
                          episode_length0, step_dt, tau=tau, min_p=min_p)


# ---------------------------------------------------------------------------------------------- the learning experiment
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-v0"
LEARNING = dict(num_envs=256, num_steps=24, hidden=(128, 128), learning_rate=1e-3, minibatch_size=1536, iterations=30,
                seed=42)
LEARNING_PROFILE = "profiles/servo_learning_oracle.json"


def learning_cfgs(num_envs=None, seed=None):
    """env and agent cfg of the learning experiment (CPU oracle and device trainer use the same)"""
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    L = LEARNING
    env_cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
    agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
    from cat_envs.tasks.locomotion.velocity.config.solo12 import cat_flat_env_cfg as E
    env_cfg.constraints, env_cfg.curriculum = E.ThreeConstraintsCfg(), E.ThreeCurriculumCfg()
    env_cfg.scene.num_envs = num_envs or L["num_envs"]
    env_cfg.seed = L["seed"] if seed is None else seed
    agent_cfg.num_steps, agent_cfg.minibatch_size = L["num_steps"], L["minibatch_size"]
    agent_cfg.learning_rate, agent_cfg.hidden = L["learning_rate"], tuple(L["hidden"])
    agent_cfg.save_interval = 10 ** 9
    return env_cfg, agent_cfg


def learning_summary(reward, violation):
    """gain of the reward (mean of the last five iterations over iteration 1) and drop of the violation share"""
    return dict(reward_gain=float(np.mean(reward[-5:]) - reward[0]), violation_drop=float(violation[0] - np.mean(violation[-5:])))


def run_oracle_learning(iterations=None, seed=None, log=None):
    """PPOOracle on the closed-loop twin env with its own torch randomness: per-iteration mean reward per env step and
    share of env steps in which some constraint is violated"""
    import torch
    from oracle import ppo_oracle
    L = LEARNING
    env_cfg, agent_cfg = learning_cfgs(seed=seed)
    n = env_cfg.scene.num_envs
    rs = np.random.RandomState(env_cfg.seed)
    env = env_oracle_from_cfg(env_cfg, n, rs.randint(0, 500, n))
    torch.manual_seed(env_cfg.seed)
    cfg = {k: getattr(agent_cfg, k) for k in ppo_oracle.PPOOracle.DEFAULT_CFG}
    orc = ppo_oracle.PPOOracle(env, n, int(env_cfg.synthetic.obs_dim), J, cfg=cfg, hidden=tuple(L["hidden"]), seed=env_cfg.seed)
    viol_steps = []
    step0 = env.step

    def step(a):
        out = step0(a)
        viol_steps.append(float(env.violated.mean()))
        return out
    env.step = step
    reward, violation = [], []
    for it in range(iterations or L["iterations"]):
        viol_steps.clear()
        orc.run_iteration()
        reward.append(float(orc.rewards.mean()))
        violation.append(float(np.mean(viol_steps)))
        if log:
            log(f"iteration {it + 1}: reward/step {reward[-1]:.4f} violation share {violation[-1]:.4f}")
    return reward, violation
