"""Numpy twin of the servo surrogate's evaluation mode (csrc/servo_sim.hip: ``fixed_command``, ``eval``).

``ServoEvalTwin`` is ``ServoTwin`` with the two descriptor fields: a fixed-command table that replaces every command draw,
and the per-env evaluation record of twelve fp32 sums.  The state row is the parent's, untouched.  Every term of the record
is a value the kernel holds in registers when it assembles the row, and every one of them is also a field of that row or
one kernel expression away from fields of it (the same fp32 operands, so the same bits): the twin reads them off the row it
just computed and adds them field by field, one rounded fp32 add each, like the kernel's owner lanes.  Test infrastructure.
"""
from __future__ import annotations

import numpy as np

import servo_twin as T

F32 = np.float32
FIELDS = ("steps", "episodes", "falls", "reward", "err_lin2", "err_yaw2", "tilt2", "torque2", "feet", "ep_return",
          "done_return", "done_length")


class ServoEvalTwin(T.ServoTwin):
    def __init__(self, *args, fixed_command=None, **kw):
        super().__init__(*args, **kw)
        self.fixed = None if fixed_command is None else np.ascontiguousarray(fixed_command, F32).reshape(self.N, 3)
        self.record = np.zeros((self.N, len(FIELDS)), F32)

    def command(self, ep, k):
        """the caller's table as it stands, for every episode and resample index (no dead zone, no standing fraction)"""
        if self.fixed is not None:
            return self.fixed.copy()
        return super().command(ep, k)

    def initial(self, episode_length):
        self.record = np.zeros((self.N, len(FIELDS)), F32)              # init mode: every env's record is zero
        return super().initial(episode_length)

    def step(self, slab, action, reset, episode_length):
        out = super().step(slab, action, reset, episode_length)
        f, n = self._f, self.N
        t = np.asarray(episode_length, np.int64)
        # ---- the kernel's values of this step, from the row they were written to
        cmd, x = f(out, "command"), f(out, "servo")
        v, roll, pitch, con = x[:, 0:3], x[:, 3], x[:, 4], x[:, 9:13]
        reward = f(out, "reward")[:, 0]
        fallen = f(out, "hard_reset")[:, 0] > 0
        ex, ey, ew = cmd[:, 0] - v[:, 0], cmd[:, 1] - v[:, 1], cmd[:, 2] - v[:, 2]
        tilt2 = roll * roll + pitch * pitch
        tau16 = np.zeros((n, 16), F32)
        tau16[:, :T.J] = f(out, "applied_torque")                       # lanes 12..15 contribute 0
        torque2 = T.tree16(tau16 * tau16)
        ncon = T.tree4(con)
        ends = (t + 1 >= self.max_len) | fallen
        # ---- one fp32 add per field
        r = self.record
        one, zero = F32(1), F32(0)
        ret = r[:, 9] + reward                                          # the running episode's return with this step
        terms = [np.full(n, one), np.where(ends, one, zero), np.where(fallen, one, zero), reward, ex * ex + ey * ey, ew * ew,
                 tilt2, torque2, ncon, reward, np.where(ends, ret, zero), np.where(ends, (t + 1).astype(F32), zero)]
        new = np.stack([(r[:, k] + np.asarray(terms[k], F32)).astype(F32) for k in range(len(FIELDS))], 1)
        new[:, 9] = np.where(ends, zero, new[:, 9])
        self.record = new
        return out


def run_eval_twin(twin: ServoEvalTwin, actions, episode_length0):
    """``servo_twin.run_twin`` with the record: (slabs [steps + 1, N, F], record [N, 12] after the last step)"""
    slabs = T.run_twin(twin, actions, episode_length0)
    return slabs, twin.record.copy()


def recount(twin: T.ServoTwin, slabs, episode_length0):
    """the countable fields of the record by a plain loop over the slabs: steps, episodes, falls per env, and the sums
    of the returns (fp32, step order) and lengths of the episodes that ended"""
    n = twin.N
    o = {k: twin.off[k][0] for k in ("reward", "hard_reset")}
    out = np.zeros((n, 5), np.float64)
    for i in range(n):
        t, ret, done_ret = int(episode_length0[i]), F32(0), F32(0)
        for s in range(1, len(slabs)):
            out[i, 0] += 1
            ret = F32(ret + slabs[s, i, o["reward"]])
            t += 1
            fell = slabs[s, i, o["hard_reset"]] > 0.5
            if fell or t >= twin.max_len:
                out[i, 1] += 1
                out[i, 2] += bool(fell)
                done_ret = F32(done_ret + ret)
                out[i, 4] += t
                t, ret = 0, F32(0)
        out[i, 3] = done_ret
    return out


# ---------------------------------------------------------------------------------------------- the evaluation experiment
EVAL = dict(num_envs=256, steps=200, grid=(4, 4, 2))        # 32 commands over the task's ranges, eight envs each
EVAL_PROFILE = "profiles/servo_eval_oracle.json"
EVAL_KEYS = ("reward_per_step", "rms_err_lin", "rms_err_yaw", "fall_rate", "mean_tilt2", "mean_torque2", "mean_feet")


def eval_commands():
    """the fixed command table of the evaluation experiment (CPU oracle and device trainer use the same)"""
    from cat_envs.tasks.utils.cleanrl.evaluate import COMMAND_RANGES, command_grid
    axes = [(lo, hi, n) for (lo, hi), n in zip(COMMAND_RANGES, EVAL["grid"])]
    return command_grid(*axes, num_envs=EVAL["num_envs"])[0]


def eval_twin_from_cfg(env_cfg, num_envs, fixed_command=None, env_offset=0):
    import math
    syn = env_cfg.synthetic
    max_len = math.ceil(env_cfg.episode_length_s / (env_cfg.sim.dt * env_cfg.decimation))
    seed = int(getattr(env_cfg, "seed", 0) or 0) + int(syn.seed_offset)
    return ServoEvalTwin(num_envs, int(syn.obs_dim), T.params_from_cfg(syn), seed, max_len, env_cfg.sim.dt, env_cfg.decimation,
                         env_offset, fixed_command=fixed_command)


def oracle_eval(agent, env_cfg, commands, steps):
    """the deterministic policy of an ``AgentOracle`` (frozen normaliser, mean action) on the eval twin, every episode
    counter starting at zero: the metrics of ``evaluate.aggregate`` over the twin's record"""
    import torch
    from cat_envs.tasks.utils.cleanrl.evaluate import aggregate
    n = len(commands)
    twin = eval_twin_from_cfg(env_cfg, n, commands)
    ep_len, reset = np.zeros(n, np.int64), np.zeros(n, bool)
    slab = twin.initial(ep_len)
    with torch.no_grad():
        for _ in range(steps):
            obs = torch.from_numpy(twin._f(slab, "obs").copy())
            a = agent.get_action_and_value(agent.obs_rms.normalize(obs), deterministic=True)[0].numpy()
            slab = twin.step(slab, a, reset, ep_len)
            ep_len += 1
            reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
            ep_len[reset] = 0
    m = aggregate(twin.record)
    return {k: m[k] for k in EVAL_KEYS}


def eval_summary(before, after):
    """what training bought, on the fixed grid: gain of the raw reward per step, drop of the rms linear tracking error"""
    return dict(reward_gain=float(after["reward_per_step"] - before["reward_per_step"]),
                err_lin_drop=float(before["rms_err_lin"] - after["rms_err_lin"]))


def run_oracle_eval_learning(iterations=None, seed=None, log=None):
    """``servo_twin.run_oracle_learning``'s training run (PPOOracle on the closed-loop twin env, ``learning_cfgs()``) with
    the policy evaluated on the fixed grid before the first and after the last iteration"""
    import torch
    from oracle import ppo_oracle
    L = T.LEARNING
    env_cfg, agent_cfg = T.learning_cfgs(seed=seed)
    n = env_cfg.scene.num_envs
    rs = np.random.RandomState(env_cfg.seed)
    env = T.env_oracle_from_cfg(env_cfg, n, rs.randint(0, 500, n))
    torch.manual_seed(env_cfg.seed)
    cfg = {k: getattr(agent_cfg, k) for k in ppo_oracle.PPOOracle.DEFAULT_CFG}
    orc = ppo_oracle.PPOOracle(env, n, int(env_cfg.synthetic.obs_dim), T.J, cfg=cfg, hidden=tuple(L["hidden"]), seed=env_cfg.seed)
    cmds = eval_commands()
    before = oracle_eval(orc.agent, env_cfg, cmds, EVAL["steps"])
    if log:
        log(f"untrained: {before}")
    for it in range(iterations or L["iterations"]):
        orc.run_iteration()
        if log:
            log(f"iteration {it + 1}: reward/step {float(orc.rewards.mean()):.4f}")
    after = oracle_eval(orc.agent, env_cfg, cmds, EVAL["steps"])
    if log:
        log(f"trained: {after}")
    return before, after
