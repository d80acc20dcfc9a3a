"""Policy evaluation on the closed-loop servo task: fixed commands, a per-env record kept on the device.

``evaluate_policy`` rolls a policy out for ``steps`` control steps with the simulator's evaluation record attached
(``catppo_servo_sim.eval``: twelve fp32 sums per env, updated inside the simulator's own launch) and, optionally, a
per-env table of fixed commands (``catppo_servo_sim.fixed_command``).  Nothing inside the loop synchronises the host; the
tables come back once, at the end, and ``aggregate`` - pure numpy, no device - turns them into metrics in fp64.
DESIGN section 9, "Evaluation".
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field

import numpy as np

from cat_envs.native import SERVO_EVAL_FIELDS as FIELDS

#: the ranges the servo simulator draws its commands from (csrc/servo_sim.hip, command_of): vx, vy, wz
COMMAND_RANGES = ((-0.3, 1.0), (-0.7, 0.7), (-0.78, 0.78))
MAX_STEPS = 2 ** 24                     # the record counts in fp32: beyond 2^24 a count stops moving


def command_grid(vx=(-0.3, 1.0, 1), vy=(-0.7, 0.7, 1), wz=(-0.78, 0.78, 1), num_envs: int = 1):
    """``(commands [num_envs, 3] fp32, bin [num_envs] int64)``: the grid of ``n`` evenly spaced values per axis, each axis
    given as ``(lo, hi, n)`` (both ends included; ``n = 1`` is the midpoint), points ordered with vx slowest and wz
    fastest; env ``i`` gets grid point ``i % n_points``.  ``num_envs`` need not be a multiple of the grid."""
    axes = []
    for lo, hi, n in (vx, vy, wz):
        n = int(n)
        if n < 1:
            raise ValueError("a grid axis needs at least one point")
        axes.append(np.array([(lo + hi) / 2.0]) if n == 1 else np.linspace(lo, hi, n))
    pts = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], 1).astype(np.float32)
    idx = np.arange(int(num_envs), dtype=np.int64) % len(pts)
    return np.ascontiguousarray(pts[idx]), idx


def aggregate(record, cat_reward=None, termination_prob=None, violations=None, term_names=()) -> dict:
    """metrics of a set of envs, in fp64, from their per-env tables: ``record`` [n, 12] (``FIELDS``), the per-env sums of
    the CaT-scaled reward and of the termination probability [n], and the per-env counts of steps with a violated
    constraint [n, len(term_names) + 1] (one column per term, the last for any term).  Ratios whose divisor is zero
    (no episode ended) are None."""
    r = np.asarray(record, np.float64).reshape(-1, len(FIELDS))
    s = {k: float(r[:, i].sum()) for i, k in enumerate(FIELDS)}
    steps, episodes = s["steps"], s["episodes"]

    def per_step(x):
        return x / steps if steps > 0 else None

    def per_episode(x):
        return x / episodes if episodes > 0 else None
    m = {"steps": steps, "episodes": episodes, "fall_rate": per_episode(s["falls"]),
         "reward_per_step": per_step(s["reward"]),
         "cat_reward_per_step": None if cat_reward is None else per_step(float(np.asarray(cat_reward, np.float64).sum())),
         "rms_err_lin": math.sqrt(s["err_lin2"] / steps) if steps > 0 else None,
         "rms_err_yaw": math.sqrt(s["err_yaw2"] / steps) if steps > 0 else None,
         "mean_tilt2": per_step(s["tilt2"]), "mean_torque2": per_step(s["torque2"]), "mean_feet": per_step(s["feet"]),
         "episode_return_mean": per_episode(s["done_return"]), "episode_length_mean": per_episode(s["done_length"]),
         "termination_prob_mean": None if termination_prob is None
         else per_step(float(np.asarray(termination_prob, np.float64).sum()))}
    if violations is not None:
        v = np.asarray(violations, np.float64).reshape(r.shape[0], -1)
        names = [*term_names, "any"]
        if v.shape[1] != len(names):
            raise ValueError(f"violations has {v.shape[1]} columns for {len(names)} names")
        for i, name in enumerate(names):
            m["violation_share/" + name] = per_step(float(v[:, i].sum()))
    return m


@dataclass
class EvalResult:
    per_env: np.ndarray                           # [N, 12] fp32: the simulator's record
    fields: tuple = FIELDS
    commands: np.ndarray | None = None            # [N, 3] fixed commands, or None (sampled by the simulator)
    cat_reward: np.ndarray | None = None          # [N] fp32 sum of the CaT-scaled reward
    termination_prob: np.ndarray | None = None    # [N] fp32 sum of the CaT termination probability
    violations: np.ndarray | None = None          # [N, terms + 1] fp32 counts of steps with a violation (last: any term)
    term_names: tuple = ()
    metrics: dict = field(default_factory=dict)

    def _aggregate(self, rows=slice(None)):
        def pick(x):
            return None if x is None else x[rows]
        return aggregate(self.per_env[rows], pick(self.cat_reward), pick(self.termination_prob), pick(self.violations),
                         self.term_names)

    def by_command(self) -> list:
        """the metrics per distinct command row, in order of first appearance: ``{"command", "envs", "metrics"}``"""
        if self.commands is None:
            return [{"command": None, "envs": int(len(self.per_env)), "metrics": dict(self.metrics)}]
        _, first, inverse = np.unique(self.commands, axis=0, return_index=True, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        out = []
        for g in np.argsort(first):
            rows = np.nonzero(inverse == g)[0]
            out.append({"command": [float(c) for c in self.commands[rows[0]]], "envs": int(len(rows)),
                        "metrics": self._aggregate(rows)})
        return out

    def to_json(self, by_command: bool = True) -> str:
        d = {"metrics": self.metrics, "num_envs": int(len(self.per_env)), "fields": list(self.fields)}
        if by_command and self.commands is not None:
            d["by_command"] = self.by_command()
        return json.dumps(d)


def evaluate_policy(env, policy, steps: int, commands=None, deterministic: bool = True,
                    fresh_cat_state: bool = False) -> EvalResult:
    """Roll ``policy`` out for ``steps`` control steps from a fresh reset and measure it.

    ``policy`` is an ``Agent`` - its observations are normalised by the frozen ``obs_rms`` and the action is the mean
    (``deterministic=False`` samples); neither its parameters nor its normaliser are modified - or any callable
    ``raw_obs [N, D] -> action [N, 12]``.  ``commands`` [N, 3] (tensor or array) fixes env i's command to row i for the
    whole evaluation; None leaves the draws to the simulator.  Needs the closed-loop simulator (``TypeError`` otherwise).

    Use a dedicated env: its episode counters, reset masks, action history and constraint episode sums are zeroed, the
    simulator is reset, and the env is LEFT IN THE EVALUATED STATE (the record and the command table are detached again,
    also when the roll-out raises).  The loop never synchronises the host.

    ``fresh_cat_state=True`` also starts the env's CaT state as at construction (``CaTEnv.fresh_cat_state``: running maxima
    and their first-call flag, probability buffers, episode sums, log ring - all in place) and keeps the curriculum from
    running for the length of the evaluation, so every term's ``max_p`` is what the caller set through ``set_term_cfg``.  The
    result is then a function of the parameters, the observation normaliser, the ``max_p`` vector, the env cfg and seed,
    ``steps`` and ``commands`` alone: two such evaluations agree bit for bit whatever the env did in between (DESIGN
    section 11).  The default leaves the CaT state as the env's last step left it."""
    import contextlib
    import torch
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    steps = int(steps)
    if steps < 1 or steps > MAX_STEPS:
        raise ValueError(f"steps must be in [1, 2^24] (the record counts in fp32), got {steps}")
    u = env.unwrapped
    if not hasattr(u, "set_eval_record"):
        raise TypeError("evaluate_policy needs a CaTEnv")
    n, dev = u.num_envs, u.device
    record = torch.zeros(n, len(FIELDS), device=dev)
    table = None
    if isinstance(commands, torch.Tensor) and commands.device == dev and commands.dtype == torch.float32:
        table = commands.detach().reshape(n, 3).contiguous().clone()       # a table of its own, without a host round trip
    elif commands is not None:
        table = torch.as_tensor(np.asarray(commands.detach().cpu() if isinstance(commands, torch.Tensor) else commands,
                                           np.float32)).reshape(n, 3).contiguous().to(dev)
    if isinstance(policy, Agent):
        agent = policy

        def policy(obs):
            return agent(obs, deterministic=deterministic)
    cm = getattr(u, "constraint_manager", None)
    names = tuple(cm.active_terms) if cm is not None else ()
    cat_reward, term_prob = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    viol = torch.zeros(n, len(names) + 1, device=dev)
    member = None                                                    # [K, terms]: column k belongs to term j
    u.episode_length_buf.zero_()
    for mask in (u.reset_buf, u.reset_terminated, u.reset_time_outs):
        mask.zero_()
    u.action_manager.reset()
    if cm is not None:
        cm._ep_viol.zero_()
        cm._ep_prob.zero_()
    u.set_eval_record(record)                                         # TypeError on the stream simulator
    frozen = contextlib.ExitStack()
    if fresh_cat_state:
        u.fresh_cat_state()
        frozen.enter_context(u.curriculum_frozen())
    try:
        u.set_fixed_commands(table)
        obs = env.reset()[0]["policy"]
        with torch.no_grad():
            for _ in range(steps):
                obs, reward, _, _, _ = env.step(policy(obs))
                obs = obs["policy"]
                cat_reward.add_(reward)
                if names:
                    term_prob.add_(cm._cstr_prob_buf)
                    if member is None:                               # the packed matrix exists after the first compute()
                        off = list(cm._term_off)
                        member = torch.zeros(off[-1], len(names), device=dev)
                        for j in range(len(names)):
                            member[off[j]:off[j + 1], j] = 1.0
                    hit = ((cm.cat._p_cstr > 0).float() @ member) > 0   # small exact integer counts
                    viol[:, :-1].add_(hit)
                    viol[:, -1].add_(hit.any(1))
    finally:
        frozen.close()
        u.set_eval_record(None)
        u.set_fixed_commands(None)
    res = EvalResult(per_env=record.cpu().numpy(), commands=None if table is None else table.cpu().numpy(),
                     cat_reward=cat_reward.cpu().numpy(), termination_prob=term_prob.cpu().numpy(),
                     violations=viol.cpu().numpy(), term_names=names)
    res.metrics = res._aggregate()
    return res
