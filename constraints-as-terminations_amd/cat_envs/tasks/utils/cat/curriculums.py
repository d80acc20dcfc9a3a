"""Curriculum terms (reference: cat/curriculums.py:21-42)."""
from __future__ import annotations

from collections.abc import Sequence


def modify_constraint_p(env, env_ids: Sequence[int], term_name: str, num_steps: int, init_max_p: float):
    """Anneal a constraint's ``max_p``: the expected time-to-termination goes linearly from 20 steps
    to ``1/init_max_p`` steps over ``num_steps`` env steps.  Host-side double arithmetic; the new
    value reaches the GPU as the next ``catppo_cat_step``'s ``term_dp`` kernel argument."""
    progress = min(env.common_step_counter / num_steps, 1.0)
    horizon_start = 20
    horizon_end = 1 / init_max_p
    max_p = 1 / (horizon_start + progress * (horizon_end - horizon_start))
    manager = env.constraint_manager
    term_cfg = manager.get_term_cfg(term_name)
    term_cfg.max_p = max_p
    manager.set_term_cfg(term_name, term_cfg)
    return max_p


def modify_reward_weight(env, env_ids: Sequence[int], term_name: str, weight: float, num_steps: int):
    """IsaacLab's rule (isaaclab.envs.mdp.curriculums.modify_reward_weight, restated; PARITY UNPINNED): once more than
    ``num_steps`` env steps have run, the reward term's weight is ``weight``.  The new weight is in the simulator's table
    before the next launch.  Returns the current weight, which the curriculum manager logs as ``Curriculum/<name>``."""
    manager = env.reward_manager
    term_cfg = manager.get_term_cfg(term_name)
    if env.common_step_counter > num_steps and term_cfg.weight != weight:
        term_cfg.weight = weight
        manager.set_term_cfg(term_name, term_cfg)
    return float(term_cfg.weight)


def modify_command_ranges(env, env_ids: Sequence[int], term_name: str, ranges: dict, num_steps: int):
    """The command-side counterpart of ``modify_reward_weight`` - this project's own rule, not IsaacLab's or the
    reference's: once more than ``num_steps`` env steps have run, the command term's ranges are ``ranges`` (a dict with any
    of ``lin_vel_x``, ``lin_vel_y``, ``ang_vel_z`` -> (lo, hi)).  The new ranges are in the simulator's block before the
    next launch; a command in flight stays until its next resample.  Returns the upper bound of ``lin_vel_x``, which the
    curriculum manager logs as ``Curriculum/<name>``."""
    manager = env.command_manager
    manager.get_term_cfg(term_name)                 # names the term: an unknown name is an error
    if env.common_step_counter > num_steps:
        manager.set_ranges(**{k: tuple(v) for k, v in ranges.items()})
    return float(manager.ranges["lin_vel_x"][1])
