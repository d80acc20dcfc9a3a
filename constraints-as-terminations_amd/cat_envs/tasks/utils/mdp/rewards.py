"""Reward terms of the servo task (the reference's ``mdp/`` path; DESIGN section 9, "Rewards").

The names and signatures are IsaacLab's ``isaaclab.envs.mdp.rewards`` / the velocity task's ``mdp.rewards`` where one
exists - PARITY UNPINNED: the rules are restated from their published form, IsaacLab is not installed next to this
package and nothing here is compared with it.  The two ``*_rational`` terms are the servo surrogate's own stand-ins.

No term computes anything in Python.  Each carries ``describe(env, **params) -> (kind, joint_mask, param)``: the entry of
the table the simulator's kernel evaluates inside its own launch (include/catppo.h, catppo_servo_reward_term).  Calling a
term directly raises ``TypeError``; a reward function without ``describe`` is an error of the manager, not a slow path.
"""
from __future__ import annotations

import types

import numpy as np

from cat_envs import native

ALL_JOINTS_MASK = 0xFFF
MAX_TERMS = native.SERVO_REWARD_MAX_TERMS
ACTION_RATE_MIN_OBS_DIM = 45             # kind 11 reads the last-action block of the observation (floats 33 .. 44)


def _f32(x) -> float:
    return float(np.float32(x))


def _refuse(name):
    raise TypeError(f"{name}: the servo task evaluates rewards inside the simulator launch; the term only describes "
                    f"itself to the reward manager (describe(env, **params)) and is never called")


def _joint_mask(env, asset_cfg) -> int:
    """bit j set: joint j of ``scene[asset_cfg.name]`` is selected (``asset_cfg`` None: all joints)"""
    if asset_cfg is None:
        return ALL_JOINTS_MASK
    if getattr(asset_cfg, "joint_names", None) is not None:
        asset_cfg.resolve(env.scene)
    ids = asset_cfg.joint_ids
    if isinstance(ids, slice):
        ids = range(*ids.indices(len(env.scene[asset_cfg.name].joint_names)))
    mask = 0
    for j in ids:
        mask |= 1 << int(j)
    return mask


def _term(describe):
    def wrap(func):
        func.describe = describe
        return func
    return wrap


K = native.SERVO_REWARD_KINDS


@_term(lambda env, std, command_name=None, asset_cfg=None: (K["track_lin_vel_xy_exp"], 0, _f32(std ** 2)))
def track_lin_vel_xy_exp(env, std: float, command_name: str, asset_cfg=None):
    """exp(-|command_xy - v_xy|^2 / std^2)"""
    _refuse("track_lin_vel_xy_exp")


@_term(lambda env, std, command_name=None, asset_cfg=None: (K["track_ang_vel_z_exp"], 0, _f32(std ** 2)))
def track_ang_vel_z_exp(env, std: float, command_name: str, asset_cfg=None):
    """exp(-(command_wz - wz)^2 / std^2)"""
    _refuse("track_ang_vel_z_exp")


@_term(lambda env, scale, command_name=None: (K["track_lin_vel_xy_rational"], 0, _f32(scale)))
def track_lin_vel_xy_rational(env, scale: float, command_name: str = "base_velocity"):
    """1 / (1 + |command_xy - v_xy|^2 / scale): the surrogate's built-in linear tracking term"""
    _refuse("track_lin_vel_xy_rational")


@_term(lambda env, scale, command_name=None: (K["track_ang_vel_z_rational"], 0, _f32(scale)))
def track_ang_vel_z_rational(env, scale: float, command_name: str = "base_velocity"):
    """1 / (1 + (command_wz - wz)^2 / scale): the surrogate's built-in yaw tracking term (weight 0.5 there)"""
    _refuse("track_ang_vel_z_rational")


@_term(lambda env, asset_cfg=None: (K["ang_vel_xy_l2"], 0, 0.0))
def ang_vel_xy_l2(env, asset_cfg=None):
    _refuse("ang_vel_xy_l2")


@_term(lambda env, asset_cfg=None: (K["flat_orientation_l2"], 0, 0.0))
def flat_orientation_l2(env, asset_cfg=None):
    _refuse("flat_orientation_l2")


@_term(lambda env, asset_cfg=None: (K["joint_torques_l2"], _joint_mask(env, asset_cfg), 0.0))
def joint_torques_l2(env, asset_cfg=None):
    _refuse("joint_torques_l2")


@_term(lambda env, asset_cfg=None: (K["joint_acc_l2"], _joint_mask(env, asset_cfg), 0.0))
def joint_acc_l2(env, asset_cfg=None):
    _refuse("joint_acc_l2")


@_term(lambda env, asset_cfg=None: (K["joint_vel_l2"], _joint_mask(env, asset_cfg), 0.0))
def joint_vel_l2(env, asset_cfg=None):
    _refuse("joint_vel_l2")


@_term(lambda env, asset_cfg=None: (K["joint_deviation_l1"], _joint_mask(env, asset_cfg), 0.0))
def joint_deviation_l1(env, asset_cfg=None):
    _refuse("joint_deviation_l1")


@_term(lambda env: (K["action_rate_l2"], 0, 0.0))
def action_rate_l2(env):
    _refuse("action_rate_l2")


@_term(lambda env: (K["action_l2"], 0, 0.0))
def action_l2(env):
    _refuse("action_l2")


@_term(lambda env, command_name=None, sensor_cfg=None, threshold=0.0: (K["feet_air_time"], 0, _f32(threshold)))
def feet_air_time(env, command_name: str, sensor_cfg, threshold: float):
    """sum over the feet of (last air time - threshold) at touch-down, for a command of more than 0.1 in the plane"""
    _refuse("feet_air_time")


@_term(lambda env, target_height, asset_cfg=None, sensor_cfg=None: (K["base_height_l2"], 0, _f32(target_height)))
def base_height_l2(env, target_height: float, asset_cfg=None, sensor_cfg=None):
    _refuse("base_height_l2")


@_term(lambda env: (K["is_terminated"], 0, 0.0))
def is_terminated(env):
    """1 in a step that ends its episode by a fall (the surrogate's only termination that is not a time-out)"""
    _refuse("is_terminated")


@_term(lambda env: (K["is_alive"], 0, 0.0))
def is_alive(env):
    _refuse("is_alive")


def cfg_items(cfg):
    items = cfg.items() if isinstance(cfg, dict) else cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None]


def build_table(cfg, joint_names, obs_dim: int):
    """(names of every configured term, table) from a ``RewardsCfg``, the robot's joint names and the observation width;
    needs no device.  ``table``: one ``(name, kind, joint_mask, weight, param)`` per term of non-zero weight, in cfg order
    (a zero-weight term is left out and logs 0.0: IsaacLab's rule).  ``ValueError`` for more than 15 such terms, a func
    without ``describe`` (named), a joint selection that matches nothing and ``action_rate_l2`` with ``obs_dim`` < 45."""
    env = types.SimpleNamespace(scene={"robot": types.SimpleNamespace(joint_names=list(joint_names), body_names=[])})
    names, table = [], []
    for name, term in cfg_items(cfg):
        names.append(name)
        if not isinstance(term.weight, (int, float)):
            raise ValueError(f"reward term '{name}': weight must be a number, got {term.weight!r}")
        describe = getattr(term.func, "describe", None)
        if describe is None:
            raise ValueError(f"reward term '{name}': {getattr(term.func, '__name__', term.func)!r} has no describe(); the "
                             f"servo task evaluates rewards inside the simulator launch and runs no Python reward function")
        if float(term.weight) == 0.0:
            continue
        kind, mask, param = describe(env, **term.params)
        if kind == K["action_rate_l2"] and int(obs_dim) < ACTION_RATE_MIN_OBS_DIM:
            raise ValueError(f"reward term '{name}': action_rate_l2 reads the last-action block of the observation, "
                             f"obs_dim {obs_dim} < {ACTION_RATE_MIN_OBS_DIM}")
        table.append((name, int(kind), int(mask), float(term.weight), float(param)))
    if len(table) > MAX_TERMS:
        raise ValueError(f"{len(table)} reward terms of non-zero weight: the simulator evaluates at most {MAX_TERMS}")
    return names, table


def fold_log(names, active, sums, max_episode_length_s: float):
    """``Episode_Reward/<name>`` from the 16 fp64 column sums of floats 16 .. 31 of the record: the ended episodes' sum of
    term k over their count over the episode length in seconds; 0.0 for a term outside the table; None if none ended"""
    count = float(sums[15])
    if count <= 0.0:
        return None
    slot = {n: i for i, n in enumerate(active)}
    return {f"Episode_Reward/{n}": (float(sums[slot[n]]) / count / float(max_episode_length_s) if n in slot else 0.0)
            for n in names}
