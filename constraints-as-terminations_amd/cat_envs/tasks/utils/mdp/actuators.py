"""Actuator models of the servo task ("Actuators").

The names and fields are IsaacLab's ``isaaclab.actuators`` cfgs (``ImplicitActuatorCfg``, ``IdealPDActuatorCfg``,
``DCMotorCfg``, ``DelayedPDActuatorCfg``) inside an ``ArticulationCfg`` - PARITY UNPINNED: the rules are restated from their
published form, IsaacLab is not installed next to this package and nothing here is compared with it.

No actuator computes anything in Python.  ``build_table`` turns the robot's ``actuators`` into one entry per simulator joint -
gains, inertia, effort limit, the DC motor's curve, the delay range and the group - and the simulator's kernel evaluates the
entries inside its own launch (include/catppo.h, catppo_servo_actuator_entry).
"""
from __future__ import annotations

import math
import re

import numpy as np

from cat_envs import native
from cat_envs.shim.actuators import (ArticulationCfg, DCMotorCfg, DelayedPDActuatorCfg, IdealPDActuatorCfg,  # noqa: F401
                                     ImplicitActuatorCfg)

ACTUATOR_CFGS = (ImplicitActuatorCfg, IdealPDActuatorCfg, DCMotorCfg, DelayedPDActuatorCfg)
#: fields of the cfgs that are accepted and do nothing in this model
INERT_ROBOT_FIELDS = ("prim_path", "spawn", "collision_group", "debug_vis", "soft_joint_pos_limit_factor")
INERT_INIT_FIELDS = ("pos", "rot", "lin_vel", "ang_vel")
INERT_ACTUATOR_FIELDS = ("effort_limit_sim", "velocity_limit_sim")
MAX_LAG_STEPS = native.SERVO_ACTUATOR_MAX_LAG_STEPS


def _f32(x) -> float:
    return float(np.float32(x))


def _kind(a) -> str:
    # the subclasses first: a DC motor and a delayed PD are ideal PDs, too
    return ("dc_motor" if isinstance(a, DCMotorCfg) else "delayed_pd" if isinstance(a, DelayedPDActuatorCfg)
            else "ideal_pd" if isinstance(a, IdealPDActuatorCfg) else "implicit")


def _select(group, patterns, joint_names):
    if isinstance(patterns, str):
        patterns = [patterns]
    if not isinstance(patterns, (list, tuple)) or not patterns:
        raise ValueError(f"actuator group '{group}': joint_names_expr must be a list of regular expressions, got {patterns!r}")
    ids = []
    for p in patterns:
        hit = [j for j, jn in enumerate(joint_names) if re.fullmatch(p, jn)]
        if not hit:
            raise ValueError(f"actuator group '{group}': joint_names_expr entry '{p}' matches no joint of {list(joint_names)}")
        ids += [j for j in hit if j not in ids]
    return sorted(ids)


def _per_joint(group, what, value, ids, joint_names, default):
    """``value`` (a number or ``{regex: number}``) per joint of the group; None or a joint no key matches gets ``default``"""
    if value is None or not isinstance(value, (dict, int, float, np.floating, np.integer)):
        out = [default] * len(ids)
    elif not isinstance(value, dict):
        out = [value] * len(ids)
    else:
        out = [default] * len(ids)
        for key, v in value.items():
            hit = [i for i, j in enumerate(ids) if re.fullmatch(key, joint_names[j])]
            if not hit:
                raise ValueError(f"actuator group '{group}': {what} key '{key}' matches no joint of the group "
                                 f"{[joint_names[j] for j in ids]}")
            for i in hit:
                out[i] = v
    res = []
    for j, v in zip(ids, out):
        v = float(v)
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"actuator group '{group}': {what} of joint '{joint_names[j]}' must be finite and >= 0, got {v}")
        res.append(_f32(v))
    return res


def build_table(robot_cfg, joint_names, synthetic_cfg, decimation: int = 4, default_joint_pos=None):
    """(entries, spec) of an ``ArticulationCfg``; pure, needs no device.  ``entries``: 12 dicts, one per simulator joint, as
    ``Solo12ServoSim.set_actuator_table`` takes them (``kp`` = stiffness, ``kd`` = damping, ``inertia`` =
    ``synthetic_cfg.servo_inertia`` + armature, ``effort_limit`` (not set: ``servo_tau_max``), the DC motor's
    ``saturation_effort`` and ``velocity_limit``, ``min_delay`` / ``max_delay`` in physics steps, ``group`` = the index of
    the joint's actuator group in cfg order).  ``spec``: JSON-serialisable, what ``ActuatorModel.spec()`` returns.
    ``ValueError`` (naming the group) for a joint of two groups or of none, a regex key that matches nothing, a value that
    is not finite or negative, friction, ``min_delay > max_delay``, ``max_delay > 3 * decimation``, a DC motor without a
    positive ``velocity_limit`` and ``saturation_effort``, and an ``init_state.joint_pos`` that is not the model's pose."""
    joint_names = list(joint_names)
    groups = getattr(robot_cfg, "actuators", None)
    if not isinstance(groups, dict) or not groups:
        raise ValueError("cfg.scene.robot has no actuators: an ArticulationCfg with at least one actuator group is needed")
    max_lag = MAX_LAG_STEPS * int(decimation)
    entries, owner, spec_groups = [None] * len(joint_names), {}, {}
    for g, (name, a) in enumerate(groups.items()):
        if not isinstance(a, ACTUATOR_CFGS):
            raise TypeError(f"Configuration for actuator group '{name}' is not one of the actuator cfgs "
                            f"({', '.join(c.__name__ for c in ACTUATOR_CFGS)}). Received: '{type(a)}'.")
        kind = _kind(a)
        ids = _select(name, a.joint_names_expr, joint_names)
        for j in ids:
            if j in owner:
                raise ValueError(f"actuator group '{name}': joint '{joint_names[j]}' already belongs to group '{owner[j]}'")
            owner[j] = name
        kp = _per_joint(name, "stiffness", a.stiffness, ids, joint_names, 0.0)
        kd = _per_joint(name, "damping", a.damping, ids, joint_names, 0.0)
        arm = _per_joint(name, "armature", a.armature, ids, joint_names, 0.0)
        eff = _per_joint(name, "effort_limit", a.effort_limit, ids, joint_names, float(synthetic_cfg.servo_tau_max))
        vlim = _per_joint(name, "velocity_limit", a.velocity_limit, ids, joint_names, 0.0)
        if any(v != 0.0 for v in _per_joint(name, "friction", a.friction, ids, joint_names, 0.0)):
            raise ValueError(f"actuator group '{name}': friction must be 0 or None, the surrogate has no joint friction")
        sat, mn, mx = 0.0, 0, 0
        if kind == "dc_motor":
            sat = a.saturation_effort
            if not (isinstance(sat, (int, float)) and math.isfinite(sat) and sat > 0.0 and all(v > 0.0 for v in vlim)):
                raise ValueError(f"actuator group '{name}': a DCMotorCfg needs a positive velocity_limit and saturation_effort, "
                                 f"got velocity_limit {a.velocity_limit!r}, saturation_effort {sat!r}")
            sat = _f32(sat)
        if kind == "delayed_pd":
            mn, mx = int(a.min_delay), int(a.max_delay)
            if mn < 0 or mn > mx:
                raise ValueError(f"actuator group '{name}': min_delay {mn} > max_delay {mx} (or negative)")
            if mx > max_lag:
                raise ValueError(f"actuator group '{name}': max_delay {mx} > 3 * decimation = {max_lag} physics steps: the "
                                 f"row keeps the processed actions of three control steps")
        for i, j in enumerate(ids):
            entries[j] = dict(kp=kp[i], kd=kd[i], inertia=_f32(np.float32(synthetic_cfg.servo_inertia) + np.float32(arm[i])),
                              effort_limit=eff[i], saturation_effort=sat, velocity_limit=vlim[i], dc_motor=kind == "dc_motor",
                              min_delay=mn, max_delay=mx, group=g)
        spec_groups[name] = {"kind": kind, "index": g, "joint_ids": ids, "joints": [joint_names[j] for j in ids],
                             "min_delay": mn, "max_delay": mx}
    for j, e in enumerate(entries):
        if e is None:
            raise ValueError(f"joint '{joint_names[j]}' belongs to no actuator group (groups: {list(groups)})")
    init = getattr(robot_cfg, "init_state", None)
    if default_joint_pos is not None and init is not None and getattr(init, "joint_pos", None):
        for j, jn in enumerate(joint_names):
            hits = [v for k, v in init.joint_pos.items() if re.fullmatch(k, jn)]
            if hits and _f32(hits[-1]) != _f32(default_joint_pos[j]):
                group = owner[j]
                raise ValueError(f"actuator group '{group}': init_state.joint_pos of joint '{jn}' is {hits[-1]}, the simulator's "
                                 f"default pose has {float(default_joint_pos[j])}; the default pose is the model's own")
        vel = getattr(init, "joint_vel", None) or {}
        if any(float(v) != 0.0 for v in vel.values()):
            raise ValueError("init_state.joint_vel must be zero: the simulator's first state is at rest")
    return entries, actuator_spec(entries, spec_groups, joint_names, robot_cfg)


def armatures(robot_cfg, joint_names) -> list:
    """the nominal armature of every simulator joint, rounded to fp32 (what ``build_table`` added to ``servo_inertia``)"""
    joint_names = list(joint_names)
    out = [0.0] * len(joint_names)
    for name, a in (getattr(robot_cfg, "actuators", None) or {}).items():
        ids = _select(name, a.joint_names_expr, joint_names)
        for j, v in zip(ids, _per_joint(name, "armature", a.armature, ids, joint_names, 0.0)):
            out[j] = v
    return out


def inert_fields(robot_cfg) -> list:
    """the fields of the robot cfg that are set and do nothing in this model"""
    out = [f for f in INERT_ROBOT_FIELDS if getattr(robot_cfg, f, None) not in (None, 0, False, 1.0)]
    init = getattr(robot_cfg, "init_state", None)
    out += [f"init_state.{f}" for f in INERT_INIT_FIELDS if init is not None and hasattr(init, f)]
    for name, a in (getattr(robot_cfg, "actuators", None) or {}).items():
        out += [f"actuators.{name}.{f}" for f in INERT_ACTUATOR_FIELDS if getattr(a, f, None) is not None]
        if not isinstance(a, DCMotorCfg) and getattr(a, "velocity_limit", None) is not None:
            out.append(f"actuators.{name}.velocity_limit")           # the surrogate has no joint velocity clamp
    return out


def actuator_spec(entries, groups, joint_names, robot_cfg=None) -> dict:
    """what a deployment needs to know of the actuators: per joint its gains, limits and group, per group its kind and
    delay range (physics steps); JSON-serialisable"""
    joints = [{"joint": joint_names[j], "joint_id": j, "group": next(n for n, g in groups.items() if g["index"] == e["group"]),
               "stiffness": e["kp"], "damping": e["kd"], "inertia": e["inertia"], "effort_limit": e["effort_limit"],
               "saturation_effort": e["saturation_effort"] if e["dc_motor"] else None,
               "velocity_limit": e["velocity_limit"] if e["dc_motor"] else None} for j, e in enumerate(entries)]
    return {"joint_order": list(joint_names), "groups": {n: dict(g) for n, g in groups.items()}, "joints": joints,
            "delay_unit": "physics steps", "inert": [] if robot_cfg is None else inert_fields(robot_cfg)}
