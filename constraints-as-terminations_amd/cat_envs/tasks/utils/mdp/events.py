"""Event terms of the servo task (the reference's ``mdp/`` path; DESIGN section 9, "Events").

The names and signatures are IsaacLab's ``isaaclab.envs.mdp.events`` and, for the push, the reference's own
``mdp/events.py`` - PARITY UNPINNED: the rules are restated from their published form, IsaacLab is not installed next to
this package and nothing here is compared with it.

No term does anything in Python.  Each carries ``describe(name, sim_dt, max_episode_length_s, **params) -> dict``: its
``kind`` (which words of the simulator's event block it fills), the mode it must be configured with, its ranges as
``(a, b)`` pairs and the params it accepts without effect (``inert``).  The event manager turns that into the block the
simulator's kernel reads inside its own launch (include/catppo.h, catppo_servo_events).  Calling a term directly raises
``TypeError``; an event function without ``describe`` is an error of the manager, not a slow path.

The three randomisation terms at the end (``randomize_actuator_gains``, ``randomize_joint_parameters``,
``randomize_rigid_body_mass``; DESIGN section 9, "Randomisation") describe themselves in the same way, for either of the modes
"startup" and "reset"; ``mdp/randomization.py`` turns them into the randomisation block (include/catppo.h, catppo_servo_randomize).
"""
from __future__ import annotations

import math

AXES6 = ("x", "y", "z", "roll", "pitch", "yaw")
ZERO = (0.0, 0.0)


def _refuse(name):
    raise TypeError(f"{name}: the servo task evaluates events inside the simulator launch; the term only describes itself "
                    f"to the event manager (describe(...)) and is never called")


def _pair(term, key, value):
    try:
        a, b = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"event term '{term}': range '{key}' must be a pair (lo, hi), got {value!r}") from None
    if not (math.isfinite(a) and math.isfinite(b)) or b < a:
        raise ValueError(f"event term '{term}': range '{key}' must be finite with lo <= hi, got {value!r}")
    return a, b


def _axes(term, what, ranges, allowed, inert=()):
    """the ranges of ``allowed`` axes out of an IsaacLab range dict (an absent key is (0, 0)); any other axis must be zero"""
    ranges = dict(ranges or {})
    unknown = [k for k in ranges if k not in AXES6]
    if unknown:
        raise ValueError(f"event term '{term}': {what} has unknown keys {unknown} (known: {list(AXES6)})")
    out = {}
    for k in AXES6:
        a, b = _pair(term, f"{what}.{k}", ranges.get(k, ZERO))
        if k in allowed:
            out[k] = (a, b)
        elif k not in inert and (a != 0.0 or b != 0.0):
            raise ValueError(f"event term '{term}': {what}['{k}'] = {(a, b)} is not modelled by the servo surrogate "
                             f"(only {list(allowed)} of {what} have an effect); it must be (0, 0)")
    return out


def _term(describe):
    def wrap(func):
        func.describe = describe
        return func
    return wrap


def _describe_push(name, sim_dt, max_episode_length_s, velocity_range=None, asset_cfg=None, probability=None):
    r = _axes(name, "velocity_range", velocity_range, ("x", "y", "yaw", "roll", "pitch"))
    p = float(sim_dt) / (2.0 * float(max_episode_length_s)) if probability is None else float(probability)
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError(f"event term '{name}': the push probability must be in [0, 1], got {p}")
    return {"kind": "push", "mode": "interval", "p": p, "ranges": [r[k] for k in ("x", "y", "yaw", "roll", "pitch")], "inert": []}


@_term(_describe_push)
def push_by_setting_velocity_with_random_envs(env, env_ids, velocity_range, asset_cfg=None):
    """every step, each env is pushed with probability ``physics_dt / (2 * max_episode_length_s)``: its planar and yaw
    velocities are SET to samples of ``velocity_range`` (an absent key is (0, 0)), roll / pitch rates kick the tilt"""
    _refuse("push_by_setting_velocity_with_random_envs")


def _describe_push_timed(name, sim_dt, max_episode_length_s, velocity_range=None, asset_cfg=None):
    r = _axes(name, "velocity_range", velocity_range, ("x", "y", "yaw", "roll", "pitch"))
    # the interval is the term's own (interval_range_s): the event manager reads it
    return {"kind": "push_timed", "mode": "interval", "ranges": [r[k] for k in ("x", "y", "yaw", "roll", "pitch")], "inert": []}


@_term(_describe_push_timed)
def push_by_setting_velocity(env, env_ids, velocity_range, asset_cfg=None):
    """whenever the env's own timer runs out (``interval_range_s`` of the term, ``is_global_time=False``), samples of
    ``velocity_range`` are ADDED to its planar and yaw velocities (an absent key is (0, 0)), roll / pitch rates kick the tilt
    ("Disturbances")"""
    _refuse("push_by_setting_velocity")


def _describe_wrench(name, sim_dt, max_episode_length_s, force_range=None, torque_range=None, asset_cfg=None):
    import re
    if force_range is None or torque_range is None:
        raise ValueError(f"event term '{name}': force_range and torque_range are required")
    bodies = _names(asset_cfg, "body_names")
    if bodies is not None and not any(re.fullmatch(p, b) for p in bodies for b in ("base_link", "base")):
        raise ValueError(f"event term '{name}': asset_cfg.body_names {bodies} must match 'base_link' or 'base', the surrogate "
                         f"takes a wrench on its base only")
    return {"kind": "wrench", "mode": None, "ranges": [_pair(name, "force_range", force_range),
                                                        _pair(name, "torque_range", torque_range)], "inert": []}


@_term(_describe_wrench)
def apply_external_force_torque(env, env_ids, force_range, torque_range, asset_cfg=None):
    """one force and one torque on the base, each component a sample of its range, constant for the episode (mode "reset") or
    for the env's whole life (mode "startup") ("Disturbances")"""
    _refuse("apply_external_force_torque")


def _describe_joints(kind):
    def describe(name, sim_dt, max_episode_length_s, position_range=None, velocity_range=None, asset_cfg=None):
        if position_range is None or velocity_range is None:
            raise ValueError(f"event term '{name}': position_range and velocity_range are required")
        pos, vel = _pair(name, "position_range", position_range), _pair(name, "velocity_range", velocity_range)
        # by scale the velocity is default_joint_vel * s, and the model's default joint velocity is zero: nothing is drawn
        return {"kind": kind, "mode": "reset", "ranges": [pos, vel if kind == "joint_offset" else ZERO],
                "inert": ["velocity_range"] if kind == "joint_scale" and vel != ZERO else []}
    return describe


@_term(_describe_joints("joint_scale"))
def reset_joints_by_scale(env, env_ids, position_range, velocity_range, asset_cfg=None):
    """first pose = default * U(position_range); first joint velocity = default (zero) * U(velocity_range)"""
    _refuse("reset_joints_by_scale")


@_term(_describe_joints("joint_offset"))
def reset_joints_by_offset(env, env_ids, position_range, velocity_range, asset_cfg=None):
    """first pose = default + U(position_range); first joint velocity = U(velocity_range)"""
    _refuse("reset_joints_by_offset")


def _describe_root(name, sim_dt, max_episode_length_s, pose_range=None, velocity_range=None, asset_cfg=None):
    pose = _axes(name, "pose_range", pose_range, ("x", "y"), inert=("yaw",))
    vel = _axes(name, "velocity_range", velocity_range, ("x", "y", "yaw"))
    yaw = _pair(name, "pose_range.yaw", dict(pose_range or {}).get("yaw", ZERO))
    return {"kind": "root", "mode": "reset", "ranges": [pose["x"], pose["y"], vel["x"], vel["y"], vel["yaw"]],
            "inert": ["pose_range.yaw"] if yaw != ZERO else []}       # no heading in the model, flat ground is isotropic


@_term(_describe_root)
def reset_root_state_uniform(env, env_ids, pose_range, velocity_range, asset_cfg=None):
    """first root position x y and first velocities vx vy wz from uniform ranges"""
    _refuse("reset_root_state_uniform")


def _describe_material(name, sim_dt, max_episode_length_s, static_friction_range=None, dynamic_friction_range=ZERO,
                       restitution_range=ZERO, num_buckets=None, asset_cfg=None, make_consistent=False):
    if static_friction_range is None or num_buckets is None:
        raise ValueError(f"event term '{name}': static_friction_range and num_buckets are required")
    if int(num_buckets) != num_buckets or int(num_buckets) < 1:
        raise ValueError(f"event term '{name}': num_buckets must be an integer >= 1, got {num_buckets!r}")
    mu = _pair(name, "static_friction_range", static_friction_range)
    if mu[0] < 0.0:
        raise ValueError(f"event term '{name}': static_friction_range must be >= 0, got {mu}")
    inert = [k for k, v in (("dynamic_friction_range", dynamic_friction_range), ("restitution_range", restitution_range))
             if _pair(name, k, v) is not None]
    return {"kind": "friction", "mode": "startup", "ranges": [mu], "num_buckets": int(num_buckets), "inert": inert}


@_term(_describe_material)
def randomize_rigid_body_material(env, env_ids, static_friction_range, dynamic_friction_range, restitution_range, num_buckets,
                                  asset_cfg=None, make_consistent=False):
    """each env draws one of ``num_buckets`` shared materials once; its static friction against the ground's 1.0 is the
    env's traction"""
    _refuse("randomize_rigid_body_material")


# ---- randomisation of the robot ("Randomisation"): the three terms describe themselves like the others;
# mdp/randomization.py turns them into the randomisation block, not the event block.  Either mode, "startup" or "reset".
OPERATIONS = ("scale", "add", "abs")


def _randomize_common(name, operation, distribution):
    if distribution != "uniform":
        raise ValueError(f"event term '{name}': distribution {distribution!r} is not supported, only 'uniform' (log_uniform "
                         f"and gaussian need exp / log / cos, which the model's arithmetic excludes)")
    if operation not in OPERATIONS:
        raise ValueError(f"event term '{name}': unknown operation {operation!r} (known: {list(OPERATIONS)})")


def _names(asset_cfg, field):
    v = getattr(asset_cfg, field, None) if asset_cfg is not None else None
    return None if v is None else [v] if isinstance(v, str) else list(v)


def _describe_gains(name, sim_dt, max_episode_length_s, asset_cfg=None, stiffness_distribution_params=None,
                    damping_distribution_params=None, operation="abs", distribution="uniform"):
    _randomize_common(name, operation, distribution)
    ranges = {k: None if v is None else _pair(name, k + "_distribution_params", v)
              for k, v in (("stiffness", stiffness_distribution_params), ("damping", damping_distribution_params))}
    return {"kind": "actuator_gains", "mode": None, "operation": operation, "quantities": ranges,
            "joint_names": _names(asset_cfg, "joint_names"), "inert": []}


@_term(_describe_gains)
def randomize_actuator_gains(env, env_ids, asset_cfg, stiffness_distribution_params=None, damping_distribution_params=None,
                             operation="abs", distribution="uniform"):
    """stiffness and damping of the selected joints become op(nominal, U(params)), per env (startup) or per episode (reset)"""
    _refuse("randomize_actuator_gains")


def _describe_joint_parameters(name, sim_dt, max_episode_length_s, asset_cfg=None, friction_distribution_params=None,
                               armature_distribution_params=None, lower_limit_distribution_params=None,
                               upper_limit_distribution_params=None, operation="abs", distribution="uniform"):
    _randomize_common(name, operation, distribution)
    if lower_limit_distribution_params is not None or upper_limit_distribution_params is not None:
        raise ValueError(f"event term '{name}': lower_limit_distribution_params / upper_limit_distribution_params must be None, "
                         f"the model has no joint limits")
    if friction_distribution_params is not None and operation == "scale":
        raise ValueError(f"event term '{name}': friction_distribution_params with operation 'scale': the nominal joint "
                         f"friction is 0, and 0 stays 0")
    ranges = {k: None if v is None else _pair(name, k + "_distribution_params", v)
              for k, v in (("friction", friction_distribution_params), ("armature", armature_distribution_params))}
    return {"kind": "joint_parameters", "mode": None, "operation": operation, "quantities": ranges,
            "joint_names": _names(asset_cfg, "joint_names"), "inert": []}


@_term(_describe_joint_parameters)
def randomize_joint_parameters(env, env_ids, asset_cfg, friction_distribution_params=None, armature_distribution_params=None,
                               lower_limit_distribution_params=None, upper_limit_distribution_params=None, operation="abs",
                               distribution="uniform"):
    """joint friction (a Coulomb torque in N m, nominally 0) and armature of the selected joints become op(nominal, U(params))"""
    _refuse("randomize_joint_parameters")


def _describe_mass(name, sim_dt, max_episode_length_s, asset_cfg=None, mass_distribution_params=None, operation="abs",
                   distribution="uniform", recompute_inertia=True):
    import re
    _randomize_common(name, operation, distribution)
    if mass_distribution_params is None:
        raise ValueError(f"event term '{name}': mass_distribution_params is required")
    bodies = _names(asset_cfg, "body_names")
    if bodies is not None and not any(re.fullmatch(p, "base_link") for p in bodies):
        raise ValueError(f"event term '{name}': asset_cfg.body_names {bodies} must match 'base_link', the surrogate has one mass")
    return {"kind": "rigid_body_mass", "mode": None, "operation": operation,
            "quantities": {"mass": _pair(name, "mass_distribution_params", mass_distribution_params)}, "joint_names": None,
            "inert": ["recompute_inertia"]}


@_term(_describe_mass)
def randomize_rigid_body_mass(env, env_ids, asset_cfg, mass_distribution_params, operation="abs", distribution="uniform",
                              recompute_inertia=True):
    """the base's mass becomes op(weight / 9.81, U(params)): the load the stance feet share and the base's velocity lag follow it"""
    _refuse("randomize_rigid_body_mass")
