"""Termination terms of the servo task (the reference's ``mdp/`` path; DESIGN section 9, "Terminations").

The names and signatures are IsaacLab's ``isaaclab.envs.mdp.terminations`` and the reference's ``mdp/terminations.py``
(``upside_down``) - PARITY UNPINNED: the rules are restated from their published form, IsaacLab is not installed next to
this package and nothing here is compared with it.  ``rolled_over`` is the servo surrogate's own flag.

No term computes anything in Python.  Each carries ``describe(env, **params) -> (kind, mask, p0, p1)``: the entry of the
table the simulator's kernel evaluates inside its own launch (include/catppo.h, catppo_servo_term_entry).  Calling a term
directly raises ``TypeError``; a termination function without ``describe`` is an error of the manager, not a slow path.
"""
from __future__ import annotations

import math
import types

import numpy as np

from cat_envs import native

K = native.SERVO_TERM_KINDS
MAX_TERMS = native.SERVO_TERM_MAX_TERMS
NUM_JOINTS, NUM_BODIES = 12, 17


def _f32(x) -> float:
    return float(np.float32(x))


def _refuse(name):
    raise TypeError(f"{name}: the servo task evaluates terminations inside the simulator launch; the term only describes "
                    f"itself to the termination manager (describe(env, **params)) and is never called")


def _mask(env, cfg, what: str, default: str) -> int:
    """bit i set: joint / body i of ``scene[cfg.name]`` is selected (``cfg`` None: all of ``scene[default]``)"""
    names_attr, ids_attr = what + "_names", what + "_ids"
    if cfg is None:
        return (1 << len(getattr(env.scene[default], names_attr))) - 1
    if getattr(cfg, names_attr, None) is not None:
        cfg.resolve(env.scene)                               # a selection that matches nothing raises ValueError
    ids = getattr(cfg, ids_attr)
    if isinstance(ids, slice):
        ids = range(*ids.indices(len(getattr(env.scene[cfg.name], names_attr))))
    mask = 0
    for i in ids:
        mask |= 1 << int(i)
    if mask == 0:
        raise ValueError(f"the {what} selection is empty")
    return mask


def _term(describe):
    def wrap(func):
        func.describe = describe
        return func
    return wrap


def _bounds(bounds):
    lo, hi = float(bounds[0]), float(bounds[1])
    if hi < lo:
        raise ValueError(f"bounds {tuple(bounds)}: hi < lo")
    return _f32(lo), _f32(hi)


@_term(lambda env: (K["time_out"], 0, 0.0, 0.0))
def time_out(env):
    """the episode length reaches the maximum: a truncation (``time_out=True``)"""
    _refuse("time_out")


@_term(lambda env, threshold, sensor_cfg: (K["illegal_contact"], _mask(env, sensor_cfg, "body", "contact_forces"),
                                           _f32(threshold), 0.0))
def illegal_contact(env, threshold: float, sensor_cfg):
    """the contact force on a selected body exceeds ``threshold`` in some slot of the sensor's history"""
    _refuse("illegal_contact")


@_term(lambda env, limit, asset_cfg=None: (K["upside_down"], 0, _f32(limit), 0.0))
def upside_down(env, limit: float, asset_cfg=None):
    """|projected gravity xy| > limit (the reference's term)"""
    _refuse("upside_down")


@_term(lambda env, limit_angle, asset_cfg=None: (K["bad_orientation"], 0, _f32(math.cos(limit_angle)), 0.0))
def bad_orientation(env, limit_angle: float, asset_cfg=None):
    """acos(-g_z) > limit_angle, evaluated as -g_z < cos(limit_angle): p0 = f32(cos(limit_angle))"""
    _refuse("bad_orientation")


@_term(lambda env, minimum_height, asset_cfg=None: (K["root_height_below_minimum"], 0, _f32(minimum_height), 0.0))
def root_height_below_minimum(env, minimum_height: float, asset_cfg=None):
    _refuse("root_height_below_minimum")


@_term(lambda env, bounds, asset_cfg=None: (K["joint_pos_out_of_manual_limit"], _mask(env, asset_cfg, "joint", "robot"),
                                            *_bounds(bounds)))
def joint_pos_out_of_manual_limit(env, bounds, asset_cfg=None):
    _refuse("joint_pos_out_of_manual_limit")


@_term(lambda env, max_velocity, asset_cfg=None: (K["joint_vel_out_of_manual_limit"], _mask(env, asset_cfg, "joint", "robot"),
                                                  _f32(max_velocity), 0.0))
def joint_vel_out_of_manual_limit(env, max_velocity: float, asset_cfg=None):
    _refuse("joint_vel_out_of_manual_limit")


@_term(lambda env: (K["rolled_over"], 0, 0.0, 0.0))
def rolled_over(env):
    """roll^2 + pitch^2 > tilt_max^2: the surrogate's own roll-over flag (this project's term)"""
    _refuse("rolled_over")


def cfg_items(cfg):
    items = cfg.items() if isinstance(cfg, dict) else cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None]


def describe_term(name, term, env):
    """the entry ``(kind, mask, p0, p1)`` of one term; every error names the term"""
    describe = getattr(term.func, "describe", None)
    if describe is None:
        raise ValueError(f"termination term '{name}': {getattr(term.func, '__name__', term.func)!r} has no describe(); the "
                         f"servo task evaluates terminations inside the simulator launch and runs no Python termination function")
    try:
        kind, mask, p0, p1 = describe(env, **term.params)
    except ValueError as e:
        raise ValueError(f"termination term '{name}': {e}") from e
    if not (math.isfinite(p0) and math.isfinite(p1)):
        raise ValueError(f"termination term '{name}': params must be finite, got {p0}, {p1}")
    if bool(term.time_out) != (kind == K["time_out"]):
        raise ValueError(f"termination term '{name}': time_out=True goes with mdp.time_out and with no other term "
                         f"(the env step's time-out is the episode length's)")
    return int(kind), int(mask), float(p0), float(p1)


def build_table(cfg, joint_names, body_names):
    """the table of a ``TerminationsCfg``: one ``(name, kind, mask, p0, p1)`` per term in cfg order, from the cfg, the robot's
    joint names and the contact sensor's body names; needs no device.  ``ValueError`` (naming the term) for a func without
    ``describe``, ``time_out=True`` on another term than ``time_out`` or ``time_out`` without it, an empty joint or body
    selection, ``bounds`` with hi < lo and more than 15 terms; and for a block that does not hold exactly one time-out term."""
    robot = types.SimpleNamespace(joint_names=list(joint_names), body_names=list(body_names))
    sensor = types.SimpleNamespace(joint_names=[], body_names=list(body_names))
    env = types.SimpleNamespace(scene={"robot": robot, "contact_forces": sensor})
    table = []
    for name, term in cfg_items(cfg):
        if len(table) == MAX_TERMS:
            raise ValueError(f"termination term '{name}': more than {MAX_TERMS} terms, the simulator evaluates at most {MAX_TERMS}")
        table.append((name, *describe_term(name, term, env)))
    outs = [row[0] for row in table if row[1] == K["time_out"]]
    if len(outs) != 1:
        raise ValueError(f"cfg.terminations needs exactly one time_out term (time_out=True), it has {len(outs)} {outs}: the env "
                         f"step's time-out is the episode length's and the block has to name it")
    return table


def fold_log(names, sums):
    """``Episode_Termination/<name>`` from the 16 fp64 column sums of the record: the share of the ended episodes whose last
    step had the term set; None if none ended"""
    count = float(sums[15])
    if count <= 0.0:
        return None
    return {f"Episode_Termination/{n}": float(sums[k]) / count for k, n in enumerate(names)}
