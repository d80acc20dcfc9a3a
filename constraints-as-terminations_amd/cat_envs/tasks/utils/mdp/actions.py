"""Joint action terms of the servo task (the reference's ``mdp/`` path; DESIGN section 9, "Actions").

The names and fields are IsaacLab's ``isaaclab.envs.mdp.actions`` (``JointPositionActionCfg``,
``RelativeJointPositionActionCfg``, ``JointVelocityActionCfg``, ``JointEffortActionCfg``) - PARITY UNPINNED: the rules are
restated from their published form, IsaacLab is not installed next to this package and nothing here is compared with it.

No term computes anything in Python.  ``build_table`` turns an ``ActionsCfg`` into one entry per simulator joint - which
action column drives it, through which scale, offset and clip, and as what kind of target - and the simulator's kernel
evaluates the entries inside its own launch (include/catppo.h, catppo_servo_action_entry).
"""
from __future__ import annotations

import math
import re

import numpy as np

from cat_envs import native
from cat_envs.shim import (JointEffortActionCfg, JointPositionActionCfg, JointVelocityActionCfg,  # noqa: F401  (the block's term cfgs)
                           RelativeJointPositionActionCfg)

K = native.SERVO_ACTION_KINDS
NUM_JOINTS = 12
KIND_NAMES = {v: k for k, v in K.items()}


def _f32(x) -> float:
    return float(np.float32(x))


# kind of a term cfg; RelativeJointPositionActionCfg first: under IsaacLab it subclasses nothing of the others, and the
# order makes no difference to the fallbacks either
KIND_OF = ((RelativeJointPositionActionCfg, K["relative_joint_position"]), (JointPositionActionCfg, K["joint_position"]),
           (JointVelocityActionCfg, K["joint_velocity"]), (JointEffortActionCfg, K["joint_effort"]))
TERM_CFGS = (JointPositionActionCfg, RelativeJointPositionActionCfg, JointVelocityActionCfg, JointEffortActionCfg)


def cfg_items(cfg):
    items = cfg.items() if isinstance(cfg, dict) else cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None]


def _select(name, patterns, joint_names, preserve_order):
    """ids of the joints that ``patterns`` select: in asset order, or in the list's order with ``preserve_order``"""
    if patterns is None or isinstance(patterns, str):
        patterns = [".*"] if patterns is None else [patterns]
    patterns = list(patterns)
    for p in patterns:
        if not any(re.fullmatch(p, jn) for jn in joint_names):
            raise ValueError(f"action term '{name}': joint_names entry '{p}' matches no joint of {list(joint_names)}")
    if preserve_order:
        ids = []
        for p in patterns:
            ids += [j for j, jn in enumerate(joint_names) if re.fullmatch(p, jn) and j not in ids]
    else:
        ids = [j for j, jn in enumerate(joint_names) if any(re.fullmatch(p, jn) for p in patterns)]
    if not ids:
        raise ValueError(f"action term '{name}': the joint selection is empty")
    return ids


def _per_joint(name, what, value, ids, joint_names, default):
    """``value`` (a number or ``{regex: number or pair}``) per selected joint; a joint no key matches gets ``default``"""
    if value is None:
        return [default] * len(ids)
    if not isinstance(value, dict):
        return [value] * len(ids)
    out = [default] * len(ids)
    for key, v in value.items():
        hit = [i for i, j in enumerate(ids) if re.fullmatch(key, joint_names[j])]
        if not hit:
            raise ValueError(f"action term '{name}': {what} key '{key}' matches no joint of the term "
                             f"{[joint_names[j] for j in ids]}")
        for i in hit:
            out[i] = v
    return out


def describe_term(name, term, joint_names, default_joint_pos):
    """the columns of one term: ``[(joint id, kind, scale, offset, clip or None), ...]`` in column order, rounded to fp32;
    every error names the term"""
    if not isinstance(term, TERM_CFGS):
        raise TypeError(f"Configuration for action term '{name}' is not one of the joint action term cfgs "
                        f"({', '.join(c.__name__ for c in TERM_CFGS)}). Received: '{type(term)}'.")
    if term.asset_name != "robot":
        raise ValueError(f"action term '{name}': asset_name '{term.asset_name}' names no articulation (the scene has 'robot')")
    kind = next(k for c, k in KIND_OF if isinstance(term, c))
    ids = _select(name, term.joint_names, joint_names, bool(term.preserve_order))
    scales = _per_joint(name, "scale", term.scale, ids, joint_names, 1.0)
    offsets = _per_joint(name, "offset", term.offset, ids, joint_names, 0.0)
    if kind == K["joint_position"] and getattr(term, "use_default_offset", True):
        offsets = [float(default_joint_pos[j]) for j in ids]
    elif kind == K["joint_velocity"] and getattr(term, "use_default_offset", True):
        offsets = [0.0] * len(ids)                           # the surrogate's default joint velocity
    elif kind == K["relative_joint_position"] and getattr(term, "use_zero_offset", True):
        offsets = [0.0] * len(ids)
    clips = _per_joint(name, "clip", term.clip, ids, joint_names, None)
    cols = []
    for j, s, o, c in zip(ids, scales, offsets, clips):
        s, o = float(s), float(o)
        if not (math.isfinite(s) and math.isfinite(o)):
            raise ValueError(f"action term '{name}': scale and offset of joint '{joint_names[j]}' must be finite, got {s}, {o}")
        if c is not None:
            lo, hi = float(c[0]), float(c[1])
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"action term '{name}': clip of joint '{joint_names[j]}' must be finite, got ({lo}, {hi})")
            if lo > hi:
                raise ValueError(f"action term '{name}': clip of joint '{joint_names[j]}' has lo {lo} > hi {hi}")
            c = (_f32(lo), _f32(hi))
        cols.append((int(j), kind, _f32(s), _f32(o), c))
    return cols


def build_table(cfg, joint_names, default_joint_pos):
    """(entries, terms) of an ``ActionsCfg``; pure, needs no device.  ``entries``: 12 ``(col, kind, scale, offset, clip)``,
    one per simulator joint (``col`` -1, kind 0 for a joint no term drives; ``clip`` None or ``(lo, hi)``): what
    ``Solo12ServoSim.set_action_table`` takes.  ``terms``: ``{name: {"kind", "slice": (first column, end), "joint_ids"}}`` in
    cfg order - the columns are the terms' concatenated in that order, within a term in asset order or, with
    ``preserve_order``, in the order of ``joint_names``.  ``ValueError`` (naming the term) for a joint two terms drive, an
    empty selection, a regex key that matches nothing, a clip with lo > hi, a value that is not finite; and for an empty
    block."""
    joint_names = list(joint_names)
    entries = [(-1, K["none"], 1.0, 0.0, None)] * len(joint_names)
    owner, terms, at = {}, {}, 0
    for name, term in cfg_items(cfg):
        cols = describe_term(name, term, joint_names, default_joint_pos)
        for i, (j, kind, s, o, c) in enumerate(cols):
            if j in owner:
                raise ValueError(f"action term '{name}': joint '{joint_names[j]}' is already driven by term '{owner[j]}'")
            owner[j] = name
            entries[j] = (at + i, kind, s, o, c)
        terms[name] = {"kind": KIND_NAMES[cols[0][1]], "slice": (at, at + len(cols)), "joint_ids": [c[0] for c in cols]}
        at += len(cols)
    if not terms:
        raise ValueError("cfg.actions has no term: nothing drives the robot (leave cfg.actions unset for the simulator's "
                         "built-in position action)")
    return entries, terms


def action_spec(entries, terms, joint_names):
    """the output contract of a deployed policy: per action column its term, the joint it drives, the kind of target, scale,
    offset and clip; JSON-serialisable"""
    width = max(t["slice"][1] for t in terms.values())
    cols = [None] * width
    for j, (col, kind, s, o, c) in enumerate(entries):
        if col >= 0:
            term = next(n for n, t in terms.items() if t["slice"][0] <= col < t["slice"][1])
            cols[col] = {"column": col, "term": term, "joint": joint_names[j], "joint_id": j, "kind": KIND_NAMES[kind],
                         "scale": s, "offset": o, "clip": None if c is None else [c[0], c[1]]}
    return {"action_dim": width, "order": "scale, offset, clip (IsaacLab JointAction.process_actions)",
            "joint_order": list(joint_names),
            "undriven_joints": [joint_names[j] for j, e in enumerate(entries) if e[0] < 0],
            "terms": {n: {"kind": t["kind"], "slice": list(t["slice"])} for n, t in terms.items()}, "columns": cols}
