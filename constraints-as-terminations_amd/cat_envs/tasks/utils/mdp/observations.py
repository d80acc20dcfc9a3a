"""Observation terms of the servo task (the reference's ``mdp/`` path; DESIGN section 9, "Observations").

The names and signatures are IsaacLab's ``isaaclab.envs.mdp.observations`` - PARITY UNPINNED: the rules are restated from
their published form, IsaacLab is not installed next to this package and nothing here is compared with it.

No term computes anything in Python.  Each carries ``describe(env, **params) -> [(src, bias), ...]``: one pair per float
of the term, ``src`` the index into the simulator row's raw 45-float observation (``ang_vel 3 | gravity 3 | command 3 |
dq 12 | qd 12 | last action 12``) and ``bias`` a constant added to it (None: none).  The observation manager turns the
pairs, the term's noise, clip and scale into the table the simulator's kernel evaluates inside its own launch
(include/catppo.h, catppo_servo_obs_entry).  Calling a term directly raises ``TypeError``; an observation function without
``describe`` is an error of the manager, not a slow path.
"""
from __future__ import annotations

RAW_ANG_VEL, RAW_GRAVITY, RAW_COMMAND, RAW_JOINT_POS, RAW_JOINT_VEL, RAW_ACTION = 0, 3, 6, 9, 21, 33
RAW_WIDTH = 45
NUM_JOINTS = 12


def _refuse(name):
    raise TypeError(f"{name}: the servo task evaluates observations inside the simulator launch; the term only describes "
                    f"itself to the observation manager (describe(env, **params)) and is never called")


def _joint_ids(env, asset_cfg) -> list:
    """the selected joints of ``scene[asset_cfg.name]`` in the order the cfg asks for (``asset_cfg`` None: all, in order)"""
    if asset_cfg is None:
        return list(range(NUM_JOINTS))
    if getattr(asset_cfg, "joint_names", None) is not None:
        asset_cfg.resolve(env.scene)
    ids = asset_cfg.joint_ids
    if isinstance(ids, slice):
        ids = range(*ids.indices(len(env.scene[asset_cfg.name].joint_names)))
    return [int(j) for j in ids]


def _term(describe):
    def wrap(func):
        func.describe = describe
        return func
    return wrap


@_term(lambda env, asset_cfg=None: [(RAW_ANG_VEL + k, None) for k in range(3)])
def base_ang_vel(env, asset_cfg=None):
    """angular velocity of the base in its own frame"""
    _refuse("base_ang_vel")


@_term(lambda env, asset_cfg=None: [(RAW_GRAVITY + k, None) for k in range(3)])
def projected_gravity(env, asset_cfg=None):
    """gravity direction in the base frame"""
    _refuse("projected_gravity")


@_term(lambda env, command_name=None: [(RAW_COMMAND + k, None) for k in range(3)])
def generated_commands(env, command_name: str):
    """the velocity command (vx, vy, wz)"""
    _refuse("generated_commands")


@_term(lambda env, asset_cfg=None: [(RAW_JOINT_POS + j, float(env.default_joint_pos[j])) for j in _joint_ids(env, asset_cfg)])
def joint_pos(env, asset_cfg=None):
    """joint positions: the raw offset from the default pose plus the joint's default (one rounded fp32 add: the model)"""
    _refuse("joint_pos")


@_term(lambda env, asset_cfg=None: [(RAW_JOINT_POS + j, None) for j in _joint_ids(env, asset_cfg)])
def joint_pos_rel(env, asset_cfg=None):
    """joint positions relative to the default pose"""
    _refuse("joint_pos_rel")


@_term(lambda env, asset_cfg=None: [(RAW_JOINT_VEL + j, None) for j in _joint_ids(env, asset_cfg)])
def joint_vel(env, asset_cfg=None):
    """joint velocities (the default joint velocity of the surrogate is zero)"""
    _refuse("joint_vel")


@_term(lambda env, asset_cfg=None: [(RAW_JOINT_VEL + j, None) for j in _joint_ids(env, asset_cfg)])
def joint_vel_rel(env, asset_cfg=None):
    """joint velocities relative to the default (zero) joint velocity"""
    _refuse("joint_vel_rel")


def _action_cols(env, action_name):
    """the columns of the raw action a ``last_action`` term shows: all twelve without ``cfg.actions``; with it the block's
    A columns, or those of the term ``action_name``"""
    terms = getattr(env, "action_terms", None)
    if terms is None:
        return range(NUM_JOINTS)
    if action_name is None:
        return range(max(b for _, b in terms.values()))
    if action_name not in terms:
        raise KeyError(f"action_name '{action_name}' names no action term of cfg.actions ({list(terms)})")
    return range(*terms[action_name])


@_term(lambda env, action_name=None: [(RAW_ACTION + k, None) for k in _action_cols(env, action_name)])
def last_action(env, action_name=None):
    """the raw action of the step that led to this state, in column order (zero in the first state of an episode)"""
    _refuse("last_action")
