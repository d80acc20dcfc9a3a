"""``ArticulationCfg`` and actuator cfg fallbacks (isaaclab's are used when importable).

The names and fields are IsaacLab's ``isaaclab.assets.ArticulationCfg`` and ``isaaclab.actuators`` cfgs.  Only what the servo
surrogate's actuator model reads does anything (``cat_envs.tasks.utils.mdp.actuators.build_table``): ``actuators`` and
``init_state.joint_pos`` / ``joint_vel``.  Every other field is accepted, kept and listed as inert.
"""
from __future__ import annotations

from typing import Any

from .configclass import MISSING, configclass

try:  # pragma: no cover
    from isaaclab.actuators import DCMotorCfg, DelayedPDActuatorCfg, IdealPDActuatorCfg, ImplicitActuatorCfg  # type: ignore
    from isaaclab.actuators import ActuatorBaseCfg  # type: ignore
    from isaaclab.assets import ArticulationCfg  # type: ignore
except Exception:

    @configclass
    class ActuatorBaseCfg:
        """the fields IsaacLab's actuator cfgs share; each value is a float or ``{regex: float}`` (None: not set)"""
        joint_names_expr: Any = MISSING          # list of regular expressions
        effort_limit: Any = None
        velocity_limit: Any = None
        effort_limit_sim: Any = None             # accepted, inert
        velocity_limit_sim: Any = None           # accepted, inert
        stiffness: Any = MISSING
        damping: Any = MISSING
        armature: Any = None
        friction: Any = None                     # must be 0 or None: the surrogate has no joint friction

    @configclass
    class ImplicitActuatorCfg(ActuatorBaseCfg):
        """PD law evaluated by the physics engine; here the explicit PD law of the ideal actuator"""

    @configclass
    class IdealPDActuatorCfg(ActuatorBaseCfg):
        """explicit PD law, torque clipped to +- effort_limit"""

    @configclass
    class DCMotorCfg(IdealPDActuatorCfg):
        """ideal PD whose torque is clipped by the motor's torque-speed curve"""
        saturation_effort: float = MISSING

    @configclass
    class DelayedPDActuatorCfg(IdealPDActuatorCfg):
        """ideal PD whose command arrives ``min_delay .. max_delay`` physics steps late"""
        min_delay: int = 0
        max_delay: int = 0

    @configclass
    class ArticulationCfg:
        @configclass
        class InitialStateCfg:
            pos: tuple = (0.0, 0.0, 0.0)
            rot: tuple = (1.0, 0.0, 0.0, 0.0)
            lin_vel: tuple = (0.0, 0.0, 0.0)
            ang_vel: tuple = (0.0, 0.0, 0.0)
            joint_pos: dict = {".*": 0.0}
            joint_vel: dict = {".*": 0.0}

        prim_path: Any = None
        spawn: Any = None
        init_state: InitialStateCfg = InitialStateCfg()
        collision_group: int = 0
        debug_vis: bool = False
        soft_joint_pos_limit_factor: float = 1.0
        actuators: dict = MISSING
