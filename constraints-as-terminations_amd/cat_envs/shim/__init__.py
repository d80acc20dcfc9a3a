"""Minimal stand-ins for the IsaacLab symbols the CaT hot path touches.

When IsaacLab is importable its own classes are used; otherwise these fallbacks give the same
surface: ``configclass`` (dataclass tolerant of un-annotated overrides, mutable defaults,
``MISSING`` placeholders; ``to_dict/replace/copy``), ``ManagerBase`` / ``ManagerTermBase`` /
``ManagerTermBaseCfg``, ``SceneEntityCfg`` (regex joint / body name resolution), ``ArticulationCfg`` with the actuator cfgs and a tiny task
registry replacing ``gym.register`` / ``gym.make`` / ``load_cfg_from_registry``.
"""
from .actuators import (ArticulationCfg, DCMotorCfg, DelayedPDActuatorCfg, IdealPDActuatorCfg,  # noqa: F401
                        ImplicitActuatorCfg)
from .configclass import MISSING, configclass  # noqa: F401
from .managers import (AdditiveUniformNoiseCfg, CurriculumTermCfg, EventTermCfg, JointEffortActionCfg,  # noqa: F401
                       JointPositionActionCfg, JointVelocityActionCfg, ManagerBase, ManagerTermBase, ManagerTermBaseCfg,
                       ObservationGroupCfg, ObservationTermCfg, RelativeJointPositionActionCfg, RewardTermCfg, SceneEntityCfg,
                       TerminationTermCfg)
from .registry import (apply_overrides, hydra_task_config, load_cfg_from_registry, make, register,  # noqa: F401
                       registry)
