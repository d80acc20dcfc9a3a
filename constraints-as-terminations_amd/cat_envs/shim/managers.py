"""ManagerBase / term cfg / SceneEntityCfg fallbacks (isaaclab's are used when importable)."""
from __future__ import annotations

import inspect
import re
from typing import Any, Callable, Sequence

from .configclass import MISSING, configclass

try:  # pragma: no cover
    from isaaclab.managers import SceneEntityCfg  # type: ignore
    from isaaclab.managers.manager_base import ManagerBase, ManagerTermBase  # type: ignore
    from isaaclab.managers.manager_term_cfg import CurriculumTermCfg, ManagerTermBaseCfg  # type: ignore
    from isaaclab.managers.manager_term_cfg import RewardTermCfg  # type: ignore
    from isaaclab.managers.manager_term_cfg import ObservationGroupCfg, ObservationTermCfg  # type: ignore
    from isaaclab.managers.manager_term_cfg import EventTermCfg  # type: ignore
    from isaaclab.managers.manager_term_cfg import TerminationTermCfg  # type: ignore
    from isaaclab.envs.mdp.actions import (JointEffortActionCfg, JointPositionActionCfg, JointVelocityActionCfg,  # type: ignore
                                           RelativeJointPositionActionCfg)
    from isaaclab.utils.noise import AdditiveUniformNoiseCfg  # type: ignore
    HAVE_ISAACLAB = True
except Exception:
    HAVE_ISAACLAB = False

    @configclass
    class ManagerTermBaseCfg:
        func: Callable | Any = MISSING
        params: dict = {}

    @configclass
    class CurriculumTermCfg(ManagerTermBaseCfg):
        pass

    @configclass
    class RewardTermCfg(ManagerTermBaseCfg):
        """IsaacLab's RewTerm: the step's reward is the sum of ``func(env, **params) * weight * dt`` over the terms"""
        weight: float = MISSING

    @configclass
    class ObservationTermCfg(ManagerTermBaseCfg):
        """IsaacLab's ObsTerm: ``func(env, **params)``, then noise, clip and scale, in this order"""
        noise: Any = None
        clip: Any = None              # (lo, hi) or None
        scale: Any = None             # a number, one per element, or None
        history_length: int = 0       # frames the term keeps, oldest first; 0 and 1: the current frame only
        flatten_history_dim: bool = True

    @configclass
    class EventTermCfg(ManagerTermBaseCfg):
        """IsaacLab's EventTerm: ``mode`` is "startup", "reset" or "interval" (the latter with ``interval_range_s``)"""
        mode: str = MISSING
        interval_range_s: Any = None
        is_global_time: bool = False

    @configclass
    class TerminationTermCfg(ManagerTermBaseCfg):
        """IsaacLab's DoneTerm: ``time_out`` marks the term whose firing is a truncation, not a termination"""
        time_out: bool = False

    @configclass
    class JointActionCfg:
        """the fields IsaacLab's joint action terms share"""
        asset_name: str = "robot"
        joint_names: Any = None                  # list of regular expressions
        scale: Any = 1.0                         # float or {regex: float}
        offset: Any = 0.0                        # float or {regex: float}
        preserve_order: bool = False             # the term's columns follow ``joint_names``, not the asset's joint order
        clip: Any = None                         # {regex: (lo, hi)} on the processed action
        debug_vis: bool = False                  # accepted, ignored

    @configclass
    class JointPositionActionCfg(JointActionCfg):
        """processed action = position target; ``use_default_offset``: the offset is the joint's default position"""
        use_default_offset: bool = True

    @configclass
    class RelativeJointPositionActionCfg(JointActionCfg):
        """processed action + current position = position target; ``use_zero_offset``: the offset is zero"""
        use_zero_offset: bool = True

    @configclass
    class JointVelocityActionCfg(JointActionCfg):
        """processed action = velocity target; ``use_default_offset``: the offset is the default joint velocity"""
        use_default_offset: bool = True

    @configclass
    class JointEffortActionCfg(JointActionCfg):
        """processed action = joint torque"""

    @configclass
    class ObservationGroupCfg:
        """IsaacLab's ObsGroup: its ObsTerm attributes in definition order are the group's terms"""
        concatenate_terms: bool = True
        enable_corruption: bool = False
        history_length: Any = None    # an int overrides history_length and flatten_history_dim of every term
        flatten_history_dim: bool = True

    @configclass
    class AdditiveUniformNoiseCfg:
        """IsaacLab's Unoise: x + U(n_min, n_max)"""
        n_min: float = -1.0
        n_max: float = 1.0
        operation: str = "add"

    class SceneEntityCfg:
        """Names are resolved to ids against ``scene[name].joint_names / body_names``."""

        def __init__(self, name: str, joint_names=None, joint_ids=slice(None), body_names=None,
                     body_ids=slice(None), preserve_order: bool = False):
            self.name, self.joint_names, self.body_names = name, joint_names, body_names
            self.joint_ids, self.body_ids, self.preserve_order = joint_ids, body_ids, preserve_order

        @staticmethod
        def _match(patterns, names, preserve_order):
            if isinstance(patterns, str):
                patterns = [patterns]
            if preserve_order:
                ids = [i for p in patterns for i, n in enumerate(names) if re.fullmatch(p, n)]
            else:
                ids = [i for i, n in enumerate(names) if any(re.fullmatch(p, n) for p in patterns)]
            if not ids:
                raise ValueError(f"no name matches {patterns} in {names}")
            return ids

        def resolve(self, scene) -> None:
            entity = scene[self.name]
            if self.joint_names is not None:
                ids = self._match(self.joint_names, entity.joint_names, self.preserve_order)
                self.joint_ids = slice(None) if ids == list(range(len(entity.joint_names))) else ids
            if self.body_names is not None:
                ids = self._match(self.body_names, entity.body_names, self.preserve_order)
                self.body_ids = slice(None) if ids == list(range(len(entity.body_names))) else ids

        def __repr__(self):
            return (f"SceneEntityCfg({self.name!r}, joint_names={self.joint_names}, body_names={self.body_names})")

    class ManagerTermBase:
        def __init__(self, cfg, env):
            self.cfg, self._env = cfg, env

        @property
        def num_envs(self):
            return self._env.num_envs

        @property
        def device(self):
            return self._env.device

        def reset(self, env_ids: Sequence[int] | None = None) -> None:
            pass

        def __call__(self, *args, **kwargs):
            raise NotImplementedError

    class ManagerBase:
        def __init__(self, cfg, env):
            self.cfg = cfg
            self._env = env
            self._prepare_terms()

        @property
        def num_envs(self) -> int:
            return self._env.num_envs

        @property
        def device(self):
            return self._env.device

        def _prepare_terms(self):
            raise NotImplementedError

        def _resolve_common_term_cfg(self, term_name: str, term_cfg, min_argc: int = 1):
            """resolve SceneEntityCfg params against the scene, instantiate class-based terms and
            check that every non-default argument of the term function is supplied."""
            for value in term_cfg.params.values():
                if isinstance(value, SceneEntityCfg) and hasattr(self._env, "scene"):
                    value.resolve(self._env.scene)
            func = term_cfg.func
            if inspect.isclass(func) and issubclass(func, ManagerTermBase):
                term_cfg.func = func = func(cfg=term_cfg, env=self._env)
            if not callable(func):
                raise AttributeError(f"The term '{term_name}' is not callable. Received: {func}")
            target = func.__call__ if isinstance(func, ManagerTermBase) else func
            try:
                sig = inspect.signature(target)
            except (TypeError, ValueError):
                return
            names = [p.name for p in sig.parameters.values()
                     if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)
                     and p.default is inspect.Parameter.empty]
            missing = [n for n in names[min_argc:] if n not in term_cfg.params]
            if missing:
                raise ValueError(f"The term '{term_name}' expects mandatory parameters: {missing}"
                                 f" and received: {list(term_cfg.params)}.")
