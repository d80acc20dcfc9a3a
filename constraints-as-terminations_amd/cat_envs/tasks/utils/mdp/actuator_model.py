"""Actuator model of the servo task ("Actuators"), reachable as ``env.actuators``.

IsaacLab's articulation calls ``compute`` of every actuator once per physics step.  This one calls nothing: it turns the
robot's ``actuators`` into the table the simulator's kernel evaluates inside its own launch
(``Solo12ServoSim.set_actuator_table``) - per joint the gains, the inertia, the effort limit, the DC motor's curve and the
delay range of its group.
"""
from __future__ import annotations

import re

import torch

from . import actuators as UM


class ActuatorModel:
    def __init__(self, robot_cfg, env, table=None, randomization=None):
        """``randomization``: the block of ``mdp.randomization.build_randomization`` when the env randomises the robot;
        ``set_gains`` then repeats its stability check on the new gains"""
        self.cfg, self._env, self._randomization = robot_cfg, env, randomization
        self._joint_names = list(env.scene["robot"].joint_names)
        if table is None:
            from cat_envs.tasks.utils.cat.cat_env import DEFAULT_JOINT_POS
            table = UM.build_table(robot_cfg, self._joint_names, env.cfg.synthetic, env.cfg.decimation, DEFAULT_JOINT_POS)
        self._entries, self._spec = [dict(e) for e in table[0]], table[1]
        self._push()

    def _push(self):
        """the table with the current gains and limits, onto the device: the next launch reads it"""
        self._env.sim.set_actuator_table(self._entries)

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def active_groups(self) -> list:
        return list(self._spec["groups"])

    def _column(self, key) -> torch.Tensor:
        return torch.tensor([e[key] for e in self._entries], dtype=torch.float32)

    @property
    def stiffness(self) -> torch.Tensor:
        return self._column("kp")

    @property
    def damping(self) -> torch.Tensor:
        return self._column("kd")

    @property
    def effort_limit(self) -> torch.Tensor:
        return self._column("effort_limit")

    @property
    def entries(self) -> list:
        """the table as the device holds it: 12 dicts, one per simulator joint"""
        return [dict(e) for e in self._entries]

    def get_group(self, name: str) -> dict:
        """kind, joints and delay range of one actuator group, with the current gains and limits of its joints"""
        if name not in self._spec["groups"]:
            raise ValueError(f"Actuator group '{name}' not found.")
        g = dict(self._spec["groups"][name])
        ids = g["joint_ids"]
        g.update(stiffness=[self._entries[j]["kp"] for j in ids], damping=[self._entries[j]["kd"] for j in ids],
                 effort_limit=[self._entries[j]["effort_limit"] for j in ids])
        return g

    def set_gains(self, stiffness=None, damping=None, effort_limit=None, joint_names=".*"):
        """new gains and effort limits (a number, or ``{regex: number}`` over the selected joints) of the joints that
        ``joint_names`` (a regex or a list of them) selects.  They are on the device before the next launch (one
        stream-ordered copy of the table, also under graph replay).  Kinds, groups and delay ranges are those of
        construction"""
        pats = [joint_names] if isinstance(joint_names, str) else list(joint_names)
        ids = [j for j, jn in enumerate(self._joint_names) if any(re.fullmatch(p, jn) for p in pats)]
        if not ids:
            raise ValueError(f"set_gains: joint_names {joint_names!r} match no joint of {self._joint_names}")
        new = [dict(e) for e in self._entries]
        for key, what, value in (("kp", "stiffness", stiffness), ("kd", "damping", damping),
                                 ("effort_limit", "effort_limit", effort_limit)):
            if value is None:
                continue
            if isinstance(value, dict):                      # a selected joint no key matches keeps its value
                for rx, v in value.items():
                    hit = [j for j in ids if re.fullmatch(rx, self._joint_names[j])]
                    for j, x in zip(hit, UM._per_joint("set_gains", what, {rx: v}, hit or ids, self._joint_names, 0.0)):
                        new[j][key] = x
            else:
                for j, x in zip(ids, UM._per_joint("set_gains", what, value, ids, self._joint_names, 0.0)):
                    new[j][key] = x
        if new != self._entries:
            if self._randomization is not None:              # the worst corner of the ranges, on the new gains
                from . import randomization as RZ
                RZ.check_corners(self._randomization, new, self._env.cfg.sim.dt)
            self._entries = new
            self._push()

    def spec(self) -> dict:
        groups = {n: {k: v for k, v in self.get_group(n).items() if k not in ("stiffness", "damping", "effort_limit")}
                  for n in self._spec["groups"]}
        return UM.actuator_spec(self._entries, groups, self._joint_names, self.cfg)

    def __str__(self) -> str:
        msg = f"<ActuatorModel> contains {len(self._spec['groups'])} actuator groups.\n"
        for name, g in self._spec["groups"].items():
            msg += f"  group {name!r}: {g['kind']}, delay {g['min_delay']} .. {g['max_delay']} physics steps\n"
        for j, e in enumerate(self._entries):
            msg += (f"  joint {j:2d} {self._joint_names[j]:<8s} stiffness {e['kp']:g} damping {e['kd']:g} inertia {e['inertia']:g} "
                    f"effort limit {e['effort_limit']:g}\n")
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """per joint: group, kind and delay range (gains and limits may move; they are part of the state)"""
        return [[int(e["group"]), bool(e["dc_motor"]), int(e["min_delay"]), int(e["max_delay"])] for e in self._entries]

    def state_dict(self) -> dict:
        return {"params": [[float(e[k]) for k in ("kp", "kd", "inertia", "effort_limit", "saturation_effort", "velocity_limit")]
                           for e in self._entries]}

    def check_state_dict(self, sd: dict):
        if not isinstance(sd, dict) or "params" not in sd:
            raise ValueError("run state: the actuators' part lacks 'params'")
        if len(sd["params"]) != len(self._entries) or any(len(p) != 6 for p in sd["params"]):
            raise ValueError("run state: the actuator table's params do not fit this env's robot")

    def load_state_dict(self, sd: dict):
        self.check_state_dict(sd)
        keys = ("kp", "kd", "inertia", "effort_limit", "saturation_effort", "velocity_limit")
        self._entries = [dict(e, **{k: float(v) for k, v in zip(keys, p)}) for e, p in zip(self._entries, sd["params"])]
        self._push()
