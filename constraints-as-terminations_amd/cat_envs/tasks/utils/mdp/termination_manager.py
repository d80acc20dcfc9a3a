"""Termination manager of the servo task ("Terminations").

IsaacLab's ``TerminationManager`` calls one torch function per term and step.  This one calls none: it turns the
``TerminationsCfg`` into the table the simulator's kernel evaluates inside its own launch
(``Solo12ServoSim.set_termination_table``).  Which terms fired in a step is float 0 of the row's ``term_state`` field; how
the ended episodes ended is the record the same launch keeps.  ``terminated`` / ``time_outs`` / ``dones`` are the env's own
``reset_terminated`` / ``reset_time_outs`` / ``reset_buf``, which ``env_pre_step`` / ``rollout_pre`` fill from the row's
``hard_reset`` field and the episode length as before.
"""
from __future__ import annotations

import torch

from cat_envs.shim import TerminationTermCfg

from . import terminations as TM


class TerminationManager:
    def __init__(self, cfg: object, env, table=None):
        self.cfg, self._env = cfg, env
        for name, term in TM.cfg_items(cfg):
            if not isinstance(term, TerminationTermCfg):
                raise TypeError(f"Configuration for term '{name}' is not TerminationTermCfg. Received: '{type(term)}'.")
        robot, sensor = env.scene["robot"], env.scene["contact_forces"]
        self._table = list(table) if table is not None else TM.build_table(cfg, robot.joint_names, sensor.body_names)
        self._names = [row[0] for row in self._table]
        self._cfgs = {n: t for n, t in TM.cfg_items(cfg)}
        self._rows = {row[0]: tuple(row[1:]) for row in self._table}                # name -> (kind, mask, p0, p1)
        self._configured = [[n, *self._rows[n]] for n in self._names]
        self._scene = env.scene
        self._push()
        self._state = env.sim.view("term_state")

    def _push(self):
        """the table with the current params, onto the device: the next launch reads it"""
        self._env.sim.set_termination_table([self._rows[n] for n in self._names])

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def active_terms(self) -> list:
        return list(self._names)

    @property
    def terminated(self) -> torch.Tensor:
        return self._env.reset_terminated

    @property
    def time_outs(self) -> torch.Tensor:
        return self._env.reset_time_outs

    @property
    def dones(self) -> torch.Tensor:
        return self._env.reset_buf

    def _index(self, name: str) -> int:
        if name not in self._rows:
            raise ValueError(f"Termination term '{name}' not found.")
        return self._names.index(name)

    def get_term(self, name: str) -> torch.Tensor:
        """bool [N]: the term fired in the last step; device ops on the row's ``term_state`` field, no synchronisation"""
        k = self._index(name)
        return (self._state[:, 0].to(torch.int32) >> k) & 1 != 0

    def get_term_cfg(self, term_name: str) -> TerminationTermCfg:
        self._index(term_name)
        return self._cfgs[term_name]

    def set_term_cfg(self, term_name: str, cfg: TerminationTermCfg):
        """new params are on the device before the next launch (one stream-ordered copy of the table, also under graph
        replay).  The term's kind, its joint or body selection and the term set are those of construction"""
        self._index(term_name)
        row = TM.describe_term(term_name, cfg, self._env)
        if row[:2] != self._rows[term_name][:2]:
            raise ValueError(f"termination term '{term_name}': the term's function and its joint or body selection are fixed "
                             f"when the env is built; only params may change")
        self._cfgs[term_name] = cfg
        if row != self._rows[term_name]:
            self._rows[term_name] = row
            self._push()

    def compute(self) -> torch.Tensor:
        """the env's ``reset_buf``.  Launches nothing - the simulator's own launch of this step has evaluated the terms"""
        return self._env.reset_buf

    def reset(self, env_ids=None):
        return {}

    @property
    def record(self) -> torch.Tensor:
        return self._env.sim.termination_record

    def pop_log(self):
        """``{"Episode_Termination/<name>": share}`` over every episode that ended since the last call: the share of them
        whose last step had the term set; None if none ended.  Then the record is zeroed in place.  One device reduction
        and one copy to the host, folded in fp64"""
        rec = self.record
        sums = rec.sum(0, dtype=torch.float64).cpu().numpy()
        rec.zero_()
        return TM.fold_log(self._names, sums)

    def __str__(self) -> str:
        kind_name = {v: k for k, v in TM.K.items()}
        msg = f"<TerminationManager> contains {len(self._names)} active terms.\n"
        for i, n in enumerate(self._names):
            kind, mask, p0, p1 = self._rows[n]
            msg += (f"  {i:2d} {n:<24s} {kind_name[kind]:<30s} time_out {str(kind == TM.K['time_out']):<5s} "
                    f"mask {mask:#07x} p0 {p0:g} p1 {p1:g}\n")
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """names, kinds and masks in table order (the params may move; they are part of the state)"""
        return [[n, int(self._rows[n][0]), int(self._rows[n][1])] for n in self._names]

    def state_dict(self) -> dict:
        return {"record": self.record, "params": {n: [float(self._rows[n][2]), float(self._rows[n][3])] for n in self._names}}

    def check_state_dict(self, sd: dict):
        if not isinstance(sd, dict) or "record" not in sd or "params" not in sd:
            raise ValueError("run state: the terminations' part lacks 'record' or 'params'")
        rec = sd["record"]
        if tuple(rec.shape) != tuple(self.record.shape) or rec.dtype != self.record.dtype:
            raise ValueError(f"run state: termination record is {tuple(rec.shape)} {rec.dtype}, this env's is "
                             f"{tuple(self.record.shape)} {self.record.dtype}")
        if list(sd["params"]) != self._names:
            raise ValueError(f"run state: termination terms {list(sd['params'])}, this env has {self._names}")

    def load_state_dict(self, sd: dict):
        """in place: the descriptor holds the record's address"""
        self.check_state_dict(sd)
        self.record.copy_(sd["record"])
        for n, (p0, p1) in sd["params"].items():
            self._rows[n] = (*self._rows[n][:2], float(p0), float(p1))
        self._push()
