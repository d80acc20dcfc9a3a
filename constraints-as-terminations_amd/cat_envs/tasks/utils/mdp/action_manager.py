"""Action manager of the servo task ("Actions").

IsaacLab's ``ActionManager`` calls ``process_actions`` and, once per physics step, ``apply_actions`` of every term.  This
one calls neither: it turns the ``ActionsCfg`` into the table the simulator's kernel evaluates inside its own launch
(``Solo12ServoSim.set_action_table``) - which action column drives which joint, through which scale, offset and clip, as
what kind of target.  ``_action`` / ``_prev_action`` are the raw action history [N, A] that the constraints, the env step's
kernels and the run state read, exactly as on an env without ``cfg.actions``.
"""
from __future__ import annotations

import torch

from . import actions as AM


class ActionManager:
    def __init__(self, cfg: object, env, table=None):
        self.cfg, self._env = cfg, env
        joint_names = env.scene["robot"].joint_names
        self._joint_names = list(joint_names)
        if table is None:
            from cat_envs.tasks.utils.cat.cat_env import DEFAULT_JOINT_POS
            table = AM.build_table(cfg, joint_names, DEFAULT_JOINT_POS)
        self._entries, self._terms = list(table[0]), dict(table[1])
        self._cfgs = {n: t for n, t in AM.cfg_items(cfg)}
        self.total_action_dim = max(t["slice"][1] for t in self._terms.values())
        n, a = env.num_envs, self.total_action_dim
        self._action = torch.zeros(n, a, device=env.device)
        self._prev_action = torch.zeros(n, a, device=env.device)
        self._push()

    def _push(self):
        """the table with the current scales, offsets and clips, onto the device: the next launch reads it"""
        self._env.sim.set_action_table(self._entries, self.total_action_dim)

    # ------------------------------------------------------------------ what _ActionManager has
    def process_action(self, action):
        self._prev_action.copy_(self._action)
        self._action.copy_(action)

    def reset(self, env_ids=None):
        """IsaacLab's ActionManager.reset: the action history of the envs that reset starts from zero (mask, index list or
        None = all)"""
        if env_ids is None or isinstance(env_ids, slice):
            self._action.zero_()
            self._prev_action.zero_()
        elif isinstance(env_ids, torch.Tensor) and env_ids.dtype == torch.bool:
            keep = (~env_ids).unsqueeze(1)
            self._action.mul_(keep)
            self._prev_action.mul_(keep)
        else:
            self._action[env_ids] = 0.0
            self._prev_action[env_ids] = 0.0
        return {}

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def action(self) -> torch.Tensor:
        return self._action

    @property
    def prev_action(self) -> torch.Tensor:
        return self._prev_action

    @property
    def active_terms(self) -> list:
        return list(self._terms)

    @property
    def action_term_dim(self) -> list:
        return [t["slice"][1] - t["slice"][0] for t in self._terms.values()]

    @property
    def entries(self) -> list:
        """the table as the device holds it: 12 ``(col, kind, scale, offset, clip)``, one per simulator joint"""
        return list(self._entries)

    def term_slice(self, name: str) -> tuple:
        if name not in self._terms:
            raise ValueError(f"Action term '{name}' not found.")
        return tuple(self._terms[name]["slice"])

    def get_term(self, name: str):
        """``raw_actions`` (a view of the action history), ``processed_actions`` (device ops on request: scale, offset, clip,
        as the kernel applies them; not on the hot path), ``action_dim``, ``joint_names``"""
        a, b = self.term_slice(name)
        ids = self._terms[name]["joint_ids"]
        mgr = self

        class _Term:
            action_dim = b - a
            joint_names = [mgr._joint_names[j] for j in ids]
            joint_ids = list(ids)

            @property
            def raw_actions(self):
                return mgr._action[:, a:b]

            @property
            def processed_actions(self):
                dev = mgr._action.device
                rows = [mgr._entries[j] for j in ids]
                p = mgr._action[:, a:b] * torch.tensor([r[2] for r in rows], device=dev) + torch.tensor([r[3] for r in rows], device=dev)
                for i, r in enumerate(rows):
                    if r[4] is not None:
                        p[:, i] = torch.where(p[:, i] < r[4][0], torch.full_like(p[:, i], r[4][0]), p[:, i])
                        p[:, i] = torch.where(p[:, i] > r[4][1], torch.full_like(p[:, i], r[4][1]), p[:, i])
                return p
        return _Term()

    def get_term_cfg(self, term_name: str):
        self.term_slice(term_name)
        return self._cfgs[term_name]

    def set_term_cfg(self, term_name: str, cfg):
        """new ``scale``, ``offset`` and ``clip`` are on the device before the next launch (one stream-ordered copy of the
        table, also under graph replay).  The term's joints, kind and columns and which joints are clipped are those of
        construction"""
        self.term_slice(term_name)
        cols = AM.describe_term(term_name, cfg, self._joint_names, self._default_joint_pos())
        old = self._terms[term_name]
        a = old["slice"][0]
        new = [(a + i, kind, s, o, c) for i, (_, kind, s, o, c) in enumerate(cols)]
        fixed = lambda rows: [(r[0], r[1], r[4] is not None) for r in rows]       # noqa: E731
        if [c[0] for c in cols] != old["joint_ids"] or fixed(new) != fixed([self._entries[j] for j in old["joint_ids"]]):
            raise ValueError(f"action term '{term_name}': the term's kind, its joints and their order, and which of them are "
                             f"clipped are fixed when the env is built; only scale, offset and clip bounds may change")
        self._cfgs[term_name] = cfg
        changed = False
        for j, row in zip(old["joint_ids"], new):
            changed |= row != self._entries[j]
            self._entries[j] = row
        if changed:
            self._push()

    def _default_joint_pos(self):
        from cat_envs.tasks.utils.cat.cat_env import DEFAULT_JOINT_POS
        return DEFAULT_JOINT_POS

    def spec(self) -> dict:
        return AM.action_spec(self._entries, self._terms, self._joint_names)

    def __str__(self) -> str:
        msg = f"<ActionManager> contains {len(self._terms)} active terms, {self.total_action_dim} columns.\n"
        for j, (col, kind, s, o, c) in enumerate(self._entries):
            clip = "-" if c is None else f"[{c[0]:g}, {c[1]:g}]"
            msg += (f"  joint {j:2d} {self._joint_names[j]:<8s} column {col:2d} {AM.KIND_NAMES[kind]:<24s} scale {s:g} "
                    f"offset {o:g} clip {clip}\n")
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """per joint: column, kind and whether it is clipped (scale, offset and bounds may move; they are part of the state)"""
        return [[int(c), int(k), cl is not None] for c, k, _, _, cl in self._entries]

    def state_dict(self) -> dict:
        return {"params": [[float(s), float(o), None if c is None else [float(c[0]), float(c[1])]] for _, _, s, o, c in self._entries]}

    def check_state_dict(self, sd: dict):
        if not isinstance(sd, dict) or "params" not in sd:
            raise ValueError("run state: the actions' part lacks 'params'")
        if len(sd["params"]) != len(self._entries) or any((p[2] is None) != (e[4] is None) for p, e in zip(sd["params"], self._entries)):
            raise ValueError("run state: the action table's params do not fit this env's action terms")

    def load_state_dict(self, sd: dict):
        self.check_state_dict(sd)
        self._entries = [(c, k, float(p[0]), float(p[1]), None if p[2] is None else (float(p[2][0]), float(p[2][1])))
                         for (c, k, *_), p in zip(self._entries, sd["params"])]
        self._push()
