"""Reward manager of the servo task ("Rewards").

IsaacLab's ``RewardManager`` calls one torch function per term and step.  This one calls none: it turns the ``RewardsCfg``
into the table the simulator's kernel evaluates inside its own launch (``Solo12ServoSim.set_reward_table``), and reads the
per-term episode sums back from the record the same launch keeps.  The step's reward is the simulator row's ``reward``
field, which ``env_pre_step`` / ``rollout_pre`` consume as before.
"""
from __future__ import annotations

import torch

from cat_envs.shim import ManagerBase, RewardTermCfg

from . import rewards as R


class RewardManager(ManagerBase):
    def __init__(self, cfg: object, env):
        self._names: list[str] = []              # every configured term, cfg order
        self._cfgs: dict[str, RewardTermCfg] = {}
        self._active: list[str] = []             # the terms of the table (non-zero weight at construction), table order
        self._rows: dict[str, tuple] = {}        # name -> (kind, joint_mask, param)
        super().__init__(cfg, env)               # -> _prepare_terms()

    # ------------------------------------------------------------------ terms
    def _prepare_terms(self):
        env = self._env
        for name, term in R.cfg_items(self.cfg):
            if not isinstance(term, RewardTermCfg):
                raise TypeError(f"Configuration for term '{name}' is not RewardTermCfg. Received: '{type(term)}'.")
            self._cfgs[name] = term
        joint_names = env.scene["robot"].joint_names
        self._names, table = R.build_table(self.cfg, joint_names, env.sim.D)       # the raw observation's width
        if not table:
            raise ValueError("cfg.rewards has no term of non-zero weight: nothing to evaluate (leave cfg.rewards unset for "
                             "the simulator's built-in reward)")
        self._active = [row[0] for row in table]
        self._rows = {row[0]: (row[1], row[2], row[4]) for row in table}
        self._push()

    def _push(self):
        """the table with the current weights, onto the device: the next launch reads it"""
        self._env.sim.set_reward_table([(*self._rows[n][:2], float(self._cfgs[n].weight), self._rows[n][2])
                                        for n in self._active])

    @property
    def active_terms(self) -> list[str]:
        return self._names

    def __str__(self) -> str:
        msg = f"<RewardManager> contains {len(self._names)} active terms.\n"
        kind_name = {v: k for k, v in R.K.items()}
        rows = []
        for index, name in enumerate(self._names):
            cfg = self._cfgs[name]
            kind, mask, param = self._rows.get(name, (0, 0, 0.0))
            rows.append([index, name, cfg.weight, kind_name.get(kind, "(zero weight: not evaluated)"),
                         f"{mask:#05x}" if mask else "-", param if kind else "-"])
        head = ["Index", "Name", "Weight", "Kernel term", "Joints", "Param"]
        try:
            from prettytable import PrettyTable
            table = PrettyTable()
            table.title = "Active Reward Terms"
            table.field_names = head
            table.align["Name"] = "l"
            table.align["Weight"] = "r"
            for r in rows:
                table.add_row(r)
            body = table.get_string()
        except ImportError:
            body = "Active Reward Terms\n" + "\n".join(" | ".join(str(c) for c in r) for r in [head, *rows])
        return msg + body + "\n"

    def get_term_cfg(self, term_name: str) -> RewardTermCfg:
        if term_name not in self._cfgs:
            raise ValueError(f"Reward term '{term_name}' not found.")
        return self._cfgs[term_name]

    def set_term_cfg(self, term_name: str, cfg: RewardTermCfg):
        """a new weight is on the device before the next launch.  The table's slots are those of construction: a term
        that had weight zero then has no slot and cannot get a weight later; one that has a slot may go to zero"""
        if term_name not in self._cfgs:
            raise ValueError(f"Reward term '{term_name}' not found.")
        if term_name not in self._rows and float(cfg.weight) != 0.0:
            raise ValueError(f"Reward term '{term_name}' had weight 0 when the env was built and is not in the simulator's "
                             f"table; configure it with a non-zero weight to anneal it")
        self._cfgs[term_name] = cfg
        if term_name in self._rows:
            self._push()

    # ------------------------------------------------------------------ step / log
    def compute(self, dt: float | None = None) -> torch.Tensor:
        """the step's reward per env: a view of the simulator row's ``reward`` field.  Launches nothing - the simulator's
        own launch of this step has computed it"""
        return self._env.sim.view("reward")[:, 0]

    @property
    def record(self) -> torch.Tensor:
        return self._env.sim.reward_record

    def pop_log(self):
        """``{"Episode_Reward/<name>": ...}`` over every episode that ended since the last call (episode-weighted:
        sum of the ended episodes' term sums / their count / max_episode_length_s), or None if none ended; then the ended
        sums and the count are zeroed in place.  One device reduction and one copy to the host, folded in fp64"""
        done = self.record[:, 16:32]
        sums = done.sum(0, dtype=torch.float64).cpu().numpy()
        done.zero_()
        return R.fold_log(self._names, self._active, sums, self._env.max_episode_length_s)

    def reset(self, env_ids=None):
        return {}

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """the table without its weights (a curriculum moves them; they are part of the state)"""
        return [[n, int(self._rows[n][0]), int(self._rows[n][1]), float(self._rows[n][2])] for n in self._active]

    def state_dict(self) -> dict:
        return {"record": self.record, "weights": {n: float(self._cfgs[n].weight) for n in self._names}}

    def check_state_dict(self, sd: dict):
        rec = sd["record"]
        if tuple(rec.shape) != tuple(self.record.shape) or rec.dtype != self.record.dtype:
            raise ValueError(f"run state: reward record is {tuple(rec.shape)} {rec.dtype}, this env's is "
                             f"{tuple(self.record.shape)} {self.record.dtype}")
        if sorted(sd["weights"]) != sorted(self._names):
            raise ValueError(f"run state: reward terms {sorted(sd['weights'])}, this env has {sorted(self._names)}")
        for n, w in sd["weights"].items():
            if n not in self._rows and float(w) != 0.0:
                raise ValueError(f"run state: reward term '{n}' has weight {w}, in this env it is not in the table")

    def load_state_dict(self, sd: dict):
        """in place: the descriptor holds the record's address"""
        self.check_state_dict(sd)
        self.record.copy_(sd["record"])
        for n, w in sd["weights"].items():
            self._cfgs[n].weight = float(w)
        self._push()
