"""Command manager of the servo task ("Commands").

IsaacLab's ``CommandManager`` calls a term's ``compute(dt)`` in Python every step.  This one calls nothing: it turns a
``CommandsCfg`` into the 16-word block the simulator's kernel reads inside its own launch
(``Solo12ServoSim.set_command_block``; include/catppo.h, catppo_servo_commands).  The command and the time left until its
timed resample live in the simulator's row, so they travel with it; what the manager owns is the ranges.  ``set_ranges``
rewrites them on the device, in stream order: the next launch - a replayed graph's, too - draws from them.
"""
from __future__ import annotations

import math

import numpy as np

from cat_envs import native
from cat_envs.tasks.utils.mdp.commands import UniformVelocityCommandCfg, UniformVelocityCommandWithDeadzoneCfg

W = native.SERVO_COMMAND_WORDS
AXES = ("lin_vel_x", "lin_vel_y", "ang_vel_z")
P_STILL = 0.01                                     # the reference's literal


def _f32(x) -> float:
    return float(np.float32(x))


def lo_width(a, b):
    """a uniform sample from (a, b) is ``lo + u * width``: lo = f32(a), width = f32(b - a)"""
    return _f32(a), _f32(float(b) - float(a))


def term_items(cfg):
    items = cfg.items() if isinstance(cfg, dict) else cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None]


def _pair(term, key, value):
    try:
        a, b = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"command term '{term}': '{key}' must be a pair (lo, hi), got {value!r}") from None
    if not (math.isfinite(a) and math.isfinite(b)) or b < a:
        raise ValueError(f"command term '{term}': '{key}' must be finite with lo <= hi, got {value!r}")
    return a, b


def _probability(term, key, p):
    p = float(p)
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError(f"command term '{term}': {key} must be in [0, 1], got {p}")
    return p


def command_term(cfg):
    """(name, term) of the one command term of a ``CommandsCfg``; errors name the offending term"""
    terms = term_items(cfg)
    if not terms:
        raise ValueError("the command cfg has no term: nothing to evaluate (leave cfg.commands unset)")
    for name, term in terms:
        if not isinstance(term, UniformVelocityCommandCfg):
            raise TypeError(f"command term '{name}': the simulator evaluates UniformVelocityCommandCfg and "
                            f"UniformVelocityCommandWithDeadzoneCfg, not {type(term).__name__}")
    if len(terms) > 1:
        raise ValueError(f"command term '{terms[1][0]}': a second command term (the first is '{terms[0][0]}'); the simulator's "
                         f"row has one command")
    return terms[0]


def build_block(cfg, sim_dt, episode_length_s):
    """a ``CommandsCfg`` -> ``{"name", "class", "flags", "dz", "p_still", "p_move", "bounds": [(a, b)] * 3, "rel_standing",
    "time": (a, b), "inert": [...]}``; pure, needs no device.  ``pack`` rounds to fp32."""
    name, term = command_term(cfg)
    if term.heading_command:
        raise ValueError(f"command term '{name}': heading_command = True, and the servo surrogate has no heading")
    ta, tb = _pair(name, "resampling_time_range", term.resampling_time_range)
    if not ta > 0.0:
        raise ValueError(f"command term '{name}': resampling_time_range must be > 0, got {term.resampling_time_range!r}")
    bounds = [_pair(name, "ranges." + k, getattr(term.ranges, k)) for k in AXES]
    rel = _probability(name, "rel_standing_envs", term.rel_standing_envs)
    inert = [f"{name}.rel_heading_envs"]
    if term.debug_vis:
        inert.append(f"{name}.debug_vis")
    if getattr(term.ranges, "heading", None) is not None:
        inert.append(f"{name}.ranges.heading")
    block = {"name": name, "class": type(term).__name__, "bounds": bounds, "time": (ta, tb), "rel_standing": rel,
             "dz": 0.0, "p_still": 0.0, "p_move": 0.0}
    if isinstance(term, UniformVelocityCommandWithDeadzoneCfg):
        block["flags"] = (native.SERVO_COMMAND_DEADZONE | native.SERVO_COMMAND_RANDOM_RESAMPLE | native.SERVO_COMMAND_YAW_FLIP)
        dz = float(term.velocity_deadzone)
        if not (math.isfinite(dz) and dz >= 0.0):
            raise ValueError(f"command term '{name}': velocity_deadzone must be >= 0, got {dz}")
        block["dz"] = dz
        block["p_still"] = _probability(name, "p_still", P_STILL if term.p_still is None else term.p_still)
        block["p_move"] = _probability(name, "p_move", float(sim_dt) / float(episode_length_s) if term.p_move is None
                                       else term.p_move)
        if rel != 0.0:                             # the reference's _update_command never applies it
            inert.insert(0, f"{name}.rel_standing_envs")
    else:
        block["flags"] = native.SERVO_COMMAND_STANDING
    block["inert"] = inert
    return block


def pack(block) -> np.ndarray:
    """the block's ``native.SERVO_COMMAND_FLOATS`` words as the device reads them (fp32 array; word 0 holds an integer)"""
    words = np.zeros(native.SERVO_COMMAND_FLOATS, np.float32)
    words.view(np.int32)[W["flags"]] = int(block["flags"])
    for k in ("dz", "p_still", "p_move", "rel_standing"):
        words[W[k]] = block[k]
    for i, (a, b) in enumerate(block["bounds"]):
        words[W["ranges"] + 2 * i], words[W["ranges"] + 2 * i + 1] = lo_width(a, b)
    words[W["T_lo"]], words[W["T_width"]] = lo_width(*block["time"])
    return words


class CommandManager:
    def __init__(self, cfg: object, env, block=None):
        self.cfg, self._env = cfg, env
        self._block = block if block is not None else build_block(cfg, env.cfg.sim.dt, env.max_episode_length_s)
        self._configured = pack(self._block)
        self._command = env.sim.view("command")
        self._push()

    def _push(self):
        self._env.sim.set_command_block(pack(self._block))

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def active_terms(self) -> list:
        return [self._block["name"]]

    @property
    def inert(self) -> list:
        """fields that are accepted and have no effect on the surrogate (``term.field``)"""
        return list(self._block["inert"])

    @property
    def block(self) -> dict:
        return self._block

    @property
    def ranges(self) -> dict:
        return {k: tuple(self._block["bounds"][i]) for i, k in enumerate(AXES)}

    def _check_name(self, name):
        if name != self._block["name"]:
            raise ValueError(f"command term '{name}' not found (the command term is '{self._block['name']}')")

    def get_command(self, name: str):
        """[N, 3] view of the row's command field; launches nothing"""
        self._check_name(name)
        return self._command

    def get_term_cfg(self, name: str):
        self._check_name(name)
        return getattr(self.cfg, name) if not isinstance(self.cfg, dict) else self.cfg[name]

    def set_ranges(self, lin_vel_x=None, lin_vel_y=None, ang_vel_z=None):
        """new (lo, hi) of the named commands from the next launch on: one stream-ordered copy of the six range words.  A
        command in flight stays what it is until its next resample."""
        name, bounds = self._block["name"], list(self._block["bounds"])
        for i, (k, v) in enumerate(zip(AXES, (lin_vel_x, lin_vel_y, ang_vel_z))):
            if v is not None:
                bounds[i] = _pair(name, "ranges." + k, v)
        if bounds != self._block["bounds"]:
            self._block["bounds"] = bounds
            self._push()

    def compute(self, dt=None):
        """launches nothing: the simulator's own launch updates the command"""

    def reset(self, env_ids=None):
        return {}

    def __str__(self) -> str:
        b = self._block
        msg = f"<CommandManager> contains 1 term.\n  {b['name']:<18s} {b['class']}  flags {b['flags']:#x}"
        msg += "".join(f"  {k} {a:g}..{c:g}" for k, (a, c) in zip(AXES, b["bounds"]))
        msg += f"  resampling {b['time'][0]:g}..{b['time'][1]:g} s  p_still {b['p_still']:g}  p_move {b['p_move']:g}\n"
        if b["inert"]:
            msg += f"  without effect on the surrogate: {', '.join(b['inert'])}\n"
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """name, class and every word of the block as configured: what a loaded state was made with (ranges that
        ``set_ranges`` has moved since are state, not fingerprint)"""
        b = self._block
        return [[b["name"], b["class"]], [int(w) for w in self._configured.view(np.int32)]]

    def state_dict(self) -> dict:
        return {"ranges": [[float(a), float(b)] for a, b in self._block["bounds"]]}

    def check_state_dict(self, sd: dict):
        r = sd.get("ranges") if isinstance(sd, dict) else None
        if r is None or len(r) != 3:
            raise ValueError("run state: the commands' part lacks 'ranges' (three (lo, hi) pairs)")
        for k, v in zip(AXES, r):
            _pair(self._block["name"], "ranges." + k, v)

    def load_state_dict(self, sd: dict):
        self.check_state_dict(sd)
        self.set_ranges(*[tuple(v) for v in sd["ranges"]])
