"""Event manager of the servo task ("Events").

IsaacLab's ``EventManager`` calls torch functions at start-up, at every reset and on interval timers.  This one calls
none: it turns an ``EventCfg`` into the 32-word block the simulator's kernel reads inside its own launch
(``Solo12ServoSim.set_event_block``; include/catppo.h, catppo_servo_events).  Every draw is stateless (Philox keyed on
seed, global env id, episode and step), so there is nothing to reset and nothing to save but the interval switch.
``set_interval_enabled`` rewrites the flag word on the device, in stream order: the next launch - a replayed graph's,
too - reads it.  Reset and startup terms stay on: they define the task.

A cfg with a timed push (``push_by_setting_velocity``) or an external wrench (``apply_external_force_torque``) packs the
extended block of 64 words ("Disturbances"); the timed push's timer lives in the simulator's row, so the
only new state here is the wrench's switch (``set_wrench_enabled``).  Any other cfg builds and packs what it did.
"""
from __future__ import annotations

import math

import numpy as np

from cat_envs import native
from cat_envs.shim import EventTermCfg

W = native.SERVO_EVENT_WORDS
WX = native.SERVO_EVENT_WORDS_EXT
FLAG = {"push": native.SERVO_EVENT_PUSH, "joint_scale": native.SERVO_EVENT_JOINT_SCALE,
        "joint_offset": native.SERVO_EVENT_JOINT_OFFSET, "root": native.SERVO_EVENT_ROOT,
        "friction": native.SERVO_EVENT_FRICTION}
MODES = ("startup", "reset", "interval")
#: kinds the randomisation block evaluates, not the event block (mdp/randomization.py; DESIGN section 9, "Randomisation")
RANDOMIZE_KINDS = ("actuator_gains", "joint_parameters", "rigid_body_mass")
#: kind -> what a second term collides with: at most one term per slot
_SLOT = {"push": "push", "joint_scale": "joint reset", "joint_offset": "joint reset", "root": "root reset", "friction": "material",
         "push_timed": "push", "wrench": "wrench"}
#: kinds of the extended block ("Disturbances"): a cfg with one of them packs 64 words, any other 32
DISTURBANCE_KINDS = ("push_timed", "wrench")


def _f32(x) -> float:
    return float(np.float32(x))


def lo_width(a, b):
    """a uniform sample from (a, b) is ``lo + u * width``: lo = f32(a), width = f32(b - a)"""
    return _f32(a), _f32(float(b) - float(a))


def term_items(cfg):
    items = cfg.items() if isinstance(cfg, dict) else cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None]


def build_block(cfg, sim_dt, max_episode_length_s):
    """an ``EventCfg`` -> ``{"flags", "p", "num_buckets", "ranges": {group: [(lo, width), ...]}, "terms": {mode: [names]},
    "kinds": {name: kind}, "inert": [...]}``; pure, needs no device, every float already rounded to fp32.  Errors name
    the term: a func without ``describe`` or an unknown mode, an interval term other than the push, a term configured with
    another mode than its own, a second term of a kind.  The three randomisation terms (``RANDOMIZE_KINDS``) are listed under
    their mode, in ``kinds`` and in ``inert`` and fill no word of this block: ``mdp.randomization.build_randomization`` reads
    them."""
    block = {"flags": 0, "p": 0.0, "num_buckets": 1,
             "ranges": {"push": [(0.0, 0.0)] * 5, "joint_pos": [(0.0, 0.0)], "joint_vel": [(0.0, 0.0)],
                        "root_pos": [(0.0, 0.0)] * 2, "root_vel": [(0.0, 0.0)] * 3, "friction": [(0.0, 0.0)]},
             "terms": {m: [] for m in MODES}, "kinds": {}, "inert": []}
    taken = {}
    for name, term in term_items(cfg):
        if not isinstance(term, EventTermCfg):
            raise TypeError(f"Configuration for event term '{name}' is not EventTermCfg. Received: '{type(term)}'.")
        describe = getattr(term.func, "describe", None)
        if describe is None:
            raise ValueError(f"event term '{name}': {getattr(term.func, '__name__', term.func)!r} has no describe(); the servo "
                             f"task evaluates events inside the simulator launch and runs no Python event function")
        if term.mode not in MODES:
            raise ValueError(f"event term '{name}': unknown mode {term.mode!r} (known: {list(MODES)})")
        spec = describe(name, sim_dt, max_episode_length_s, **(term.params or {}))
        kind = spec["kind"]
        if kind in RANDOMIZE_KINDS:
            if term.mode not in ("startup", "reset"):
                raise ValueError(f"event term '{name}': {term.func.__name__} is a 'startup' or 'reset' event, configured as "
                                 f"{term.mode!r} (interval-mode randomisation is out of scope)")
            if kind in taken:
                raise ValueError(f"event term '{name}': a second {term.func.__name__} term (the first is '{taken[kind]}'); at "
                                 f"most one is evaluated")
            taken[kind] = name
            block["terms"][term.mode].append(name)
            block["kinds"][name] = kind
            block["inert"] += [f"{name}.{k}" for k in spec["inert"]]
            continue
        if term.mode == "interval" and kind not in ("push", "push_timed"):
            raise ValueError(f"event term '{name}': the only interval event the simulator evaluates is "
                             f"push_by_setting_velocity_with_random_envs (interval events with per-env timers are out of scope)")
        if kind != "wrench" and term.mode != spec["mode"]:         # the wrench takes either of "startup" and "reset"
            raise ValueError(f"event term '{name}': {term.func.__name__} is a {spec['mode']!r} event, configured as {term.mode!r}")
        slot = _SLOT[kind]
        if slot in taken:
            raise ValueError(f"event term '{name}': a second {slot} term (the first is '{taken[slot]}'); at most one is evaluated")
        pairs = [lo_width(a, b) for a, b in spec["ranges"]]
        r = block["ranges"]
        if kind == "push_timed":
            # IsaacLab's interval rule on a per-env timer; the global timer is out of scope
            if getattr(term, "is_global_time", False):
                raise ValueError(f"event term '{name}': is_global_time=True is not supported, the timed push runs on the env's "
                                 f"own timer (DESIGN section 9, \"Disturbances\")")
            try:
                a, b = (float(v) for v in term.interval_range_s)
            except (TypeError, ValueError):
                raise ValueError(f"event term '{name}': an interval event needs interval_range_s = (a, b), got "
                                 f"{getattr(term, 'interval_range_s', None)!r}") from None
            if not (math.isfinite(a) and math.isfinite(b) and 0.0 < a <= b):
                raise ValueError(f"event term '{name}': interval_range_s must be finite with 0 < a <= b, got {(a, b)}")
            taken[slot] = name
            block["flags_ext"] = block.get("flags_ext", 0) | native.SERVO_EVENT_PUSH_TIMED
            block["interval_range"], r["push"] = lo_width(a, b), pairs
        elif kind == "wrench":
            taken[slot] = name
            block["flags_ext"] = block.get("flags_ext", 0) | native.SERVO_EVENT_WRENCH | (
                native.SERVO_EVENT_WRENCH_RESET if term.mode == "reset" else 0)
            block["wrench"] = {"force": pairs[0], "torque": pairs[1], "mode": term.mode}
        else:
            taken[slot] = name
            block["flags"] |= FLAG[kind]
        if kind == "push":
            block["p"], r["push"] = _f32(spec["p"]), pairs
        elif kind in ("joint_scale", "joint_offset"):
            r["joint_pos"], r["joint_vel"] = [pairs[0]], [pairs[1]]
        elif kind == "root":
            r["root_pos"], r["root_vel"] = pairs[:2], pairs[2:]
        elif kind == "friction":
            r["friction"], block["num_buckets"] = pairs, int(spec["num_buckets"])
        block["terms"][term.mode].append(name)
        block["kinds"][name] = kind
        block["inert"] += [f"{name}.{k}" for k in spec["inert"]]
    if not block["kinds"]:
        raise ValueError("the event cfg has no term: nothing to evaluate (leave cfg.events unset)")
    return block


def extended(block) -> bool:
    """the cfg has a timed push or a wrench: its block is the 64-word one"""
    return bool(block.get("flags_ext", 0))


def pack(block, interval_enabled: bool = True, wrench_enabled: bool = True) -> np.ndarray:
    """the block's words as the device reads them (fp32 array; words 0 and 2 hold integers): ``native.SERVO_EVENT_FLOATS`` of
    them, or ``native.SERVO_EVENT_FLOATS_EXT`` for a cfg with a timed push or a wrench"""
    ext = extended(block)
    words = np.zeros(native.SERVO_EVENT_FLOATS_EXT if ext else native.SERVO_EVENT_FLOATS, np.float32)
    ints = words.view(np.int32)
    flags = int(block["flags"]) | int(block.get("flags_ext", 0))
    if not interval_enabled:
        flags &= ~(native.SERVO_EVENT_PUSH | native.SERVO_EVENT_PUSH_TIMED)
    if not wrench_enabled:
        flags &= ~(native.SERVO_EVENT_WRENCH | native.SERVO_EVENT_WRENCH_RESET)
    if "interval_range" in block:
        words[WX["T_lo"]], words[WX["T_width"]] = block["interval_range"]
    if "wrench" in block:
        for k in ("force", "torque"):
            words[WX[k]], words[WX[k] + 1] = block["wrench"][k]
    ints[W["flags"]], ints[W["num_buckets"]] = flags, int(block["num_buckets"])
    words[W["p"]] = block["p"]
    for group, pairs in block["ranges"].items():
        for i, (lo, width) in enumerate(pairs):
            words[W[group] + 2 * i], words[W[group] + 2 * i + 1] = lo, width
    return words


class EventManager:
    def __init__(self, cfg: object, env, block=None, interval_enabled: bool = True, randomization=None):
        """``randomization``: the block of ``mdp.randomization.build_randomization`` when the cfg carries such terms"""
        self.cfg, self._env = cfg, env
        self._block = block if block is not None else build_block(cfg, env.cfg.sim.dt, env.max_episode_length_s)
        self._interval = bool(interval_enabled)
        self._has_wrench, self._wrench = "wrench" in self._block, True
        self._rnd, self._rnd_enabled = randomization, True
        # an EventCfg of randomisation terms alone launches no event pack
        self._has_events = any(k not in RANDOMIZE_KINDS for k in self._block["kinds"].values())
        self._push()
        self._push_randomization()

    def _push(self):
        if self._has_events:
            self._env.sim.set_event_block(pack(self._block, self._interval, self._wrench))

    def _push_randomization(self):
        if self._rnd is not None:
            from . import randomization as RZ
            self._env.sim.set_randomize_block(RZ.pack(self._rnd, self._rnd_enabled))

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def active_terms(self) -> dict:
        return {m: list(v) for m, v in self._block["terms"].items() if v}

    @property
    def available_modes(self) -> list:
        return [m for m, v in self._block["terms"].items() if v]

    @property
    def inert(self) -> list:
        """params that are accepted and have no effect on the surrogate (``term.param``)"""
        return list(self._block["inert"])

    @property
    def block(self) -> dict:
        return self._block

    @property
    def interval_enabled(self) -> bool:
        return self._interval

    def set_interval_enabled(self, on: bool):
        """pushes on or off from the next launch on: one stream-ordered copy of the flag word; reset and startup terms stay"""
        on = bool(on)
        if on != self._interval:
            self._interval = on
            self._push()                       # only word 0 differs: the simulator copies that word alone

    @property
    def wrench_enabled(self) -> bool:
        return self._has_wrench and self._wrench

    def set_wrench_enabled(self, on: bool):
        """the external wrench on or off from the next launch on: one stream-ordered copy of the flag word, in the next launch
        also under graph replay"""
        if not self._has_wrench:
            raise TypeError("the wrench needs an EventCfg with apply_external_force_torque")
        on = bool(on)
        if on != self._wrench:
            self._wrench = on
            self._push()                       # only word 0 differs: the simulator copies that word alone

    @property
    def randomization(self):
        """the spec of the randomisation terms (kind, mode, operation, ranges and joints per term), or None"""
        return None if self._rnd is None else self._rnd["spec"]

    @property
    def randomization_enabled(self) -> bool:
        return self._rnd is not None and self._rnd_enabled

    def set_randomization_enabled(self, on: bool):
        """the randomised robot on or off (off: the nominal robot) from the next launch on: one stream-ordered copy of the
        flag word, in the next launch also under graph replay"""
        if self._rnd is None:
            raise TypeError("randomization needs an EventCfg with randomize_actuator_gains, randomize_joint_parameters or "
                            "randomize_rigid_body_mass")
        on = bool(on)
        if on != self._rnd_enabled:
            self._rnd_enabled = on
            self._push_randomization()         # only word 0 differs: the simulator copies that word alone

    def apply(self, mode: str, env_ids=None, dt=None, global_env_step_count=None):
        """launches nothing: the simulator's own launch evaluates every mode"""
        if mode not in MODES:
            raise ValueError(f"unknown event mode {mode!r}")

    def reset(self, env_ids=None):
        return {}

    def __str__(self) -> str:
        b = self._block
        msg = f"<EventManager> contains {len(b['kinds'])} terms (pushes {'on' if self._interval else 'off'}).\n"
        for mode, names in b["terms"].items():
            for n in names:
                extra = f" p = {b['p']:g}" if b["kinds"][n] == "push" else ""
                if b["kinds"][n] == "push_timed":
                    lo, width = b["interval_range"]
                    extra = f" every {lo:g} .. {lo + width:g} s per env"
                if b["kinds"][n] == "wrench":
                    extra = f" ({'on' if self._wrench else 'off'})"
                msg += f"  {mode:<9s} {n:<22s} {b['kinds'][n]}{extra}\n"
        for n, t in (self._rnd["spec"]["terms"] if self._rnd is not None else {}).items():
            ranges = ", ".join(f"{q} {tuple(r)}" for q, r in t["ranges"].items() if r is not None)
            msg += f"  randomisation ({'on' if self._rnd_enabled else 'off'}) {n}: {t['operation']} {ranges}, {len(t['joints'])} joints / bodies\n"
        if b["inert"]:
            msg += f"  without effect on the surrogate: {', '.join(b['inert'])}\n"
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """names, kinds and every word of the block (pushes as configured): what a loaded state was made with"""
        b = self._block
        words = pack(b, True, True)                # 32 words, or 64 only with a timed push or a wrench
        fp = [[n, b["kinds"][n]] for n in b["kinds"]] + [[int(w) for w in words.view(np.int32)]]
        if self._rnd is not None:                  # only then: older run states keep their fingerprint
            from . import randomization as RZ
            fp.append([int(w) for w in RZ.pack(self._rnd, True).view(np.int32)])
        return fp

    def state_dict(self) -> dict:
        sd = {"interval": bool(self._interval)}
        if self._has_wrench:                       # only then: older run states load unchanged
            sd["wrench"] = bool(self._wrench)
        if self._rnd is not None:
            sd["randomization"] = bool(self._rnd_enabled)
        return sd

    def check_state_dict(self, sd: dict):
        if "interval" not in sd:
            raise ValueError("run state: the events' part lacks 'interval'")
        if self._has_wrench and "wrench" not in sd:
            raise ValueError("run state: the events' part lacks 'wrench'")
        if self._rnd is not None and "randomization" not in sd:
            raise ValueError("run state: the events' part lacks 'randomization'")

    def load_state_dict(self, sd: dict):
        self.check_state_dict(sd)
        self._interval = bool(sd["interval"])
        if self._has_wrench:
            self._wrench = bool(sd["wrench"])
        self._push()
        if self._rnd is not None:
            self._rnd_enabled = bool(sd["randomization"])
            self._push_randomization()
