"""Observation manager of the servo task ("Observations").

IsaacLab's ``ObservationManager`` calls one torch function per term and step, then adds noise, clips, scales and
concatenates.  This one calls none: it turns the policy group of an ``ObservationsCfg`` into the table the simulator's
kernel evaluates in a post-pass of its own launch (``Solo12ServoSim.set_observation_table``); the policy observation is a
field of the simulator's row, next to the raw one.  ``set_corruption`` rewrites the entries' noise bits on the device, in
stream order: the next launch - a replayed graph's, too - reads them.

History ("History"; PARITY UNPINNED: restated from IsaacLab's published ``ObservationManager`` and
``CircularBuffer``): a term's ``history_length`` H keeps its last H processed frames, oldest first, in a second field of the
row that the same launch shifts and fills; a group's ``history_length`` overrides every term's.  The table then comes with a
map of one word per float of that field (``Solo12ServoSim.set_history_table``).
"""
from __future__ import annotations

import math

import numpy as np

from cat_envs import native
from cat_envs.shim import AdditiveUniformNoiseCfg, ObservationTermCfg

from . import observations as O

MAX_WIDTH = native.SERVO_OBS_MAX_WIDTH
MAX_HISTORY_FLOATS, MAX_DEPTH = native.SERVO_OBS_HISTORY_MAX_FLOATS, native.SERVO_OBS_HISTORY_MAX_DEPTH
NEWEST = native.SERVO_HISTORY_NEWEST
SWITCHES = ("concatenate_terms", "enable_corruption", "history_length", "flatten_history_dim")
BIAS, NOISE, CLIP = native.SERVO_OBS_BIAS, native.SERVO_OBS_NOISE, native.SERVO_OBS_CLIP
ENTRY_FIELDS = ("src", "flags", "bias", "noise_lo", "noise_width", "clip_lo", "clip_hi", "scale")


def _f32(x) -> float:
    return float(np.float32(x))


def _switch(group_cfg, name, default) -> bool:
    return bool(group_cfg.get(name, default) if isinstance(group_cfg, dict) else getattr(group_cfg, name, default))


def group_items(group_cfg):
    """(name, ObsTerm) of a group cfg in definition order; unset terms and the group's own switches are left out (the
    switches are read by ``build_table``, history among them)"""
    items = group_cfg.items() if isinstance(group_cfg, dict) else group_cfg.__dict__.items()
    return [(n, t) for n, t in items if t is not None and n not in SWITCHES]


def _group_value(group_cfg, name, default):
    return group_cfg.get(name, default) if isinstance(group_cfg, dict) else getattr(group_cfg, name, default)


def term_depth(group_cfg, name, term) -> int:
    """the effective depth H = max(history_length, 1) of a term; the group's ``history_length``, when it is not None, overrides
    the term's ``history_length`` and ``flatten_history_dim``.  ``ValueError``s name the term"""
    length, flatten = getattr(term, "history_length", 0), getattr(term, "flatten_history_dim", True)
    group_length = _group_value(group_cfg, "history_length", None)
    if group_length is not None:
        length, flatten = group_length, _group_value(group_cfg, "flatten_history_dim", True)
    if isinstance(length, bool) or not isinstance(length, int):
        raise ValueError(f"observation term '{name}': history_length must be an int, got {length!r}")
    if length < 0:
        raise ValueError(f"observation term '{name}': history_length must be >= 0, got {length}")
    depth = max(length, 1)
    if depth > MAX_DEPTH:
        raise ValueError(f"observation term '{name}': history_length {length} is above the {MAX_DEPTH} frames a term keeps")
    if depth > 1 and not flatten:
        raise ValueError(f"observation term '{name}': flatten_history_dim=False is not supported; the policy observation is "
                         f"one flat field of the simulator's row")
    return depth


def history_map(widths, depths):
    """one word per float of the history field, ``cur | w << 8 | newest << 16``: a term of frame width w and depth H owns
    H * w consecutive floats, oldest frame first; ``cur`` is the float of the current frame a float shows when it is new"""
    words, at = [], 0
    for w, depth in zip(widths, depths):
        for slot in range(depth):
            words += [(at + k) | w << 8 | (NEWEST if slot == depth - 1 else 0) for k in range(w)]
        at += w
    return words


class ObsTable(tuple):
    """what ``build_table`` returns: the pair ``(entries, group_obs_term_dim)`` with the history beside it - ``depths``
    ``{term name: H}``, ``widths`` ``{term name: frame width}`` and ``history`` the map's words (``history_map``)"""

    def __new__(cls, entries, dims, depths, widths):
        self = super().__new__(cls, (entries, dims))
        self.depths, self.widths = dict(depths), dict(widths)
        self.history = history_map(list(widths.values()), list(depths.values()))
        return self

    @property
    def history_floats(self) -> int:
        return len(self.history)

    @property
    def has_history(self) -> bool:
        return any(h > 1 for h in self.depths.values())


def build_table(group_cfg, joint_names, default_joint_pos=None, action_terms=None):
    """(entries, group_obs_term_dim) from an observation group cfg and the robot's joint names; pure, needs no device.
    ``entries``: one ``(src, flags, bias, noise_lo, noise_width, clip_lo, clip_hi, scale)`` per float of the current frame
    of the policy observation, terms concatenated in cfg order, every float already rounded to fp32; the noise bit is set for every term
    that has a noise cfg (the corruption switch masks it later).  ``group_obs_term_dim``: ``{term name: (H * width,)}`` in the
    same order, H the term's depth (``term_depth``); the returned pair is an ``ObsTable`` that also carries the depths and the
    history map.  ``ValueError``s name the term.  ``action_terms`` (envs with ``cfg.actions``): ``{term: (first column, end)}``
    of the action block - a ``last_action`` term then has the block's width, or with ``action_name`` that term's columns."""
    import types
    if default_joint_pos is None:
        from cat_envs.tasks.utils.cat.cat_env import DEFAULT_JOINT_POS as default_joint_pos
    if not _switch(group_cfg, "concatenate_terms", True):
        raise ValueError("observation group: concatenate_terms=False is not supported; the policy observation is one "
                         "concatenated field of the simulator's row")
    env = types.SimpleNamespace(scene={"robot": types.SimpleNamespace(joint_names=list(joint_names), body_names=[])},
                                default_joint_pos=[float(v) for v in default_joint_pos], action_terms=action_terms)
    entries, dims, depths, widths, total = [], {}, {}, {}, 0
    for name, term in group_items(group_cfg):
        if not isinstance(term, ObservationTermCfg):
            raise TypeError(f"Configuration for observation term '{name}' is not ObservationTermCfg. Received: '{type(term)}'.")
        describe = getattr(term.func, "describe", None)
        if describe is None:
            raise ValueError(f"observation term '{name}': {getattr(term.func, '__name__', term.func)!r} has no describe(); "
                             f"the servo task evaluates observations inside the simulator launch and runs no Python "
                             f"observation function")
        try:
            pairs = list(describe(env, **(term.params or {})))
        except KeyError as e:
            raise ValueError(f"observation term '{name}': {e.args[0]}") from e
        width = len(pairs)
        depth = term_depth(group_cfg, name, term)
        scale = term.scale
        if scale is None:
            scales = [1.0] * width
        elif isinstance(scale, (int, float)):
            scales = [float(scale)] * width
        else:
            scales = [float(s) for s in scale]
            if len(scales) != width:
                raise ValueError(f"observation term '{name}': scale has {len(scales)} elements, the term has {width}")
        if not all(math.isfinite(s) for s in scales):
            raise ValueError(f"observation term '{name}': scale must be finite, got {scale!r}")
        flags, noise_lo, noise_width, clip_lo, clip_hi = 0, 0.0, 0.0, 0.0, 0.0
        noise = term.noise
        if noise is not None:
            additive = isinstance(noise, AdditiveUniformNoiseCfg) and getattr(noise, "operation", "add") == "add"
            if not additive or not all(isinstance(v, (int, float)) for v in (noise.n_min, noise.n_max)):
                raise ValueError(f"observation term '{name}': only additive uniform noise with scalar bounds "
                                 f"(AdditiveUniformNoiseCfg) is evaluated in the simulator launch, got {noise!r}")
            if float(noise.n_max) < float(noise.n_min):
                raise ValueError(f"observation term '{name}': noise n_max {noise.n_max} < n_min {noise.n_min}")
            flags |= NOISE
            noise_lo, noise_width = _f32(noise.n_min), _f32(float(noise.n_max) - float(noise.n_min))
        if term.clip is not None:
            lo, hi = (float(v) for v in term.clip)
            if lo > hi:
                raise ValueError(f"observation term '{name}': clip lo {lo} > hi {hi}")
            flags |= CLIP
            clip_lo, clip_hi = _f32(lo), _f32(hi)
        for (src, bias), s in zip(pairs, scales):
            if not 0 <= int(src) < O.RAW_WIDTH:
                raise ValueError(f"observation term '{name}': source index {src} outside the raw {O.RAW_WIDTH}-float observation")
            entries.append((int(src), flags | (BIAS if bias is not None else 0), _f32(0.0 if bias is None else bias),
                            noise_lo, noise_width, clip_lo, clip_hi, _f32(s)))
        dims[name], depths[name], widths[name] = (depth * width,), depth, width
        total += depth * width
        if len(entries) > MAX_WIDTH:
            raise ValueError(f"observation term '{name}': the policy observation reaches {len(entries)} floats, the simulator "
                             f"evaluates at most {MAX_WIDTH}")
        if total > MAX_HISTORY_FLOATS:
            raise ValueError(f"observation term '{name}': with its history the policy observation reaches {total} floats, the "
                             f"simulator's row keeps at most {MAX_HISTORY_FLOATS}")
    if not entries:
        raise ValueError("the observation group has no term: nothing to evaluate (leave cfg.observations unset for the "
                         "simulator's raw observation)")
    return ObsTable(entries, dims, depths, widths)


def policy_group(observations_cfg):
    """the policy group of an ``ObservationsCfg``; any other configured group is out of scope and refused"""
    items = observations_cfg.items() if isinstance(observations_cfg, dict) else observations_cfg.__dict__.items()
    groups = {n: g for n, g in items if g is not None}
    other = [n for n in groups if n != "policy"]
    if "policy" not in groups or other:
        raise ValueError(f"cfg.observations must configure exactly the group 'policy' (got {sorted(groups)}): there is one "
                         f"policy observation per row and no separate critic group")
    return groups["policy"]


def with_corruption(entries, on: bool):
    """the entries as the device reads them: the noise bit survives only while corruption is on"""
    return list(entries) if on else [(e[0], e[1] & ~NOISE, *e[2:]) for e in entries]


def observation_spec(dims, entries, joint_names, depths=None):
    """the input contract of a deployed policy: per term its slice of the policy observation, raw sources (named), bias,
    scale, clip and noise range; JSON-serialisable.  ``depths`` ``{term: H}``: a term's slice then holds its last H processed
    frames, oldest first (``frame_slice``: the term's floats within one frame)"""
    depths = {n: 1 for n in dims} if depths is None else depths
    raw = (["base_ang_vel_" + a for a in "xyz"] + ["projected_gravity_" + a for a in "xyz"]
           + ["command_" + a for a in ("vx", "vy", "wz")] + ["joint_pos_rel:" + j for j in joint_names]
           + ["joint_vel:" + j for j in joint_names] + ["last_action:" + j for j in joint_names])
    terms, at, col = [], 0, 0
    for name, (hw,) in dims.items():
        w = hw // depths[name]
        rows = entries[at:at + w]
        e0 = rows[0]
        terms.append({"name": name, "slice": [col, col + hw], "history_length": depths[name], "frame_slice": [at, at + w],
                      "src": [r[0] for r in rows], "src_names": [raw[r[0]] for r in rows],
                      "bias": [r[2] if r[1] & BIAS else 0.0 for r in rows], "scale": [r[7] for r in rows],
                      "clip": [e0[5], e0[6]] if e0[1] & CLIP else None,
                      "noise": [e0[3], _f32(np.float32(e0[3]) + np.float32(e0[4]))] if e0[1] & NOISE else None})
        at, col = at + w, col + hw
    return {"obs_dim": col, "frame_dim": at, "frame_order": "oldest first",
            "history": "a term's slice holds its last history_length processed frames (each with the noise it was drawn "
                       "with), oldest first; the first frame of an episode fills every slot.  The deployer owns this ring: "
                       "the exported model takes the obs_dim floats as they are",
            "order": "noise, clip, scale (IsaacLab ObservationManager)", "joint_order": list(joint_names),
            "raw_observation": raw, "terms": terms}


class ObservationManager:
    def __init__(self, cfg: object, env, entries=None, dims=None, depths=None):
        """``entries``, ``dims``, ``depths``: what ``build_table`` has returned for the policy group (``dims`` per term
        ``(H * width,)``; ``depths`` None: every term at depth 1); without them the table is built here"""
        self.cfg, self._env = cfg, env
        group = policy_group(cfg)
        if entries is None:
            table = build_table(group, env.scene["robot"].joint_names)
            (entries, dims), depths = table, table.depths
        self._entries, self._dims = list(entries), dict(dims)
        self._depths = {n: 1 for n in self._dims} if depths is None else dict(depths)
        self._widths = {n: hw // self._depths[n] for n, (hw,) in self._dims.items()}
        self._corruption = _switch(group, "enable_corruption", False)
        self._push()
        # with every depth 1 no history descriptor is attached: the policy reads the current frame, as it always has
        if self.has_history:
            self._env.sim.set_history_table(history_map(list(self._widths.values()), list(self._depths.values())))

    def _push(self):
        self._env.sim.set_observation_table(with_corruption(self._entries, self._corruption))

    @property
    def has_history(self) -> bool:
        return any(h > 1 for h in self._depths.values())

    @property
    def history_lengths(self) -> dict:
        """``{term name: H}``, the effective depth of every term"""
        return dict(self._depths)

    # ------------------------------------------------------------------ IsaacLab's names
    @property
    def active_terms(self) -> dict:
        return {"policy": list(self._dims)}

    @property
    def group_obs_dim(self) -> dict:
        return {"policy": (sum(hw for hw, in self._dims.values()),)}

    @property
    def group_obs_term_dim(self) -> dict:
        return {"policy": list(self._dims.values())}

    @property
    def entries(self) -> list:
        """the table as built (noise bits as configured, whatever the switch says)"""
        return list(self._entries)

    @property
    def corruption(self) -> bool:
        return self._corruption

    def set_corruption(self, on: bool):
        """noise on or off from the next launch on: one stream-ordered copy of the table; nothing already computed moves -
        the frames a history holds keep the noise they were drawn with"""
        on = bool(on)
        if on != self._corruption:
            self._corruption = on
            self._push()

    def compute(self) -> dict:
        """launches nothing: the simulator's launch of this step has filled the field"""
        return {"policy": self._env.sim.view("policy_obs_hist" if self.has_history else "policy_obs")}

    def reset(self, env_ids=None):
        return {}

    def spec(self) -> dict:
        return observation_spec(self._dims, self._entries, self._env.scene["robot"].joint_names, self._depths)

    def __str__(self) -> str:
        msg = f"<ObservationManager> contains 1 group, {len(self._dims)} terms, {self.group_obs_dim['policy'][0]} floats " \
              f"({len(self._entries)} per frame; corruption {'on' if self._corruption else 'off'}).\n"
        at = 0
        for name, w in self._widths.items():
            e = self._entries[at]
            noise = f"U({e[3]:g}, {e[3] + e[4]:g})" if e[1] & NOISE else "-"
            clip = f"[{e[5]:g}, {e[6]:g}]" if e[1] & CLIP else "-"
            msg += f"  {at:2d}:{at + w:2d}  {name:<20s} history {self._depths[name]:<2d} noise {noise:<18s} clip {clip:<12s} scale {[x[7] for x in self._entries[at:at + w]]}\n"
            at += w
        return msg

    # ------------------------------------------------------------------ run state
    def fingerprint(self) -> list:
        """names, the whole table (noise bits as configured) and every depth above 1: what a loaded state's policy
        observation was made with (a term at depth 1 keeps the entry it had before there was a history)"""
        out, at = [], 0
        for name, w in self._widths.items():
            out.append([name, [[int(e[0]), int(e[1]), *(float(v) for v in e[2:])] for e in self._entries[at:at + w]]])
            if self._depths[name] > 1:
                out[-1].append(int(self._depths[name]))
            at += w
        return out

    def state_dict(self) -> dict:
        return {"corruption": bool(self._corruption)}

    def check_state_dict(self, sd: dict):
        if "corruption" not in sd:
            raise ValueError("run state: the observations' part lacks 'corruption'")

    def load_state_dict(self, sd: dict):
        self.check_state_dict(sd)
        self._corruption = bool(sd["corruption"])
        self._push()
