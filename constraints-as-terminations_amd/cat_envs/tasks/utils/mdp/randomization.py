"""Randomisation of the robot in the servo task ("Randomisation").

IsaacLab's ``randomize_actuator_gains``, ``randomize_joint_parameters`` and ``randomize_rigid_body_mass`` write per-env
tensors at start-up or at every reset.  Here nothing is written and nothing is stored: ``build_randomization`` turns the three
event terms of an ``EventCfg`` into the 32-word block the simulator's kernel reads inside its own launch
(``Solo12ServoSim.set_randomize_block``; include/catppo.h, catppo_servo_randomize), and every lane re-derives its env's gains,
joint friction, armature and base mass in every step from stateless Philox draws keyed on the env and - in reset mode - the
episode.  PARITY UNPINNED: friction is a Coulomb torque, not PhysX's coefficient; the mass acts on the foot load and the
base's velocity lag only; at most one term of each of the three kinds.
"""
from __future__ import annotations

import math
import re

import numpy as np

from cat_envs import native
from cat_envs.shim import EventTermCfg

from .event_manager import RANDOMIZE_KINDS as KINDS
from .event_manager import lo_width, term_items

MODES = ("startup", "reset")
QUANTITIES = ("stiffness", "damping", "friction", "armature", "mass")
GRAVITY = 9.81
_RESET_FLAG = {"actuator_gains": "gains_reset", "joint_parameters": "joint_reset", "rigid_body_mass": "mass_reset"}
_OP_SHIFT = {"actuator_gains": 0, "joint_parameters": 8, "rigid_body_mass": 16}


def _f32(x) -> float:
    return float(np.float32(x))


def is_randomization_term(term) -> bool:
    """does the event term's func describe itself as one of the three randomisation kinds?"""
    describe = getattr(getattr(term, "func", None), "describe", None)
    return describe is not None and getattr(term.func, "__name__", "") in (
        "randomize_actuator_gains", "randomize_joint_parameters", "randomize_rigid_body_mass")


def split_events(events_cfg):
    """(names of the terms the event block evaluates, names of the randomisation terms) of an ``EventCfg`` (None: none)"""
    if events_cfg is None:
        return [], []
    items = term_items(events_cfg)
    rnd = [n for n, t in items if is_randomization_term(t)]
    return [n for n, _ in items if n not in rnd], rnd


def _corners(op, x, lo, width):
    """the two ends of op(x, s) for s in [lo, lo + width], each one rounded fp32 operation like the kernel's"""
    F = np.float32
    out = []
    for s in (F(lo), F(F(lo) + F(width))):
        out.append(float(F(x) * s if op == "scale" else F(x) + s if op == "add" else s))
    return min(out), max(out)


def check_corners(block, actuator_entries, sim_dt):
    """the worst corner of the configured ranges, per joint: ``ValueError`` naming the term unless kp', kd', fr, armature'
    are >= 0, m' > 0, and the semi-implicit step stays stable, 2 a + b < 4 with a = kd' dt / I' and b = kp' dt^2 / I' at the
    largest kp', the largest kd' and the smallest I' (the Jury conditions of its characteristic polynomial)"""
    terms = block["spec"]["terms"]
    dt = float(sim_dt)
    si = block["servo_inertia"]
    for j, e in enumerate(actuator_entries):
        kp_hi, kd_hi, i_lo, who = float(e["kp"]), float(e["kd"]), float(e["inertia"]), None
        for name, t in terms.items():
            if t["kind"] == "actuator_gains" and j in t["joint_ids"]:
                for q, key in (("stiffness", "kp"), ("damping", "kd")):
                    if t["ranges"][q] is not None:
                        lo, hi = _corners(t["operation"], e[key], *lo_width(*t["ranges"][q]))
                        if lo < 0.0:
                            raise ValueError(f"event term '{name}': {q} of joint {j} can become {lo:g} < 0 "
                                             f"({t['operation']} {t['ranges'][q]} on {e[key]:g})")
                        kp_hi, kd_hi = (hi, kd_hi) if key == "kp" else (kp_hi, hi)
                        who = who or name
            if t["kind"] == "joint_parameters" and j in t["joint_ids"]:
                if t["ranges"]["friction"] is not None:
                    lo, _ = _corners(t["operation"], 0.0, *lo_width(*t["ranges"]["friction"]))
                    if lo < 0.0:
                        raise ValueError(f"event term '{name}': the friction of joint {j} can become {lo:g} < 0")
                if t["ranges"]["armature"] is not None:
                    lo, _ = _corners(t["operation"], block["armatures"][j], *lo_width(*t["ranges"]["armature"]))
                    if lo < 0.0:
                        raise ValueError(f"event term '{name}': the armature of joint {j} can become {lo:g} < 0")
                    i_lo = float(np.float32(si) + np.float32(lo))
                    who = name
        a, b = kd_hi * dt / i_lo, kp_hi * dt * dt / i_lo
        if who is not None and not 2.0 * a + b < 4.0:
            raise ValueError(f"event term '{who}': joint {j} is unstable at the worst corner of the ranges (stiffness {kp_hi:g}, "
                             f"damping {kd_hi:g}, inertia {i_lo:g}, dt {dt:g}): 2 a + b = {2.0 * a + b:.4g} must stay below 4 "
                             f"(a = kd dt / I, b = kp dt^2 / I)")
    for name, t in terms.items():
        if t["kind"] == "rigid_body_mass":
            lo, _ = _corners(t["operation"], block["m0"], *lo_width(*t["ranges"]["mass"]))
            if not lo > 0.0:
                raise ValueError(f"event term '{name}': the mass can become {lo:g} <= 0 ({t['operation']} {t['ranges']['mass']} "
                                 f"on {block['m0']:g} kg)")


#: a row of the plant table (include/catppo.h, "Pinned plants"): the quantity's pin bit and the word that holds its value
PLANT_BITS = {"kp_scale": 0x1, "kd_scale": 0x2, "friction": 0x4, "armature": 0x8, "mass_scale": 0x10, "lag": 0x20}
PLANT_WORDS = {"kp_scale": 1, "kd_scale": 2, "friction": 3, "armature": 4, "mass_scale": 5, "lag": 6}
PLANT_FLOATS = 8


def check_plant_table(table, decimation, sim_dt, actuator_entries, servo_inertia):
    """every row of a plant table [N, 8] (fp32; words 0 and 6 integers): ``ValueError`` naming the row and the quantity unless
    all values are finite, no unknown bit is set, kp_scale, kd_scale, friction and armature are >= 0, mass_scale > 0, the lag
    lies in 0 .. 3 * decimation, and every joint stays stable at the pinned kp', kd' and inertia' (``check_corners``' condition
    2 a + b < 4 with a = kd' dt / I', b = kp' dt^2 / I'; an unpinned quantity counts with the actuator entry's value).  Pure,
    needs no device.  What a row holds for a quantity whose bit is clear is not read by the launch, but must be finite"""
    t = np.ascontiguousarray(table, np.float32)
    if t.ndim != 2 or t.shape[1] != PLANT_FLOATS:
        raise ValueError(f"the plant table has {PLANT_FLOATS} words per row, got shape {t.shape}")
    ints = t.view(np.int32)
    dt, max_lag = float(sim_dt), min(3 * int(decimation), 255)
    f32 = np.float32
    for i in range(t.shape[0]):
        bits, lag = int(ints[i, 0]), int(ints[i, PLANT_WORDS["lag"]])
        if bits & ~sum(PLANT_BITS.values()):
            raise ValueError(f"plant table row {i}: pin bits {bits:#x} has unknown bits")
        for name in ("kp_scale", "kd_scale", "friction", "armature", "mass_scale"):
            v = float(t[i, PLANT_WORDS[name]])
            if not math.isfinite(v):
                raise ValueError(f"plant table row {i}: {name} must be finite, got {v}")
            if name == "mass_scale":
                if bits & PLANT_BITS[name] and not v > 0.0:
                    raise ValueError(f"plant table row {i}: mass_scale must be > 0, got {v:g}")
            elif bits & PLANT_BITS[name] and v < 0.0:
                raise ValueError(f"plant table row {i}: {name} must be >= 0, got {v:g}")
        if ints[i, 7] != 0:
            raise ValueError(f"plant table row {i}: the spare word 7 must be zero")
        if not 0 <= lag <= max_lag:
            raise ValueError(f"plant table row {i}: lag must be in 0 .. {max_lag} physics steps (three control steps), got {lag}")
        if bits & (PLANT_BITS["kp_scale"] | PLANT_BITS["kd_scale"] | PLANT_BITS["armature"]):
            for j, e in enumerate(actuator_entries):
                kp, kd, inertia = f32(e["kp"]), f32(e["kd"]), f32(e["inertia"])
                if bits & PLANT_BITS["kp_scale"]:
                    kp = kp * t[i, PLANT_WORDS["kp_scale"]]
                if bits & PLANT_BITS["kd_scale"]:
                    kd = kd * t[i, PLANT_WORDS["kd_scale"]]
                if bits & PLANT_BITS["armature"]:
                    inertia = f32(servo_inertia) + t[i, PLANT_WORDS["armature"]]
                a, b = float(kd) * dt / float(inertia), float(kp) * dt * dt / float(inertia)
                if not 2.0 * a + b < 4.0:
                    raise ValueError(f"plant table row {i}: joint {j} is unstable at the pinned plant (stiffness {float(kp):g}, "
                                     f"damping {float(kd):g}, inertia {float(inertia):g}, dt {dt:g}): 2 a + b = {2.0 * a + b:.4g} "
                                     f"must stay below 4 (a = kd dt / I, b = kp dt^2 / I)")


def build_randomization(events_cfg, actuator_entries, joint_names, synthetic_cfg, sim_dt, decimation, armatures=None):
    """(block, spec) of the randomisation terms of an ``EventCfg``, or (None, None) when it has none; pure, needs no device,
    every float already rounded to fp32.  ``actuator_entries``: the twelve entries of ``mdp.actuators.build_table`` (None: the
    simulator's own scalars on every joint); ``armatures``: the twelve nominal armatures (None: zero).  ``block``: flags
    (without the enable bit), operations, masks, (lo, width) pairs, m0, g, servo_inertia, armatures, and ``terms`` / ``kinds`` /
    ``inert`` as the event block has them.  ``spec`` is JSON-serialisable: per term its kind, mode, operation, ranges and joints.
    Errors name the term."""
    joint_names = list(joint_names)
    J = len(joint_names)
    if actuator_entries is None:
        actuator_entries = [dict(kp=_f32(synthetic_cfg.servo_kp), kd=_f32(synthetic_cfg.servo_kd),
                                 inertia=_f32(synthetic_cfg.servo_inertia))] * J
    arm = [0.0] * J if armatures is None else [_f32(a) for a in armatures]
    FL = native.SERVO_RANDOMIZE_FLAGS
    block = {"flags": 0, "ops": 0, "masks": [0, 0, 0], "ranges": {q: (0.0, 0.0) for q in QUANTITIES},
             "m0": _f32(float(synthetic_cfg.servo_weight) / GRAVITY), "g": _f32(GRAVITY),
             "servo_inertia": _f32(synthetic_cfg.servo_inertia), "armatures": arm,
             "terms": {m: [] for m in MODES}, "kinds": {}, "inert": []}
    spec_terms, taken = {}, {}
    for name, term in ([] if events_cfg is None else term_items(events_cfg)):
        if not isinstance(term, EventTermCfg) or not is_randomization_term(term):
            continue
        if term.mode not in MODES:
            raise ValueError(f"event term '{name}': {term.func.__name__} is a 'startup' or 'reset' event, configured as "
                             f"{term.mode!r} (interval-mode randomisation is out of scope)")
        d = term.func.describe(name, sim_dt, None, **(term.params or {}))
        kind = d["kind"]
        if kind in taken:
            raise ValueError(f"event term '{name}': a second {term.func.__name__} term (the first is '{taken[kind]}'); at most "
                             f"one is evaluated")
        taken[kind] = name
        ids = list(range(J))
        if kind != "rigid_body_mass" and d["joint_names"] is not None:
            ids = [j for j, jn in enumerate(joint_names) if any(re.fullmatch(p, jn) for p in d["joint_names"])]
            if not ids:
                raise ValueError(f"event term '{name}': asset_cfg.joint_names {d['joint_names']} match no joint of {joint_names}")
        for q, r in d["quantities"].items():
            if r is not None:
                block["flags"] |= FL[q]
                block["ranges"][q] = lo_width(*r)
        if not any(r is not None for r in d["quantities"].values()):
            raise ValueError(f"event term '{name}': no distribution params are set, the term randomises nothing")
        if term.mode == "reset":
            block["flags"] |= FL[_RESET_FLAG[kind]]
        block["ops"] |= native.SERVO_RANDOMIZE_OPS[d["operation"]] << _OP_SHIFT[kind]
        mask = sum(1 << j for j in ids)
        block["masks"][KINDS.index(kind)] = 1 if kind == "rigid_body_mass" else mask
        block["terms"][term.mode].append(name)
        block["kinds"][name] = kind
        block["inert"] += [f"{name}.{k}" for k in d["inert"]]
        spec_terms[name] = {"kind": kind, "func": term.func.__name__, "mode": term.mode, "operation": d["operation"],
                            "distribution": "uniform",
                            "ranges": {q: None if r is None else [float(r[0]), float(r[1])] for q, r in d["quantities"].items()},
                            "joint_ids": [] if kind == "rigid_body_mass" else ids,
                            "joints": ["base_link"] if kind == "rigid_body_mass" else [joint_names[j] for j in ids]}
    if not spec_terms:
        return None, None
    spec = {"terms": spec_terms, "nominal_mass": block["m0"], "gravity": block["g"], "friction_unit": "N m (Coulomb torque)",
            "inert": list(block["inert"])}
    block["spec"] = spec
    check_corners(block, actuator_entries, sim_dt)
    if not (math.isfinite(block["m0"]) and block["m0"] > 0.0):
        raise ValueError(f"servo_weight must be > 0 for a randomised mass, got {synthetic_cfg.servo_weight}")
    return block, spec


def pack(block, enabled: bool = True) -> np.ndarray:
    """the block's ``native.SERVO_RANDOMIZE_FLOATS`` words as the device reads them (fp32 array; words 0 .. 4 hold integers)"""
    W = native.SERVO_RANDOMIZE_WORDS
    words = np.zeros(native.SERVO_RANDOMIZE_FLOATS, np.float32)
    ints = words.view(np.int32)
    ints[W["flags"]] = int(block["flags"]) | (native.SERVO_RANDOMIZE_FLAGS["enable"] if enabled else 0)
    ints[W["ops"]] = int(block["ops"])
    ints[W["gains_mask"]], ints[W["joint_mask"]], ints[W["body_mask"]] = (int(m) for m in block["masks"])
    for q, (lo, width) in block["ranges"].items():
        words[W[q]], words[W[q] + 1] = lo, width
    words[W["m0"]], words[W["g"]], words[W["servo_inertia"]] = block["m0"], block["g"], block["servo_inertia"]
    words[W["armatures"]:] = block["armatures"]
    return words
