"""Policy evaluation on the closed-loop servo task: fixed commands, a per-env record kept on the device.

``evaluate_policy`` rolls a policy out for ``steps`` control steps with the simulator's evaluation record attached
(``catppo_servo_sim.eval``: twelve fp32 sums per env, updated inside the simulator's own launch) and, optionally, a
per-env table of fixed commands (``catppo_servo_sim.fixed_command``).  Nothing inside the loop synchronises the host; the
tables come back once, at the end, and ``aggregate`` - pure numpy, no device - turns them into metrics in fp64.
DESIGN section 9, "Evaluation".

Robustness ("Robustness"): ``plant`` is a per-env table of pinned plants (``plant_grid``; gains, joint
friction, armature, base mass and actuator lag, ``catppo_servo_plant``) that the simulator's launch puts in the place of the
randomised or nominal robot; ``sweep`` crosses it with a command grid, ``EvalResult.by_plant`` and ``robustness`` - pure
numpy again - say where in the range the policy breaks.

Step responses ("Step responses"): ``commands`` may be a schedule ``[S, N, 3]`` of ``segment_steps``
control steps per segment (``command_sequence``), and ``trace_envs = K`` has the simulator write one row of 72 floats per
step for each of its first K envs (``catppo_servo_sim.trace``, inside the same launch).  ``step_response`` - pure numpy
as well - reads rise time, settling time, overshoot and steady-state error of every command change off the trace.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field

import numpy as np

from cat_envs.native import SERVO_EVAL_FIELDS as FIELDS
from cat_envs.native import SERVO_PLANT_BITS as PLANT_BITS
from cat_envs.native import SERVO_PLANT_FLOATS as PLANT_FLOATS
from cat_envs.native import SERVO_PLANT_WORDS as PLANT_WORDS
from cat_envs.native import SERVO_TRACE_FIELDS as TRACE_FIELDS
from cat_envs.native import SERVO_TRACE_FLOATS as TRACE_FLOATS
from cat_envs.native import SERVO_TRACE_PUSHED as TRACE_PUSHED

#: the ranges the servo simulator draws its commands from (csrc/servo_sim.hip, command_of): vx, vy, wz
COMMAND_RANGES = ((-0.3, 1.0), (-0.7, 0.7), (-0.78, 0.78))
MAX_STEPS = 2 ** 24                     # the record counts in fp32: beyond 2^24 a count stops moving


def command_grid(vx=(-0.3, 1.0, 1), vy=(-0.7, 0.7, 1), wz=(-0.78, 0.78, 1), num_envs: int = 1):
    """``(commands [num_envs, 3] fp32, bin [num_envs] int64)``: the grid of ``n`` evenly spaced values per axis, each axis
    given as ``(lo, hi, n)`` (both ends included; ``n = 1`` is the midpoint), points ordered with vx slowest and wz
    fastest; env ``i`` gets grid point ``i % n_points``.  ``num_envs`` need not be a multiple of the grid."""
    axes = []
    for lo, hi, n in (vx, vy, wz):
        n = int(n)
        if n < 1:
            raise ValueError("a grid axis needs at least one point")
        axes.append(np.array([(lo + hi) / 2.0]) if n == 1 else np.linspace(lo, hi, n))
    pts = np.stack([g.reshape(-1) for g in np.meshgrid(*axes, indexing="ij")], 1).astype(np.float32)
    idx = np.arange(int(num_envs), dtype=np.int64) % len(pts)
    return np.ascontiguousarray(pts[idx]), idx


PLANT_QUANTITIES = tuple(PLANT_BITS)         # kp_scale kd_scale friction armature mass_scale lag, in the order of their words


def pack_plant(named: dict) -> np.ndarray:
    """the ``[P, 8]`` fp32 packing of a named table: ``named[q]`` is ``[P]`` fp64 for every pinned quantity ``q`` (NaN: this row
    leaves ``q`` alone), absent or None for a quantity nobody pins.  Word 0 holds the pin bits and word 6 the lag as integers"""
    cols = {q: np.asarray(v, np.float64).reshape(-1) for q, v in named.items() if q in PLANT_BITS and v is not None}
    unknown = [q for q in named if q not in PLANT_BITS and q != "packed"]
    if unknown:
        raise ValueError(f"unknown plant quantities {unknown} (known: {list(PLANT_QUANTITIES)})")
    if not cols:
        raise ValueError("a plant table pins at least one quantity")
    rows = {len(v) for v in cols.values()}
    if len(rows) != 1:
        raise ValueError(f"the quantities of a plant table have one length, got {sorted(rows)}")
    t = np.zeros((rows.pop(), PLANT_FLOATS), np.float32)
    ints = t.view(np.int32)
    for q, v in cols.items():
        on = ~np.isnan(v)
        ints[on, PLANT_WORDS["bits"]] |= PLANT_BITS[q]
        if q == "lag":
            if (v[on] != np.round(v[on])).any():
                raise ValueError("the lag of a plant is a whole number of physics steps")
            ints[on, PLANT_WORDS[q]] = v[on].astype(np.int32)
        else:
            t[on, PLANT_WORDS[q]] = v[on].astype(np.float32)
    return t


def plant_grid(kp_scale=None, kd_scale=None, friction=None, armature=None, mass_scale=None, lag=None, num_envs: int = 1) -> dict:
    """A named table of pinned plants: ``{quantity: [num_envs] fp64 for every pinned quantity, "packed": [num_envs, 8] fp32}``.
    Each argument is None (not pinned: the env keeps its draw or its nominal value), a scalar, or ``(lo, hi, n)`` like an axis
    of ``command_grid`` (both ends included, ``n = 1`` the midpoint; the lag's points are rounded to whole physics steps).  The
    table is the full product of the axes, ``kp_scale`` slowest and ``lag`` fastest; env ``i`` gets point ``i % n_points``."""
    given = dict(kp_scale=kp_scale, kd_scale=kd_scale, friction=friction, armature=armature, mass_scale=mass_scale, lag=lag)
    axes = {}
    for q, a in given.items():
        if a is None:
            continue
        if np.ndim(a) == 0:
            pts = np.array([float(a)])
        else:
            if len(a) != 3:
                raise ValueError(f"plant_grid: {q} is None, a scalar or (lo, hi, n), got {a!r}")
            lo, hi, n = float(a[0]), float(a[1]), int(a[2])
            if n < 1:
                raise ValueError(f"plant_grid: the axis {q} needs at least one point")
            pts = np.array([(lo + hi) / 2.0]) if n == 1 else np.linspace(lo, hi, n)
        if not np.isfinite(pts).all():
            raise ValueError(f"plant_grid: {q} must be finite, got {a!r}")
        axes[q] = np.round(pts) if q == "lag" else pts
    if not axes:
        raise ValueError("plant_grid: at least one quantity must be pinned")
    if int(num_envs) < 1:
        raise ValueError("num_envs must be at least 1")
    mesh = np.meshgrid(*axes.values(), indexing="ij")
    idx = np.arange(int(num_envs), dtype=np.int64) % mesh[0].size
    named = {q: np.ascontiguousarray(g.reshape(-1)[idx]) for q, g in zip(axes, mesh)}
    named["packed"] = pack_plant(named)
    return named


def parse_plant_axes(specs) -> dict:
    """the keyword arguments of ``plant_grid`` from command-line words ``name=value`` or ``name=lo:hi:n`` (play.py --eval_plant)"""
    axes = {}
    for spec in specs:
        name, eq, text = str(spec).partition("=")
        parts = text.split(":")
        if not eq or name not in PLANT_BITS or name in axes or len(parts) not in (1, 3):
            raise ValueError(f"--eval_plant takes name=value or name=lo:hi:n with each name of {list(PLANT_QUANTITIES)} at most once, "
                             f"got '{spec}'")
        try:
            axes[name] = float(parts[0]) if len(parts) == 1 else (float(parts[0]), float(parts[1]), int(parts[2]))
        except ValueError:
            raise ValueError(f"--eval_plant: '{spec}' holds no numbers (name=value or name=lo:hi:n)") from None
    return axes


def _plant_rows(plant) -> np.ndarray:
    """``[P, 8]`` fp32 of a named table, or of a packing handed over as it is"""
    if isinstance(plant, dict):
        return np.ascontiguousarray(plant["packed"] if "packed" in plant else pack_plant(plant), np.float32)
    rows = np.ascontiguousarray(plant, np.float32)
    if rows.ndim != 2 or rows.shape[1] != PLANT_FLOATS:
        raise ValueError(f"a plant table is a plant_grid() dict or [P, {PLANT_FLOATS}] fp32, got shape {rows.shape}")
    return rows


def sweep(commands, plants):
    """``(commands [C * P, 3] fp32, plant table)`` for N = C x P envs from ``commands`` [C, 3] and ``plants`` (a
    ``plant_grid`` dict or a packing [P, 8]): env ``i`` gets command ``i % C`` and plant ``i // C``.  The plant table comes
    back as it came: a named dict (every array repeated, ``packed`` included) or a packing"""
    cmd = np.asarray(commands, np.float32)
    if cmd.ndim != 2 or cmd.shape[1] != 3 or len(cmd) < 1:
        raise ValueError(f"sweep: commands are [C, 3] with C >= 1, got {cmd.shape}")
    rows = _plant_rows(plants)
    if len(rows) < 1:
        raise ValueError("sweep: the plant table needs at least one row")
    C, P = len(cmd), len(rows)
    tiled = np.ascontiguousarray(np.tile(cmd, (P, 1)))
    if isinstance(plants, dict):
        out = {q: np.repeat(np.asarray(v), C, axis=0) for q, v in plants.items() if q != "packed" and v is not None}
        out["packed"] = np.ascontiguousarray(np.repeat(rows, C, axis=0))
        return tiled, out
    return tiled, np.ascontiguousarray(np.repeat(rows, C, axis=0))


def plant_of_row(row) -> dict:
    """``{quantity: value}`` of the quantities one packed row pins (the lag an int)"""
    row = np.ascontiguousarray(row, np.float32)
    bits = int(row.view(np.int32)[PLANT_WORDS["bits"]])
    return {q: (int(row.view(np.int32)[PLANT_WORDS[q]]) if q == "lag" else float(row[PLANT_WORDS[q]]))
            for q in PLANT_QUANTITIES if bits & PLANT_BITS[q]}


def command_sequence(points, num_envs: int):
    """``[S, num_envs, 3]`` fp32 from ``points`` [S, 3]: every env follows the same sequence of commands"""
    pts = np.asarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or len(pts) < 1:
        raise ValueError(f"a command sequence is [S, 3] with S >= 1, got {pts.shape}")
    if int(num_envs) < 1:
        raise ValueError("num_envs must be at least 1")
    return np.ascontiguousarray(np.broadcast_to(pts[:, None, :], (len(pts), int(num_envs), 3)))


AXES = ("vx", "vy", "wz")
_COL = {name: (a, w) for name, a, w in TRACE_FIELDS}


def step_response(trace, segment_steps: int, tolerance: float = 0.1) -> list:
    """Rise, settling, overshoot and steady-state error of every command change in a trace ``[T, K, 72]``, in fp64.

    For each traced env, within its first episode only (the rows before its first ``ends``, that row included: the step
    that ends an episode is still a step of it), the rows are cut into segments of ``segment_steps`` by their ``t``.
    For segment s >= 1 of length L and each axis a whose command changed (delta = c_s[a] - c_{s-1}[a] != 0), with
    e_k = v_k[a] - c_s[a] for the k-th step of the segment, k = 1 .. L:
      ``rise_steps``    first k with |e_k| <= tolerance |delta|, else None
      ``settle_steps``  smallest k such that |e_j| <= tolerance |delta| for all j >= k, else None
      ``overshoot``     max(0, max_k sign(delta) e_k) / |delta|
      ``steady_error``  |mean of e_k over the last ceil(L / 4) steps|
    One dict per (env, segment, axis): ``{"env", "segment", "axis", "from", "to", "complete", ...}``; a segment that the
    end of the episode (or of the trace) cut short has ``complete: False`` and no figures."""
    tr = np.asarray(trace, np.float64)
    if tr.ndim != 3 or tr.shape[2] != TRACE_FLOATS:
        raise ValueError(f"a trace is [T, K, {TRACE_FLOATS}], got {tr.shape}")
    L = int(segment_steps)
    if L < 1:
        raise ValueError("segment_steps must be at least 1")
    c0, v0 = _COL["command"][0], _COL["v"][0]
    out = []
    for i in range(tr.shape[1]):
        rows = tr[:, i]
        ended = np.nonzero(rows[:, _COL["ends"][0]] > 0.5)[0]
        rows = rows[:int(ended[0]) + 1] if len(ended) else rows
        seg = (rows[:, 0] // L).astype(np.int64)                       # by the row's own t: the run may start at t > 0
        for s in np.unique(seg):
            at = np.nonzero(seg == s)[0]
            before = np.nonzero(seg == s - 1)[0]
            if s < 1 or len(before) == 0:
                continue
            c_new, c_old = rows[at[0], c0:c0 + 3], rows[before[-1], c0:c0 + 3]
            for a in range(3):
                delta = c_new[a] - c_old[a]
                if delta == 0:
                    continue
                r = {"env": i, "segment": int(s), "axis": AXES[a], "from": float(c_old[a]), "to": float(c_new[a]),
                     "complete": len(at) == L}
                if r["complete"]:
                    e = rows[at, v0 + a] - c_new[a]
                    inside = np.abs(e) <= tolerance * abs(delta)
                    first = np.nonzero(inside)[0]
                    outside = np.nonzero(~inside)[0]
                    settle = 1 if len(outside) == 0 else int(outside[-1]) + 2
                    tail = e[L - math.ceil(L / 4):]
                    r.update(rise_steps=int(first[0]) + 1 if len(first) else None,
                             settle_steps=settle if settle <= L else None,
                             overshoot=float(max(0.0, float(np.max(np.sign(delta) * e))) / abs(delta)),
                             steady_error=float(abs(tail.mean())))
                out.append(r)
    return out


def summarise_step_response(responses) -> dict:
    """per axis the medians of the figures over the complete responses (None where no response has the figure), and the
    count of incomplete ones"""
    summary = {"incomplete": sum(1 for r in responses if not r["complete"])}
    for axis in AXES:
        done = [r for r in responses if r["complete"] and r["axis"] == axis]
        block = {"responses": len(done)}
        for key in ("rise_steps", "settle_steps", "overshoot", "steady_error"):
            vals = [r[key] for r in done if r[key] is not None]
            block[key] = float(np.median(vals)) if vals else None
        summary[axis] = block
    return summary


def push_recovery(trace, tol: float = 0.1) -> list:
    """How the traced envs take their pushes, from a trace ``[T, K, 72]`` taken with events on (float 14 of a row is 1 in a
    step whose env was pushed).  Pure numpy, fp64, like ``step_response``.  One dict per (env, pushed step), in env then
    step order.  The window of a push starts at the pushed step and ends with its episode (the row whose ``ends`` is set,
    inclusive), with the trace, or before the env's next push, whichever comes first.
    ``recover_steps``: the smallest k >= 0 such that ``|v - command| <= tol`` on all three axes in every step from window
    step k to the window's end; None if there is none.  ``peak_error``: the largest ``|v - command|`` over axes and window.
    ``fell``: the episode ended in a fall inside the window at or before the step recovery would have needed, i.e. the
    window's last row has ``fallen`` set and the env had not recovered before it."""
    tr = np.asarray(trace, np.float64)
    if tr.ndim != 3 or tr.shape[2] != TRACE_FLOATS:
        raise ValueError(f"push_recovery wants a trace [T, K, {TRACE_FLOATS}], got {tr.shape}")
    steps, envs = tr.shape[:2]
    out = []
    for e in range(envs):
        pushed = np.nonzero(tr[:, e, TRACE_PUSHED] > 0.5)[0]
        for s in pushed:
            later = pushed[pushed > s]
            end = int(later[0]) if len(later) else steps                  # exclusive
            done = np.nonzero(tr[s:end, e, 1] > 0.5)[0]
            if len(done):
                end = s + int(done[0]) + 1
            err = np.abs(tr[s:end, e, 7:10] - tr[s:end, e, 4:7])
            ok = (err <= tol).all(1)
            bad = np.nonzero(~ok)[0]
            k = 0 if not len(bad) else int(bad[-1]) + 1
            recover = k if k < len(ok) else None
            fell = bool(tr[end - 1, e, 2] > 0.5) and (recover is None)
            out.append({"env": int(e), "step": int(s), "t": int(tr[s, e, 0]), "window": int(end - s),
                        "recover_steps": recover, "peak_error": float(err.max()), "fell": fell})
    return out


def summarise_push_recovery(rows) -> dict:
    """counts and medians over ``push_recovery``'s rows; JSON-serialisable"""
    rec = [r["recover_steps"] for r in rows if r["recover_steps"] is not None]
    return {"pushes": len(rows), "recovered": len(rec), "fell": sum(1 for r in rows if r["fell"]),
            "recover_steps_median": float(np.median(rec)) if rec else None,
            "peak_error_median": float(np.median([r["peak_error"] for r in rows])) if rows else None}


def aggregate(record, cat_reward=None, termination_prob=None, violations=None, term_names=()) -> dict:
    """metrics of a set of envs, in fp64, from their per-env tables: ``record`` [n, 12] (``FIELDS``), the per-env sums of
    the CaT-scaled reward and of the termination probability [n], and the per-env counts of steps with a violated
    constraint [n, len(term_names) + 1] (one column per term, the last for any term).  Ratios whose divisor is zero
    (no episode ended) are None."""
    r = np.asarray(record, np.float64).reshape(-1, len(FIELDS))
    s = {k: float(r[:, i].sum()) for i, k in enumerate(FIELDS)}
    steps, episodes = s["steps"], s["episodes"]

    def per_step(x):
        return x / steps if steps > 0 else None

    def per_episode(x):
        return x / episodes if episodes > 0 else None
    m = {"steps": steps, "episodes": episodes, "fall_rate": per_episode(s["falls"]),
         "reward_per_step": per_step(s["reward"]),
         "cat_reward_per_step": None if cat_reward is None else per_step(float(np.asarray(cat_reward, np.float64).sum())),
         "rms_err_lin": math.sqrt(s["err_lin2"] / steps) if steps > 0 else None,
         "rms_err_yaw": math.sqrt(s["err_yaw2"] / steps) if steps > 0 else None,
         "mean_tilt2": per_step(s["tilt2"]), "mean_torque2": per_step(s["torque2"]), "mean_feet": per_step(s["feet"]),
         "episode_return_mean": per_episode(s["done_return"]), "episode_length_mean": per_episode(s["done_length"]),
         "termination_prob_mean": None if termination_prob is None
         else per_step(float(np.asarray(termination_prob, np.float64).sum()))}
    if violations is not None:
        v = np.asarray(violations, np.float64).reshape(r.shape[0], -1)
        names = [*term_names, "any"]
        if v.shape[1] != len(names):
            raise ValueError(f"violations has {v.shape[1]} columns for {len(names)} names")
        for i, name in enumerate(names):
            m["violation_share/" + name] = per_step(float(v[:, i].sum()))
    return m


@dataclass
class EvalResult:
    per_env: np.ndarray                           # [N, 12] fp32: the simulator's record
    fields: tuple = FIELDS
    commands: np.ndarray | None = None            # [N, 3] fixed commands, [S, N, 3] schedule, or None (sampled)
    cat_reward: np.ndarray | None = None          # [N] fp32 sum of the CaT-scaled reward
    termination_prob: np.ndarray | None = None    # [N] fp32 sum of the CaT termination probability
    violations: np.ndarray | None = None          # [N, terms + 1] fp32 counts of steps with a violation (last: any term)
    term_names: tuple = ()
    metrics: dict = field(default_factory=dict)
    trace: np.ndarray | None = None               # [steps, K, 72] fp32: the simulator's step trace of envs 0 .. K - 1
    trace_fields: tuple = TRACE_FIELDS
    segment_steps: int | None = None              # control steps per segment when ``commands`` is a schedule
    pushes: bool = False                          # the env has cfg.events and ran with its interval events on
    termination_share: dict | None = None         # envs with cfg.terminations: {term: share of the ended episodes it ended}
    plant: np.ndarray | None = None               # [N, 8] fp32: the pinned plants (``plant_grid``), or None

    def push_recovery(self, tolerance: float = 0.1) -> list:
        """``push_recovery`` of this evaluation's trace (needs a trace)"""
        if self.trace is None:
            raise ValueError("push recovery needs a trace (trace_envs > 0)")
        return push_recovery(self.trace, tolerance)

    def step_response(self, tolerance: float = 0.1) -> list:
        """``step_response`` of this evaluation's trace (needs a schedule and a trace)"""
        if self.trace is None or self.segment_steps is None:
            raise ValueError("step responses need a command schedule and a trace (commands [S, N, 3], trace_envs > 0)")
        return step_response(self.trace, self.segment_steps, tolerance)

    def _aggregate(self, rows=slice(None)):
        def pick(x):
            return None if x is None else x[rows]
        return aggregate(self.per_env[rows], pick(self.cat_reward), pick(self.termination_prob), pick(self.violations),
                         self.term_names)

    def by_command(self) -> list:
        """the metrics per distinct command row, in order of first appearance: ``{"command", "envs", "metrics"}``"""
        if self.commands is None or self.commands.ndim == 3:         # drawn, or a schedule: one group
            return [{"command": None, "envs": int(len(self.per_env)), "metrics": dict(self.metrics)}]
        _, first, inverse = np.unique(self.commands, axis=0, return_index=True, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        out = []
        for g in np.argsort(first):
            rows = np.nonzero(inverse == g)[0]
            out.append({"command": [float(c) for c in self.commands[rows[0]]], "envs": int(len(rows)),
                        "metrics": self._aggregate(rows)})
        return out

    def by_plant(self) -> list:
        """the metrics per distinct plant row, in order of first appearance: ``{"plant", "envs", "metrics"}``, ``plant`` being
        ``{quantity: value}`` of what the row pins; without a plant table one group with ``plant`` None"""
        if self.plant is None:
            return [{"plant": None, "envs": int(len(self.per_env)), "metrics": dict(self.metrics)}]
        _, first, inverse = np.unique(self.plant.view(np.uint32), axis=0, return_index=True, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        out = []
        for g in np.argsort(first):
            rows = np.nonzero(inverse == g)[0]
            out.append({"plant": plant_of_row(self.plant[rows[0]]), "envs": int(len(rows)), "metrics": self._aggregate(rows)})
        return out

    def robustness(self, metric: str = "reward_per_step") -> dict:
        """where in the pinned range the policy breaks, from ``by_plant()`` in fp64: per pinned quantity ``metric`` against
        each value of it (the mean over the groups that share the value, values ascending), the best and the worst group with
        their plants, and the spread best - worst.  Groups whose ``metric`` is None (no step, no ended episode) are left out"""
        if self.plant is None:
            raise ValueError("robustness needs a plant table (evaluate_policy(plant=...))")
        groups = [g for g in self.by_plant() if g["metrics"].get(metric) is not None]
        if not groups:
            if metric not in self.metrics:
                raise ValueError(f"unknown metric '{metric}' (known: {sorted(self.metrics)})")
            return {"metric": metric, "groups": 0, "by_quantity": {}, "best": None, "worst": None, "spread": None}
        value = np.array([g["metrics"][metric] for g in groups], np.float64)
        by_quantity = {}
        for q in PLANT_QUANTITIES:
            pinned = [(g["plant"][q], v) for g, v in zip(groups, value) if q in g["plant"]]
            if pinned:
                xs = sorted({x for x, _ in pinned})
                by_quantity[q] = [{"value": x, "groups": sum(1 for y, _ in pinned if y == x),
                                   metric: float(np.mean([v for y, v in pinned if y == x]))} for x in xs]
        hi, lo = int(np.argmax(value)), int(np.argmin(value))
        pick = lambda i: {"plant": groups[i]["plant"], "envs": groups[i]["envs"], metric: float(value[i])}   # noqa: E731
        return {"metric": metric, "groups": len(groups), "by_quantity": by_quantity, "best": pick(hi), "worst": pick(lo),
                "spread": float(value[hi] - value[lo])}

    def to_json(self, by_command: bool = True) -> str:
        d = {"metrics": self.metrics, "num_envs": int(len(self.per_env)), "fields": list(self.fields)}
        if by_command and self.commands is not None:
            d["by_command"] = self.by_command()
        if self.trace is not None and self.segment_steps is not None:
            responses = self.step_response()
            d["segment_steps"] = int(self.segment_steps)
            d["step_response"] = {"summary": summarise_step_response(responses), "responses": responses}
        if self.trace is not None and self.pushes:
            rows = self.push_recovery()
            d["push_recovery"] = {"summary": summarise_push_recovery(rows), "pushes": rows}
        if self.termination_share is not None:
            d["termination_share"] = dict(self.termination_share)
        if self.plant is not None:
            d["by_plant"] = self.by_plant()
            d["robustness"] = self.robustness()
        return json.dumps(d)


def evaluate_policy(env, policy, steps: int, commands=None, deterministic: bool = True,
                    fresh_cat_state: bool = False, segment_steps: int | None = None, trace_envs: int = 0,
                    corruption: bool | None = None, pushes: bool | None = None,
                    randomization: bool | None = None, plant=None, wrench: bool | None = None) -> EvalResult:
    """Roll ``policy`` out for ``steps`` control steps from a fresh reset and measure it.

    ``policy`` is an ``Agent`` - its observations are normalised by the frozen ``obs_rms`` and the action is the mean
    (``deterministic=False`` samples); neither its parameters nor its normaliser are modified - or any callable
    ``raw_obs [N, D] -> action [N, 12]``.  ``commands`` [N, 3] (tensor or array) fixes env i's command to row i for the
    whole evaluation; None leaves the draws to the simulator.  Needs the closed-loop simulator (``TypeError`` otherwise).
    ``commands`` [S, N, 3] with ``segment_steps`` = L is a schedule: a step that starts at episode length t uses segment
    ``min(t // L, S - 1)``, and an episode that ends restarts it.  ``trace_envs`` = K > 0 attaches a zeroed trace
    ``[steps, K, 72]`` of the first K envs, written by the simulator's own launch: ``EvalResult.trace``.

    Use a dedicated env: its episode counters, reset masks, action history and constraint episode sums are zeroed, the
    simulator is reset, and the env is LEFT IN THE EVALUATED STATE (the record and the command table are detached again,
    also when the roll-out raises).  The loop never synchronises the host.

    ``fresh_cat_state=True`` also starts the env's CaT state as at construction (``CaTEnv.fresh_cat_state``: running maxima
    and their first-call flag, probability buffers, episode sums, log ring - all in place) and keeps the curriculum from
    running for the length of the evaluation, so every term's ``max_p`` is what the caller set through ``set_term_cfg``.  The
    result is then a function of the parameters, the observation normaliser, the ``max_p`` vector, the env cfg and seed,
    ``steps`` and ``commands`` alone: two such evaluations agree bit for bit whatever the env did in between (DESIGN
    section 11).  The default leaves the CaT state as the env's last step left it.

    ``corruption`` (envs with ``cfg.observations``): None leaves the env's observation-noise switch as it is; a bool sets it
    for the evaluation and puts it back afterwards, also when the roll-out raises.  The record and the trace read state,
    not observations: the noise reaches them only through the actions the policy takes on what it sees.

    ``pushes`` (envs with ``cfg.events``): None leaves the env's interval-event switch as it is; a bool sets it for the
    evaluation and puts it back afterwards, also when the roll-out raises.  Reset and startup terms stay as configured.

    ``randomization`` (envs whose ``cfg.events`` randomises the robot): None leaves the switch as it is; a bool sets it for
    the evaluation (False: the nominal robot) and puts it back afterwards, likewise.

    ``wrench`` (envs whose ``cfg.events`` has ``apply_external_force_torque``): None leaves the switch as it is; a bool sets it
    for the evaluation (False: no external force or torque) and puts it back afterwards, likewise.

    ``plant`` (a ``plant_grid`` dict or a packing [N, 8]): env i's plant is what row i pins - gains, joint friction, armature,
    base mass, actuator lag - for the whole evaluation, inside the simulator's launch (``CaTEnv.set_fixed_plant``); the table
    is attached for the call and detached afterwards, also when the roll-out raises.  Orthogonal to ``randomization``: a
    quantity that a row does not pin keeps the env's draw, or its nominal value with the switch off.  ``EvalResult.plant``,
    ``by_plant()`` and ``robustness()`` read the result per plant.

    On an env with ``cfg.terminations`` the result carries ``termination_share``: per term, the share of the episodes that
    ended during the evaluation whose last step had the term set (the termination manager's record, which the reset zeroes
    and this call pops; empty when no episode ended).  Without the block the result is what it was."""
    import contextlib
    import torch
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    steps = int(steps)
    if steps < 1 or steps > MAX_STEPS:
        raise ValueError(f"steps must be in [1, 2^24] (the record counts in fp32), got {steps}")
    u = env.unwrapped
    if not hasattr(u, "set_eval_record"):
        raise TypeError("evaluate_policy needs a CaTEnv")
    n, dev = u.num_envs, u.device
    trace_envs = int(trace_envs)
    if trace_envs < 0 or trace_envs > n:
        raise ValueError(f"trace_envs must be in [0, {n}], got {trace_envs}")
    lead = ()                                                        # (S,) when the commands are a schedule
    if commands is not None and len(np.shape(commands)) == 3:                # np.shape reads a tensor's own .shape
        if segment_steps is None or int(segment_steps) < 1:
            raise ValueError("a command schedule [S, N, 3] needs segment_steps >= 1")
        segment_steps = int(segment_steps)
        lead = (int(np.shape(commands)[0]),)
    elif segment_steps is not None:
        raise ValueError("segment_steps goes with a command schedule [S, N, 3]")
    record = torch.zeros(n, len(FIELDS), device=dev)
    table = None
    if isinstance(commands, torch.Tensor) and commands.device == dev and commands.dtype == torch.float32:
        table = commands.detach().reshape(*lead, n, 3).contiguous().clone()   # a table of its own, without a host round trip
    elif commands is not None:
        table = torch.as_tensor(np.asarray(commands.detach().cpu() if isinstance(commands, torch.Tensor) else commands,
                                           np.float32)).reshape(*lead, n, 3).contiguous().to(dev)
    plant_table = None
    if plant is not None:
        rows = _plant_rows(plant)
        if len(rows) != n:
            raise ValueError(f"the plant table has {len(rows)} rows, the env {n} envs (plant_grid(..., num_envs={n}))")
        plant_table = torch.from_numpy(rows.copy()).to(dev)
    if isinstance(policy, Agent):
        agent = policy

        def policy(obs):
            return agent(obs, deterministic=deterministic)
    cm = getattr(u, "constraint_manager", None)
    names = tuple(cm.active_terms) if cm is not None else ()
    cat_reward, term_prob = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    viol = torch.zeros(n, len(names) + 1, device=dev)
    member = None                                                    # [K, terms]: column k belongs to term j
    u.episode_length_buf.zero_()
    for mask in (u.reset_buf, u.reset_terminated, u.reset_time_outs):
        mask.zero_()
    u.action_manager.reset()
    if cm is not None:
        cm._ep_viol.zero_()
        cm._ep_prob.zero_()
    u.set_eval_record(record)                                         # TypeError on the stream simulator
    trace = torch.zeros(steps, trace_envs, TRACE_FLOATS, device=dev) if trace_envs else None
    om = getattr(u, "observation_manager", None)
    if corruption is not None and om is None:
        u.set_eval_record(None)
        raise TypeError("evaluate_policy(corruption=...) needs an env with cfg.observations")
    corruption_before = None if om is None else om.corruption
    em = getattr(u, "event_manager", None)
    if pushes is not None and em is None:
        u.set_eval_record(None)
        raise TypeError("evaluate_policy(pushes=...) needs an env with cfg.events")
    if randomization is not None and (em is None or em.randomization is None):
        u.set_eval_record(None)
        raise TypeError("evaluate_policy(randomization=...) needs an env whose cfg.events randomises the robot")
    if wrench is not None and (em is None or "wrench" not in em.block):
        u.set_eval_record(None)
        raise TypeError("evaluate_policy(wrench=...) needs an env whose cfg.events has apply_external_force_torque")
    wrench_before = None if em is None else em.wrench_enabled
    randomization_before = None if em is None else em.randomization_enabled
    pushes_before = None if em is None else em.interval_enabled
    pushes_on = bool(em is not None and (pushes_before if pushes is None else pushes)
                     and (em.block["flags"] & 1 or "interval_range" in em.block))   # a push term (per step or timed) is on
    frozen = contextlib.ExitStack()
    if fresh_cat_state:
        u.fresh_cat_state()
        frozen.enter_context(u.curriculum_frozen())
    try:
        if corruption is not None:
            om.set_corruption(corruption)
        if pushes is not None:
            em.set_interval_enabled(pushes)
        if randomization is not None:
            em.set_randomization_enabled(randomization)
        if wrench is not None:
            em.set_wrench_enabled(wrench)
        if lead:
            u.set_fixed_commands(table, segment_steps)
        else:
            u.set_fixed_commands(table)
        if trace is not None:
            u.set_trace(trace)
        if plant_table is not None:
            u.set_fixed_plant(plant_table)                           # ValueError names the row and the quantity
        obs = env.reset()[0]["policy"]
        with torch.no_grad():
            for _ in range(steps):
                obs, reward, _, _, _ = env.step(policy(obs))
                obs = obs["policy"]
                cat_reward.add_(reward)
                if names:
                    term_prob.add_(cm._cstr_prob_buf)
                    if member is None:                               # the packed matrix exists after the first compute()
                        off = list(cm._term_off)
                        member = torch.zeros(off[-1], len(names), device=dev)
                        for j in range(len(names)):
                            member[off[j]:off[j + 1], j] = 1.0
                    hit = ((cm.cat._p_cstr > 0).float() @ member) > 0   # small exact integer counts
                    viol[:, :-1].add_(hit)
                    viol[:, -1].add_(hit.any(1))
    finally:
        frozen.close()
        if plant_table is not None:
            u.set_fixed_plant(None)
        if trace is not None:
            u.set_trace(None)
        u.set_eval_record(None)
        u.set_fixed_commands(None)
        if corruption is not None:
            om.set_corruption(corruption_before)
        if pushes is not None:
            em.set_interval_enabled(pushes_before)
        if randomization is not None:
            em.set_randomization_enabled(randomization_before)
        if wrench is not None:
            em.set_wrench_enabled(wrench_before)
    res = EvalResult(per_env=record.cpu().numpy(), commands=None if table is None else table.cpu().numpy(),
                     cat_reward=cat_reward.cpu().numpy(), termination_prob=term_prob.cpu().numpy(),
                     violations=viol.cpu().numpy(), term_names=names, trace=None if trace is None else trace.cpu().numpy(),
                     segment_steps=segment_steps if lead else None, pushes=pushes_on,
                     plant=None if plant_table is None else plant_table.cpu().numpy())
    res.metrics = res._aggregate()
    tm = getattr(u, "termination_manager", None)
    if tm is not None:
        log = tm.pop_log() or {}
        res.termination_share = {k.split("/", 1)[1]: float(v) for k, v in log.items()}
    return res
