"""Numpy twin of the servo surrogate's step-response mode (csrc/servo_sim.hip: ``fixed_segments``, ``trace``; DESIGN
section 9, "Step responses").

``ServoTraceTwin`` is ``ServoEvalTwin`` with a command schedule ``[S, N, 3]`` in place of the fixed table and with the
step trace ``[T, K, 72]``.  The state row and the record are the parents', untouched.  Every value of a trace row but ``t``
and the action is a field of the row the step just wrote (or, for ``ends`` and the feet count, one kernel expression away
from fields of it, with the same fp32 operands), so the twin reads them from there.  Test infrastructure.
"""
from __future__ import annotations

import numpy as np

import servo_eval_twin as E
import servo_twin as T

F32 = np.float32
TRACE_FLOATS = 72
#: (name, first float, width) - restated here, compared with native.SERVO_TRACE_FIELDS by the tests
TRACE_FIELDS = (("t", 0, 1), ("ends", 1, 1), ("fallen", 2, 1), ("reward", 3, 1), ("command", 4, 3), ("v", 7, 3),
                ("roll", 10, 1), ("pitch", 11, 1), ("z", 12, 1), ("ncon", 13, 1), ("zero", 14, 2), ("contact", 16, 4),
                ("fz", 20, 4), ("q", 24, 12), ("qd", 36, 12), ("tau_w", 48, 12), ("action", 60, 12))
COL = {name: slice(a, a + w) for name, a, w in TRACE_FIELDS}


class ServoTraceTwin(E.ServoEvalTwin):
    def __init__(self, *args, schedule=None, segment_steps=None, trace_envs=0, trace_capacity=0, **kw):
        super().__init__(*args, **kw)
        self.schedule = None
        if schedule is not None:
            self.schedule = np.ascontiguousarray(schedule, F32).reshape(-1, self.N, 3)
            self.segment_steps = int(segment_steps)
            assert self.segment_steps >= 1 and self.fixed is None
        self.K, self.T = int(trace_envs), int(trace_capacity)
        self.trace = np.zeros((self.T, self.K, TRACE_FLOATS), F32) if self.K else None
        self._t = None                                    # the episode lengths of the call in flight

    def command(self, ep, k):
        """the schedule's row min(t // L, S - 1) of every env: ``t`` is the episode length the running ``step`` or
        ``initial`` was given; the parent asks for the post-reset command with a scalar resample index 0 (t = 0)"""
        if self.schedule is None:
            return super().command(ep, k)
        t = np.zeros(self.N, np.int64) if np.isscalar(k) else self._t
        seg = np.minimum(t // self.segment_steps, len(self.schedule) - 1)
        return self.schedule[seg, np.arange(self.N)].copy()

    def initial(self, episode_length):
        self._t = np.asarray(episode_length, np.int64).copy()
        return super().initial(episode_length)              # init mode writes no trace row; the caller zeroes the buffer

    def step(self, slab, action, reset, episode_length):
        t = self._t = np.asarray(episode_length, np.int64).copy()
        slot = self.record[:, 0].astype(np.int64)           # steps counted before this one
        out = super().step(slab, action, reset, episode_length)
        if self.trace is None:
            return out
        f, n = self._f, self.N
        x = f(out, "servo")
        fallen = f(out, "hard_reset")[:, 0] > 0
        row = np.zeros((n, TRACE_FLOATS), F32)
        row[:, COL["t"]] = t.astype(F32)[:, None]
        row[:, 1] = ((t + 1 >= self.max_len) | fallen).astype(F32)
        row[:, 2] = fallen.astype(F32)
        row[:, 3] = f(out, "reward")[:, 0]
        row[:, COL["command"]] = f(out, "command")
        row[:, COL["v"]] = x[:, 0:3]
        row[:, 10], row[:, 11] = x[:, 3], x[:, 4]
        row[:, 12] = f(out, "root_pos_w")[:, 2]
        row[:, 13] = T.tree4(x[:, 9:13])
        row[:, COL["contact"]] = x[:, 9:13]
        row[:, COL["fz"]] = f(out, "forces").reshape(n, T.H, T.B, 3)[:, 0, T.FOOT_BODY, 2]
        row[:, COL["q"]], row[:, COL["qd"]] = f(out, "joint_pos"), f(out, "joint_vel")
        row[:, COL["tau_w"]] = f(out, "applied_torque")
        row[:, COL["action"]] = np.asarray(action, F32)
        for i in range(self.K):
            if 0 <= slot[i] < self.T:                       # slots past the capacity are dropped
                self.trace[slot[i], i] = row[i]
        return out


def run_trace_twin(twin: ServoTraceTwin, actions, episode_length0):
    """``servo_eval_twin.run_eval_twin`` with the trace: (slabs, record, trace [T, K, 72] or None)"""
    slabs, rec = E.run_eval_twin(twin, actions, episode_length0)
    return slabs, rec, None if twin.trace is None else twin.trace.copy()


def episode_lengths(twin, slabs, episode_length0):
    """[steps, N] int64: the episode length every step started from, by a plain recount over the slabs"""
    o = twin.off["hard_reset"][0]
    t = np.asarray(episode_length0, np.int64).copy()
    out = np.zeros((len(slabs) - 1, twin.N), np.int64)
    for s in range(1, len(slabs)):
        out[s - 1] = t
        t = t + 1
        t[(slabs[s, :, o] > 0.5) | (t >= twin.max_len)] = 0
    return out
