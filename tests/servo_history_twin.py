"""Numpy twin of the servo surrogate's observation history (csrc/servo_sim_kernel.h: the history-on instances of
servo_sim_history.hip, include/catppo.h catppo_servo_history; DESIGN section 9, "History").

``ServoHistoryTwin`` wraps a twin whose row has the ``policy_obs`` field (``servo_obs_twin`` and everything on top of it) and
extends that row by the field ``policy_obs_hist`` behind it: T floats padded with zeros to a multiple of four, outside the
part of the row the inner twin knows (``row_floats``), so a slab here is ``stride`` = ``row_floats`` + pad4(T) floats wide.
The history adds no arithmetic: after the inner twin's ``initial`` / ``step`` every float of the field is selected from the
written row's ``policy_obs`` (the fp32 values of ``servo_obs_twin``) or copied from the input row's float one slot later, by the
map's words ``cur | w << 8 | newest << 16`` and the header's formula, clamps included.  Everything the wrapper does not define is the inner
twin's.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
NEWEST = 0x10000
MAX_FLOATS, MAX_DEPTH = 512, 16


def history_map(widths, depths):
    """the map of terms of frame widths ``widths`` and depths ``depths`` in table order, restated here"""
    words, at = [], 0
    for w, depth in zip(widths, depths):
        for slot in range(depth):
            words += [(at + k) | w << 8 | (NEWEST if slot == depth - 1 else 0) for k in range(w)]
        at += w
    return np.asarray(words, np.uint32)


class ServoHistoryTwin:
    def __init__(self, inner, words):
        self.inner = inner
        self.set_history(words)
        self.T = len(self.hist_map)
        assert 1 <= self.T <= MAX_FLOATS
        self.row_floats = inner.F
        self.off = dict(inner.off)
        self.off["policy_obs_hist"] = (inner.F, self.T)
        self.F = self.stride = inner.F + (self.T + 3) // 4 * 4

    def __getattr__(self, name):                                             # whatever is not defined here is the inner twin's
        return getattr(self.inner, name)

    def set_history(self, words):
        self.hist_map = np.asarray(words, np.uint32).copy()

    def _f(self, slab, name):
        a, w = self.off[name]
        return slab[:, a:a + w]

    def _widen(self, row, hist):
        out = np.zeros((self.N, self.stride), F32)
        out[:, :self.row_floats] = row
        self._f(out, "policy_obs_hist")[:] = hist
        return out

    def history(self, frame, hin, fill):
        """the field [N, T]: ``frame`` [N, P] the written row's current frame, ``hin`` [N, T] the input row's field (None with
        ``fill`` all set), ``fill`` [N] the frame is the first of an episode"""
        P, T = frame.shape[1], self.T
        i = np.arange(T)
        cur = np.minimum((self.hist_map & 0xFF).astype(np.int64), P - 1)
        nxt = np.minimum(i + ((self.hist_map >> 8) & 0xFF).astype(np.int64), T - 1)
        newest = (self.hist_map & NEWEST) != 0
        fresh = np.asarray(fill, bool)[:, None] | newest[None, :]
        old = np.zeros((self.N, T), F32) if hin is None else hin[:, nxt]
        return np.where(fresh, frame[:, cur], old).astype(F32)

    def initial(self, episode_length):
        row = self.inner.initial(episode_length)
        return self._widen(row, self.history(self.inner._f(row, "policy_obs"), None, np.ones(self.N, bool)))

    def step(self, slab, action, reset, episode_length):
        assert slab.shape == (self.N, self.stride)
        row = self.inner.step(np.ascontiguousarray(slab[:, :self.row_floats]), action, reset, episode_length)
        t = np.asarray(episode_length, np.int64)
        ends = (t + 1 >= self.inner.max_len) | (self.inner._f(row, "hard_reset")[:, 0] > 0)
        return self._widen(row, self.history(self.inner._f(row, "policy_obs"), self._f(slab, "policy_obs_hist"), ends))


def run_history_twin(twin, actions, episode_length0, switch=None):
    """slabs [steps + 1, N, stride]; ``switch`` = (step index, entries): the observation table is replaced before that step.
    The bookkeeping around the twin is ``servo_twin.run_twin``'s"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs = [slab]
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.inner.set_obs_table(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs)
