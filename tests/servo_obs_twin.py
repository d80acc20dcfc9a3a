"""Numpy twin of the servo surrogate's policy observation (csrc/servo_sim.hip: the post-pass of the obs-on instances,
include/catppo.h catppo_servo_obs; DESIGN section 9, "Observations").

``ServoObsTwin`` sits on top of the reward twin.  Its row has the extra field ``policy_obs`` behind everything else, on a
16-byte boundary, padded with zeros to a multiple of four floats.  After the parent's ``initial`` / ``step`` it fills the
field from the written row's raw ``obs`` field, the table and the Philox words of ``oracle/rng_oracle.py`` with the header's
formula, one ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_reward_twin as RT
import servo_twin as T

F32 = np.float32
TAG_OBS = 0x4F42534E                                        # "OBSN": fourth counter word
BIAS, NOISE, CLIP = 1, 2, 4
RAW = 45


def identity_table(noise=None):
    """scale 1, the simulator's order, no bias / clip; ``noise`` = (lo, width) sets the noise bit on every float"""
    lo, width = (0.0, 0.0) if noise is None else noise
    return [(j, NOISE if noise is not None else 0, 0.0, lo, width, 0.0, 0.0, 1.0) for j in range(RAW)]


def with_corruption(entries, on):
    return list(entries) if on else [(e[0], e[1] & ~NOISE, *e[2:]) for e in entries]


class ServoObsTwin(RT.ServoRewardTwin):
    def __init__(self, *args, obs_table=(), **kw):
        super().__init__(*args, **kw)
        assert self.D == RAW
        self.set_obs_table(obs_table)
        self.P = len(self.obs_table)
        assert 1 <= self.P <= 64
        self.off = dict(self.off)
        self.off["policy_obs"] = (self.F, self.P)
        self.F_raw = self.F
        self.F += (self.P + 3) // 4 * 4

    def set_obs_table(self, entries):
        self.obs_table = [(int(e[0]), int(e[1]), *(F32(v) for v in e[2:])) for e in entries]

    def uniforms(self, ep, t):
        """[N, P] fp32: u of float j for envs whose observation describes (episode ``ep``, episode length ``t``)"""
        blocks = (self.P + 3) // 4
        t = np.asarray(t, np.int64)
        assert (t >= 0).all() and (t < 2 ** 27).all()
        u = [self._philox(np.asarray(ep, np.uint32), ((t << 4) | b).astype(np.uint32), TAG_OBS) for b in range(blocks)]
        return np.concatenate(u, 1)[:, :self.P]

    def policy(self, raw, ep, t):
        """the field [N, P] from the raw observation [N, 45]"""
        u = self.uniforms(ep, t)
        out = np.zeros((self.N, self.P), F32)
        for j, (src, flags, bias, nlo, nwidth, clo, chi, scale) in enumerate(self.obs_table):
            x = raw[:, min(max(src, 0), RAW - 1)].astype(F32)
            if flags & BIAS:
                x = x + bias
            if flags & NOISE:
                x = (x + u[:, j] * nwidth) + nlo
            if flags & CLIP:
                x = np.where(x < clo, clo, x).astype(F32)
                x = np.where(x > chi, chi, x).astype(F32)
            out[:, j] = x * scale
        return out

    def initial(self, episode_length):
        slab = super().initial(episode_length)
        zero = np.zeros(self.N, np.int64)
        self._f(slab, "policy_obs")[:] = self.policy(self._f(slab, "obs"), zero, zero)
        return slab

    def key_of(self, out, episode_length):
        """(ep', t') of the observation in the written row ``out`` of a step that started at ``episode_length``"""
        t = np.asarray(episode_length, np.int64)
        ends = (t + 1 >= self.max_len) | (self._f(out, "hard_reset")[:, 0] > 0)
        ep_out = self._f(out, "servo")[:, 13].astype(np.uint32)         # already counts the episode that ended
        return ep_out, np.where(ends, 0, t + 1)

    def step(self, slab, action, reset, episode_length):
        out = super().step(slab, action, reset, episode_length)
        ep, t = self.key_of(out, episode_length)
        self._f(out, "policy_obs")[:] = self.policy(self._f(out, "obs"), ep, t)
        return out


def make_twin(cfg, n, obs_table, table=(), env_offset=0, seed=RT.SEED, max_len=RT.MAX_LEN, **kw):
    return ServoObsTwin(n, RAW, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, env_offset,
                        table=table, obs_table=obs_table, **kw)


def run_obs_twin(twin, actions, episode_length0, switch=None):
    """slabs [steps + 1, N, F]; ``switch`` = (step index, entries): the table is replaced before that step"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs = [slab]
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_obs_table(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs)
