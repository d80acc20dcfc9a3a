"""Numpy twin of the servo surrogate's events (csrc/servo_sim.hip: the events-on instances, include/catppo.h
catppo_servo_events; DESIGN section 9, "Events").

``ServoEventsTwin`` sits on top of the observation twin and touches none of its parents.  The parents already derive the
next row from an input row, so the events are restated as what they are - changes to the state a step starts from:

* the first state of an episode (joint-reset and root-reset terms) is patched into a copy of the input slab for the envs
  whose reset flag is set, and the parents then step that copy with no reset flag at all;
* a push overwrites the three velocities and kicks roll and pitch of that copy;
* the traction scales the three velocity rows of ``G`` per env (``G`` broadcasts: ``[5, N, 16]``).

What the parents cannot know is fixed up on the written row: the angular rates keep differentiating against the un-kicked
tilt, a post-reset observation shows the next episode's first joint velocities and yaw rate, the reward terms read the
un-kicked input row, trace float 14 is the push mask; the policy observation is then recomputed from the final raw one.
One ``np.float32`` operation per rounded kernel operation.  With ``obs_table`` None the row has no policy field.
Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T
from oracle import rng_oracle as R

F32 = np.float32
TAG_PUSH, TAG_JVEL, TAG_ROOT, TAG_FRIC = 0x50555348, 0x4A56454C, 0x524F4F54, 0x46524943       # "PUSH" "JVEL" "ROOT" "FRIC"
PUSH, JOINT_SCALE, JOINT_OFFSET, ROOT, FRICTION = 1, 2, 4, 8, 16
FLOATS = 32
#: word offsets of the block, restated here; the tests compare them with native.SERVO_EVENT_WORDS
WORDS = {"flags": 0, "p": 1, "num_buckets": 2, "push": 4, "joint_pos": 14, "joint_vel": 16, "root_pos": 18, "root_vel": 22,
         "friction": 28}
TRACE_PUSHED = 14


def block(flags=0, p=0.0, num_buckets=1, **ranges):
    """the 32 words from (a, b) ranges: ``push=[(a, b)] * 5`` (vx vy wz roll-rate pitch-rate), ``joint_pos=[(a, b)]``,
    ``joint_vel``, ``root_pos=[x, y]``, ``root_vel=[x, y, yaw]``, ``friction=[(a, b)]``; lo = f32(a), width = f32(b - a)"""
    w = np.zeros(FLOATS, F32)
    w.view(np.int32)[WORDS["flags"]], w.view(np.int32)[WORDS["num_buckets"]] = int(flags), int(num_buckets)
    w[WORDS["p"]] = p
    for name, pairs in ranges.items():
        for i, (a, b) in enumerate(pairs):
            w[WORDS[name] + 2 * i], w[WORDS[name] + 2 * i + 1] = F32(a), F32(float(b) - float(a))
    return w


class ServoEventsTwin(OT.ServoObsTwin):
    def __init__(self, *args, events=None, obs_table=None, **kw):
        self.has_policy = obs_table is not None
        super().__init__(*args, obs_table=obs_table if self.has_policy else OT.identity_table(), **kw)
        if not self.has_policy:                             # no observation table: the row ends behind the private state
            self.off = {k: v for k, v in self.off.items() if k != "policy_obs"}
            self.F, self.P = self.F_raw, 0
        self.G0 = self.G
        self.set_events(np.zeros(FLOATS, F32) if events is None else events)
        self.pushed = np.zeros(self.N, bool)                # the push mask of the last step
        self._raw_slab = None

    def set_events(self, words):
        w = np.ascontiguousarray(words, F32).copy()
        assert w.shape == (FLOATS,)
        self.ev = w
        self.flags = int(w.view(np.int32)[WORDS["flags"]])
        self.buckets = int(w.view(np.int32)[WORDS["num_buckets"]])

    def _pair(self, name, i=0):
        return self.ev[WORDS[name] + 2 * i], self.ev[WORDS[name] + 2 * i + 1]

    # ------------------------------------------------------------------ randomness
    def _uniform(self, c0, c1, c2, tag):
        """[N, 4] fp32 in (0, 1): Philox4x32-10 with key = seed and counter {c0, c1, c2, tag}"""
        n = self.N
        col = lambda x: np.full(n, x, np.uint32) if np.isscalar(x) else np.asarray(x).astype(np.uint32)   # noqa: E731
        ctr = np.stack([col(c0), col(c1), col(c2), col(tag)], -1)
        key = np.broadcast_to(np.array([self.seed & 0xFFFFFFFF, self.seed >> 32], np.uint32), (n, 2))
        return R.uniform_open(R.philox4x32_10(ctr, key))

    @staticmethod
    def _sample(u, pair):
        lo, width = pair
        return (lo + u * width).astype(F32)

    # ------------------------------------------------------------------ the first state of (env, episode)
    def first_joint(self, ep):
        """(q0, qd0) [N, 12]: the built-in pose at rest, or the joint-reset term's"""
        u = np.concatenate([self._uniform(self.gid, ep, blk, T.TAG_INIT) for blk in range(3)], 1)
        qd0 = np.zeros((self.N, T.J), F32)
        if self.flags & (JOINT_SCALE | JOINT_OFFSET):
            s = self._sample(u, self._pair("joint_pos"))
            q0 = T.DEFAULT_JOINT_POS * s if self.flags & JOINT_SCALE else T.DEFAULT_JOINT_POS + s
            if self.flags & JOINT_OFFSET:
                u2 = np.concatenate([self._uniform(self.gid, ep, blk, TAG_JVEL) for blk in range(3)], 1)
                qd0 = self._sample(u2, self._pair("joint_vel"))
        else:
            q0 = T.DEFAULT_JOINT_POS + (u - F32(0.5)) * self.p["init_noise"]
        return q0.astype(F32), qd0

    def init_q(self, ep):
        return self.first_joint(ep)[0]

    def first_root(self, ep):
        """(xy [N, 2], v0 [N, 3]): zeros without the root-reset term"""
        xy, v0 = np.zeros((self.N, 2), F32), np.zeros((self.N, 3), F32)
        if self.flags & ROOT:
            a, b = self._uniform(self.gid, ep, 0, TAG_ROOT), self._uniform(self.gid, ep, 1, TAG_ROOT)
            for k in range(2):
                xy[:, k] = self._sample(a[:, k], self._pair("root_pos", k))
            for k in range(3):
                v0[:, k] = self._sample(b[:, k], self._pair("root_vel", k))
        return xy, v0

    def friction(self):
        """(bucket [N], mu [N]) of every env: once for all episodes"""
        u = self._uniform(self.gid, 0, 0, TAG_FRIC)[:, 0]
        bucket = (u * F32(self.buckets)).astype(np.int32)                  # truncation, like the kernel's (int)
        bucket = np.maximum(np.minimum(bucket, self.buckets - 1), 0)
        mu = self._sample(self._uniform(bucket, 0, 1, TAG_FRIC)[:, 0], self._pair("friction"))
        return bucket, mu

    def traction(self):
        if not self.flags & FRICTION:
            return np.ones(self.N, F32)
        mu = self.friction()[1]
        return np.where(mu < F32(1), mu, F32(1)).astype(F32)

    def push(self, ep, t):
        """(pushed [N] bool, v [N, 3], kick [N, 2]): the push of the step that starts episode ``ep`` at length ``t``"""
        n = self.N
        if not self.flags & PUSH:
            return np.zeros(n, bool), np.zeros((n, 3), F32), np.zeros((n, 2), F32)
        t = np.asarray(t, np.int64)
        assert (t >= 0).all() and (t < 2 ** 27).all()
        u0 = self._uniform(self.gid, ep, (t << 1), TAG_PUSH)
        u1 = self._uniform(self.gid, ep, (t << 1) | 1, TAG_PUSH)
        pushed = u0[:, 0] < self.ev[WORDS["p"]]
        v = np.stack([self._sample(u0[:, 1 + k], self._pair("push", k)) for k in range(3)], 1)
        kick = np.stack([(self._sample(u1[:, k], self._pair("push", 3 + k)) * self.step_dt).astype(F32) for k in range(2)], 1)
        return pushed, v, kick

    # ------------------------------------------------------------------ rows
    def _base(self):
        return OT.ServoObsTwin if self.has_policy else RT.ServoRewardTwin

    def _finish(self, out, ep, t):
        if self.has_policy:
            self._f(out, "policy_obs")[:] = self.policy(self._f(out, "obs"), ep, t)
        return out

    def initial(self, episode_length):
        slab = self._base().initial(self, episode_length)
        zero = np.zeros(self.N, np.int64)
        qd0 = self.first_joint(zero)[1]
        xy, v0 = self.first_root(zero)
        f = self._f
        f(slab, "joint_vel")[:] = qd0
        f(slab, "root_pos_w")[:, 0:2] = xy
        f(slab, "servo")[:, 0:3] = v0
        obs = f(slab, "obs")
        obs[:, 21:33], obs[:, 2] = qd0, v0[:, 2]
        return self._finish(slab, zero, zero)

    def raw_terms(self, slab, out, action, reset, episode_length):
        """the reward terms read the input row before the push: ``ang`` differentiates against the un-kicked tilt"""
        return super().raw_terms(self._raw_slab, out, action, reset, episode_length)

    def step(self, slab, action, reset, episode_length):
        f, n = self._f, self.N
        rst = np.asarray(reset).astype(bool)
        t = np.asarray(episode_length, np.int64)
        start = np.array(slab, F32, copy=True)
        ep = f(start, "servo")[:, 13].astype(np.uint32)
        # ---- the first state of episode `ep`, for the envs that ended their episode in the previous step
        q0, qd0 = self.first_joint(ep)
        xy, v0 = self.first_root(ep)
        first = np.zeros((n, self.F), F32)
        f(first, "joint_pos")[:], f(first, "joint_vel")[:] = q0, qd0
        f(first, "root_pos_w")[:, 0:2] = xy
        x = f(first, "servo")
        x[:, 0:3], x[:, 9:13], x[:, 13] = v0, F32(1), f(start, "servo")[:, 13]
        start = np.where(rst[:, None], first, start).astype(F32)          # everything else of a first state is zero
        self._raw_slab = start.copy()
        # ---- the push of this step, on the state the step starts from
        pushed, pv, kick = self.push(ep, t)
        x = f(start, "servo")
        x[:, 0:3] = np.where(pushed[:, None], pv, x[:, 0:3])
        x[:, 3:5] = np.where(pushed[:, None], x[:, 3:5] + kick, x[:, 3:5])
        self.pushed = pushed
        # ---- traction: one more rounded multiply on the three velocity rows
        m = self.traction()
        self.G = np.stack([(self.G0[k][None, :] * m[:, None]).astype(F32) if k < 3 else np.tile(self.G0[k], (n, 1))
                           for k in range(5)])
        slot = self.record[:, 0].astype(np.int64)
        out = self._base().step(self, start, action, np.zeros(n, bool), t)
        # ---- what the parents cannot know
        ends = (t + 1 >= self.max_len) | (f(out, "hard_reset")[:, 0] > 0)
        ep_out = f(out, "servo")[:, 13].astype(np.uint32)
        obs, xo, x0 = f(out, "obs"), f(out, "servo"), f(self._raw_slab, "servo")
        nqd0 = self.first_joint(ep_out)[1]
        nwz0 = self.first_root(ep_out)[1][:, 2]
        for k in range(2):
            obs[:, k] = np.where(ends, F32(0), (xo[:, 3 + k] - x0[:, 3 + k]) / self.step_dt)
        obs[:, 2] = np.where(ends, nwz0, obs[:, 2])
        obs[:, 21:33] = np.where(ends[:, None], nqd0, obs[:, 21:33])
        if self.trace is not None and self.flags & PUSH:
            for i in range(self.K):
                if 0 <= slot[i] < self.T:
                    self.trace[slot[i], i, TRACE_PUSHED] = F32(pushed[i])
        return self._finish(out, *self.key_of(out, t))


def make_twin(cfg, n, events, obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=12, **kw):
    return ServoEventsTwin(n, OT.RAW, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, env_offset,
                           table=table, obs_table=obs_table, events=events, **kw)


def run_events_twin(twin, actions, episode_length0, switch=None):
    """(slabs [steps + 1, N, F], push masks [steps, N]); ``switch`` = (step index, words): the block is replaced before
    that step"""
    ep_len = np.asarray(episode_length0, np.int64).copy()
    slab = twin.initial(ep_len)
    reset = np.zeros(twin.N, bool)
    slabs, masks = [slab], []
    for s, a in enumerate(actions):
        if switch is not None and s == switch[0]:
            twin.set_events(switch[1])
        slab = twin.step(slab, a, reset, ep_len)
        masks.append(twin.pushed.copy())
        ep_len += 1
        reset = (ep_len >= twin.max_len) | (twin._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    return np.stack(slabs), np.stack(masks) if masks else np.zeros((0, twin.N), bool)
