"""Numpy twin of the servo surrogate's pinned plants (csrc/servo_sim_kernel.h: the plant-on instances of servo_sim_plant.hip,
include/catppo.h catppo_servo_plant; DESIGN section 9, "Robustness").

The pins stand where the lag draw and the randomisation block's draws left their values, so ``_PlantLoop`` subclasses
``servo_randomize_twin._RandomizeLoop`` and restates nothing of its step: it overrides ``robot`` and ``lag``, calls the parent's
and replaces, per env, the quantities whose bit is set in word 0 of the env's row.  It is listed last among the bases of the
twins below, so that it lies right before ``_RandomizeLoop`` in their method resolution order and every parent runs as it is.
With a history the pinned twin is the inner twin of ``servo_history_twin.ServoHistoryTwin``, which adds no arithmetic.  None of
the parents is edited.

The table is the [N, 8] fp32 words the device reads (``table(...)`` below builds them; the tests compare the layout with
``native.SERVO_PLANT_WORDS``).  One ``np.float32`` operation per rounded kernel operation.  Test infrastructure only.
"""
from __future__ import annotations

import numpy as np

import servo_actions_twin as AT
import servo_actuators_twin as UT
import servo_obs_twin as OT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T

F32 = np.float32
FLOATS = 8
KP, KD, FRICTION, ARMATURE, MASS, LAG = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
BITS = {"kp_scale": KP, "kd_scale": KD, "friction": FRICTION, "armature": ARMATURE, "mass_scale": MASS, "lag": LAG}
#: the word of a row that holds the quantity, restated here
WORDS = {"bits": 0, "kp_scale": 1, "kd_scale": 2, "friction": 3, "armature": 4, "mass_scale": 5, "lag": 6}
QUANTITIES = tuple(BITS)


def table(n, **pins):
    """the [n, 8] words: ``pins`` maps a quantity to a scalar or to [n] values; NaN in an array leaves that env unpinned"""
    t = np.zeros((n, FLOATS), F32)
    ints = t.view(np.int32)
    for name, v in pins.items():
        v = np.broadcast_to(np.asarray(v, np.float64), (n,))
        on = ~np.isnan(v)
        ints[on, 0] |= BITS[name]
        if name == "lag":
            ints[on, WORDS[name]] = v[on].astype(np.int32)
        else:
            t[on, WORDS[name]] = v[on].astype(F32)
    return t


def mixed_table(n, decimation=4, seed=5):
    """every row another plant, all six bits mixed: the row's bits are drawn, its values lie well inside the stable range of
    the mixed robot; row 0 pins nothing and row 1 everything when there are that many"""
    r = np.random.RandomState(seed)
    bits = r.randint(0, 64, n)
    bits[:1] = 0
    bits[1:2] = 63
    t = np.zeros((n, FLOATS), F32)
    ints = t.view(np.int32)
    ints[:, 0] = bits
    t[:, 1], t[:, 2] = r.uniform(0.6, 1.4, n), r.uniform(0.5, 1.5, n)
    t[:, 3], t[:, 4] = r.uniform(0.0, 0.4, n), r.uniform(0.0, 0.02, n)
    t[:, 5] = r.uniform(0.3, 1.6, n)                                          # below one half the velocity-lag gain is capped
    ints[:, 6] = r.randint(0, 3 * decimation + 1, n)
    return t


class _PlantLoop(ZT._RandomizeLoop):
    """``_RandomizeLoop`` with the pinned quantities of every env's row in the place of the drawn ones"""

    def set_plant(self, words):
        t = np.zeros((self.N, FLOATS), F32) if words is None else np.ascontiguousarray(words, F32).copy()
        assert t.shape == (self.N, FLOATS)
        self.plant = t

    def _pinned(self, name):
        return (self.plant.view(np.int32)[:, 0] & BITS[name]) != 0

    def robot(self, ep):
        rb = super().robot(ep)
        n, t, w, p = self.N, self.plant, self.rnd, self.p
        col = lambda name: t[:, WORDS[name]][:, None]                         # noqa: E731
        tile = lambda x: np.tile(np.asarray(x, F32), (n, 1))                  # noqa: E731
        on = lambda name: self._pinned(name)[:, None]                         # noqa: E731
        kp = np.where(on("kp_scale"), tile(self.u_kp) * col("kp_scale"), rb["kp"]).astype(F32)
        kd = np.where(on("kd_scale"), tile(self.u_kd) * col("kd_scale"), rb["kd"]).astype(F32)
        fr = np.where(on("friction"), np.broadcast_to(col("friction"), (n, T.J)), rb["fr"]).astype(F32)
        inertia = np.where(on("armature"), np.broadcast_to(w[ZT.WORDS["servo_inertia"]] + col("armature"), (n, T.J)),
                           rb["inertia"]).astype(F32)
        df = np.where(on("friction") | on("armature"), ((fr / inertia) * self.dt).astype(F32), rb["df"]).astype(F32)
        m0 = w[ZT.WORDS["m0"]]
        with np.errstate(divide="ignore", invalid="ignore"):                  # an unpinned row may hold anything
            m = (m0 * t[:, WORDS["mass_scale"]]).astype(F32)
            weight = (m * w[ZT.WORDS["g"]]).astype(F32)
            rho = (m / m0).astype(F32)
            av = np.minimum(p["vel_alpha"] / rho, F32(1)).astype(F32)
        pm = self._pinned("mass_scale")
        rb.update(kp=kp, kd=kd, fr=fr, inertia=inertia, df=df, weight=np.where(pm, weight, rb["weight"]).astype(F32),
                  av=np.where(pm, av, rb["av"]).astype(F32), m=np.where(pm, m, rb["m"]).astype(F32),
                  rho=np.where(pm, rho, rb["rho"]).astype(F32))
        return rb

    def lag(self, ep):
        L = super().lag(ep)
        word = self.plant.view(np.uint32)[:, WORDS["lag"]].astype(np.int64)
        return np.where(self._pinned("lag")[:, None], np.minimum(word, 255)[:, None], L)


class _Plant:
    """the top of the chain: the table (None: all zero, which pins nothing)"""

    def __init__(self, *args, plant=None, **kw):
        super().__init__(*args, **kw)
        self.set_plant(plant)


class ServoPlantTwin(_Plant, ZT._Randomize, UT._Actuators, AT._Actions, RT.ServoRewardTwin, _PlantLoop):
    """pinned plants (behind the randomisation block) on the simulator without further descriptors"""


class ServoPlantTerminationsTwin(_Plant, ZT._Randomize, UT._Actuators, AT._Actions, TT.ServoTerminationsTwin, _PlantLoop):
    """pinned plants on top of the whole chain: observations, events, commands, terminations, actions, actuators, randomisation"""


class ServoPlantTerminationsPlainTwin(_Plant, ZT._Randomize, UT._Actuators, AT._Actions, TT.ServoTerminationsPlainTwin, _PlantLoop):
    """... without a command block"""


def make_twin(cfg, n, plant=None, randomize=None, actuators=None, actions=None, width=T.J, terminations=None, commands=None,
              events=None, obs_table=None, table=(), env_offset=0, seed=RT.SEED, max_len=25, obs_dim=None, **kw):
    """as ``servo_randomize_twin.make_twin``, with the plant table (None: all zero)"""
    params = T.params_from_cfg(cfg.synthetic)
    if terminations is None:
        assert commands is None and events is None and obs_table is None
        d = int(cfg.synthetic.obs_dim if obs_dim is None else obs_dim)
        return ServoPlantTwin(n, d, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset, table=table, actions=actions,
                              width=width, actuators=actuators, randomize=randomize, plant=plant, **kw)
    args = (n, OT.RAW, params, seed, max_len, cfg.sim.dt, cfg.decimation, env_offset)
    if commands is None:
        return ServoPlantTerminationsPlainTwin(*args, table=table, obs_table=obs_table, events=events, terminations=terminations,
                                               actions=actions, width=width, actuators=actuators, randomize=randomize,
                                               plant=plant, **kw)
    return ServoPlantTerminationsTwin(*args, table=table, obs_table=obs_table, events=events, commands=commands,
                                      terminations=terminations, actions=actions, width=width, actuators=actuators,
                                      randomize=randomize, plant=plant, **kw)


#: the bookkeeping around the twin is ``servo_randomize_twin.run_randomize_twin``'s (``servo_history_twin.run_history_twin``'s
#: around a history wrapper)
run_plant_twin = ZT.run_randomize_twin
