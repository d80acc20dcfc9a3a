"""The servo task's pinned plants without a device ("Robustness"): the descriptor, and properties of the numpy
twin - that a table with no bit set is the randomise twin bit for bit; that a table which pins the same plant in every env is
the existing randomise twin, which knows nothing of pins, run with zero-width ranges at the same values (all six quantities
together and each alone); every refusal of the table's writer and of ``plant_grid`` / ``sweep``; and ``by_plant()`` /
``robustness()`` on a hand-made record."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_plant_twin as PT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_randomize_twin as ZC
import test_servo_terminations_twin as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
STEPS, MAX_LEN = ZC.STEPS, ZC.MAX_LEN
#: the plant every env is pinned to in the cross-check: values that are no round fp32 numbers, inside the stable range
PINNED = dict(kp_scale=0.83, kd_scale=1.27, friction=0.11, armature=0.0043, mass_scale=1.31, lag=6)


def zero_width_reference(only=None):
    """(block, actuator entries) of the existing randomise twin that computes the plant ``PINNED`` (``only``: that quantity
    alone) in every env: zero-width ranges at the pinned values, operations scale, scale, abs, abs, scale on every joint, and
    an actuator table whose every group has min_delay == max_delay == the pinned lag"""
    on = lambda q: only in (None, q)                                          # noqa: E731
    same = lambda q: (PINNED[q], PINNED[q]) if on(q) else None                # noqa: E731
    words = ZT.block(ZC.params(), stiffness=same("kp_scale"), damping=same("kd_scale"), friction=same("friction"),
                     armature=same("armature"), mass=same("mass_scale"), gains_op="scale", joint_op="abs", mass_op="scale",
                     armatures=[0.001 * (1 + j % 3) for j in range(12)])
    robot = UC.mixed_entries()
    if on("lag"):
        robot = [dict(e, min_delay=PINNED["lag"], max_delay=PINNED["lag"]) for e in robot]
    return words, robot


def pinned_table(n, only=None):
    return PT.table(n, **{q: v for q, v in PINNED.items() if only in (None, q)})


def _run(make, n=17, **kw):
    acts, ep0 = AC.recipe(n, 12)
    tw = make(TC.env_cfg(TC.LIVE_TILT_MAX), n, max_len=MAX_LEN, table=RT.ALL_NON_EXP, trace_envs=5, trace_capacity=STEPS, **kw)
    return tw, ZT.run_randomize_twin(tw, acts, ep0)


def _same(a, b):
    (ta, sa), (tb, sb) = a, b
    np.testing.assert_array_equal(sa.view(U32), sb.view(U32))
    for name in ("record", "trace", "reward_record"):
        np.testing.assert_array_equal(getattr(ta, name).view(U32), getattr(tb, name).view(U32), err_msg=name)


# ------------------------------------------------------------------------------------------ (c) descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoPlant._fields_] == ["table", "reserved"]
    assert ctypes.sizeof(native.ServoPlant) == 16 and native.ServoPlant.reserved.offset == 8
    assert issubclass(native.ServoSimPlant, native.ServoSimHistory) and ctypes.sizeof(native.ServoSimHistory) == 504
    assert native.ServoSimPlant.plant.offset == ctypes.sizeof(native.ServoSimHistory) and ctypes.sizeof(native.ServoSimPlant) == 520
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_plant, hist\) == (\d+) && offsetof\(catppo_servo_sim_plant, plant\) == (\d+) &&\s*"
                  r"sizeof\(catppo_servo_plant\) == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [488, 504, 16]
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_PLANT (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_PLANT
    assert native.SERVO_EXT_PLANT == int.from_bytes(b"PLN1", "big")
    assert int(re.search(r"#define CATPPO_SERVO_PLANT_FLOATS (\d+)", src).group(1)) == native.SERVO_PLANT_FLOATS == PT.FLOATS == 8
    for name, q in (("KP", "kp_scale"), ("KD", "kd_scale"), ("FRICTION", "friction"), ("ARMATURE", "armature"),
                    ("MASS", "mass_scale"), ("LAG", "lag")):
        value = int(re.search(rf"#define CATPPO_SERVO_PLANT_{name} (0x[0-9A-Fa-f]+)u", src).group(1), 16)
        assert value == native.SERVO_PLANT_BITS[q] == PT.BITS[q] == getattr(PT, name), name
    assert native.SERVO_PLANT_WORDS == PT.WORDS
    # the ninth level, behind the history level; no new export
    assert len(native.SERVO_EXTS) == 9 and native.SERVO_EXTS[8][1:3] == (native.SERVO_EXT_PLANT, native.ServoSimPlant)
    assert native.SERVO_EXTS[7][2] is native.ServoSimHistory and len({e[1] for e in native.SERVO_EXTS}) == 9
    assert len(native.EXPORTS) == 59
    from cat_envs.tasks.utils.mdp import randomization as RZ
    assert RZ.PLANT_BITS == native.SERVO_PLANT_BITS and RZ.PLANT_FLOATS == 8
    assert {q: w for q, w in native.SERVO_PLANT_WORDS.items() if q != "bits"} == RZ.PLANT_WORDS


def test_servo_sim_step_refuses_a_descriptor_without_the_plant_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs(), native.ServoSimRandomize(), native.ServoSimHistory()):
        short.reserved = native.SERVO_EXT_PLANT
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimPlant"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


def test_every_instance_of_the_new_packs_is_reachable_and_none_is_a_training_instance():
    csrc = os.path.join(ROOT, "constraints-as-terminations_amd", "csrc")
    src = open(os.path.join(csrc, "servo_sim_plant.hip")).read()
    calls = re.findall(r"launch\(mode, rew, nblk, lds_bytes, st, d, ([^)]*)\); \},\s*([^)]*)\);", src)
    assert calls == [("*x.obs, opt..., *x.ac, *x.au, *x.rn, *x.hs, *x.pl", "x.ev, x.cm, x.tm"),
                     ("opt..., *x.ac, *x.au, *x.rn, *x.pl", "x.obs, x.ev, x.cm, x.tm")]
    assert len(re.findall(r"\blaunch\(", src)) == 2
    for unit in ("servo_sim.hip", "servo_sim_actions.hip", "servo_sim_actuators.hip", "servo_sim_randomize.hip", "servo_sim_history.hip"):
        assert "x.pl" not in open(os.path.join(csrc, unit)).read().replace("if (x.pl) catppo_internal_servo_sim_launch_plant", "")
    kernel = open(os.path.join(csrc, "servo_sim_kernel.h")).read()
    assert "static_assert((kRnd && kMode == kStepResponse) || !kPlant" in kernel


# ------------------------------------------------------------------------------------------ (a) nothing pinned
@pytest.mark.parametrize("which", ["none", "zeros", "values but no bit"])
def test_an_all_clear_table_is_the_randomise_twin(which):
    n = 17
    loud = PT.mixed_table(n)
    loud.view(np.int32)[:, 0] = 0
    plant = {"none": None, "zeros": np.zeros((n, 8), F32), "values but no bit": loud}[which]
    kw = dict(randomize=ZC.recipe_block(), actuators=UC.mixed_entries())
    pinned = _run(PT.make_twin, plant=plant, **kw)
    parent = _run(ZT.make_twin, **kw)
    assert pinned[0].F == parent[0].F and pinned[0].off == parent[0].off     # the row gets no new state
    _same(pinned, parent)


# ------------------------------------------------------------------------------------------ (b) against the twin without pins
@pytest.mark.parametrize("only,block", [(None, "off"), (None, "recipe"), *((q, "off") for q in PT.QUANTITIES)])
def test_a_pinned_plant_is_the_randomise_twin_at_zero_width_ranges(only, block):
    """the pins ignore the block: all six pinned on top of the recipe's draws and on top of a switched-off block alike.  With
    one quantity alone the reference draws nothing else, so the block under the pin is switched off there"""
    n = 17
    words, robot = zero_width_reference(only)
    under = ZC.recipe_block(enabled=block == "recipe")
    under[ZT.WORDS["armatures"]:] = words[ZT.WORDS["armatures"]:]
    pinned = _run(PT.make_twin, plant=pinned_table(n, only), randomize=under, actuators=UC.mixed_entries())
    ref = _run(ZT.make_twin, randomize=words, actuators=robot)
    _same(pinned, ref)
    nominal = _run(ZT.make_twin, randomize=ZC.recipe_block(enabled=False), actuators=UC.mixed_entries())
    assert (pinned[1] != nominal[1]).any(), "the pin changes the run"


def test_every_row_its_own_plant():
    n = 17
    t = PT.mixed_table(n)
    bits = t.view(np.int32)[:, 0]
    assert bits[0] == 0 and bits[1] == 63 and len({r.tobytes() for r in t}) == n
    from cat_envs.tasks.utils.mdp import randomization as RZ
    RZ.check_plant_table(t, 4, TC.env_cfg().sim.dt, UC.mixed_entries(), ZC.params()["inertia"])
    kw = dict(randomize=ZC.recipe_block(), actuators=UC.mixed_entries())
    tw, slabs = _run(PT.make_twin, plant=t, **kw)
    parent = _run(ZT.make_twin, **kw)[1]
    # an env that pins nothing is the parent's env; one that pins everything is not
    np.testing.assert_array_equal(slabs[:, 0].view(U32), parent[:, 0].view(U32))
    assert (slabs[:, 1] != parent[:, 1]).any()
    # the velocity-lag gain is capped in some pinned envs and not in others, the lags reach different slots
    mass = (bits & PT.MASS) != 0
    assert (t[mass, 5] < 0.5).any() and (t[mass, 5] > 0.5).any()
    lag = t.view(np.int32)[(bits & PT.LAG) != 0, 6]
    assert lag.min() <= 8 < lag.max()                                        # two and three control steps back


# ------------------------------------------------------------------------------------------ (d) the writers' refusals
def test_the_tables_writer_names_the_row_and_the_quantity():
    from cat_envs.tasks.utils.mdp import randomization as RZ
    entries, si, dt = UC.mixed_entries(), float(ZC.params()["inertia"]), TC.env_cfg().sim.dt
    ok = PT.mixed_table(5)
    RZ.check_plant_table(ok, 4, dt, entries, si)

    def edit(row, word, value, as_int=False, bits=None):
        t = ok.copy()
        (t.view(np.int32) if as_int else t)[row, word] = value
        if bits is not None:
            t.view(np.int32)[row, 0] = bits
        return t
    W = PT.WORDS
    for bad, what in ((edit(3, 0, 0x40, True), r"row 3: pin bits 0x40 has unknown bits"),
                      (edit(2, W["kp_scale"], float("nan")), r"row 2: kp_scale must be finite"),
                      (edit(0, W["armature"], float("inf")), r"row 0: armature must be finite"),
                      (edit(1, W["kp_scale"], -0.5, bits=63), r"row 1: kp_scale must be >= 0, got -0.5"),
                      (edit(1, W["kd_scale"], -1.0, bits=63), r"row 1: kd_scale must be >= 0"),
                      (edit(4, W["friction"], -0.1, bits=PT.FRICTION), r"row 4: friction must be >= 0"),
                      (edit(4, W["armature"], -0.001, bits=PT.ARMATURE), r"row 4: armature must be >= 0"),
                      (edit(2, W["mass_scale"], 0.0, bits=PT.MASS), r"row 2: mass_scale must be > 0, got 0"),
                      (edit(2, W["lag"], 13, True), r"row 2: lag must be in 0 \.\. 12 physics steps"),
                      (edit(2, W["lag"], -1, True), r"row 2: lag must be in 0 \.\. 12"),
                      (edit(3, 7, 1, True), r"row 3: the spare word 7 must be zero"),
                      (edit(1, W["kd_scale"], 300.0, bits=PT.KD), r"row 1: joint 0 is unstable at the pinned plant .* 2 a \+ b"),
                      (ok[:, :7], r"8 words per row")):
        with pytest.raises(ValueError, match=what):
            RZ.check_plant_table(bad, 4, dt, entries, si)
    # a value behind a clear bit is not read: only its finiteness is asked for
    RZ.check_plant_table(edit(1, W["kp_scale"], -0.5, bits=PT.LAG), 4, dt, entries, si)
    # the stability condition is check_corners' own: 2 a + b < 4 at the pinned kp', kd', inertia'
    kd, inertia = F32(entries[0]["kd"]), F32(entries[0]["inertia"])
    edge = 2.0 * float(inertia) / (float(kd) * dt)                             # 2 a = 4 at this scale (b > 0 is on top)
    RZ.check_plant_table(edit(1, W["kd_scale"], 0.5 * edge, bits=PT.KD), 4, dt, entries, si)
    with pytest.raises(ValueError, match="unstable"):
        RZ.check_plant_table(edit(1, W["kd_scale"], edge, bits=PT.KD), 4, dt, entries, si)
    with pytest.raises(ValueError, match="unstable"):                          # a small pinned inertia under the nominal gains
        RZ.check_plant_table(PT.table(2, armature=0.0), 4, dt, [dict(kp=400.0, kd=8.0, inertia=1.0)] * 12, 0.001)


def test_plant_grid_and_sweep():
    from cat_envs.tasks.utils.cleanrl import evaluate as E
    g = E.plant_grid(kp_scale=(0.8, 1.2, 3), mass_scale=1.3, lag=(0, 8, 3), num_envs=11)
    assert sorted(g) == ["kp_scale", "lag", "mass_scale", "packed"] and g["packed"].shape == (11, 8) and g["packed"].dtype == F32
    np.testing.assert_array_equal(g["kp_scale"], np.repeat([0.8, 1.0, 1.2], 3)[np.arange(11) % 9])
    np.testing.assert_array_equal(g["lag"], np.tile([0.0, 4.0, 8.0], 3)[np.arange(11) % 9])
    ints = g["packed"].view(np.int32)
    assert (ints[:, 0] == (PT.KP | PT.MASS | PT.LAG)).all() and (ints[:, 6] == g["lag"]).all() and not ints[:, 7].any()
    np.testing.assert_array_equal(g["packed"][:, 1], g["kp_scale"].astype(F32))
    assert (g["packed"][:, 5] == F32(1.3)).all() and not g["packed"][:, [2, 3, 4]].any()
    np.testing.assert_array_equal(g["packed"].view(U32), PT.table(11, kp_scale=g["kp_scale"], mass_scale=1.3, lag=g["lag"]).view(U32))
    assert E.plant_grid(friction=(0.0, 0.4, 1))["friction"].tolist() == [0.2]   # n = 1 is the midpoint
    for kw, what in ((dict(), "at least one quantity"), (dict(kp_scale=(1.0, 2.0)), r"kp_scale is None, a scalar or \(lo, hi, n\)"),
                     (dict(lag=(0, 4, 0)), "the axis lag needs at least one point"), (dict(armature=float("nan")), "armature must be finite"),
                     (dict(kd_scale=1.0, num_envs=0), "num_envs must be at least 1")):
        with pytest.raises(ValueError, match=what):
            E.plant_grid(**kw)
    with pytest.raises(ValueError, match="unknown plant quantities"):
        E.pack_plant({"stiffness": [1.0]})
    # the command line's words: name=value or name=lo:hi:n
    assert E.parse_plant_axes(["kp_scale=0.8:1.2:3", "lag=4"]) == {"kp_scale": (0.8, 1.2, 3), "lag": 4.0}
    for words, what in ((["stiffness=1"], "takes name=value or name=lo:hi:n"), (["lag=1:2"], "takes name=value"),
                        (["lag=1", "lag=2"], "at most once"), (["lag=soon"], "holds no numbers")):
        with pytest.raises(ValueError, match=what):
            E.parse_plant_axes(words)
    # sweep: env i gets command i % C and plant i // C
    cmds = E.command_grid(vx=(0.0, 1.0, 2), vy=(-0.5, 0.5, 2), wz=(0.0, 0.0, 1), num_envs=4)[0]
    plants = E.plant_grid(kd_scale=(0.5, 1.5, 3), num_envs=3)
    c, p = E.sweep(cmds, plants)
    assert c.shape == (12, 3) and p["packed"].shape == (12, 8) and p["kd_scale"].shape == (12,)
    for i in range(12):
        np.testing.assert_array_equal(c[i], cmds[i % 4])
        np.testing.assert_array_equal(p["packed"][i].view(U32), plants["packed"][i // 4].view(U32))
        assert p["kd_scale"][i] == plants["kd_scale"][i // 4]
    c2, p2 = E.sweep(cmds, plants["packed"])
    np.testing.assert_array_equal(p2.view(U32), p["packed"].view(U32))
    for args, what in (((cmds[:, :2], plants), r"commands are \[C, 3\]"), ((cmds, np.zeros((3, 7), F32)), r"\[P, 8\]"),
                       ((cmds, np.zeros((0, 8), F32)), "at least one row")):
        with pytest.raises(ValueError, match=what):
            E.sweep(*args)


# ------------------------------------------------------------------------------------------ (e) reading a result
def test_by_plant_and_robustness_on_a_hand_made_record():
    import json
    from cat_envs.tasks.utils.cleanrl import evaluate as E
    # six envs, three plants (kp 0.8 lag 0 | kp 0.8 lag 8 | kp 1.2 lag 8), in the order b a b c a c; ten steps each
    order = [1, 0, 1, 2, 0, 2]
    rows = PT.table(3, kp_scale=[0.8, 0.8, 1.2], lag=[0, 8, 8])[order]
    reward = np.array([2.0, 10.0, 4.0, 5.0, 8.0, 7.0])                          # group sums: a 18, b 6, c 12
    rec = np.zeros((6, 12), F32)
    f = {k: i for i, k in enumerate(E.FIELDS)}
    rec[:, f["steps"]], rec[:, f["reward"]] = 10, reward
    rec[:, f["episodes"]], rec[:, f["falls"]] = 1, [1, 0, 1, 0, 0, 0]
    res = E.EvalResult(per_env=rec, plant=rows)
    res.metrics = res._aggregate()
    groups = res.by_plant()
    kp = float(F32(0.8))
    assert [g["plant"] for g in groups] == [{"kp_scale": kp, "lag": 8}, {"kp_scale": kp, "lag": 0}, {"kp_scale": float(F32(1.2)), "lag": 8}]
    assert [g["envs"] for g in groups] == [2, 2, 2]
    assert [g["metrics"]["reward_per_step"] for g in groups] == [0.3, 0.9, 0.6]
    assert [g["metrics"]["fall_rate"] for g in groups] == [1.0, 0.0, 0.0]
    assert set(groups[0]) == {"plant", "envs", "metrics"} and set(groups[0]["metrics"]) == set(res.by_command()[0]["metrics"])
    rb = res.robustness()
    assert rb["metric"] == "reward_per_step" and rb["groups"] == 3
    assert rb["by_quantity"]["kp_scale"] == [{"value": kp, "groups": 2, "reward_per_step": (0.3 + 0.9) / 2},
                                             {"value": float(F32(1.2)), "groups": 1, "reward_per_step": 0.6}]
    assert rb["by_quantity"]["lag"] == [{"value": 0, "groups": 1, "reward_per_step": 0.9},
                                        {"value": 8, "groups": 2, "reward_per_step": (0.3 + 0.6) / 2}]
    assert rb["best"] == {"plant": {"kp_scale": kp, "lag": 0}, "envs": 2, "reward_per_step": 0.9}
    assert rb["worst"] == {"plant": {"kp_scale": kp, "lag": 8}, "envs": 2, "reward_per_step": 0.3}
    assert rb["spread"] == 0.9 - 0.3
    falls = res.robustness("fall_rate")
    assert falls["best"]["fall_rate"] == 1.0 and falls["worst"]["fall_rate"] == 0.0 and falls["spread"] == 1.0
    d = json.loads(res.to_json())
    assert d["by_plant"] == json.loads(json.dumps(groups)) and d["robustness"] == json.loads(json.dumps(rb))
    # without a table: one group, and robustness has nothing to say
    plain = E.EvalResult(per_env=rec)
    plain.metrics = plain._aggregate()
    assert plain.by_plant() == [{"plant": None, "envs": 6, "metrics": plain.metrics}]
    assert "by_plant" not in json.loads(plain.to_json()) and "robustness" not in json.loads(plain.to_json())
    with pytest.raises(ValueError, match="needs a plant table"):
        plain.robustness()
