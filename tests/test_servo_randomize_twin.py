"""The servo task's randomisation block without a device ("Randomisation"): the descriptor, and properties of
the numpy twin - that a block with no quantity on, or with the switch off, is the actuator twin bit for bit, alone and with all
six blocks; that startup draws hold for the whole run of an env and reset draws change with the episode; that unselected
joints keep the table's value and every sample lies in its range; and that in the recipe the device test compares every
operation occurs, joints stick and slip, the velocity-lag gain is capped in some envs and not in others, the torque clamp is
reached and not reached and every env begins at least two episodes, which is what keeps that comparison from being vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_actuators_twin as UT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import servo_twin as T
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
STEPS, MAX_LEN = CC.STEPS, CC.MAX_LEN
GAINS_MASK = 0xFFF & ~(0b111 << 6)                 # every joint but HL_* (the DC motors keep the table's gains)
JOINT_MASK = 0xFFF & ~0b1                          # every joint but FL_HAA
HL, FL_HAA = [6, 7, 8], 0


def params():
    return T.params_from_cfg(TC.env_cfg().synthetic)


def recipe_block(enabled=True, only=None, reset=None):
    """the liveness block: gains scaled once per env on every joint but HL_*, friction 0 .. 0.3 N m and an absolute armature of
    0 .. 0.01 per episode on every joint but FL_HAA, -2 .. +1 kg on the base's 2.55 kg per episode (below half the nominal mass
    the velocity-lag gain is capped at 1).  ``only``: that term alone; ``reset``: every term in that mode"""
    kw = {}
    if only in (None, "gains"):
        kw.update(stiffness=(0.7, 1.3), damping=(0.5, 1.5), gains_op="scale", gains_mask=GAINS_MASK,
                  gains_reset=False if reset is None else reset)
    if only in (None, "joint"):
        kw.update(friction=(0.0, 0.3), armature=(0.0, 0.01), joint_op="abs", joint_mask=JOINT_MASK,
                  joint_reset=True if reset is None else reset)
    if only in (None, "mass"):
        kw.update(mass=(-2.0, 1.0), mass_op="add", mass_reset=True if reset is None else reset)
    return ZT.block(params(), enabled=enabled, armatures=[0.001 * (1 + j % 3) for j in range(12)], **kw)


def run_recipe(n=17, words=None, **kw):
    """(twin, slabs, stats [steps, N, 12] per key) of the recipe: 60 steps of N(0, 1) actions, episodes of 25 steps, the mixed
    robot of test_servo_actuators_twin.py"""
    acts, ep0 = CC.recipe(n)
    tw = ZT.make_twin(TC.env_cfg(), n, randomize=recipe_block() if words is None else words, actuators=UC.mixed_entries(),
                      max_len=MAX_LEN, **kw)
    slabs = ZT.run_randomize_twin(tw, acts, ep0)
    return tw, slabs, {k: np.stack([s[k] for s in tw.live_steps]) for k in tw.live_steps[0]}


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoRandomize._fields_] == ["block", "reserved"]
    assert ctypes.sizeof(native.ServoRandomize) == 16 and native.ServoRandomize.reserved.offset == 8
    assert issubclass(native.ServoSimRandomize, native.ServoSimActuators) and ctypes.sizeof(native.ServoSimActuators) == 472
    assert native.ServoSimRandomize.rnd.offset == 472 and ctypes.sizeof(native.ServoSimRandomize) == 488
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_randomize, actu\) == (\d+) && offsetof\(catppo_servo_sim_randomize, rnd\) == (\d+) &&\s*"
                  r"sizeof\(catppo_servo_randomize\) == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [456, 472, 16]
    assert int(re.search(r"sizeof\(catppo_servo_sim_randomize\) == (\d+)", hip).group(1)) == 488
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_RANDOMIZE (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_RANDOMIZE
    assert native.SERVO_EXT_RANDOMIZE == int.from_bytes(b"RND1", "big")
    assert native.SERVO_EXT_RANDOMIZE not in (0, native.SERVO_EXT_OBS, native.SERVO_EXT_EVENTS, native.SERVO_EXT_COMMANDS,
                                              native.SERVO_EXT_TERMINATIONS, native.SERVO_EXT_ACTIONS, native.SERVO_EXT_ACTUATORS)
    assert int(re.search(r"#define CATPPO_SERVO_RANDOMIZE_FLOATS (\d+)", src).group(1)) == native.SERVO_RANDOMIZE_FLOATS == ZT.FLOATS
    for name, bit in (("ENABLE", "enable"), ("KP", "stiffness"), ("KD", "damping"), ("FRICTION", "friction"), ("ARMATURE", "armature"),
                      ("MASS", "mass"), ("GAINS_RESET", "gains_reset"), ("JOINT_RESET", "joint_reset"), ("MASS_RESET", "mass_reset")):
        value = int(re.search(rf"#define CATPPO_SERVO_RANDOMIZE_{name} (0x[0-9A-Fa-f]+)u", src).group(1), 16)
        assert value == native.SERVO_RANDOMIZE_FLAGS[bit] == getattr(ZT, name), name
    assert native.SERVO_RANDOMIZE_WORDS == ZT.WORDS and native.SERVO_RANDOMIZE_OPS == ZT.OPS
    kernel = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_kernel.h")).read()
    tags = re.search(r"kTagGains = (0x[0-9A-Fa-f]+)u, kTagJointPar = (0x[0-9A-Fa-f]+)u, kTagMass = (0x[0-9A-Fa-f]+)u", kernel)
    assert [int(x, 16) for x in tags.groups()] == [ZT.TAG_GAINS, ZT.TAG_JOINT, ZT.TAG_MASS] == \
        [int.from_bytes(t, "big") for t in (b"AGAN", b"JPAR", b"MASS")]
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_descriptor_without_the_randomisation_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs(), native.ServoSimEvents(), native.ServoSimCommands(),
                  native.ServoSimTerminations(), native.ServoSimActions(), native.ServoSimActuators()):
        short.reserved = native.SERVO_EXT_RANDOMIZE
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimRandomize"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


def test_every_instance_of_the_new_packs_is_reachable():
    """16 packs end with the action, actuator and randomisation descriptors; the one launch of servo_sim_randomize.hip reaches each of them:
    with_present hands it whichever of the four optional descriptors are there, in the pack's order (all 16 combinations:
    tests/test_servo_sim_host.py), and the unit's own descriptors follow them"""
    src = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_randomize.hip")).read()
    calls = re.findall(r"with_present\(\[&\]\(const auto&\.\.\. opt\) \{ launch\(mode, rew, nblk, lds_bytes, st, d, ([^)]*)\); \},\s*([^)]*)\);", src)
    assert calls == [("opt..., *x.ac, *x.au, *x.rn", "x.obs, x.ev, x.cm, x.tm")]
    assert len(re.findall(r"\blaunch\(", src)) == 1                          # and nothing else launches here


# ------------------------------------------------------------------------------------------ the twin
def _off_blocks():
    """blocks that must change nothing: all zero, the switch alone, every range set but no quantity bit, the recipe's block
    with the switch off"""
    none = recipe_block()
    none.view(np.int32)[ZT.WORDS["flags"]] = ZT.ENABLE | ZT.GAINS_RESET | ZT.JOINT_RESET | ZT.MASS_RESET
    return {"zero": None, "switch alone": ZT.block(params()), "no quantity": none, "switch off": recipe_block(enabled=False)}


@pytest.mark.parametrize("which", ["zero", "switch alone", "no quantity", "switch off"])
def test_nothing_on_is_the_actuator_twin_alone(which):
    n = 17
    acts, ep0 = AC.recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    kw = dict(max_len=MAX_LEN, table=RT.ALL_NON_EXP, trace_envs=5, trace_capacity=STEPS + 3, actuators=UC.mixed_entries())
    tw = ZT.make_twin(cfg, n, randomize=_off_blocks()[which], **kw)
    parent = UT.make_twin(cfg, n, **kw)
    assert tw.F == parent.F and tw.off == parent.off                          # the row does not grow
    got = ZT.run_randomize_twin(tw, acts, ep0)
    np.testing.assert_array_equal(got.view(U32), UT.run_actuators_twin(parent, acts, ep0).view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.record.view(U32), parent.record.view(U32))
    np.testing.assert_array_equal(tw.trace.view(U32), parent.trace.view(U32))


@pytest.mark.parametrize("which", ["zero", "switch off"])
def test_nothing_on_is_the_actuator_twin_with_all_six_blocks(which):
    n = 17
    acts, ep0 = AC.recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    _, obs_table, events = AC.reference_blocks()
    kw = dict(commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=MAX_LEN,
              terminations=TC.entries_of(TC.liveness_cfg()), actions=AC.reference_perm()[0], actuators=UC.mixed_entries())
    tw = ZT.make_twin(cfg, n, randomize=_off_blocks()[which], **kw)
    parent = UT.make_twin(cfg, n, **kw)
    assert tw.F == parent.F == 364 + 48
    got = ZT.run_randomize_twin(tw, acts, ep0)
    np.testing.assert_array_equal(got.view(U32), UT.run_actuators_twin(parent, acts, ep0).view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.term_record.view(U32), parent.term_record.view(U32))


def test_startup_values_hold_for_an_env_and_reset_values_change_with_the_episode():
    n = 17
    for mode, same in ((False, True), (True, False)):
        tw, _, st = run_recipe(n, words=recipe_block(reset=mode))
        ep = st["ep"][:, :, 0]
        assert (ep.max(0) - ep.min(0) >= 2).all()                            # every env sees at least three episodes
        for key in ("kp", "kd", "fr", "inertia", "m"):
            x = st[key]
            constant = (x == x[:1]).all()
            assert constant == same, (mode, key)
            # within an episode the values never move
            for i in range(n):
                for e in np.unique(ep[:, i]):
                    rows = x[ep[:, i] == e, i]
                    assert (rows == rows[:1]).all()
            # ... and they differ between envs
            sel = [j for j in range(12) if j not in HL + [FL_HAA]]
            assert len(np.unique(x[0][:, sel[0]])) > n // 2, key


def test_unselected_joints_keep_the_tables_value_and_samples_lie_in_their_ranges():
    tw, _, st = run_recipe()
    E = UC.mixed_entries()
    for j in HL:
        assert (st["kp"][:, :, j] == F32(E[j]["kp"])).all() and (st["kd"][:, :, j] == F32(E[j]["kd"])).all()
    assert (st["fr"][:, :, FL_HAA] == 0).all() and (st["inertia"][:, :, FL_HAA] == F32(E[FL_HAA]["inertia"])).all()
    sel = [j for j in range(12) if j not in HL]
    assert (st["kp"][:, :, sel] != np.array([E[j]["kp"] for j in sel], F32)).any()
    # every sample in [lo, hi], for every env and every episode of the run
    w = tw.rnd
    for step in range(0, STEPS, 7):
        ep = st["ep"][step, :, 0].astype(np.uint32)
        samples = tw.robot(ep)["samples"]
        assert sorted(samples) == ["armature", "damping", "friction", "mass", "stiffness"]
        for q, s in samples.items():
            lo, width = w[ZT.WORDS[q]], w[ZT.WORDS[q] + 1]
            assert (s >= lo).all() and (s <= F32(lo + width)).all(), q
    # the operations: scale on the gains, abs on the joint parameters, add on the mass
    rb = tw.robot(np.zeros(17, np.uint32))
    np.testing.assert_array_equal(rb["kp"][:, 1], (F32(E[1]["kp"]) * rb["samples"]["stiffness"][:, 1]).astype(F32))
    np.testing.assert_array_equal(rb["fr"][:, 1], rb["samples"]["friction"][:, 1])
    np.testing.assert_array_equal(rb["inertia"][:, 1], (w[ZT.WORDS["servo_inertia"]] + rb["samples"]["armature"][:, 1]).astype(F32))
    np.testing.assert_array_equal(rb["m"], (w[ZT.WORDS["m0"]] + rb["samples"]["mass"]).astype(F32))
    np.testing.assert_array_equal(rb["weight"], (rb["m"] * F32(9.81)).astype(F32))


def test_the_recipe_exercises_every_rule_of_the_randomisation():
    """conditions on the inputs of the device comparison: 17 envs, 60 steps of N(0, 1) actions, episodes of 25 steps, the
    mixed robot"""
    tw, slabs, st = run_recipe(table=RT.ALL_NON_EXP)
    assert st["stick"].shape[:2] == (STEPS, 17) and np.isfinite(slabs).all()
    ops = int(tw.rnd.view(np.int32)[ZT.WORDS["ops"]])
    assert {ops & 0xFF, (ops >> 8) & 0xFF, (ops >> 16) & 0xFF} == {0, 1, 2}     # every operation occurs
    sel = [j for j in range(12) if j != FL_HAA]
    assert st["stick"][:, :, sel].any() and st["slip"][:, :, sel].any()         # joints stick and slip
    assert not st["stick"][:, :, FL_HAA].any() and not st["slip"][:, :, FL_HAA].any()
    capped = st["capped"][:, :, 0]
    assert capped.any() and (~capped).any()                                     # a_v is capped at 1 in some envs, not in others
    assert capped.any(0).sum() >= 2 and (~capped).any(0).sum() >= 2
    assert st["clamped"].any() and st["free"].any()                             # the torque clamp is reached and not reached
    begins = st["fresh"][1:, :, 0].sum(0)
    assert (begins >= 2).all() and st["fresh"][0].all()                          # every env begins at least two episodes
    # the randomised run is not the nominal one
    nominal = ZT.run_randomize_twin(ZT.make_twin(TC.env_cfg(), 17, actuators=UC.mixed_entries(), max_len=MAX_LEN, table=RT.ALL_NON_EXP),
                                    *CC.recipe(17))
    assert (slabs != nominal).any()
    # joint_acc is tau_w over the env's own inertia
    lo = tw.off["applied_torque"][0]
    tau = slabs[1:, :, lo:lo + 12]
    acc = slabs[1:, :, tw.off["joint_acc"][0]:tw.off["joint_acc"][0] + 12]
    np.testing.assert_array_equal(acc.view(U32), (tau / st["inertia"]).astype(F32).view(U32))
    # each term alone is live, too
    for only in ("gains", "joint", "mass"):
        _, one, _ = run_recipe(words=recipe_block(only=only))
        assert (one != nominal).any(), only
