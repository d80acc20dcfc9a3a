"""The servo task's actuator table without a device ("Actuators"): the actuator descriptor, and properties of
the numpy twin - that the identity table is the parent chain bit for bit, alone and with all six blocks, and that in the
recipe the device test compares every lag occurs, the third history slot is used, both bounds of the DC motor and the ideal
clamp bind and do not bind, and every env refills its history at least twice, which is what keeps that comparison from being
vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_actions_twin as AT
import servo_actuators_twin as UT
import servo_reward_twin as RT
import servo_twin as T
import test_servo_actions_twin as AC
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
STEPS, MAX_LEN = CC.STEPS, CC.MAX_LEN
DECIMATION = 4
LATE, IDEAL, MOTOR = [9, 10, 11], [0, 1, 2, 3, 4, 5], [6, 7, 8]         # HR_* | FL_* FR_* | HL_*
PURE_DAMPER = 5                                                          # FR_KFE: stiffness 0 under a position target


def mixed_entries(only=None):
    """the liveness robot, one entry per simulator joint.  Group 0 "late": HR_*, the reference's gains as a delayed PD with a
    lag of 0 .. 3 * decimation physics steps.  Group 1 "front": FL_* and FR_*, ideal PD with per-joint gains, inertias and
    effort limits; FR_KFE has stiffness 0.  Group 2 "motor": HL_*, a DC motor whose saturation torque of 4 Nm lies above its
    effort limit of 3 Nm and whose no-load speed is 12 rad/s, so that each bound is cut by the joint speed in some substeps
    and left alone in others.  ``only``: that group as described, the two others plain ideal PD at the reference's gains"""
    plain = dict(kp=4.0, kd=0.2, inertia=0.024, effort_limit=3.0)
    E = []
    for j, name in enumerate(T.JOINTS):
        part = j % 3
        if name.startswith("HR"):
            e = dict(plain, min_delay=0, max_delay=3 * DECIMATION, group=0) if only in (None, "late") else dict(plain, group=0)
        elif name.startswith("F"):
            e = dict(kp=0.0 if j == PURE_DAMPER else (2.0, 4.0, 6.0)[part], kd=0.1 + 0.05 * part, inertia=0.02 + 0.004 * part,
                     effort_limit=2.5 + 0.5 * part, group=1) if only in (None, "front") else dict(plain, group=1)
        else:
            e = dict(plain, saturation_effort=4.0, velocity_limit=12.0, dc_motor=True, group=2) if only in (None, "motor") \
                else dict(plain, group=2)
        E.append(e)
    return E


def run_mixed(n=17, only=None, **kw):
    """(twin, slabs, stats [steps, N, 12] per key) of the recipe: 60 steps of N(0, 1) actions, episodes of 25 steps"""
    acts, ep0 = CC.recipe(n)
    tw = UT.make_twin(TC.env_cfg(), n, actuators=mixed_entries(only), max_len=MAX_LEN, **kw)
    slabs = UT.run_actuators_twin(tw, acts, ep0)
    return tw, slabs, {k: np.stack([s[k] for s in tw.live_steps]) for k in tw.live_steps[0]}


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoActuators._fields_] == ["table", "off_act_hist", "reserved"]
    assert ctypes.sizeof(native.ServoActuators) == 16 and native.ServoActuators.off_act_hist.offset == 8
    assert ctypes.sizeof(native.ServoActuatorEntry) == 32 and native.ServoActuatorEntry.flags.offset == 24
    assert [f[0] for f in native.ServoActuatorEntry._fields_] == ["kp", "kd", "inertia", "effort_limit", "saturation_effort",
                                                                  "velocity_limit", "flags", "delay"]
    assert issubclass(native.ServoSimActuators, native.ServoSimActions) and ctypes.sizeof(native.ServoSimActions) == 456
    assert native.ServoSimActuators.actu.offset == 456 and ctypes.sizeof(native.ServoSimActuators) == 472
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_actuators, act\) == (\d+) && offsetof\(catppo_servo_sim_actuators, actu\) == (\d+) &&\s*"
                  r"sizeof\(catppo_servo_actuator_entry\) == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [440, 456, 32]
    assert int(re.search(r"sizeof\(catppo_servo_sim_actuators\) == (\d+)", hip).group(1)) == 472
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_ACTUATORS (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_ACTUATORS
    assert native.SERVO_EXT_ACTUATORS == int.from_bytes(b"ACU1", "big")
    assert native.SERVO_EXT_ACTUATORS not in (0, native.SERVO_EXT_OBS, native.SERVO_EXT_EVENTS, native.SERVO_EXT_COMMANDS,
                                              native.SERVO_EXT_TERMINATIONS, native.SERVO_EXT_ACTIONS)
    assert int(re.search(r"#define CATPPO_SERVO_ACT_HIST_FLOATS (\d+)", src).group(1)) == native.SERVO_ACT_HIST_FLOATS == UT.HIST_FLOATS
    assert int(re.search(r"#define CATPPO_SERVO_ACTUATOR_DC_MOTOR (0x[0-9A-Fa-f]+)u", src).group(1), 16) == native.SERVO_ACTUATOR_DC_MOTOR
    kernel = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_kernel.h")).read()
    assert int(re.search(r"kTagActDelay = (0x[0-9A-Fa-f]+)u", kernel).group(1), 16) == UT.TAG_ACT_DELAY == int.from_bytes(b"ADLY", "big")
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_descriptor_without_the_actuator_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs(), native.ServoSimEvents(), native.ServoSimCommands(),
                  native.ServoSimTerminations(), native.ServoSimActions()):
        short.reserved = native.SERVO_EXT_ACTUATORS
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimActuators"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


def test_every_instance_of_the_new_packs_is_reachable():
    """16 packs end with the action and the actuator descriptors; the one launch of servo_sim_actuators.hip reaches each of them:
    with_present hands it whichever of the four optional descriptors are there, in the pack's order (all 16 combinations:
    tests/test_servo_sim_host.py), and the unit's own descriptors follow them"""
    src = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_actuators.hip")).read()
    calls = re.findall(r"with_present\(\[&\]\(const auto&\.\.\. opt\) \{ launch\(mode, rew, nblk, lds_bytes, st, d, ([^)]*)\); \},\s*([^)]*)\);", src)
    assert calls == [("opt..., *x.ac, *x.au", "x.obs, x.ev, x.cm, x.tm")]
    assert len(re.findall(r"\blaunch\(", src)) == 1                          # and nothing else launches here


# ------------------------------------------------------------------------------------------ the twin
def test_identity_table_is_the_parent_twin_alone():
    """kp, kd, inertia, tau_max of the simulator on every joint, ideal PD, no delay: slabs (the history field apart),
    records and trace of the parent chain"""
    n = 17
    acts, ep0 = AC.recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    kw = dict(max_len=MAX_LEN, table=RT.ALL_NON_EXP, trace_envs=5, trace_capacity=STEPS + 3)
    tw = UT.make_twin(cfg, n, **kw)
    parent = AT.make_twin(cfg, n, **kw)
    assert tw.F == parent.F + UT.HIST_FLOATS and tw.off["act_hist"] == (parent.F, UT.HIST_FLOATS)
    assert {k: v for k, v in tw.off.items() if k != "act_hist"} == parent.off
    got = UT.run_actuators_twin(tw, acts, ep0)
    np.testing.assert_array_equal(got[:, :, :parent.F].view(U32), AT.run_actions_twin(parent, acts, ep0).view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.record.view(U32), parent.record.view(U32))
    np.testing.assert_array_equal(tw.trace.view(U32), parent.trace.view(U32))
    assert tw.actu_live["clamped"].any() and tw.actu_live["free"].any()
    # the history field: zero behind the init launch, then p | p of the step before | p of two steps before
    hist = got[:, :, parent.F:].reshape(STEPS + 1, n, 3, 16)
    assert not hist[0].any() and (hist[1:, :, 0, 12] == 1).all() and not hist[:, :, :, 13:].any() and not hist[:, :, 1:, 12].any()
    p = F32(0.5) * acts + T.DEFAULT_JOINT_POS
    np.testing.assert_array_equal(hist[1:, :, 0, :12].view(U32), p.view(U32))


def test_identity_table_is_the_parent_twin_with_all_six_blocks():
    n = 17
    acts, ep0 = AC.recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    _, obs_table, events = AC.reference_blocks()
    kw = dict(commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=MAX_LEN,
              terminations=TC.entries_of(TC.liveness_cfg()), actions=AC.reference_perm()[0])
    tw = UT.make_twin(cfg, n, **kw)
    parent = AT.make_twin(cfg, n, **kw)
    assert tw.F == parent.F + UT.HIST_FLOATS == 364 + 48
    got = UT.run_actuators_twin(tw, acts, ep0)
    np.testing.assert_array_equal(got[:, :, :parent.F].view(U32), AT.run_actions_twin(parent, acts, ep0).view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.term_record.view(U32), parent.term_record.view(U32))
    assert parent.stats["ended_by_termination"] >= 5


def test_the_recipe_exercises_every_rule_of_the_actuator_model():
    """conditions on the inputs of the device comparison: 17 envs, 60 steps of N(0, 1) actions, episodes of 25 steps, the
    mixed robot"""
    assert TC.env_cfg().decimation == DECIMATION
    tw, slabs, st = run_mixed(table=RT.ALL_NON_EXP)
    steps, n = st["lag"].shape[:2]
    assert (steps, n) == (STEPS, 17) and np.isfinite(slabs).all()
    # every lag 0 .. 12 occurs in some env, shared by the joints of the group; the other groups have none
    assert set(st["lag"][:, :, LATE[0]].ravel().tolist()) == set(range(3 * DECIMATION + 1))
    assert (st["lag"][:, :, LATE] == st["lag"][:, :, LATE[:1]]).all() and not st["lag"][:, :, IDEAL + MOTOR].any()
    # some env uses history slot 2 (k = 3), every slot 0 .. 2 is used, the undelayed joints use none
    assert {0, 1, 2, 3} == set(st["slot"][:, :, LATE].ravel().tolist()) and not st["slot"][:, :, IDEAL + MOTOR].any()
    # the delayed target differs from the undelayed one in some substeps and equals it in others (a refilled history)
    assert st["late"][:, :, LATE].any() and st["same"][:, :, LATE].any() and not st["late"][:, :, IDEAL + MOTOR].any()
    # each of the DC motor's bounds binds in some substeps and not in others; the other joints have no such bounds
    for k in ("hi_binds", "hi_free", "lo_binds", "lo_free"):
        assert st[k][:, :, MOTOR].any() and not st[k][:, :, IDEAL + LATE].any(), k
    # ... and where it binds below the effort limit the reported torque shows it: |tau_w| < effort_limit although clamped
    tau = slabs[1:, :, tw.off["applied_torque"][0]:tw.off["applied_torque"][0] + 12]
    assert (np.abs(tau[:, :, MOTOR]) <= F32(3.0)).all() and (np.abs(tau[:, :, IDEAL + LATE]) <= F32(3.5)).all()
    # the ideal clamp is reached and not reached, at the joint's own limit
    ideal = [j for j in IDEAL if j != PURE_DAMPER]
    assert st["clamped"][:, :, ideal].any() and st["free"][:, :, ideal].any()
    assert np.abs(tau[:, :, 2]).max() == F32(3.5) and np.abs(tau[:, :, 1]).max() == F32(3.0) and np.abs(tau[:, :, 0]).max() <= F32(2.5)
    # the joint with stiffness 0 is a pure damper: its torque is -kd qd of some substep, whatever the action says
    assert np.abs(tau[:, :, PURE_DAMPER]).max() < 0.2 < np.abs(tau[:, :, 2]).max()
    # at least two episodes begin per env behind the first state: the history is refilled
    begins = st["fresh"][1:, :, 0].sum(0)
    assert (begins >= 2).all() and st["fresh"][0].all()
    # joint_acc is tau_w over the joint's own inertia
    acc = slabs[1:, :, tw.off["joint_acc"][0]:tw.off["joint_acc"][0] + 12]
    np.testing.assert_array_equal(acc.view(U32), (tau / tw.u_inertia).astype(F32).view(U32))
    # each group alone is live, too
    for only, js in (("late", LATE), ("front", ideal), ("motor", MOTOR)):
        _, _, one = run_mixed(only=only)
        assert one["clamped"][:, :, js].any() and one["free"][:, :, js].any(), only
    assert run_mixed(only="late")[2]["late"][:, :, LATE].any() and run_mixed(only="motor")[2]["hi_binds"][:, :, MOTOR].any()


def test_a_lag_of_one_control_step_reproduces_the_row_one_step_late():
    """min = max = decimation: every substep acts on slot 0, i.e. on the processed action of the step before"""
    n = 5
    acts, ep0 = CC.recipe(n, 12)
    plain = dict(kp=4.0, kd=0.2, inertia=0.024, effort_limit=3.0)
    late = [dict(plain, min_delay=DECIMATION, max_delay=DECIMATION)] * 12
    cfg = TC.env_cfg()
    a = UT.run_actuators_twin(UT.make_twin(cfg, n, actuators=late, max_len=1000), acts, np.zeros(n, np.int64))
    shifted = np.concatenate([acts[:1], acts[:-1]])                            # the first step refills with its own p
    b = UT.run_actuators_twin(UT.make_twin(cfg, n, actuators=[plain] * 12, max_len=1000), shifted, np.zeros(n, np.int64))
    for name in ("joint_pos", "joint_vel", "applied_torque", "joint_acc"):
        lo, w = UT.make_twin(cfg, n).off[name]
        np.testing.assert_array_equal(a[:, :, lo:lo + w].view(U32), b[:, :, lo:lo + w].view(U32))
