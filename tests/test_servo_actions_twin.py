"""The servo task's action block without a device ("Actions"): the action descriptor, and properties of the
numpy twin - that the identity block is the parent twin bit for bit, that the reference's block is a permutation of the
action's columns and nothing else, and that in the recipe the device test compares every kind drives a joint, every clip
bound binds and the torque clamp is reached for every kind, which is what keeps that comparison from being vacuous."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_actions_twin as AT
import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Actions-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Actions-v0"
STEPS, MAX_LEN = CC.STEPS, CC.MAX_LEN
#: the reward table of the comparisons that may not reorder a sum over the action's columns: ALL_NON_EXP without kinds 11, 12
NO_ACTION_SUMS = [row for row in RT.ALL_NON_EXP if row[0] not in (11, 12)]


def _am():
    from cat_envs.tasks.utils.mdp import actions as AM
    return AM


def mixed_cfg(only=None):
    """the liveness block, A = 8: all four kinds, clips on one joint of each, four joints no term drives.  With kp 3, kd 0.2
    and tau_max 3.5 the clamp needs |p - q| > 1.17 rad (position), |p| > 1.17 (relative), |p - qd| > 17.5 rad/s (velocity),
    |p| > 3.5 Nm (effort); the scales put a tenth to a third of N(0, 1) actions beyond that, the clips a little further out.
    ``only``: that term alone"""
    AM = _am()
    block = {
        "legs": AM.JointPositionActionCfg(joint_names=["FL_.*"], scale={".*_HAA": 0.25, ".*_HFE": 0.5, ".*_KFE": 1.5},
                                          clip={"FL_KFE": (-2.6, 1.0)}),
        "swing": AM.RelativeJointPositionActionCfg(joint_names=["FR_HFE", "FR_HAA"], scale=1.0, preserve_order=True,
                                                   clip={".*": (-1.5, 1.5)}),
        "spin": AM.JointVelocityActionCfg(joint_names=["HL_HAA", "HL_HFE"], scale=10.0, clip={"HL_HFE": (-25.0, 22.0)}),
        "push": AM.JointEffortActionCfg(joint_names=["HR_KFE"], scale=2.5, offset=0.5, clip={"HR_KFE": (-4.0, 4.5)}),
    }
    return block if only is None else {only: block[only]}


def entries_of(cfg):
    """(entries, width) of an ``ActionsCfg`` as ``set_action_table`` and the twin take them"""
    entries, terms = _am().build_table(cfg, T.JOINTS, T.DEFAULT_JOINT_POS)
    return entries, max(t["slice"][1] for t in terms.values())


def recipe(n, width, steps=STEPS):
    acts, ep0 = CC.recipe(n, steps)
    return np.ascontiguousarray(acts[:, :, :width]), ep0


def reference_blocks(push_probability=0.25):
    """the other blocks of the Reference-Actions task: its rewards, observations and events (pushes raised to 0.25 so that they
    occur in 60 steps); the commands and terminations of the comparisons are the test cfgs of their own suites"""
    from cat_envs.tasks.utils.mdp import event_manager as EM
    from cat_envs.tasks.utils.mdp import observation_manager as OM
    from cat_envs.tasks.utils.mdp import rewards as R
    cfg = CC._cfg(REFERENCE)
    push = cfg.events.push_robot
    push.params = {**push.params, "probability": push_probability}
    table = [tuple(row[1:]) for row in R.build_table(cfg.rewards, T.JOINTS, 45)[1]]
    obs_table = OM.build_table(OM.policy_group(cfg.observations), T.JOINTS, T.DEFAULT_JOINT_POS)[0]
    events = EM.pack(EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s))
    return table, obs_table, events


def reference_perm():
    """ids[k]: the simulator joint that column k of the reference's block drives"""
    entries, width = entries_of(CC._cfg(TASK).actions)
    assert width == 12
    ids = [None] * 12
    for j, e in enumerate(entries):
        ids[e[0]] = j
    return entries, ids


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoActions._fields_] == ["table", "width", "reserved"]
    assert ctypes.sizeof(native.ServoActions) == 16 and native.ServoActions.width.offset == 8
    assert ctypes.sizeof(native.ServoActionEntry) == 32
    assert [f[0] for f in native.ServoActionEntry._fields_] == ["col", "flags", "scale", "offset", "clip_lo", "clip_hi", "zero"]
    assert issubclass(native.ServoSimActions, native.ServoSimTerminations) and ctypes.sizeof(native.ServoSimTerminations) == 440
    assert native.ServoSimActions.act.offset == 440 and ctypes.sizeof(native.ServoSimActions) == 456
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_actions, act\) == (\d+) &&\s*sizeof\(catppo_servo_action_entry\) == (\d+) && "
                  r"sizeof\(catppo_servo_actions\) == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [440, 32, 16]
    assert int(re.search(r"sizeof\(catppo_servo_sim_actions\) == (\d+)", hip).group(1)) == 456
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_ACTIONS (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_ACTIONS
    assert native.SERVO_EXT_ACTIONS == int.from_bytes(b"ACT1", "big")
    assert native.SERVO_EXT_ACTIONS not in (0, native.SERVO_EXT_OBS, native.SERVO_EXT_EVENTS, native.SERVO_EXT_COMMANDS,
                                            native.SERVO_EXT_TERMINATIONS)
    assert int(re.search(r"#define CATPPO_SERVO_ACTION_KIND_MASK (0x[0-9A-Fa-f]+)u", src).group(1), 16) == native.SERVO_ACTION_KIND_MASK
    assert int(re.search(r"#define CATPPO_SERVO_ACTION_CLIP (0x[0-9A-Fa-f]+)u", src).group(1), 16) == native.SERVO_ACTION_CLIP
    assert native.SERVO_ACTION_KINDS == AT.KINDS and max(AT.KINDS.values()) <= native.SERVO_ACTION_KIND_MASK
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_descriptor_without_the_action_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs(), native.ServoSimEvents(), native.ServoSimCommands(),
                  native.ServoSimTerminations()):
        short.reserved = native.SERVO_EXT_ACTIONS
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimActions"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


def test_every_instance_of_the_new_packs_is_reachable():
    """16 packs end with the action descriptor; the one launch of servo_sim_actions.hip reaches each of them:
    with_present hands it whichever of the four optional descriptors are there, in the pack's order (all 16 combinations:
    tests/test_servo_sim_host.py), and the unit's own descriptors follow them"""
    src = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_actions.hip")).read()
    calls = re.findall(r"with_present\(\[&\]\(const auto&\.\.\. opt\) \{ launch\(mode, rew, nblk, lds_bytes, st, d, ([^)]*)\); \},\s*([^)]*)\);", src)
    assert calls == [("opt..., *x.ac", "x.obs, x.ev, x.cm, x.tm")]
    assert len(re.findall(r"\blaunch\(", src)) == 1                          # and nothing else launches here


# ------------------------------------------------------------------------------------------ the twin
def test_identity_block_is_the_parent_twin_alone():
    """col = j, kind 1, scale = servo_action_scale, offset = default pose, no clip: slabs, records and trace of the parent"""
    n = 17
    acts, ep0 = recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    kw = dict(max_len=MAX_LEN, table=RT.ALL_NON_EXP, trace_envs=5, trace_capacity=STEPS + 3)
    tw = AT.make_twin(cfg, n, **kw)
    parent = RT.make_twin(cfg, n, **kw)
    np.testing.assert_array_equal(AT.run_actions_twin(tw, acts, ep0).view(U32), RT.run_reward_twin(parent, acts, ep0)[0].view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.record.view(U32), parent.record.view(U32))
    np.testing.assert_array_equal(tw.trace.view(U32), parent.trace.view(U32))
    assert tw.live["clamped"].any() and tw.live["free"].any()


def test_identity_block_is_the_parent_twin_with_all_five_other_blocks():
    n = 17
    acts, ep0 = recipe(n, 12)
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    table, obs_table, events = reference_blocks()
    assert {11, 12} <= {row[0] for row in RT.ALL_NON_EXP}                     # the two kinds that read the action are among them
    kw = dict(commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=MAX_LEN)
    terms = TC.entries_of(TC.liveness_cfg())
    tw = AT.make_twin(cfg, n, terminations=terms, **kw)
    parent = TT.make_twin(cfg, n, terms, **kw)
    assert tw.F == parent.F and tw.off == parent.off
    ref, bits = TT.run_terminations_twin(parent, acts, ep0)
    np.testing.assert_array_equal(AT.run_actions_twin(tw, acts, ep0).view(U32), ref.view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.term_record.view(U32), parent.term_record.view(U32))
    assert parent.stats["ended_by_termination"] >= 5


def test_reference_block_permutes_the_columns_and_nothing_else():
    """FL FR HR HL against the simulator's FL FR HL HR: fed ``a[:, perm]`` the block gives the rows of the block-free twin fed
    ``a``, the last-action floats permuted"""
    n = 17
    acts, ep0 = recipe(n, 12)
    entries, ids = reference_perm()
    assert ids == [0, 1, 2, 3, 4, 5, 9, 10, 11, 6, 7, 8]
    assert all(e[1:] == (1, 0.5, float(T.DEFAULT_JOINT_POS[j]), None) for j, e in enumerate(entries))
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    assert float(cfg.synthetic.servo_action_scale) == 0.5
    kw = dict(max_len=MAX_LEN, table=NO_ACTION_SUMS, trace_envs=n, trace_capacity=STEPS)
    tw = AT.make_twin(cfg, n, actions=entries, **kw)
    parent = RT.make_twin(cfg, n, **kw)
    got = AT.run_actions_twin(tw, acts[:, :, ids], ep0)
    ref = RT.run_reward_twin(parent, acts, ep0)[0]
    a = tw.off["obs"][0] + 33
    assert np.abs(ref[1:, :, a:a + 12]).max() > 0
    np.testing.assert_array_equal(got[:, :, a:a + 12].view(U32), ref[:, :, a:a + 12][:, :, ids].view(U32))
    got[:, :, a:a + 12] = ref[:, :, a:a + 12]
    np.testing.assert_array_equal(got.view(U32), ref.view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    np.testing.assert_array_equal(tw.record.view(U32), parent.record.view(U32))
    np.testing.assert_array_equal(tw.trace[:, :, :60].view(U32), parent.trace[:, :, :60].view(U32))
    np.testing.assert_array_equal(tw.trace[:, :, 60:].view(U32), parent.trace[:, :, 60:][:, :, ids].view(U32))
    # without the permutation of the input the hind legs swap: the block is not the identity
    assert (AT.run_actions_twin(AT.make_twin(cfg, n, actions=entries, **kw), acts, ep0) != ref).any()


def run_mixed(n=17, only=None, **kw):
    entries, width = entries_of(mixed_cfg(only))
    acts, ep0 = recipe(n, width)
    tw = AT.make_twin(TC.env_cfg(), n, actions=entries, width=width, max_len=MAX_LEN, **kw)
    ep_len = np.asarray(ep0, np.int64).copy()
    slab = tw.initial(ep_len)
    reset = np.zeros(n, bool)
    slabs, live = [slab], []
    for a in acts:
        slab = tw.step(slab, a, reset, ep_len)
        live.append(tw.live)
        ep_len += 1
        reset = (ep_len >= tw.max_len) | (tw._f(slab, "hard_reset")[:, 0] > 0.5)
        ep_len[reset] = 0
        slabs.append(slab)
    stats = {k: np.stack([s[k] for s in live]) for k in live[0]}          # [steps, N, 12]
    return tw, entries, np.stack(slabs), stats


def test_every_kind_drives_clips_and_saturates_in_the_recipe():
    """conditions on the inputs of the device comparison: 17 envs, 60 steps of N(0, 1) actions, the mixed block"""
    tw, entries, slabs, stats = run_mixed(table=RT.ALL_NON_EXP)
    assert tw.A == 8 and [e[0] for e in entries] == [0, 1, 2, 4, 3, -1, 5, 6, -1, -1, -1, 7]
    kinds = [e[1] for e in entries]
    assert kinds == [1, 1, 1, 2, 2, 0, 3, 3, 0, 0, 0, 4] and set(kinds) == {0, 1, 2, 3, 4}
    clipped = [j for j, e in enumerate(entries) if e[4] is not None]
    assert clipped == [2, 3, 4, 7, 11] and {kinds[j] for j in clipped} == {1, 2, 3, 4}
    total = stats["below"].shape[0] * stats["below"].shape[1]
    for j in clipped:                                        # each bound binds in some joint-steps and not in others
        below, above = int(stats["below"][:, :, j].sum()), int(stats["above"][:, :, j].sum())
        assert 0 < below < total and 0 < above < total and below + above < total, (j, below, above)
    # the torque clamp is reached and not reached, for every kind (FL_HAA at scale 0.25 never reaches it: a kind, not a joint)
    for kind in (1, 2, 3, 4):
        js = [j for j in range(12) if kinds[j] == kind]
        assert stats["clamped"][:, :, js].any() and stats["free"][:, :, js].any()
    # the last-action block and the trace hold the raw columns, zero past the width
    a = tw.off["obs"][0] + 33
    assert not slabs[:, :, a + 8:a + 12].any() and np.abs(slabs[1:, :, a:a + 8]).max() > 1
    # an undriven joint stays near its default pose; a driven one leaves it
    q = slabs[1:, :, tw.off["joint_pos"][0]:tw.off["joint_pos"][0] + 12] - T.DEFAULT_JOINT_POS
    assert np.abs(q[:, :, [5, 8, 9, 10]]).max() < 0.11 and np.abs(q[:, :, 0]).max() > 0.2
    # each kind alone drives, too
    for only in ("legs", "swing", "spin", "push"):
        one, ent, sl, st = run_mixed(only=only)
        js = [j for j, e in enumerate(ent) if e[1] != 0]
        assert st["clamped"][:, :, js].any() and st["free"][:, :, js].any(), only


def test_clamped_column_and_unknown_kind_stay_inside_the_action():
    """whatever the table holds: a column outside 0 .. A - 1 is clamped, an unknown kind is "not driven" """
    n = 5
    entries, width = entries_of(mixed_cfg())
    acts, ep0 = recipe(n, width, 8)
    wild = list(entries)
    wild[0] = (99, 1, *entries[0][2:])
    wild[1] = (-7, 1, *entries[1][2:])
    tame = list(entries)
    tame[0] = (width - 1, 1, *entries[0][2:])
    tame[1] = (0, 1, *entries[1][2:])
    cfg = TC.env_cfg()
    a = AT.run_actions_twin(AT.make_twin(cfg, n, actions=wild, width=width, max_len=MAX_LEN), acts, ep0)
    b = AT.run_actions_twin(AT.make_twin(cfg, n, actions=tame, width=width, max_len=MAX_LEN), acts, ep0)
    np.testing.assert_array_equal(a.view(U32), b.view(U32))
    odd = list(entries)
    odd[11] = (entries[11][0], 6, *entries[11][2:])
    none = list(entries)
    none[11] = (entries[11][0], 0, *entries[11][2:])
    a = AT.run_actions_twin(AT.make_twin(cfg, n, actions=odd, width=width, max_len=MAX_LEN), acts, ep0)
    b = AT.run_actions_twin(AT.make_twin(cfg, n, actions=none, width=width, max_len=MAX_LEN), acts, ep0)
    np.testing.assert_array_equal(a.view(U32), b.view(U32))
