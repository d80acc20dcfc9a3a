"""The servo task's terminations without a device ("Terminations"): the termination descriptor, table
building from a ``TerminationsCfg``, the errors that name the term, the manager's run state, and properties of the numpy twin -
above all that every kind of term decides the end of some episode in the recipe the device test compares, which is what
keeps that comparison from being vacuous."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import servo_commands_twin as CT
import servo_terminations_twin as TT
import servo_twin as T
import test_servo_commands_twin as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Terminations-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Terminations-v0"
STEPS, MAX_LEN = CC.STEPS, CC.MAX_LEN
#: the liveness block: all eight kinds, limits near the 99th percentile of what 17 envs under N(0, 1) actions reach in 60
#: steps (found on the CPU, recorded in DESIGN section 9 "Terminations"); the model's tilt_max is lowered to 0.21 with them
LIVE_TILT_MAX = 0.21
HAA_MASK, FEET_AND_BASE = 0x249, 0x11111
#: what 17 envs end their episodes with under the liveness block: per term, and the number of ended episodes
LIVE_COUNTS_17 = {"time_out": 31, "contact": 7, "upside_down": 3, "bad_orientation": 1, "height": 6, "joint_pos": 4,
                  "joint_vel": 2, "rolled_over": 7}
LIVE_ENDED_17 = 53


def _tm():
    from cat_envs.shim import SceneEntityCfg
    from cat_envs.shim import TerminationTermCfg as DoneTerm
    from cat_envs.tasks.utils.mdp import terminations as TM
    return TM, DoneTerm, SceneEntityCfg


def env_cfg(tilt_max=None):
    """the servo task's cfg as the simulator tests use it (a command every three steps)"""
    cfg = CC._cfg(T.TASK)
    cfg.synthetic.servo_resample_steps = 3
    if tilt_max is not None:
        cfg.synthetic.servo_tilt_max = tilt_max
    return cfg


def liveness_cfg(only=None):
    """the liveness block as a ``TerminationsCfg`` (a dict); ``only``: the time-out and that term alone"""
    TM, Done, Entity = _tm()
    block = {
        "time_out": Done(func=TM.time_out, time_out=True),
        "contact": Done(func=TM.illegal_contact, params={"threshold": 110.0, "sensor_cfg": Entity(
            "contact_forces", body_names=["base_link", ".*_FOOT"])}),
        "upside_down": Done(func=TM.upside_down, params={"limit": 0.215}),
        "bad_orientation": Done(func=TM.bad_orientation, params={"limit_angle": 0.22}),
        "height": Done(func=TM.root_height_below_minimum, params={"minimum_height": 0.186}),
        "joint_pos": Done(func=TM.joint_pos_out_of_manual_limit, params={"bounds": (-1.36, 1.0)}),
        "joint_vel": Done(func=TM.joint_vel_out_of_manual_limit, params={"max_velocity": 17.5, "asset_cfg": Entity(
            "robot", joint_names=[".*_HAA"])}),
        "rolled_over": Done(func=TM.rolled_over),
    }
    return block if only is None else {k: v for k, v in block.items() if k in ("time_out", only)}


def entries_of(cfg):
    """the table's entries ``(kind, mask, p0, p1)`` of a ``TerminationsCfg``"""
    return [tuple(row[1:]) for row in _tm()[0].build_table(cfg, T.JOINTS, T.BODIES)]


def builtin_cfg():
    from cat_envs.tasks.locomotion.velocity.config.solo12.cat_flat_env_cfg import BuiltinTerminationsCfg
    return BuiltinTerminationsCfg()


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoTerminations._fields_] == ["table", "rec", "terms", "off_term_state"]
    assert ctypes.sizeof(native.ServoTerminations) == 24 and native.ServoTerminations.rec.offset == 8
    assert native.ServoTerminations.terms.offset == 16 and native.ServoTerminations.off_term_state.offset == 20
    assert ctypes.sizeof(native.ServoTermEntry) == 16 and [f[0] for f in native.ServoTermEntry._fields_] == ["kind", "mask", "p0", "p1"]
    assert issubclass(native.ServoSimTerminations, native.ServoSimCommands) and ctypes.sizeof(native.ServoSimCommands) == 416
    assert native.ServoSimTerminations.term.offset == 416 and ctypes.sizeof(native.ServoSimTerminations) == 440
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_terminations, term\) == (\d+) &&\s*sizeof\(catppo_servo_term_entry\) == (\d+) && "
                  r"sizeof\(catppo_servo_terminations\) == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [416, 16, 24]
    assert int(re.search(r"sizeof\(catppo_servo_sim_terminations\) == (\d+)", hip).group(1)) == 440
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_TERMINATIONS (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_TERMINATIONS
    assert native.SERVO_EXT_TERMINATIONS not in (0, native.SERVO_EXT_OBS, native.SERVO_EXT_EVENTS, native.SERVO_EXT_COMMANDS)
    assert int(re.search(r"#define CATPPO_SERVO_TERM_FLOATS (\d+)", src).group(1)) == native.SERVO_TERM_FLOATS == TT.REC_FLOATS
    assert int(re.search(r"#define CATPPO_SERVO_TERM_MAX_TERMS (\d+)", src).group(1)) == native.SERVO_TERM_MAX_TERMS == TT.MAX_TERMS
    assert native.SERVO_TERM_KINDS == TT.KINDS
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_descriptor_without_the_termination_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs(), native.ServoSimEvents(), native.ServoSimCommands()):
        short.reserved = native.SERVO_EXT_TERMINATIONS
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimTerminations"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


# ------------------------------------------------------------------------------------------ table building
def test_tables_of_the_three_cfgs():
    TM = _tm()[0]
    for task in (TASK, REFERENCE, TASK.replace("-v0", "-Play-v0"), REFERENCE.replace("-v0", "-Play-v0")):
        table = TM.build_table(CC._cfg(task).terminations, T.JOINTS, T.BODIES)
        upper = sum(1 << i for i, b in enumerate(T.BODIES) if b == "base_link" or b.endswith("_UPPER_LEG"))
        assert upper == 0x4445
        assert table == [("time_out", 1, 0, 0.0, 0.0), ("base_contact", 2, 0x4445, 1.0, 0.0),
                         ("upside_down", 3, 0, float(F32(0.1)), 0.0)]
    assert TM.build_table(builtin_cfg(), T.JOINTS, T.BODIES) == [("time_out", 1, 0, 0.0, 0.0), ("rolled_over", 8, 0, 0.0, 0.0)]
    live = TM.build_table(liveness_cfg(), T.JOINTS, T.BODIES)
    assert [row[1] for row in live] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert live[1][2] == FEET_AND_BASE and live[5][2] == 0xFFF and live[6][2] == HAA_MASK
    assert live[3][3] == float(F32(math.cos(0.22))) and live[3][4] == 0.0      # p0 = f32(cos(limit_angle))
    assert live[5][3:] == (float(F32(-1.36)), 1.0) and live[6][3] == 17.5
    # the other tasks carry no block
    for task in (CC.TASK, CC.REFERENCE, T.TASK):
        assert getattr(CC._cfg(task), "terminations", None) is None


def test_errors_name_the_term():
    TM, Done, Entity = _tm()
    build = lambda cfg: TM.build_table(cfg, T.JOINTS, T.BODIES)                # noqa: E731
    out = Done(func=TM.time_out, time_out=True)
    with pytest.raises(ValueError, match="exactly one time_out term.*has 0"):
        build({"fell": Done(func=TM.rolled_over)})
    with pytest.raises(ValueError, match="exactly one time_out term.*has 2"):
        build({"a": out, "b": Done(func=TM.time_out, time_out=True)})
    with pytest.raises(ValueError, match="'fell'.*time_out=True"):
        build({"a": out, "fell": Done(func=TM.rolled_over, time_out=True)})
    with pytest.raises(ValueError, match="'late'.*time_out=True"):
        build({"late": Done(func=TM.time_out)})
    with pytest.raises(ValueError, match="'t15'.*more than 15"):
        build({"a": out, **{f"t{i}": Done(func=TM.rolled_over) for i in range(1, 16)}})
    assert len(build({"a": out, **{f"t{i}": Done(func=TM.rolled_over) for i in range(1, 15)}})) == 15
    with pytest.raises(ValueError, match="'touch'"):
        build({"a": out, "touch": Done(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": Entity(
            "contact_forces", body_names=["no_such_body"])})})
    with pytest.raises(ValueError, match="'touch'.*empty"):
        build({"a": out, "touch": Done(func=TM.illegal_contact, params={"threshold": 1.0, "sensor_cfg": Entity(
            "contact_forces", body_ids=[])})})
    with pytest.raises(ValueError, match="'fast'"):
        build({"a": out, "fast": Done(func=TM.joint_vel_out_of_manual_limit, params={"max_velocity": 1.0, "asset_cfg": Entity(
            "robot", joint_names=["nothing"])})})
    with pytest.raises(ValueError, match="'bent'.*hi < lo"):
        build({"a": out, "bent": Done(func=TM.joint_pos_out_of_manual_limit, params={"bounds": (1.0, -1.0)})})
    with pytest.raises(ValueError, match="'mine'.*no describe"):
        build({"a": out, "mine": Done(func=lambda env: None)})
    for func, args in ((TM.time_out, ()), (TM.illegal_contact, (1.0, None)), (TM.upside_down, (0.1,)), (TM.bad_orientation, (1.0,)),
                       (TM.root_height_below_minimum, (0.1,)), (TM.joint_pos_out_of_manual_limit, ((0, 1),)),
                       (TM.joint_vel_out_of_manual_limit, (1.0,)), (TM.rolled_over, ())):
        with pytest.raises(TypeError, match=func.__name__):
            func(None, *args)


# ------------------------------------------------------------------------------------------ the manager
class _Sim:
    def __init__(self, n):
        import torch
        self.table, self.termination_record, self.state = None, torch.zeros(n, 16), torch.zeros(n, 4)

    def set_termination_table(self, entries):
        self.table = list(entries)

    def view(self, name):
        assert name == "term_state"
        return self.state


def _fake_env(n=5):
    import torch
    scene = {"robot": types.SimpleNamespace(joint_names=list(T.JOINTS), body_names=list(T.BODIES)),
             "contact_forces": types.SimpleNamespace(joint_names=[], body_names=list(T.BODIES))}
    z = torch.zeros(n, dtype=torch.bool)
    return types.SimpleNamespace(scene=scene, sim=_Sim(n), reset_terminated=z, reset_time_outs=z.clone(), reset_buf=z.clone())


def test_manager_fingerprint_and_run_state_round_trip():
    import torch
    from cat_envs.tasks.utils.mdp.termination_manager import TerminationManager
    TM, Done, Entity = _tm()
    env = _fake_env()
    mgr = TerminationManager(liveness_cfg(), env)
    assert mgr.active_terms == list(LIVE_COUNTS_17) and env.sim.table == entries_of(liveness_cfg())
    assert mgr.fingerprint()[1] == ["contact", 2, FEET_AND_BASE] and "upside_down" in str(mgr)
    assert mgr.compute() is env.reset_buf and mgr.terminated is env.reset_terminated and mgr.time_outs is env.reset_time_outs
    assert mgr.dones is env.reset_buf
    # get_term reads bit k of the row's field
    env.sim.state[:, 0] = torch.tensor([0.0, 1.0, 4.0, 5.0, 128.0])
    assert mgr.get_term("time_out").tolist() == [False, True, False, True, False]
    assert mgr.get_term("upside_down").tolist() == [False, False, True, True, False]
    assert mgr.get_term("rolled_over").tolist() == [False, False, False, False, True]
    with pytest.raises(ValueError, match="'nope' not found"):
        mgr.get_term("nope")
    # pop_log: shares of the ended episodes, then zeros; None when none ended
    assert mgr.pop_log() is None
    env.sim.termination_record[:, 15] = torch.tensor([1.0, 0.0, 2.0, 0.0, 1.0])
    env.sim.termination_record[:, 0] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0])
    env.sim.termination_record[:, 2] = torch.tensor([0.0, 0.0, 1.0, 0.0, 1.0])
    state = {k: (v.clone() if hasattr(v, "clone") else dict(v)) for k, v in mgr.state_dict().items()}
    log = mgr.pop_log()
    assert log["Episode_Termination/time_out"] == 0.5 and log["Episode_Termination/upside_down"] == 0.5
    assert log["Episode_Termination/contact"] == 0.0 and len(log) == 8 and mgr.pop_log() is None
    # params move in place; kind and selection are fixed
    mgr.set_term_cfg("upside_down", Done(func=TM.upside_down, params={"limit": 0.3}))
    assert env.sim.table[2] == (3, 0, float(F32(0.3)), 0.0) and mgr.get_term_cfg("upside_down").params["limit"] == 0.3
    with pytest.raises(ValueError, match="'upside_down'.*fixed"):
        mgr.set_term_cfg("upside_down", Done(func=TM.rolled_over))
    with pytest.raises(ValueError, match="'joint_vel'.*fixed"):
        mgr.set_term_cfg("joint_vel", Done(func=TM.joint_vel_out_of_manual_limit, params={"max_velocity": 17.5}))
    assert mgr.fingerprint() == TerminationManager(liveness_cfg(), _fake_env()).fingerprint()
    # the state taken before the change comes back: record and params
    mgr.load_state_dict(state)
    assert env.sim.table == entries_of(liveness_cfg()) and float(env.sim.termination_record[:, 15].sum()) == 4.0
    other = TerminationManager(builtin_cfg(), _fake_env())
    assert other.fingerprint() == [["time_out", 1, 0], ["rolled_over", 8, 0]] != mgr.fingerprint()
    with pytest.raises(ValueError, match="termination terms"):
        other.check_state_dict(state)
    with pytest.raises(ValueError, match="termination record"):
        TerminationManager(liveness_cfg(), _fake_env(6)).check_state_dict(state)


# ------------------------------------------------------------------------------------------ the twin
def test_every_kind_decides_an_episode_end_in_the_recipe():
    """a condition on the inputs of the device comparison: under the liveness block every kind is set at the end of at least
    one episode and unset at the end of at least one, and episodes end by time-out and by termination"""
    n = 17
    acts, ep0 = CC.recipe(n)
    terms = entries_of(liveness_cfg())
    tw = TT.make_twin(env_cfg(LIVE_TILT_MAX), n, terms, commands=CC.words_of(CC.commands_cfg_of()), max_len=MAX_LEN)
    assert tw.off["cmd_state"] == (308, 4) and tw.off["term_state"] == (312, 4) and tw.F == 316
    slabs, bits = TT.run_terminations_twin(tw, acts, ep0)
    ended = tw.term_record.sum(0)
    assert ended[15] == LIVE_ENDED_17 and dict(zip(LIVE_COUNTS_17, ended[:8].astype(int))) == LIVE_COUNTS_17
    assert all(0 < c < LIVE_ENDED_17 for c in ended[:8]) and not ended[8:15].any()
    assert tw.stats["ended_by_time_out"] == 29 and tw.stats["ended_by_termination"] == 24
    # term_state holds the bits; hard_reset is the OR of the bits that are no time-out
    a, h = tw.off["term_state"][0], tw.off["hard_reset"][0]
    np.testing.assert_array_equal(slabs[1:, :, a], bits.astype(F32))
    assert not slabs[:, :, a + 1:a + 4].any() and not slabs[0, :, a].any()
    np.testing.assert_array_equal(slabs[1:, :, h] > 0, (bits & ~U32(1)) != 0)
    # the roll-over override of the written gravity follows the model's flag, which ends no episode by itself
    g = tw.off["projected_gravity_b"][0]
    over = (slabs[1:, :, g:g + 3] == np.array([0, 0, 1], F32)).all(-1)
    np.testing.assert_array_equal(over, (bits >> U32(7)) & 1 == 1)
    assert over.any()
    # each kind alone fires, too
    for name in list(LIVE_COUNTS_17)[1:]:
        one = TT.make_twin(env_cfg(LIVE_TILT_MAX), n, entries_of(liveness_cfg(name)), commands=CC.words_of(CC.commands_cfg_of()),
                           max_len=MAX_LEN)
        TT.run_terminations_twin(one, acts, ep0)
        assert 0 < one.term_record[:, 1].sum() < one.term_record[:, 15].sum(), name


@pytest.mark.parametrize("commands", [True, False])
def test_builtin_block_reproduces_the_parent_twin(commands):
    """``time_out`` + ``rolled_over`` is today's rule: the rows, ``term_state`` apart, are the parent twin's byte for byte"""
    import servo_events_twin as ET
    n = 17
    acts, ep0 = CC.recipe(n)
    cfg = env_cfg(LIVE_TILT_MAX)                               # falls do occur at this tilt_max
    words = CC.words_of(CC.commands_cfg_of()) if commands else None
    tw = TT.make_twin(cfg, n, entries_of(builtin_cfg()), commands=words, max_len=MAX_LEN, table=TT.RT.ALL_NON_EXP)
    slabs, bits = TT.run_terminations_twin(tw, acts, ep0)
    if commands:
        parent = CT.make_twin(cfg, n, words, max_len=MAX_LEN, table=TT.RT.ALL_NON_EXP)
        ref = CT.run_commands_twin(parent, acts, ep0)[0]
    else:
        parent = ET.make_twin(cfg, n, None, max_len=MAX_LEN, table=TT.RT.ALL_NON_EXP)
        ref = ET.run_events_twin(parent, acts, ep0)[0]
    assert tw.F == parent.F + 4 and tw.off["term_state"] == (parent.F, 4)
    np.testing.assert_array_equal(slabs[:, :, :parent.F].view(U32), ref.view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), parent.reward_record.view(U32))
    assert tw.stats["ended_by_termination"] >= 5 and tw.stats["ended_by_time_out"] >= 5
    assert {0, 1, 2} <= set(int(b) for b in np.unique(bits)) <= {0, 1, 2, 3}
