"""``mdp.actions`` and the action manager without a device ("Actions"): table building from an ``ActionsCfg``
- column order with and without ``preserve_order``, dict scales, default and zero offsets, clips - the errors that name the
term, the manager's ``spec()``, run state and ``set_term_cfg``, and the ``actions.json`` that ``export_policy`` writes."""
import json
import os
import types

import numpy as np
import pytest

import servo_twin as T
import test_servo_actions_twin as AC
import test_servo_commands_twin as CC

F32 = np.float32
DEF = [float(v) for v in T.DEFAULT_JOINT_POS]


def build(cfg):
    return AC._am().build_table(cfg, T.JOINTS, T.DEFAULT_JOINT_POS)


def test_cfg_classes_are_exported_like_the_other_term_cfgs():
    import cat_envs.shim as shim
    from cat_envs.tasks.utils import mdp
    AM = AC._am()
    for name in ("JointPositionActionCfg", "RelativeJointPositionActionCfg", "JointVelocityActionCfg", "JointEffortActionCfg"):
        assert getattr(shim, name) is getattr(AM, name) is getattr(mdp.actions, name)
    term = AM.JointPositionActionCfg(joint_names=[".*"])
    assert (term.asset_name, term.scale, term.offset, term.use_default_offset, term.preserve_order, term.clip, term.debug_vis) == \
        ("robot", 1.0, 0.0, True, False, None, False)
    assert AM.RelativeJointPositionActionCfg().use_zero_offset is True and AM.JointVelocityActionCfg().use_default_offset is True


def test_tables_of_the_task_cfgs():
    for task in (AC.TASK, AC.REFERENCE, AC.TASK.replace("-v0", "-Play-v0"), AC.REFERENCE.replace("-v0", "-Play-v0")):
        entries, terms = build(CC._cfg(task).actions)
        # the reference's columns are FL FR HR HL: hind right before hind left, as its observations are
        assert [e[0] for e in entries] == [0, 1, 2, 3, 4, 5, 9, 10, 11, 6, 7, 8]
        assert all(e[1:] == (1, 0.5, float(F32(DEF[j])), None) for j, e in enumerate(entries))
        assert terms == {"joint_pos": {"kind": "joint_position", "slice": (0, 12), "joint_ids": [0, 1, 2, 3, 4, 5, 9, 10, 11, 6, 7, 8]}}
    from cat_envs.tasks.locomotion.velocity.config.solo12 import cat_flat_env_cfg as E
    assert CC._cfg(AC.REFERENCE).observations.policy.joint_pos.params["asset_cfg"].joint_names == E.OBS_JOINTS
    # all six blocks on the Reference-Actions task; the other tasks carry no action block and keep what they had
    ref = CC._cfg(AC.REFERENCE)
    assert all(getattr(ref, k) is not None for k in ("rewards", "observations", "events", "commands", "terminations", "actions"))
    for task in (CC.TASK, CC.REFERENCE, T.TASK, "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Terminations-v0"):
        assert getattr(CC._cfg(task), "actions", None) is None


def test_column_order_scales_offsets_and_clips():
    AM = AC._am()
    # asset order without preserve_order, whatever the list's order; the list's order with it
    hind = ["HR_.*", "HL_KFE", "FL_HAA"]
    e, t = build({"a": AM.JointPositionActionCfg(joint_names=hind)})
    assert t["a"]["joint_ids"] == [0, 8, 9, 10, 11] and [x[0] for x in e] == [0, -1, -1, -1, -1, -1, -1, -1, 1, 2, 3, 4]
    e, t = build({"a": AM.JointPositionActionCfg(joint_names=hind, preserve_order=True)})
    assert t["a"]["joint_ids"] == [9, 10, 11, 8, 0] and [x[0] for x in e] == [4, -1, -1, -1, -1, -1, -1, -1, 3, 0, 1, 2]
    assert [x[1] for x in e] == [1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
    # terms are concatenated in cfg order
    e, t = build({"vel": AM.JointVelocityActionCfg(joint_names=[".*_KFE"]), "pos": AM.JointPositionActionCfg(joint_names=[".*_HAA"])})
    assert t["vel"]["slice"] == (0, 4) and t["pos"]["slice"] == (4, 8)
    assert [x[0] for x in e] == [4, -1, 0, 5, -1, 1, 6, -1, 2, 7, -1, 3]
    # dict scales (IsaacLab's scale={".*_HAA": 0.25, ...}); a joint no key matches keeps 1.0
    e, _ = build({"a": AM.JointPositionActionCfg(joint_names=[".*"], scale={".*_HAA": 0.25, ".*_HFE": 0.5})})
    assert [x[2] for x in e] == [0.25, 0.5, 1.0] * 4
    # offsets: the default pose for a position term, zero for a velocity term's default velocity and a relative term
    e, _ = build({"a": AM.JointPositionActionCfg(joint_names=[".*"], offset=7.0)})
    assert [x[3] for x in e] == [float(F32(v)) for v in DEF]
    e, _ = build({"a": AM.JointPositionActionCfg(joint_names=[".*"], offset={".*_KFE": 0.125}, use_default_offset=False)})
    assert [x[3] for x in e] == [0.0, 0.0, 0.125] * 4
    e, _ = build({"a": AM.JointVelocityActionCfg(joint_names=[".*"], offset=3.0)})
    assert [x[3] for x in e] == [0.0] * 12
    e, _ = build({"a": AM.JointVelocityActionCfg(joint_names=[".*"], offset=3.0, use_default_offset=False)})
    assert [x[3] for x in e] == [3.0] * 12
    e, _ = build({"a": AM.RelativeJointPositionActionCfg(joint_names=[".*"], offset=0.5)})
    assert [x[3] for x in e] == [0.0] * 12 and {x[1] for x in e} == {2}
    e, _ = build({"a": AM.RelativeJointPositionActionCfg(joint_names=[".*"], offset=0.5, use_zero_offset=False)})
    assert [x[3] for x in e] == [0.5] * 12
    e, _ = build({"a": AM.JointEffortActionCfg(joint_names=["FL_HAA"], scale=0.1, offset=-0.2, debug_vis=True)})
    assert e[0] == (0, 4, float(F32(0.1)), float(F32(-0.2)), None)
    # clips per regex, rounded to fp32
    e, _ = build({"a": AM.JointPositionActionCfg(joint_names=[".*"], clip={".*_KFE": (-2.1, -0.3), "FL_HAA": (-0.5, 0.5)})})
    assert e[0][4] == (-0.5, 0.5) and e[2][4] == (float(F32(-2.1)), float(F32(-0.3))) and e[1][4] is None and e[3][4] is None
    # the liveness block of the device tests
    e, t = build(AC.mixed_cfg())
    assert [x[0] for x in e] == [0, 1, 2, 4, 3, -1, 5, 6, -1, -1, -1, 7] and list(t) == ["legs", "swing", "spin", "push"]


def test_errors_name_the_term():
    AM = AC._am()
    pos = AM.JointPositionActionCfg
    with pytest.raises(ValueError, match="'b'.*'FL_HAA' is already driven by term 'a'"):
        build({"a": pos(joint_names=["FL_.*"]), "b": AM.JointEffortActionCfg(joint_names=[".*_HAA"])})
    with pytest.raises(ValueError, match="'a'.*empty"):
        build({"a": pos(joint_names=[])})
    with pytest.raises(ValueError, match="'a'.*'nothing' matches no joint"):
        build({"a": pos(joint_names=["FL_.*", "nothing"])})
    with pytest.raises(ValueError, match="'a'.*scale key 'HR_.*' matches no joint of the term"):
        build({"a": pos(joint_names=["FL_.*"], scale={"HR_.*": 0.5})})
    with pytest.raises(ValueError, match="'a'.*offset key 'x' matches no joint"):
        build({"a": pos(joint_names=["FL_.*"], offset={"x": 0.5}, use_default_offset=False)})
    with pytest.raises(ValueError, match="'a'.*clip key 'x' matches no joint"):
        build({"a": pos(joint_names=["FL_.*"], clip={"x": (0, 1)})})
    with pytest.raises(ValueError, match="'a'.*lo 1.0 > hi -1.0"):
        build({"a": pos(joint_names=["FL_.*"], clip={".*": (1.0, -1.0)})})
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="'a'.*finite"):
            build({"a": pos(joint_names=["FL_.*"], scale=bad)})
        with pytest.raises(ValueError, match="'a'.*finite"):
            build({"a": pos(joint_names=["FL_.*"], offset=bad, use_default_offset=False)})
        with pytest.raises(ValueError, match="'a'.*finite"):
            build({"a": pos(joint_names=["FL_.*"], clip={".*": (0.0, bad)})})
    with pytest.raises(ValueError, match="no term"):
        build({})
    with pytest.raises(ValueError, match="no term"):
        build({"a": None})
    with pytest.raises(ValueError, match="'a'.*asset_name 'arm'"):
        build({"a": pos(asset_name="arm", joint_names=[".*"])})
    with pytest.raises(TypeError, match="'a'.*joint action term cfgs"):
        build({"a": types.SimpleNamespace(joint_names=[".*"])})
    # an observation term that names an action term the block does not have
    from cat_envs.shim import ObservationTermCfg as ObsTerm
    from cat_envs.tasks.utils.mdp import observation_manager as OM
    from cat_envs.tasks.utils.mdp import observations as O
    group = {"last": ObsTerm(func=O.last_action, params={"action_name": "spin"})}
    assert [e[0] for e in OM.build_table(group, T.JOINTS, T.DEFAULT_JOINT_POS, action_terms={"legs": (0, 3), "spin": (5, 7)})[0]] == [38, 39]
    assert len(OM.build_table({"last": ObsTerm(func=O.last_action)}, T.JOINTS, T.DEFAULT_JOINT_POS, action_terms={"legs": (0, 3)})[0]) == 3
    assert len(OM.build_table({"last": ObsTerm(func=O.last_action)}, T.JOINTS, T.DEFAULT_JOINT_POS)[0]) == 12
    with pytest.raises(ValueError, match="'last'.*'spin' names no action term"):
        OM.build_table(group, T.JOINTS, T.DEFAULT_JOINT_POS, action_terms={"legs": (0, 3)})


# ------------------------------------------------------------------------------------------ the manager
class _Sim:
    def __init__(self):
        self.table, self.width, self.pushes = None, None, 0

    def set_action_table(self, entries, width):
        self.table, self.width, self.pushes = list(entries), width, self.pushes + 1


def _fake_env(n=5):
    scene = {"robot": types.SimpleNamespace(joint_names=list(T.JOINTS), body_names=list(T.BODIES))}
    return types.SimpleNamespace(scene=scene, sim=_Sim(), num_envs=n, device="cpu")


def test_manager_spec_run_state_and_set_term_cfg():
    import torch
    from cat_envs.tasks.utils.mdp.action_manager import ActionManager
    AM = AC._am()
    env = _fake_env()
    mgr = ActionManager(AC.mixed_cfg(), env)
    entries = build(AC.mixed_cfg())[0]
    assert env.sim.table == entries and env.sim.width == mgr.total_action_dim == 8 and env.sim.pushes == 1
    assert mgr.active_terms == ["legs", "swing", "spin", "push"] and mgr.action_term_dim == [3, 2, 2, 1]
    assert mgr.action.shape == mgr.prev_action.shape == (5, 8) and mgr.action is mgr._action and "HL_HFE" in str(mgr)
    # the history moves as _ActionManager's does
    a = torch.arange(40, dtype=torch.float32).reshape(5, 8)
    mgr.process_action(a)
    mgr.process_action(a + 1)
    assert torch.equal(mgr.prev_action, a) and torch.equal(mgr.action, a + 1)
    mgr.reset(torch.tensor([True, False, False, False, True]))
    assert not mgr.action[[0, 4]].any() and not mgr.prev_action[[0, 4]].any() and torch.equal(mgr.action[1:4], (a + 1)[1:4])
    term = mgr.get_term("spin")
    assert term.action_dim == 2 and term.joint_names == ["HL_HAA", "HL_HFE"] and torch.equal(term.raw_actions, mgr.action[:, 5:7])
    want = mgr.action[:, 5:7] * 10.0
    want[:, 1] = want[:, 1].clamp(-25.0, 22.0)
    assert torch.equal(term.processed_actions, want)
    # spec: one entry per column
    spec = mgr.spec()
    assert spec["action_dim"] == 8 and spec["undriven_joints"] == ["FR_KFE", "HL_KFE", "HR_HAA", "HR_HFE"]
    assert [c["joint"] for c in spec["columns"]] == ["FL_HAA", "FL_HFE", "FL_KFE", "FR_HFE", "FR_HAA", "HL_HAA", "HL_HFE", "HR_KFE"]
    assert spec["columns"][3] == {"column": 3, "term": "swing", "joint": "FR_HFE", "joint_id": 4, "kind": "relative_joint_position",
                                  "scale": 1.0, "offset": 0.0, "clip": [-1.5, 1.5]}
    assert spec["terms"]["push"] == {"kind": "joint_effort", "slice": [7, 8]} and json.loads(json.dumps(spec)) == spec
    # scale, offset and clip bounds move in place; joints, kinds, columns and the clipped set are fixed
    state = mgr.state_dict()
    mgr.set_term_cfg("push", AM.JointEffortActionCfg(joint_names=["HR_KFE"], scale=0.5, offset=0.25, clip={"HR_KFE": (-1.0, 1.0)}))
    assert env.sim.table[11] == (7, 4, 0.5, 0.25, (-1.0, 1.0)) and env.sim.pushes == 2 and mgr.get_term_cfg("push").scale == 0.5
    mgr.set_term_cfg("push", mgr.get_term_cfg("push"))
    assert env.sim.pushes == 2                                                # nothing changed: nothing copied
    for bad in (AM.JointEffortActionCfg(joint_names=["HR_HFE"], clip={".*": (-1.0, 1.0)}),
                AM.JointEffortActionCfg(joint_names=["HR_KFE"]), AM.JointPositionActionCfg(joint_names=["HR_KFE"], clip={".*": (-1.0, 1.0)}),
                AM.JointEffortActionCfg(joint_names=["HR_KFE", "HR_HFE"], clip={"HR_KFE": (-1.0, 1.0)})):
        with pytest.raises(ValueError, match="'push'.*fixed"):
            mgr.set_term_cfg("push", bad)
    with pytest.raises(ValueError, match="'nope' not found"):
        mgr.set_term_cfg("nope", AM.JointEffortActionCfg(joint_names=["HR_KFE"]))
    assert mgr.fingerprint() == ActionManager(AC.mixed_cfg(), _fake_env()).fingerprint()
    assert mgr.fingerprint()[3] == [4, 2, True] and mgr.fingerprint()[5] == [-1, 0, False]
    mgr.load_state_dict(state)
    assert env.sim.table == entries and env.sim.pushes == 3
    other = ActionManager(CC._cfg(AC.TASK).actions, _fake_env())
    assert other.fingerprint() != mgr.fingerprint() and other.total_action_dim == 12
    with pytest.raises(ValueError, match="do not fit"):
        other.check_state_dict(state)
    with pytest.raises(ValueError, match="lacks 'params'"):
        mgr.check_state_dict({})


def test_eval_env_cfg_keeps_the_actions():
    """unlike events and terminations: the policy's output means nothing without the block"""
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    cfg = make_eval_env_cfg(CC._cfg(AC.REFERENCE), 16)
    assert cfg.actions is not None and cfg.events is None and cfg.terminations is None
    assert build(cfg.actions) == build(CC._cfg(AC.REFERENCE).actions)


def test_export_writes_the_output_contract_next_to_the_models(tmp_path):
    from cat_envs.tasks.utils.cleanrl import export as EX
    from cat_envs.tasks.utils.mdp.action_manager import ActionManager
    from oracle import ppo_oracle as PO
    sd = PO.AgentOracle(45, 12).state_dict()
    spec = ActionManager(CC._cfg(AC.REFERENCE).actions, _fake_env()).spec()
    out = EX.export_policy(sd, str(tmp_path / "exported"), action_spec=spec)
    assert sorted(out) == ["actions", "jit", "onnx"] and all(os.path.isfile(p) for p in out.values())
    got = json.load(open(out["actions"]))
    assert got == spec and got["action_dim"] == 12 and got["joint_order"] == T.JOINTS and got["undriven_joints"] == []
    assert [c["joint"] for c in got["columns"]][6:] == ["HR_HAA", "HR_HFE", "HR_KFE", "HL_HAA", "HL_HFE", "HL_KFE"]
    assert got["columns"][6] == {"column": 6, "term": "joint_pos", "joint": "HR_HAA", "joint_id": 9, "kind": "joint_position",
                                 "scale": 0.5, "offset": float(F32(-0.05)), "clip": None}
    plain = EX.export_policy(sd, str(tmp_path / "plain"))                   # without a spec: the two models only, as before
    assert sorted(plain) == ["jit", "onnx"] and not os.path.exists(tmp_path / "plain" / "actions.json")
