"""The servo task's robot cfg without a device ("Actuators"): the cfg classes, the asset, ``build_table`` on the
reference's robot, on regex dicts and on several groups, every error that names the actuator group, ``.replace`` and the list
of inert fields."""
import copy
import json

import numpy as np
import pytest

import servo_twin as T
import test_servo_commands_twin as CC

F32 = np.float32
TASKS = ("Actuators", "Reference-Actuators", "DelayedActuators")


def _um():
    from cat_envs.tasks.utils.mdp import actuators as UM
    return UM


def _shim():
    import cat_envs.shim as S
    return S


def _syn():
    return CC._cfg(T.TASK).synthetic


def build(robot, decimation=4):
    return _um().build_table(robot, T.JOINTS, _syn(), decimation, T.DEFAULT_JOINT_POS)


def robot_of(groups, **kw):
    from cat_envs.assets.odri import SOLO12_CFG
    return SOLO12_CFG.replace(actuators=groups, **kw)


def test_cfg_classes_and_asset():
    S = _shim()
    from cat_envs.assets import SOLO12_CFG, SOLO12_MINIMAL_CFG
    from cat_envs.assets.odri import SOLO12_CFG as again
    assert again is SOLO12_CFG and SOLO12_MINIMAL_CFG is not SOLO12_CFG
    assert issubclass(S.DCMotorCfg, S.IdealPDActuatorCfg) and issubclass(S.DelayedPDActuatorCfg, S.IdealPDActuatorCfg)
    assert not issubclass(S.ImplicitActuatorCfg, S.IdealPDActuatorCfg)
    legs = SOLO12_CFG.actuators["legs"]
    assert isinstance(legs, S.IdealPDActuatorCfg) and list(SOLO12_CFG.actuators) == ["legs"]
    assert legs.stiffness == {".*": 4.0} and legs.damping == {".*": 0.2} and legs.armature == 0.00036207
    assert legs.effort_limit == 10.0 and legs.velocity_limit == 100.0 and sorted(legs.joint_names_expr) == sorted(T.JOINTS)
    assert [SOLO12_CFG.init_state.joint_pos[j] for j in T.JOINTS] == [float(v) for v in T.DEFAULT_JOINT_POS.astype(np.float64).round(6)]
    assert SOLO12_CFG.init_state.joint_vel == {".*": 0.0}
    d = S.DelayedPDActuatorCfg(joint_names_expr=[".*"], stiffness=1.0, damping=0.1)
    assert (d.min_delay, d.max_delay) == (0, 0)
    # .replace and .copy give objects of their own
    other = SOLO12_CFG.replace(soft_joint_pos_limit_factor=0.9)
    assert other.soft_joint_pos_limit_factor == 0.9 and SOLO12_CFG.soft_joint_pos_limit_factor == 1.0
    dup = SOLO12_CFG.copy()
    dup.actuators["legs"].stiffness[".*"] = 7.0
    assert SOLO12_CFG.actuators["legs"].stiffness == {".*": 4.0}


def test_table_of_the_reference_robot_and_of_the_tasks():
    from cat_envs.assets import SOLO12_MINIMAL_CFG
    entries, spec = build(SOLO12_MINIMAL_CFG)
    syn = _syn()
    inertia = float(F32(syn.servo_inertia) + F32(0.00036207))
    assert entries == [dict(kp=4.0, kd=float(F32(0.2)), inertia=inertia, effort_limit=10.0, saturation_effort=0.0,
                            velocity_limit=100.0, dc_motor=False, min_delay=0, max_delay=0, group=0)] * 12
    assert spec["groups"] == {"legs": dict(kind="ideal_pd", index=0, joint_ids=list(range(12)), joints=T.JOINTS, min_delay=0,
                                           max_delay=0)}
    assert [j["joint"] for j in spec["joints"]] == T.JOINTS and spec["joints"][3]["stiffness"] == 4.0
    assert spec["joints"][0]["velocity_limit"] is None and spec["delay_unit"] == "physics steps"
    json.dumps(spec)
    for name in TASKS:
        for suffix in ("", "-Play"):
            cfg = CC._cfg(f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{name}{suffix}-v0")
            got, sp = build(cfg.scene.robot, cfg.decimation)
            lag = (0, 4) if name == "DelayedActuators" else (0, 0)
            assert [(e["min_delay"], e["max_delay"]) for e in got] == [lag] * 12
            assert [{k: v for k, v in e.items() if "delay" not in k} for e in got] == \
                [{k: v for k, v in e.items() if "delay" not in k} for e in entries]
            assert sp["groups"]["legs"]["kind"] == ("delayed_pd" if name == "DelayedActuators" else "ideal_pd")
            assert (cfg.actions is not None if hasattr(cfg, "actions") else False) == (name == "Reference-Actuators")
    # an existing task has no robot and keeps its scene
    assert CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Actions-v0").scene.robot is None


def test_regex_dicts_several_groups_and_every_kind():
    S = _shim()
    robot = robot_of({
        "late": S.DelayedPDActuatorCfg(joint_names_expr=["HR_.*"], stiffness=4.0, damping=0.2, armature=0.02, effort_limit=3.0,
                                       min_delay=0, max_delay=12),
        "front": S.IdealPDActuatorCfg(joint_names_expr=["FL_.*", "FR_.*"], stiffness={".*_HAA": 2.0, ".*_HFE": 4.0, "FL_KFE": 6.0,
                                                                                       "FR_KFE": 0.0},
                                      damping={".*_HAA": 0.1, ".*_HFE": 0.15, ".*_KFE": 0.2}, armature={".*_KFE": 0.01}),
        "motor": S.DCMotorCfg(joint_names_expr=["HL_HAA", "HL_HFE"], stiffness=4.0, damping=0.2, effort_limit=3.0,
                              saturation_effort=4.0, velocity_limit=12.0),
        "knee": S.ImplicitActuatorCfg(joint_names_expr=["HL_KFE"], stiffness=1.0, damping=0.0, friction=0.0),
    })
    entries, spec = build(robot)
    syn = _syn()
    assert [e["group"] for e in entries] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 0, 0, 0]
    assert [e["kp"] for e in entries[:6]] == [2.0, 4.0, 6.0, 2.0, 4.0, 0.0]
    assert [e["kd"] for e in entries[:3]] == [float(F32(0.1)), float(F32(0.15)), float(F32(0.2))]
    assert entries[2]["inertia"] == float(F32(syn.servo_inertia) + F32(0.01)) and entries[1]["inertia"] == float(F32(syn.servo_inertia))
    assert entries[0]["effort_limit"] == float(F32(syn.servo_tau_max))           # not set: the simulator's own limit
    assert [e["dc_motor"] for e in entries] == [False] * 6 + [True, True] + [False] * 4
    assert entries[6]["saturation_effort"] == 4.0 and entries[6]["velocity_limit"] == 12.0
    assert [(e["min_delay"], e["max_delay"]) for e in entries[9:]] == [(0, 12)] * 3 and entries[8]["max_delay"] == 0
    assert {n: g["kind"] for n, g in spec["groups"].items()} == {"late": "delayed_pd", "front": "ideal_pd", "motor": "dc_motor",
                                                                 "knee": "implicit"}
    assert spec["groups"]["motor"]["joints"] == ["HL_HAA", "HL_HFE"] and spec["joints"][6]["velocity_limit"] == 12.0
    assert build(robot, decimation=8)[0] == entries                           # a longer control step admits the lag, too


def test_errors_name_the_group():
    S = _shim()
    pd = lambda names, **kw: S.IdealPDActuatorCfg(joint_names_expr=names, **{**dict(stiffness=4.0, damping=0.2), **kw})   # noqa: E731
    with pytest.raises(ValueError, match="'b'.*'FL_HAA' already belongs to group 'a'"):
        build(robot_of({"a": pd(["F.*"]), "b": pd(["FL_HAA", "H.*"])}))
    with pytest.raises(ValueError, match="'HR_KFE' belongs to no actuator group"):
        build(robot_of({"a": pd(["F.*", "HL_.*", "HR_HAA", "HR_HFE"])}))
    with pytest.raises(ValueError, match="'a'.*joint_names_expr entry 'XX_.*' matches no joint"):
        build(robot_of({"a": pd([".*", "XX_.*"])}))
    with pytest.raises(ValueError, match="'a'.*stiffness key 'nope' matches no joint"):
        build(robot_of({"a": pd([".*"], stiffness={".*": 1.0, "nope": 2.0})}))
    with pytest.raises(ValueError, match="'a'.*damping key 'H.*' matches no joint of the group"):
        build(robot_of({"a": pd(["F.*"], damping={"H.*": 1.0}), "b": pd(["H.*"])}))
    for field, bad in (("stiffness", float("nan")), ("damping", -0.1), ("armature", float("inf")), ("effort_limit", -1.0),
                       ("velocity_limit", float("nan")), ("stiffness", {".*_KFE": -2.0})):
        with pytest.raises(ValueError, match=f"'a'.*{field}.*finite and >= 0"):
            build(robot_of({"a": pd([".*"], **{field: bad})}))
    with pytest.raises(ValueError, match="'a'.*friction must be 0 or None"):
        build(robot_of({"a": pd([".*"], friction=0.01)}))
    late = lambda lo, hi: S.DelayedPDActuatorCfg(joint_names_expr=[".*"], stiffness=4.0, damping=0.2, min_delay=lo, max_delay=hi)   # noqa: E731
    with pytest.raises(ValueError, match="'late'.*min_delay 5 > max_delay 4"):
        build(robot_of({"late": late(5, 4)}))
    with pytest.raises(ValueError, match=r"'late'.*max_delay 13 > 3 \* decimation = 12"):
        build(robot_of({"late": late(0, 13)}))
    assert build(robot_of({"late": late(12, 12)}))[0][0]["min_delay"] == 12
    with pytest.raises(ValueError, match=r"'late'.*max_delay 7 > 3 \* decimation = 6"):
        build(robot_of({"late": late(0, 7)}), decimation=2)
    motor = lambda **kw: S.DCMotorCfg(joint_names_expr=[".*"], stiffness=4.0, damping=0.2, **kw)   # noqa: E731
    for kw in (dict(saturation_effort=4.0), dict(saturation_effort=4.0, velocity_limit=0.0), dict(velocity_limit=12.0),
               dict(saturation_effort=0.0, velocity_limit=12.0), dict(saturation_effort=4.0, velocity_limit={"FL_.*": 12.0})):
        with pytest.raises(ValueError, match="'m'.*DCMotorCfg needs a positive velocity_limit and saturation_effort"):
            build(robot_of({"m": motor(**kw)}))
    from cat_envs.assets import SOLO12_CFG
    moved = copy.deepcopy(SOLO12_CFG)
    moved.init_state.joint_pos["HL_KFE"] = -1.0
    with pytest.raises(ValueError, match="'legs'.*init_state.joint_pos of joint 'HL_KFE' is -1.0.*default pose"):
        build(moved)
    with pytest.raises(TypeError, match="'a' is not one of the actuator cfgs"):
        build(robot_of({"a": {"stiffness": 1.0}}))
    with pytest.raises(ValueError, match="no actuators"):
        build(robot_of({}))


def test_inert_fields_are_listed():
    S = _shim()
    from cat_envs.assets import SOLO12_CFG
    robot = SOLO12_CFG.replace(prim_path="{ENV_REGEX_NS}/Robot", spawn={"usd_path": "solo12.usd", "rigid_props": {"disable_gravity": False}})
    robot.actuators["legs"].effort_limit_sim = 12.0
    entries, spec = build(robot)
    assert entries == build(SOLO12_CFG)[0]                                    # they change nothing
    assert spec["inert"] == ["prim_path", "spawn", "init_state.pos", "init_state.rot", "init_state.lin_vel", "init_state.ang_vel",
                             "actuators.legs.effort_limit_sim", "actuators.legs.velocity_limit"]
    dc = robot_of({"m": S.DCMotorCfg(joint_names_expr=[".*"], stiffness=4.0, damping=0.2, saturation_effort=4.0, velocity_limit=12.0)})
    assert "actuators.m.velocity_limit" not in build(dc)[1]["inert"]          # a DC motor reads it


def test_eval_env_cfg_keeps_the_robot_and_export_adds_the_actuators(tmp_path):
    """like cfg.actions: the robot is what the policy was trained against"""
    import os

    from cat_envs.tasks.utils.cleanrl import export as EX
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    from oracle import ppo_oracle as PO
    task = "Isaac-Velocity-CaT-Flat-Solo12-Servo-DelayedActuators-v0"
    cfg = make_eval_env_cfg(CC._cfg(task), 16)
    assert cfg.scene.robot is not None and cfg.scene.num_envs == 16
    entries, spec = build(cfg.scene.robot, cfg.decimation)
    assert entries == build(CC._cfg(task).scene.robot)[0]
    sd = PO.AgentOracle(45, 12).state_dict()
    out = EX.export_policy(sd, str(tmp_path / "exported"), actuator_spec=spec)
    assert sorted(out) == ["actions", "jit", "onnx"] and all(os.path.isfile(p) for p in out.values())
    got = json.load(open(out["actions"]))
    assert list(got) == ["actuators"] and got["actuators"] == spec
    assert got["actuators"]["groups"]["legs"]["max_delay"] == 4 and got["actuators"]["joints"][0]["stiffness"] == 4.0
    both = EX.export_policy(sd, str(tmp_path / "both"), action_spec={"action_dim": 12}, actuator_spec=spec)
    assert json.load(open(both["actions"])) == {"action_dim": 12, "actuators": spec}
    plain = EX.export_policy(sd, str(tmp_path / "plain"))                   # without a spec: the two models only, as before
    assert sorted(plain) == ["jit", "onnx"] and not os.path.exists(tmp_path / "plain" / "actions.json")
