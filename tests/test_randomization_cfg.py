"""The servo task's randomisation cfg without a device ("Randomisation"): the three event terms,
``build_randomization`` for each operation, mask and mode, every error that names the term, the stability bound at a corner
just above and just below ``2 a + b = 4``, the pack layout against ``native``, ``build_block`` unchanged for the reference's
``EventCfg``, the tasks, and what ``actions.json`` says."""
import json

import numpy as np
import pytest

import servo_randomize_twin as ZT
import servo_twin as T
import test_servo_commands_twin as CC

F32 = np.float32
DT, DEC = 0.005, 4
TASKS = ("Randomized", "Reference-Randomized")


def _mods():
    from cat_envs.shim import EventTermCfg, SceneEntityCfg
    from cat_envs.tasks.utils.mdp import event_manager as EM
    from cat_envs.tasks.utils.mdp import events as EV
    from cat_envs.tasks.utils.mdp import randomization as RZ
    return RZ, EM, EV, EventTermCfg, SceneEntityCfg


def _syn():
    return CC._cfg(T.TASK).synthetic


def _robot():
    from cat_envs.assets.odri import SOLO12_MINIMAL_CFG
    from cat_envs.tasks.utils.mdp import actuators as UM
    entries = UM.build_table(SOLO12_MINIMAL_CFG, T.JOINTS, _syn(), DEC, T.DEFAULT_JOINT_POS)[0]
    return entries, UM.armatures(SOLO12_MINIMAL_CFG, T.JOINTS)


def gains(mode="startup", joints=".*", **params):
    RZ, EM, EV, Term, Entity = _mods()
    return Term(func=EV.randomize_actuator_gains, mode=mode, params={"asset_cfg": Entity("robot", joint_names=joints), **params})


def joint(mode="reset", joints=".*", **params):
    RZ, EM, EV, Term, Entity = _mods()
    return Term(func=EV.randomize_joint_parameters, mode=mode, params={"asset_cfg": Entity("robot", joint_names=joints), **params})


def mass(mode="startup", bodies="base_link", **params):
    RZ, EM, EV, Term, Entity = _mods()
    return Term(func=EV.randomize_rigid_body_mass, mode=mode, params={"asset_cfg": Entity("robot", body_names=bodies), **params})


def build(cfg, entries="robot", dt=DT):
    ent, arm = _robot()
    if entries == "robot":
        return _mods()[0].build_randomization(cfg, ent, T.JOINTS, _syn(), dt, DEC, armatures=arm)
    return _mods()[0].build_randomization(cfg, entries, T.JOINTS, _syn(), dt, DEC)


def test_block_values_for_each_operation_mask_and_mode():
    RZ = _mods()[0]
    from cat_envs import native
    FL, OP = native.SERVO_RANDOMIZE_FLAGS, native.SERVO_RANDOMIZE_OPS
    cfg = {"g": gains(stiffness_distribution_params=(0.8, 1.2), operation="scale", joints=[".*_HAA", "FL_KFE"]),
           "j": joint(friction_distribution_params=(0.0, 0.05), armature_distribution_params=(0.0, 0.001), operation="add",
                      joints="H.*"),
           "m": mass(mode="reset", mass_distribution_params=(1.5, 3.0), operation="abs", recompute_inertia=False)}
    block, spec = build(cfg)
    assert block["flags"] == FL["stiffness"] | FL["friction"] | FL["armature"] | FL["mass"] | FL["joint_reset"] | FL["mass_reset"]
    assert block["ops"] == OP["scale"] | OP["add"] << 8 | OP["abs"] << 16
    assert block["masks"] == [0b001001001101, 0b111111000000, 1]
    assert block["ranges"]["stiffness"] == (float(F32(0.8)), float(F32(1.2 - 0.8))) and block["ranges"]["damping"] == (0.0, 0.0)
    assert block["ranges"]["mass"] == (1.5, 1.5) and block["ranges"]["armature"] == (0.0, float(F32(0.001)))
    assert block["m0"] == float(F32(25.0 / 9.81)) and block["g"] == float(F32(9.81)) and block["servo_inertia"] == float(F32(0.004))
    assert block["armatures"] == [float(F32(0.00036207))] * 12
    assert block["terms"] == {"startup": ["g"], "reset": ["j", "m"]} and block["inert"] == ["m.recompute_inertia"]
    assert spec["terms"]["g"]["joints"] == ["FL_HAA", "FL_KFE", "FR_HAA", "HL_HAA", "HR_HAA"] and spec["terms"]["m"]["joints"] == ["base_link"]
    assert spec["terms"]["j"]["ranges"] == {"friction": [0.0, 0.05], "armature": [0.0, 0.001]} and spec["terms"]["j"]["mode"] == "reset"
    json.dumps(spec)
    # either mode for each func; damping alone; the default selection is every joint
    block, _ = build({"g": gains(mode="reset", damping_distribution_params=(0.1, 0.3), operation="abs", joints=None)})
    assert block["flags"] == FL["damping"] | FL["gains_reset"] and block["ops"] == OP["abs"] and block["masks"] == [0xFFF, 0, 0]
    block, _ = build({"j": joint(mode="startup", friction_distribution_params=(0.0, 0.1))})
    assert block["flags"] == FL["friction"] and block["ops"] == OP["abs"] << 8
    assert build({"push": CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Events-v0").events.push_robot}) == (None, None)
    # without a robot: the simulator's own scalars, no armature
    block, _ = build({"g": gains(stiffness_distribution_params=(0.5, 2.0), operation="scale")}, entries=None)
    assert block["armatures"] == [0.0] * 12


def test_pack_layout_against_native_and_the_twin():
    RZ = _mods()[0]
    from cat_envs import native
    cfg = CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Randomized-v0")
    block, _ = build(cfg.events)
    words = RZ.pack(block)
    assert words.shape == (native.SERVO_RANDOMIZE_FLOATS,) and words.dtype == np.float32 and native.SERVO_RANDOMIZE_WORDS == ZT.WORDS
    params = T.params_from_cfg(cfg.synthetic)
    twin = ZT.block(params, stiffness=(0.8, 1.2), damping=(0.8, 1.2), friction=(0.0, 0.05), mass=(-0.5, 1.0), gains_op="scale",
                    joint_op="abs", mass_op="add", joint_reset=True, armatures=[0.00036207] * 12)
    np.testing.assert_array_equal(words.view(np.uint32), twin.view(np.uint32))
    off = RZ.pack(block, enabled=False)
    assert int(off.view(np.int32)[0]) == int(words.view(np.int32)[0]) & ~1 and (off[1:].view(np.uint32) == words[1:].view(np.uint32)).all()
    assert words[5] == 0 and words[19] == 0


def test_errors_name_the_term():
    cases = [
        ({"g": gains(stiffness_distribution_params=(0.8, 1.2), distribution="log_uniform")}, "'g'.*'log_uniform' is not supported"),
        ({"g": gains(stiffness_distribution_params=(0.8, 1.2), distribution="gaussian")}, "'g'.*'gaussian' is not supported"),
        ({"g": gains(stiffness_distribution_params=(0.8, 1.2), operation="mul")}, "'g'.*unknown operation 'mul'"),
        ({"g": gains(stiffness_distribution_params=(1.2, 0.8))}, "'g'.*stiffness_distribution_params.*lo <= hi"),
        ({"g": gains()}, "'g'.*randomises nothing"),
        ({"g": gains(stiffness_distribution_params=(0.8, 1.2), joints="XX_.*")}, "'g'.*match no joint"),
        ({"g": gains(mode="interval", stiffness_distribution_params=(0.8, 1.2))}, "'g'.*'startup' or 'reset' event"),
        ({"g": gains(stiffness_distribution_params=(0.8, 1.2)), "h": gains(damping_distribution_params=(0.8, 1.2))},
         "'h'.*a second randomize_actuator_gains term.*'g'"),
        ({"j": joint(friction_distribution_params=(0.5, 1.5), operation="scale")}, "'j'.*'scale'.*0 stays 0"),
        ({"j": joint(friction_distribution_params=(0.0, 0.1), lower_limit_distribution_params=(0.9, 1.0))}, "'j'.*no joint limits"),
        ({"j": joint(friction_distribution_params=(0.0, 0.1), upper_limit_distribution_params=(0.9, 1.0))}, "'j'.*no joint limits"),
        ({"j": joint(friction_distribution_params=(-0.1, 0.1))}, "'j'.*friction of joint 0 can become -0.1 < 0"),
        ({"j": joint(armature_distribution_params=(-0.001, 0.001), operation="add")}, "'j'.*armature of joint 0 can become"),
        ({"g": gains(damping_distribution_params=(-0.5, 0.5), operation="add")}, "'g'.*damping of joint 0 can become"),
        ({"m": mass(mass_distribution_params=(-3.0, 1.0), operation="add")}, "'m'.*mass can become"),
        ({"m": mass(mass_distribution_params=(0.0, 1.0), operation="scale")}, "'m'.*mass can become 0 <= 0"),
        ({"m": mass(mass_distribution_params=(0.5, 1.0), bodies=".*_FOOT")}, "'m'.*must match 'base_link'"),
        ({"m": mass()}, "'m'.*mass_distribution_params is required"),
    ]
    for cfg, what in cases:
        with pytest.raises(ValueError, match=what):
            build(cfg)
    assert build({"m": mass(mass_distribution_params=(0.5, 1.0), bodies=[".*"])})[0]["masks"][2] == 1
    RZ, EM, EV, Term, Entity = _mods()
    for func in (EV.randomize_actuator_gains, EV.randomize_joint_parameters, EV.randomize_rigid_body_mass):
        with pytest.raises(TypeError, match="evaluates events inside the simulator launch"):
            func(None, None, None, (0.5, 1.0))


def test_stability_is_refused_just_above_the_bound_and_accepted_just_below():
    """2 a + b = (2 kd dt + kp dt^2) / I at the largest kp, the largest kd and the smallest I of the ranges"""
    I, kp = float(F32(0.004)), 3.0
    entries = [dict(kp=kp, kd=0.2, inertia=I)] * 12
    edge = (4.0 * I - kp * DT * DT) / (2.0 * DT)                              # the damping at which 2 a + b = 4
    ok = {"g": gains(damping_distribution_params=(0.1, edge * 0.999), operation="abs")}
    bad = {"g": gains(damping_distribution_params=(0.1, edge * 1.001), operation="abs")}
    assert build(ok, entries=entries)[0] is not None
    with pytest.raises(ValueError, match="'g'.*unstable at the worst corner.*2 a \\+ b = 4.0"):
        build(bad, entries=entries)
    # the smallest inertia counts: an absolute armature range that reaches 0 brings the reference's robot to I = 0.004
    ent, arm = _robot()
    stiff = (4.0 * I - 2.0 * float(F32(0.2)) * DT) / (DT * DT)                # kp at the bound with I = servo_inertia
    cfg = lambda s: {"g": gains(stiffness_distribution_params=(1.0, s), operation="abs"),    # noqa: E731
                     "j": joint(armature_distribution_params=(0.0, 0.001), operation="abs")}
    assert build(cfg(stiff * 0.999))[0] is not None
    with pytest.raises(ValueError, match="unstable at the worst corner"):
        build(cfg(stiff * 1.001))
    assert build({"g": gains(stiffness_distribution_params=(1.0, stiff * 1.001), operation="abs")})[0] is not None   # I = 0.00436207
    # an unselected joint is judged on the table's gains
    assert build({"g": gains(damping_distribution_params=(0.1, edge * 1.001), operation="abs", joints="FL_.*")},
                 entries=[dict(kp=kp, kd=0.2, inertia=I if j >= 3 else 2 * I) for j in range(12)])[0] is not None


def test_build_block_is_unchanged_for_the_reference_event_cfg_and_lists_the_new_terms():
    RZ, EM, EV, Term, Entity = _mods()
    from cat_envs import native
    ref = CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Actuators-v0")
    rnd = CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Randomized-v0")
    a = EM.build_block(ref.events, ref.sim.dt, ref.episode_length_s)
    b = EM.build_block(rnd.events, rnd.sim.dt, rnd.episode_length_s)
    assert sorted(a) == ["flags", "inert", "kinds", "num_buckets", "p", "ranges", "terms"] and "spec" not in a
    assert a["flags"] == b["flags"] == 1 | 2 | 8 | 16 and a["ranges"] == b["ranges"] and a["p"] == b["p"]
    np.testing.assert_array_equal(EM.pack(a).view(np.uint32), EM.pack(b).view(np.uint32))
    assert b["terms"]["startup"] == a["terms"]["startup"] + ["actuator_gains", "add_base_mass"]
    assert b["terms"]["reset"] == a["terms"]["reset"] + ["joint_parameters"] and b["terms"]["interval"] == ["push_robot"]
    assert b["inert"] == a["inert"] + ["add_base_mass.recompute_inertia"]
    assert RZ.split_events(rnd.events) == (list(a["kinds"]), ["actuator_gains", "joint_parameters", "add_base_mass"])
    assert RZ.split_events(ref.events) == (list(a["kinds"]), []) and RZ.split_events(None) == ([], [])
    assert build(ref.events) == (None, None)
    only = CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Randomized-v0")
    c = EM.build_block(only.events, only.sim.dt, only.episode_length_s)
    assert c["flags"] == 0 and set(c["kinds"].values()) == set(EM.RANDOMIZE_KINDS) and RZ.split_events(only.events)[0] == []
    assert len(native.EXPORTS) == 59


def test_tasks_eval_cfg_and_export(tmp_path):
    import os

    from cat_envs.tasks.utils.cleanrl import export as EX
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    from oracle import ppo_oracle as PO
    for name in TASKS:
        for suffix in ("", "-Play"):
            cfg = CC._cfg(f"Isaac-Velocity-CaT-Flat-Solo12-Servo-{name}{suffix}-v0")
            block, spec = build(cfg.events, dt=cfg.sim.dt)
            assert sorted(spec["terms"]) == ["actuator_gains", "add_base_mass", "joint_parameters"] and cfg.scene.robot is not None
            assert spec["terms"]["actuator_gains"]["ranges"] == {"stiffness": [0.8, 1.2], "damping": [0.8, 1.2]}
            assert spec["terms"]["joint_parameters"]["ranges"] == {"friction": [0.0, 0.05], "armature": None}
            assert spec["terms"]["add_base_mass"]["ranges"] == {"mass": [-0.5, 1.0]} and spec["terms"]["add_base_mass"]["operation"] == "add"
            assert [spec["terms"][n]["mode"] for n in ("actuator_gains", "joint_parameters", "add_base_mass")] == ["startup", "reset", "startup"]
            if suffix:
                assert cfg.pushes is False and cfg.scene.num_envs == 50
    # existing tasks keep their cfg; the evaluator's env drops the events, so Eval/* is measured on the nominal robot
    assert not hasattr(CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Actuators-v0"), "events")
    ecfg = make_eval_env_cfg(CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Randomized-v0"), 16)
    assert ecfg.events is None and ecfg.scene.robot is not None
    sd = PO.AgentOracle(45, 12).state_dict()
    _, spec = build(CC._cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Randomized-v0").events)
    out = EX.export_policy(sd, str(tmp_path / "exported"), actuator_spec={"groups": {}}, randomization_spec=spec)
    got = json.load(open(out["actions"]))
    assert got == {"actuators": {"groups": {}, "randomization": spec}}
    alone = EX.export_policy(sd, str(tmp_path / "alone"), randomization_spec=spec)
    assert json.load(open(alone["actions"])) == {"actuators": {"randomization": spec}}
    plain = EX.export_policy(sd, str(tmp_path / "plain"))
    assert sorted(plain) == ["jit", "onnx"] and not os.path.exists(tmp_path / "plain" / "actions.json")
