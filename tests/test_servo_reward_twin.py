"""The servo task's reward terms without a device ("Rewards"): the descriptor's reward tail, table
building from a ``RewardsCfg``, the numpy twin against a plain recount, the arithmetic of ``pop_log`` and the reward
weight curriculum."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_reward_twin as RT
import servo_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _cfg():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(T.TASK, "env_cfg_entry_point")
    cfg.synthetic.servo_resample_steps = 3
    return cfg


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_tail():
    from cat_envs import native
    assert issubclass(native.ServoSimRewards, native.ServoSimStep)
    assert [f[0] for f in native.ServoSimRewards._fields_] == ["reward_terms", "reward_rec", "reward_table"]
    assert native.ServoSimRewards.reward_terms.offset == ctypes.sizeof(native.ServoSimStep)   # the tail starts where it ended
    assert native.ServoSimRewards.reward_rec.offset % 8 == 0
    d = native.ServoSimRewards()
    assert d.reward_terms == 0 and d.reward_rec is None and d.reward_table is None and d.trace is None
    src = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    pinned = re.search(r"static_assert\(sizeof\(catppo_servo_sim\) == (\d+)", src)
    assert pinned and ctypes.sizeof(native.ServoSimRewards) == int(pinned.group(1))
    assert ctypes.sizeof(native.ServoRewardTerm) == 16
    assert native.SERVO_REWARD_KINDS == RT.KINDS and native.SERVO_REWARD_FLOATS == RT.REC_FLOATS


def test_servo_sim_step_refuses_a_shorter_descriptor():
    from cat_envs import native
    for short in (native.ServoSim(), native.ServoSimStep()):
        with pytest.raises(TypeError, match="ServoSimRewards"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


# ------------------------------------------------------------------------------------------ table building
def _terms():
    from cat_envs.shim import RewardTermCfg as RewTerm
    from cat_envs.shim import SceneEntityCfg
    from cat_envs.tasks.utils.mdp import rewards
    return RewTerm, SceneEntityCfg, rewards


def test_names_map_to_kinds_and_masks():
    RewTerm, SceneEntityCfg, rewards = _terms()
    from cat_envs.tasks.locomotion.velocity.config.solo12 import cat_flat_env_cfg as E
    names, table = rewards.build_table(E.RewardsCfg(), T.JOINTS, 45)
    assert names == ["track_lin_vel_xy_exp", "track_ang_vel_z_exp"]
    assert table == [("track_lin_vel_xy_exp", 1, 0, 1.0, 0.25), ("track_ang_vel_z_exp", 2, 0, 0.5, 0.25)]
    import inspect
    for name in RT.KINDS:
        func = getattr(rewards, name)
        required = [p.name for p in list(inspect.signature(func).parameters.values())[1:] if p.default is p.empty]
        with pytest.raises(TypeError, match="inside the simulator launch"):       # a term is never called
            func(None, **{p: 1.0 for p in required})
        assert len(func.describe(types.SimpleNamespace(scene={}), **{p: 1.0 for p in required})) == 3
    cfg = {"a": RewTerm(func=rewards.joint_deviation_l1, weight=-0.1,
                        params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*_HAA"])}),
           "off": RewTerm(func=rewards.action_l2, weight=0.0),
           "b": RewTerm(func=rewards.joint_torques_l2, weight=-1e-4,
                        params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*_HAA", ".*_HFE", ".*_KFE"])}),
           "c": RewTerm(func=rewards.feet_air_time, weight=0.25,
                        params={"command_name": "base_velocity", "threshold": 0.3, "sensor_cfg": None}),
           "d": RewTerm(func=rewards.track_lin_vel_xy_exp, weight=1.0, params={"command_name": "x", "std": 0.3})}
    names, table = rewards.build_table(cfg, T.JOINTS, 45)
    assert names == ["a", "off", "b", "c", "d"]                              # a zero weight is dropped from the table only
    assert [r[0] for r in table] == ["a", "b", "c", "d"]
    assert table[0][1:3] == (10, (1 << 0) | (1 << 3) | (1 << 6) | (1 << 9)) and table[0][2] == RT.HAA_MASK
    assert table[1][1:3] == (7, 0xFFF)
    assert table[2][1] == 13 and table[2][4] == float(F32(0.3))
    assert table[3][4] == float(F32(0.3 ** 2))                               # param = f32(std ** 2)
    shaped = rewards.build_table(E.ShapedRewardsCfg(), T.JOINTS, 45)[1]
    assert len(shaped) == 9 and [r[1] for r in shaped] == [1, 2, 5, 6, 7, 11, 10, 13, 15]


def test_table_errors():
    RewTerm, SceneEntityCfg, rewards = _terms()
    many = {f"t{i}": RewTerm(func=rewards.action_l2, weight=-0.1 * (i + 1)) for i in range(16)}
    with pytest.raises(ValueError, match="at most 15"):
        rewards.build_table(many, T.JOINTS, 45)
    many["t3"].weight = 0.0                                                  # fifteen non-zero terms fit
    assert len(rewards.build_table(many, T.JOINTS, 45)[1]) == 15
    with pytest.raises(ValueError, match="'mine'.*describe"):
        rewards.build_table({"mine": RewTerm(func=lambda env: 0.0, weight=1.0)}, T.JOINTS, 45)
    with pytest.raises(ValueError, match="obs_dim 44"):
        rewards.build_table({"rate": RewTerm(func=rewards.action_rate_l2, weight=-0.01)}, T.JOINTS, 44)
    assert rewards.build_table({"rate": RewTerm(func=rewards.action_rate_l2, weight=-0.01)}, T.JOINTS, 45)[1][0][1] == 11
    with pytest.raises(ValueError, match="no name matches"):
        rewards.build_table({"x": RewTerm(func=rewards.joint_vel_l2, weight=-1.0,
                                          params={"asset_cfg": SceneEntityCfg("robot", joint_names=["nothing"])})}, T.JOINTS, 45)


def test_tasks_are_registered_and_existing_cfgs_have_no_rewards():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    for task in ("Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-v0", "Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-Play-v0"):
        cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
        assert cfg.synthetic.kind == "servo" and list(cfg.rewards.__dict__) == ["track_lin_vel_xy_exp", "track_ang_vel_z_exp"]
    for task in ("Isaac-Velocity-CaT-Flat-Solo12-v0", T.TASK):
        assert not hasattr(load_cfg_from_registry(task, "env_cfg_entry_point"), "rewards")


# ------------------------------------------------------------------------------------------ the twin
@pytest.fixture(scope="module", params=[1, 17, 64])
def run(request):
    n = request.param
    tw = RT.make_twin(_cfg(), n, RT.ALL_NON_EXP)
    acts, ep0 = RT.recipe(n)
    slabs, rec, values = RT.run_reward_twin(tw, acts, ep0)
    return n, tw, acts, ep0, slabs, rec, values


def test_recipe_has_falls_timeouts_touchdowns_and_every_term(run):
    n, tw, acts, ep0, slabs, rec, values = run
    assert tw.stats["falls"] == {1: 3, 17: 21, 64: 81}[n] and tw.stats["timeouts"] > 0
    assert tw.stats["touch_air"] == {1: 9, 17: 112, 64: 444}[n]
    assert (values != 0).any(axis=(0, 1)).all(), "a configured term is zero in every step"
    assert sorted(k for k, _, _, _ in RT.ALL_NON_EXP) == list(range(3, 17))
    assert len({w for _, _, w, _ in RT.ALL_NON_EXP}) == len(RT.ALL_NON_EXP) and any(w < 0 for _, _, w, _ in RT.ALL_NON_EXP)


def test_reward_is_the_sequential_sum_and_the_rest_of_the_row_is_the_parents(run):
    n, tw, acts, ep0, slabs, rec, values = run
    o = tw.off["reward"][0]
    want = np.zeros(values.shape[:2], F32)
    for k in range(values.shape[2]):
        want = (want + values[:, :, k]).astype(F32)
    np.testing.assert_array_equal(slabs[1:, :, o].view(np.uint32), want.view(np.uint32))
    plain = T.run_twin(T.ServoTwin(n, tw.D, tw.p, RT.SEED, RT.MAX_LEN, tw.dt, tw.dec), acts, ep0)
    keep = np.arange(tw.F) != o
    np.testing.assert_array_equal(slabs[:, :, keep].view(np.uint32), plain[:, :, keep].view(np.uint32))
    assert (slabs[1:, :, o] != plain[1:, :, o]).any()


def test_record_equals_a_plain_recount(run):
    n, tw, acts, ep0, slabs, rec, values = run
    want = RT.recount_record(tw, slabs, values, ep0)
    np.testing.assert_array_equal(rec.view(np.uint32), want.view(np.uint32))
    assert (rec[:, 15] == 0).all() and (rec[:, 31] >= 6).all()
    assert (rec[:, 14] == 0).all() and (rec[:, 30] == 0).all()               # fourteen terms: slot 14 is unused


def test_exp_kinds_use_the_correctly_rounded_exp():
    tw = RT.make_twin(_cfg(), 17, [(1, 0, 1.0, 0.25), (2, 0, 0.5, 0.25)])
    acts, ep0 = RT.recipe(17)
    slabs, rec, values = RT.run_reward_twin(tw, acts, ep0)
    assert (values > 0).all() and (values[:, :, 0] <= tw.step_dt).all()


# ------------------------------------------------------------------------------------------ pop_log, curriculum
def test_pop_log_arithmetic():
    from cat_envs.tasks.utils.mdp import rewards
    rec = np.zeros((3, 32), F32)
    rec[:, 16] = [1.5, 2.5, 0.0]
    rec[:, 17] = [-4.0, 0.0, 1.0]
    rec[:, 31] = [2, 1, 1]
    sums = rec[:, 16:32].astype(np.float64).sum(0)
    log = rewards.fold_log(["a", "zero", "b"], ["a", "b"], sums, 10.0)
    assert log == {"Episode_Reward/a": 4.0 / 4 / 10.0, "Episode_Reward/zero": 0.0, "Episode_Reward/b": -3.0 / 4 / 10.0}
    assert rewards.fold_log(["a"], ["a"], np.zeros(16), 10.0) is None           # no episode ended


def test_modify_reward_weight():
    from cat_envs.shim import RewardTermCfg as RewTerm
    from cat_envs.tasks.utils.cat import curriculums
    from cat_envs.tasks.utils.mdp import rewards
    term = RewTerm(func=rewards.action_rate_l2, weight=-0.01)
    pushed = []
    mgr = types.SimpleNamespace(get_term_cfg=lambda name: term, set_term_cfg=lambda name, cfg: pushed.append((name, cfg.weight)))
    env = types.SimpleNamespace(reward_manager=mgr, common_step_counter=10)
    assert curriculums.modify_reward_weight(env, None, "rate", -0.1, num_steps=10) == -0.01 and not pushed   # not yet: > num_steps
    env.common_step_counter = 11
    assert curriculums.modify_reward_weight(env, None, "rate", -0.1, num_steps=10) == -0.1
    assert pushed == [("rate", -0.1)]
    assert curriculums.modify_reward_weight(env, None, "rate", -0.1, num_steps=10) == -0.1 and len(pushed) == 1
