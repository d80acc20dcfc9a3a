"""The servo task's events without a device ("Events"): the event descriptor, block building from an
``EventCfg``, the errors that name the term, properties of the numpy twin and ``push_recovery`` on a hand-made trace."""
import copy
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import servo_events_twin as ET
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Events-v0"
N, STEPS, MAX_LEN, P = 64, 40, 12, 0.25


def _cfg(task=TASK):
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.synthetic.servo_resample_steps = 3
    return cfg


def _em():
    from cat_envs.shim import EventTermCfg as EventTerm
    from cat_envs.tasks.utils.mdp import event_manager as EM
    from cat_envs.tasks.utils.mdp import events as EV
    return EM, EV, EventTerm


def recipe(n, steps=STEPS, scale=2.0):
    rs = np.random.RandomState(3)
    return (rs.standard_normal((steps, n, 12)) * scale).astype(F32), rs.randint(0, MAX_LEN, n)


#: all four kinds: pushes with p = 0.25, the reference's scale reset, a root reset with velocities, 100 friction buckets
ALL = dict(flags=ET.PUSH | ET.JOINT_SCALE | ET.ROOT | ET.FRICTION, p=P, num_buckets=100,
           push=[(-0.5, 0.5), (-0.5, 0.5), (0.0, 0.0), (-20.0, 20.0), (-20.0, 20.0)], joint_pos=[(0.95, 1.05)],
           root_pos=[(-0.05, 0.05)] * 2, root_vel=[(-0.1, 0.1), (-0.1, 0.1), (-0.2, 0.2)], friction=[(0.5, 1.25)])


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoEvents._fields_] == ["block", "floats", "reserved"]
    assert ctypes.sizeof(native.ServoEvents) == 16 and native.ServoEvents.floats.offset == 8
    assert issubclass(native.ServoSimEvents, native.ServoSimObs) and ctypes.sizeof(native.ServoSimObs) == 384
    assert native.ServoSimEvents.obs.offset == 368 and native.ServoSimEvents.ev.offset == 384
    assert ctypes.sizeof(native.ServoSimEvents) == 400
    # the header's static_assert states the same numbers
    hip = open(os.path.join(ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim.hip")).read()
    m = re.search(r"offsetof\(catppo_servo_sim_events, obs\) == (\d+) && offsetof\(catppo_servo_sim_events, ev\) == (\d+) &&\s*"
                  r"sizeof\(catppo_servo_events\) == (\d+) && sizeof\(catppo_servo_sim_events\) == (\d+) && "
                  r"CATPPO_SERVO_EVENT_FLOATS == (\d+)", hip)
    assert [int(x) for x in m.groups()] == [368, 384, 16, 400, native.SERVO_EVENT_FLOATS]
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_EVENTS (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_EVENTS
    assert native.SERVO_EXT_EVENTS not in (0, native.SERVO_EXT_OBS)
    assert int(re.search(r"#define CATPPO_SERVO_EVENT_FLOATS (\d+)", src).group(1)) == native.SERVO_EVENT_FLOATS == ET.FLOATS
    assert native.SERVO_EVENT_FLOATS % 16 == 0
    for name, bit in (("PUSH", ET.PUSH), ("JOINT_SCALE", ET.JOINT_SCALE), ("JOINT_OFFSET", ET.JOINT_OFFSET), ("ROOT", ET.ROOT),
                      ("FRICTION", ET.FRICTION)):
        assert int(re.search(rf"#define CATPPO_SERVO_EVENT_{name} (\d+)u", src).group(1)) == bit == getattr(native, "SERVO_EVENT_" + name)
    assert native.SERVO_EVENT_WORDS == ET.WORDS
    assert native.SERVO_TRACE_PUSHED == ET.TRACE_PUSHED == 14
    assert [f for f in native.SERVO_TRACE_FIELDS if f[0] == "zero"] == [("zero", 14, 2)]          # pinned elsewhere, unchanged
    tags = {ET.TAG_PUSH, ET.TAG_JVEL, ET.TAG_ROOT, ET.TAG_FRIC, T.TAG_COMMAND, T.TAG_INIT, OT.TAG_OBS}
    assert len(tags) == 7
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_descriptor_without_the_event_tail():
    from cat_envs import native
    for short in (native.ServoSimRewards(), native.ServoSimObs()):
        short.reserved = native.SERVO_EXT_EVENTS
        with pytest.raises(TypeError, match="ServoSimObs|ServoSimEvents"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)


# ------------------------------------------------------------------------------------------ block building
def test_reference_cfg_builds_the_reference_block():
    EM = _em()[0]
    cfg = _cfg()
    before = copy.deepcopy(cfg.events)
    b = EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s)
    again = EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s)
    assert b == again and repr(vars(before)) == repr(vars(cfg.events))       # pure: same result, cfg untouched
    assert b["p"] == float(F32(0.00025)) == float(F32(cfg.sim.dt / (2 * cfg.episode_length_s)))
    assert b["flags"] == ET.PUSH | ET.JOINT_SCALE | ET.ROOT | ET.FRICTION and b["num_buckets"] == 100
    f = lambda x: float(F32(x))                                               # noqa: E731
    assert b["ranges"]["friction"] == [(0.5, 0.75)]                           # (0.5, 1.25)
    assert b["ranges"]["joint_pos"] == [(f(0.95), f(1.05 - 0.95))] and b["ranges"]["joint_vel"] == [(0.0, 0.0)]
    assert b["ranges"]["push"] == [(-0.5, 1.0), (-0.5, 1.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0)]    # the yaw rate is zeroed
    assert b["ranges"]["root_pos"] == [(f(-0.05), f(0.1))] * 2
    assert all(w == 0.0 for _, w in b["ranges"]["root_vel"])
    assert b["terms"] == {"startup": ["physics_material"], "reset": ["reset_base", "reset_robot_joints"], "interval": ["push_robot"]}
    assert set(b["inert"]) == {"physics_material.dynamic_friction_range", "physics_material.restitution_range",
                               "reset_base.pose_range.yaw", "reset_robot_joints.velocity_range"}
    words = EM.pack(b)
    np.testing.assert_array_equal(words.view(U32), ET.block(
        flags=b["flags"], p=0.00025, num_buckets=100, push=[(-0.5, 0.5), (-0.5, 0.5), (0, 0), (0, 0), (0, 0)],
        joint_pos=[(0.95, 1.05)], root_pos=[(-0.05, 0.05)] * 2, root_vel=[(-0.0, 0.0)] * 3, friction=[(0.5, 1.25)]).view(U32))
    off = EM.pack(b, interval_enabled=False)
    assert off.view(np.int32)[0] == b["flags"] & ~ET.PUSH and (off[1:].view(U32) == words[1:].view(U32)).all()
    # the play cfgs keep reset and startup terms and run with pushes off; Full has all three blocks
    play = _cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Events-Play-v0")
    assert play.pushes is False and EM.build_block(play.events, play.sim.dt, play.episode_length_s)["flags"] == b["flags"]
    full = _cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Full-v0")
    assert full.rewards is not None and full.observations is not None and full.events is not None
    assert _cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Full-Play-v0").observations.policy.enable_corruption is False


def test_probability_param_and_offset_mode():
    EM, EV, Term = _em()
    cfg = {"push": Term(func=EV.push_by_setting_velocity_with_random_envs, mode="interval",
                        params={"velocity_range": {"x": (-1, 1), "roll": (-3, 3), "pitch": (0, 2), "yaw": (-0.5, 0.5)},
                                "probability": 0.25}),
           "joints": Term(func=EV.reset_joints_by_offset, mode="reset", params={"position_range": (-0.1, 0.2),
                                                                                "velocity_range": (-0.5, 0.5)})}
    b = EM.build_block(cfg, 0.005, 10.0)
    assert b["p"] == 0.25 and b["flags"] == ET.PUSH | ET.JOINT_OFFSET and b["inert"] == []
    assert b["ranges"]["push"] == [(-1.0, 2.0), (0.0, 0.0), (-0.5, 1.0), (-3.0, 6.0), (0.0, 2.0)]
    assert b["ranges"]["joint_vel"] == [(-0.5, 1.0)]


def test_terms_describe_and_are_never_called():
    EM, EV, Term = _em()
    for fn in (EV.push_by_setting_velocity_with_random_envs, EV.reset_joints_by_scale, EV.reset_joints_by_offset,
               EV.reset_root_state_uniform, EV.randomize_rigid_body_material):
        assert callable(fn.describe)
        with pytest.raises(TypeError, match="never called"):
            fn(None, None, *([None] * (fn.__code__.co_argcount - 2 - len(fn.__defaults__ or ()))))


def test_block_errors_name_the_term():
    EM, EV, Term = _em()
    build = lambda cfg: EM.build_block(cfg, 0.005, 10.0)                      # noqa: E731
    push = lambda **kw: Term(func=EV.push_by_setting_velocity_with_random_envs, mode="interval", params=kw)   # noqa: E731
    root = lambda **kw: Term(func=EV.reset_root_state_uniform, mode="reset", params=kw)                       # noqa: E731
    mat = lambda **kw: Term(func=EV.randomize_rigid_body_material, mode="startup",                           # noqa: E731
                            params={"static_friction_range": (0.5, 1.25), "dynamic_friction_range": (0.5, 1.25),
                                    "restitution_range": (0.0, 0.0), "num_buckets": 100, **kw})
    scale = Term(func=EV.reset_joints_by_scale, mode="reset", params={"position_range": (0.9, 1.1), "velocity_range": (0, 0)})
    offset = Term(func=EV.reset_joints_by_offset, mode="reset", params={"position_range": (-0.1, 0.1), "velocity_range": (0, 0)})
    with pytest.raises(ValueError, match=r"'shove'.*velocity_range\['z'\]"):
        build({"shove": push(velocity_range={"x": (-1, 1), "z": (0.0, 0.5)})})
    with pytest.raises(ValueError, match="'shove'.*probability"):
        build({"shove": push(velocity_range={}, probability=1.5)})
    for key in ("z", "roll", "pitch"):
        with pytest.raises(ValueError, match=rf"'base'.*pose_range\['{key}'\]"):
            build({"base": root(pose_range={key: (-0.1, 0.1)}, velocity_range={})})
        with pytest.raises(ValueError, match=rf"'base'.*velocity_range\['{key}'\]"):
            build({"base": root(pose_range={}, velocity_range={key: (-0.1, 0.1)})})
    assert build({"base": root(pose_range={"yaw": (-3, 3)}, velocity_range={"yaw": (-1, 1)})})["inert"] == ["base.pose_range.yaw"]
    with pytest.raises(ValueError, match="'mat'.*num_buckets"):
        build({"mat": mat(num_buckets=0)})
    with pytest.raises(ValueError, match="'b'.*second joint reset.*'a'"):
        build({"a": scale, "b": offset})
    with pytest.raises(ValueError, match="'p2'.*second push.*'p1'"):
        build({"p1": push(velocity_range={}), "p2": push(velocity_range={})})
    with pytest.raises(ValueError, match="'m2'.*second material"):
        build({"m1": mat(), "m2": mat()})
    with pytest.raises(ValueError, match="'custom'.*no describe"):
        build({"custom": Term(func=lambda env, env_ids: None, mode="reset")})
    with pytest.raises(ValueError, match="'odd'.*unknown mode"):
        build({"odd": Term(func=EV.reset_joints_by_scale, mode="sometimes", params=scale.params)})
    with pytest.raises(ValueError, match="'timed'.*only interval event"):
        build({"timed": Term(func=EV.reset_joints_by_scale, mode="interval", params=scale.params)})
    with pytest.raises(ValueError, match="'late'.*'interval' event, configured as 'reset'"):
        build({"late": Term(func=EV.push_by_setting_velocity_with_random_envs, mode="reset", params={"velocity_range": {}})})
    with pytest.raises(TypeError, match="'plain'.*not EventTermCfg"):
        build({"plain": types.SimpleNamespace(func=EV.reset_joints_by_scale, mode="reset", params={})})
    with pytest.raises(ValueError, match="'j'.*lo <= hi"):
        build({"j": Term(func=EV.reset_joints_by_scale, mode="reset", params={"position_range": (1.1, 0.9), "velocity_range": (0, 0)})})
    with pytest.raises(ValueError, match="no term"):
        build({})


def test_manager_switch_and_run_state():
    EM = _em()[0]
    cfg = _cfg()
    pushed = []
    env = types.SimpleNamespace(cfg=cfg, max_episode_length_s=cfg.episode_length_s,
                                sim=types.SimpleNamespace(set_event_block=lambda w: pushed.append(w.copy())))
    mgr = EM.EventManager(cfg.events, env)
    assert mgr.interval_enabled and len(pushed) == 1 and pushed[0].view(np.int32)[0] & ET.PUSH
    assert mgr.active_terms == {"startup": ["physics_material"], "reset": ["reset_base", "reset_robot_joints"],
                                "interval": ["push_robot"]} and "reset_base.pose_range.yaw" in mgr.inert
    mgr.set_interval_enabled(True)
    assert len(pushed) == 1                                                   # nothing to copy
    mgr.set_interval_enabled(False)
    assert len(pushed) == 2 and not pushed[1].view(np.int32)[0] & ET.PUSH
    assert pushed[1].view(np.int32)[0] == ET.JOINT_SCALE | ET.ROOT | ET.FRICTION      # reset and startup terms stay on
    assert (pushed[1][1:].view(U32) == pushed[0][1:].view(U32)).all()
    assert mgr.state_dict() == {"interval": False} and "pushes off" in str(mgr)
    fp = mgr.fingerprint()
    mgr.load_state_dict({"interval": True})
    assert mgr.interval_enabled and pushed[-1].view(np.int32)[0] & ET.PUSH and mgr.fingerprint() == fp
    with pytest.raises(ValueError, match="interval"):
        mgr.check_state_dict({})
    off = EM.EventManager(cfg.events, env, interval_enabled=False)
    assert not off.interval_enabled and not pushed[-1].view(np.int32)[0] & ET.PUSH


def test_eval_env_cfg_drops_the_events():
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    cfg = _cfg("Isaac-Velocity-CaT-Flat-Solo12-Servo-Full-v0")
    ecfg = make_eval_env_cfg(cfg, 16)
    assert ecfg.events is None and cfg.events is not None and ecfg.rewards is not None


# ------------------------------------------------------------------------------------------ the twin
@pytest.fixture(scope="module")
def runs():
    cfg = _cfg()
    acts, ep0 = recipe(N)
    table = OT.identity_table(noise=(-0.1, 0.2))
    out = {}
    for name, kw in (("off", dict(flags=0)), ("all", ALL), ("one_bucket", dict(ALL, num_buckets=1)),
                     ("three_buckets", dict(ALL, num_buckets=3))):
        tw = ET.make_twin(cfg, N, ET.block(**kw), obs_table=table, table=RT.ALL_NON_EXP, max_len=MAX_LEN)
        slabs, masks = ET.run_events_twin(tw, acts, ep0)
        slabs.setflags(write=False)
        out[name] = (tw, slabs, masks)
    plain = OT.make_twin(cfg, N, table, table=RT.ALL_NON_EXP, max_len=MAX_LEN)
    return acts, ep0, out, (plain, OT.run_obs_twin(plain, acts, ep0))


def test_all_flags_zero_is_the_observation_twin_byte_for_byte(runs):
    acts, ep0, out, (plain, ref) = runs
    tw, slabs, masks = out["off"]
    assert tw.F == plain.F and tw.off == plain.off and not masks.any()
    np.testing.assert_array_equal(slabs.view(U32), ref.view(U32))
    np.testing.assert_array_equal(tw.reward_record.view(U32), plain.reward_record.view(U32))
    # without an observation table the row is the reward twin's
    cfg = _cfg()
    bare = ET.make_twin(cfg, 17, None, table=RT.ALL_NON_EXP, max_len=MAX_LEN)
    rt = RT.make_twin(cfg, 17, RT.ALL_NON_EXP, obs_dim=45, max_len=MAX_LEN)
    a17, e17 = recipe(17)
    assert bare.F == rt.F == 308 and "policy_obs" not in bare.off
    np.testing.assert_array_equal(ET.run_events_twin(bare, a17, e17)[0].view(U32), RT.run_reward_twin(rt, a17, e17)[0].view(U32))


def test_push_count_and_ranges(runs):
    acts, ep0, out, _ = runs
    tw, slabs, masks = out["all"]
    total = N * STEPS
    sd = math.sqrt(total * P * (1 - P))
    assert abs(int(masks.sum()) - P * total) <= 5 * sd, int(masks.sum())
    # every pushed start velocity lies inside its range: recompute the draws of the pushed (env, step) pairs
    t = RT_lengths(tw, slabs, ep0)
    so = tw.off["servo"][0]
    seen = 0
    for s in range(STEPS):
        ep = slabs[s, :, so + 13].astype(U32)
        pushed, v, kick = tw.push(ep, t[s])
        np.testing.assert_array_equal(pushed, masks[s])
        assert (np.abs(v[pushed, 0:2]) <= 0.5).all() and (v[pushed, 2] == 0).all()
        assert (np.abs(kick[pushed]) <= F32(20.0) * tw.step_dt).all()
        seen += int(pushed.sum())
    assert seen == int(masks.sum()) > 0


def RT_lengths(tw, slabs, ep0):
    import servo_trace_twin as ST
    return ST.episode_lengths(tw, slabs, ep0)


def test_a_push_ends_an_episode_in_a_fall(runs):
    """the kicks of ALL (up to 20 rad/s * 0.02 s = 0.4 rad against tilt_max 0.35) are large enough: some env's history first
    departs from the same run without roll / pitch kicks in a step in which it was pushed and fell"""
    acts, ep0, out, _ = runs
    assert pushed_falls(_cfg(), N, acts, ep0, out["all"]) > 0


def pushed_falls(cfg, n, acts, ep0, kicked_run):
    tw, slabs, masks = kicked_run
    calm = dict(ALL, push=ALL["push"][:3] + [(0.0, 0.0)] * 2)
    tw0 = ET.make_twin(cfg, n, ET.block(**calm), obs_table=OT.identity_table(noise=(-0.1, 0.2)), table=RT.ALL_NON_EXP, max_len=MAX_LEN)
    slabs0, masks0 = ET.run_events_twin(tw0, acts, ep0)
    h = tw.off["hard_reset"][0]
    fell, fell0 = slabs[1:, :, h] > 0, slabs0[1:, :, h] > 0
    count = 0
    for i in range(n):
        d = np.nonzero(fell[:, i] != fell0[:, i])[0]
        if len(d) and fell[d[0], i] and masks[d[0], i]:
            count += 1
    return count


def test_friction_buckets(runs):
    acts, ep0, out, _ = runs
    tw = out["all"][0]
    bucket, mu = tw.friction()
    assert bucket.min() >= 0 and bucket.max() <= 99 and len(np.unique(mu)) <= 100
    assert (mu >= F32(0.5)).all() and (mu <= F32(1.25)).all()
    for b in np.unique(bucket):
        assert len(np.unique(mu[bucket == b])) == 1                           # one material per bucket, shared by its envs
    assert len(np.unique(bucket)) > 30 and (tw.traction() <= 1).all() and (tw.traction() == np.minimum(mu, F32(1))).all()
    assert len(np.unique(out["one_bucket"][0].friction()[1])) == 1
    b3, mu3 = out["three_buckets"][0].friction()
    assert set(np.unique(b3)) == {0, 1, 2} and len(np.unique(mu3)) <= 3
    # another shard of the same run sees the same materials: the bucket's value is keyed on the bucket alone
    hi = ET.make_twin(_cfg(), 32, ET.block(**ALL), env_offset=32, max_len=MAX_LEN)
    np.testing.assert_array_equal(hi.friction()[1].view(U32), mu[32:].view(U32))
    # the traction scales the three velocity rows only; the tilt rows are the fixed matrix
    assert (tw.G[3:] == np.broadcast_to(tw.G0[3:, None, :], tw.G[3:].shape)).all()


def test_first_poses_lie_inside_the_scaled_default(runs):
    acts, ep0, out, _ = runs
    tw, slabs, masks = out["all"]
    for ep in (0, 1, 5):
        q0, qd0 = tw.first_joint(np.full(N, ep, U32))
        lo, hi = np.minimum(T.DEFAULT_JOINT_POS * F32(0.95), T.DEFAULT_JOINT_POS * F32(1.05)), \
            np.maximum(T.DEFAULT_JOINT_POS * F32(0.95), T.DEFAULT_JOINT_POS * F32(1.05))
        ulp = np.spacing(np.abs(hi).astype(F32))
        assert (q0 >= lo - ulp).all() and (q0 <= hi + ulp).all() and (qd0 == 0).all()
    jp = tw.off["joint_pos"][0]
    np.testing.assert_array_equal(slabs[0, :, jp:jp + 12], tw.first_joint(np.zeros(N, U32))[0])
    # the init row and the first observation show the root term's velocities
    xy, v0 = tw.first_root(np.zeros(N, U32))
    so, ob, rp = tw.off["servo"][0], tw.off["obs"][0], tw.off["root_pos_w"][0]
    np.testing.assert_array_equal(slabs[0, :, so:so + 3], v0)
    np.testing.assert_array_equal(slabs[0, :, ob + 2], v0[:, 2])
    np.testing.assert_array_equal(slabs[0, :, rp:rp + 2], xy)
    assert (np.abs(xy) <= 0.05).all() and (np.abs(v0[:, 2]) <= 0.2).all() and (v0 != 0).any()


def test_the_gyro_shows_the_kick_and_the_lag_starts_from_the_kicked_tilt(runs):
    acts, ep0, out, _ = runs
    tw, slabs, masks = out["all"]
    so, ob, h = tw.off["servo"][0], tw.off["obs"][0], tw.off["hard_reset"][0]
    t = RT_lengths(tw, slabs, ep0)
    checked = 0
    for s in range(STEPS):
        ends = (t[s] + 1 >= MAX_LEN) | (slabs[s + 1, :, h] > 0)
        started = np.zeros(N, bool) if s == 0 else ((t[s] == 0))
        rows = np.nonzero(masks[s] & ~ends & ~started)[0]
        for i in rows:
            roll0, roll1 = slabs[s, i, so + 3], slabs[s + 1, i, so + 3]
            np.testing.assert_array_equal(slabs[s + 1, i, ob], (roll1 - roll0) / tw.step_dt)
            checked += 1
    assert checked > 50


# ------------------------------------------------------------------------------------------ push recovery
def test_push_recovery_on_a_hand_made_trace():
    from cat_envs.tasks.utils.cleanrl.evaluate import push_recovery, summarise_push_recovery
    T_, K = 12, 3
    tr = np.zeros((T_, K, 72), F32)
    tr[:, :, 4:7] = [0.5, 0.0, 0.1]                                           # the command
    tr[:, :, 7:10] = [0.5, 0.0, 0.1]                                          # tracked exactly ...
    tr[:, :, 0] = np.arange(T_)[:, None]
    # env 0: pushed at step 2, errors 0.6, 0.3, 0.12, 0.05 on vy, then fine: recovers after 3 steps
    tr[2, 0, 14] = 1
    tr[2:6, 0, 8] = [0.6, 0.3, 0.12, 0.05]
    # env 1: pushed at step 1 and falls at step 3 before recovering; pushed again at step 8 with no error at all
    tr[1, 1, 14] = 1
    tr[1:4, 1, 9] = [0.1 + 0.4, 0.1 + 0.5, 0.1 - 0.7]
    tr[3, 1, 1:3] = 1
    tr[8, 1, 14] = 1
    # env 2: pushed at step 9, the error never settles inside the trace
    tr[9, 2, 14] = 1
    tr[9:, 2, 7] = 0.5 + 0.3
    rows = push_recovery(tr, tol=0.1)
    assert [(r["env"], r["step"]) for r in rows] == [(0, 2), (1, 1), (1, 8), (2, 9)]
    a, b, c, d = rows
    assert a["recover_steps"] == 3 and a["fell"] is False and a["window"] == 10 and abs(a["peak_error"] - 0.6) < 1e-6
    assert b["recover_steps"] is None and b["fell"] is True and b["window"] == 3 and abs(b["peak_error"] - 0.7) < 1e-6
    assert c["recover_steps"] == 0 and c["fell"] is False and c["peak_error"] == 0.0 and c["window"] == 4
    assert d["recover_steps"] is None and d["fell"] is False and abs(d["peak_error"] - 0.3) < 1e-6
    assert summarise_push_recovery(rows) == {"pushes": 4, "recovered": 2, "fell": 1, "recover_steps_median": 1.5,
                                             "peak_error_median": pytest.approx(0.45, abs=1e-6)}
    assert push_recovery(np.zeros((5, 2, 72), F32)) == []
    with pytest.raises(ValueError, match="trace"):
        push_recovery(np.zeros((5, 72), F32))
