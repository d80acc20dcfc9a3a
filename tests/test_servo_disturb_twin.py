"""The servo task's disturbances without a device ("Disturbances"): the extended event block from IsaacLab's
stock ``EventCfg`` and from ``DisturbanceEventCfg``, the errors that name the term, the manager's switches and run state, and
properties of the numpy twin - among them that the recipe the device test shares shows every case it is meant to show."""
import copy
import types

import numpy as np
import pytest

import servo_disturb_twin as DT
import servo_events_twin as ET
import test_servo_events_twin as CE
from oracle import rng_oracle as R

F32, U32 = np.float32, np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Disturbances-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Disturbances-v0"
STEPS, MAX_LEN = 40, 12
#: the timer's range: at a step of 0.02 s a timer of 0.01 .. 0.05 s runs out after one to three steps
T_RANGE = (0.01, 0.05)
#: the liveness block: the timed push with the events suite's push ranges, a wrench per episode whose Fz reaches from below to
#: above the weight of 25 N (so the load is clamped in some envs and not in others), the scale reset, the root reset, friction
RECIPE = dict(flags=DT.PUSH_TIMED | DT.WRENCH | DT.WRENCH_RESET | ET.JOINT_SCALE | ET.ROOT | ET.FRICTION, num_buckets=100,
              interval=T_RANGE, force=(-10.0, 40.0), torque=(-1.0, 1.0), push=CE.ALL["push"], joint_pos=CE.ALL["joint_pos"],
              root_pos=CE.ALL["root_pos"], root_vel=CE.ALL["root_vel"], friction=CE.ALL["friction"])
TIMED_ALONE = dict(flags=DT.PUSH_TIMED, interval=T_RANGE, push=CE.ALL["push"])
WRENCH_ALONE = dict(flags=DT.WRENCH | DT.WRENCH_RESET, force=(-10.0, 40.0), torque=(-1.0, 1.0))
WRENCH_PER_ENV = dict(flags=DT.WRENCH, force=(-10.0, 40.0), torque=(-1.0, 1.0))
recipe = CE.recipe


def liveness(tw, slabs, masks, resets, clamps):
    """what a run of the recipe must show, so that no case is silently missing"""
    assert (masks.sum(0) >= 2).all(), "every env fires at least twice"
    assert (masks[1:] & masks[:-1]).any(), "some env fires in consecutive steps"
    assert resets.any(), "some step starts an episode"
    if tw.xflags & DT.WRENCH:
        assert clamps.any() and not clamps.all(), "W - F[2] is clamped in some env and not clamped in another"
        assert clamps.any(0).any() and not clamps.any(0).all()


@pytest.fixture(scope="module")
def runs():
    """the recipe on 64 envs: (twin, actions, ep0, slabs, masks, resets, clamps)"""
    acts, ep0 = recipe(64)
    tw = DT.make_twin(CE._cfg(), 64, DT.block(**RECIPE), max_len=MAX_LEN)
    out = DT.run_disturb_twin(tw, acts, ep0)
    return (tw, acts, ep0, *out)


# ------------------------------------------------------------------------------------------ ABI constants
def test_constants_and_the_pins_of_the_descriptor_chain():
    from cat_envs import native
    assert len(native.EXPORTS) == 59 and len(native.SERVO_EXTS) == 9
    assert native.SERVO_EVENT_FLOATS == 32 == ET.FLOATS and native.SERVO_EVENT_FLOATS_EXT == 64 == DT.FLOATS_EXT
    assert native.SERVO_EVENT_WORDS == ET.WORDS and native.SERVO_EVENT_WORDS_EXT == DT.WORDS_EXT
    assert (native.SERVO_EVENT_PUSH_TIMED, native.SERVO_EVENT_WRENCH, native.SERVO_EVENT_WRENCH_RESET) == (32, 64, 128)
    assert [f[0] for f in native.ServoEvents._fields_] == ["block", "floats", "reserved"]
    import os
    import re
    src = open(os.path.join(CE.ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EVENT_FLOATS_EXT (\d+)", src).group(1)) == 64
    for name, bit in (("PUSH_TIMED", 32), ("WRENCH", 64), ("WRENCH_RESET", 128)):
        assert int(re.search(rf"#define CATPPO_SERVO_EVENT_{name} (\d+)u", src).group(1)) == bit
    kernel = open(os.path.join(CE.ROOT, "constraints-as-terminations_amd", "csrc", "servo_sim_kernel.h")).read()
    # the two new tags are the twin's, and no two tags of the kernel are the same
    assert f"0x{DT.TAG_PUSH_TIME:08X}u" in kernel and f"0x{DT.TAG_WRENCH:08X}u" in kernel
    tags = set(int(t, 16) for t in re.findall(r"kTag\w+ = (0x[0-9A-F]{8})u", kernel))
    assert len(tags) == len(re.findall(r"kTag\w+ = 0x[0-9A-F]{8}u", kernel)) and {DT.TAG_PUSH_TIME, DT.TAG_WRENCH} <= tags


# ------------------------------------------------------------------------------------------ block building
def _stock_isaaclab_event_cfg():
    """IsaacLab's velocity-task ``EventCfg`` as its robot cfgs run it on flat ground (the base's reset velocities zeroed, as
    those cfgs do): five terms, among them the two the servo task used to refuse"""
    EM, EV, Term = CE._em()
    from cat_envs.shim import SceneEntityCfg
    return {
        "physics_material": Term(func=EV.randomize_rigid_body_material, mode="startup",
                                 params={"asset_cfg": SceneEntityCfg("robot", body_names=".*"), "static_friction_range": (0.8, 0.8),
                                         "dynamic_friction_range": (0.6, 0.6), "restitution_range": (0.0, 0.0), "num_buckets": 64}),
        "base_external_force_torque": Term(func=EV.apply_external_force_torque, mode="reset",
                                           params={"asset_cfg": SceneEntityCfg("robot", body_names="base"),
                                                   "force_range": (0.0, 0.0), "torque_range": (-0.0, 0.0)}),
        "reset_base": Term(func=EV.reset_root_state_uniform, mode="reset",
                           params={"pose_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5), "yaw": (-3.14, 3.14)},
                                   "velocity_range": {"x": (0.0, 0.0), "y": (0.0, 0.0), "z": (0.0, 0.0), "roll": (0.0, 0.0),
                                                      "pitch": (0.0, 0.0), "yaw": (0.0, 0.0)}}),
        "reset_robot_joints": Term(func=EV.reset_joints_by_scale, mode="reset",
                                   params={"position_range": (0.5, 1.5), "velocity_range": (0.0, 0.0)}),
        "push_robot": Term(func=EV.push_by_setting_velocity, mode="interval", interval_range_s=(10.0, 15.0),
                           params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})}


def test_the_stock_isaaclab_event_cfg_builds_and_packs_64_words():
    EM = CE._em()[0]
    cfg = _stock_isaaclab_event_cfg()
    before = repr({k: vars(v) for k, v in cfg.items()})
    b = EM.build_block(cfg, 0.005, 20.0)
    assert b == EM.build_block(cfg, 0.005, 20.0) and repr({k: vars(v) for k, v in cfg.items()}) == before
    assert b["flags"] == ET.JOINT_SCALE | ET.ROOT | ET.FRICTION and b["flags_ext"] == DT.PUSH_TIMED | DT.WRENCH | DT.WRENCH_RESET
    assert b["interval_range"] == (10.0, 5.0) and b["wrench"] == {"force": (0.0, 0.0), "torque": (0.0, 0.0), "mode": "reset"}
    assert b["terms"] == {"startup": ["physics_material"], "reset": ["base_external_force_torque", "reset_base", "reset_robot_joints"],
                          "interval": ["push_robot"]}
    assert b["kinds"]["push_robot"] == "push_timed" and b["kinds"]["base_external_force_torque"] == "wrench" and b["p"] == 0.0
    words = EM.pack(b)
    expect = DT.block(flags=b["flags"] | b["flags_ext"], num_buckets=64, interval=(10.0, 15.0), force=(0.0, 0.0), torque=(-0.0, 0.0),
                      push=[(-0.5, 0.5), (-0.5, 0.5), (0, 0), (0, 0), (0, 0)], joint_pos=[(0.5, 1.5)],
                      root_pos=[(-0.5, 0.5)] * 2, friction=[(0.8, 0.8)])
    assert words.shape == (64,) and not words[38:].any()
    np.testing.assert_array_equal(words.view(U32), expect.view(U32))
    off = EM.pack(b, interval_enabled=False, wrench_enabled=False)
    assert off.view(np.int32)[0] == b["flags"] and (off[1:].view(U32) == words[1:].view(U32)).all()
    assert EM.pack(b, wrench_enabled=False).view(np.int32)[0] == b["flags"] | DT.PUSH_TIMED


def test_the_disturbance_cfg_and_its_tasks():
    EM = CE._em()[0]
    cfg = CE._cfg(TASK)
    b = EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s)
    assert b["flags"] == ET.JOINT_SCALE | ET.ROOT | ET.FRICTION and b["flags_ext"] == DT.PUSH_TIMED | DT.WRENCH | DT.WRENCH_RESET
    assert b["terms"]["interval"] == ["push_robot"] and "base_external_force_torque" in b["terms"]["reset"]
    words = EM.pack(b)
    expect = DT.block(flags=b["flags"] | b["flags_ext"], num_buckets=100, interval=(2.0, 4.0), force=(-3.0, 3.0), torque=(-0.3, 0.3),
                      push=[(-0.5, 0.5), (-0.5, 0.5), (0, 0), (0, 0), (0, 0)], joint_pos=[(0.95, 1.05)],
                      root_pos=[(-0.05, 0.05)] * 2, root_vel=[(-0.0, 0.0)] * 3, friction=[(0.5, 1.25)])
    np.testing.assert_array_equal(words.view(U32), expect.view(U32))
    assert words[DT.WORDS_EXT["force"] + 1] > 0                              # a non-zero force range
    assert 4.0 < cfg.episode_length_s                                         # the timer fires inside an episode
    # the reference's own cfg still packs its 32 words, byte for byte
    ref = CE._cfg()
    rb = EM.build_block(ref.events, ref.sim.dt, ref.episode_length_s)
    assert "flags_ext" not in rb and "interval_range" not in rb and "wrench" not in rb and not EM.extended(rb)
    np.testing.assert_array_equal(EM.pack(rb).view(U32), ET.block(
        flags=rb["flags"], p=0.00025, num_buckets=100, push=[(-0.5, 0.5), (-0.5, 0.5), (0, 0), (0, 0), (0, 0)],
        joint_pos=[(0.95, 1.05)], root_pos=[(-0.05, 0.05)] * 2, root_vel=[(-0.0, 0.0)] * 3, friction=[(0.5, 1.25)]).view(U32))
    assert EM.pack(rb).shape == (32,)
    # the four tasks; the play cfgs run with pushes off; the reference one has all six MDP blocks and the robot
    for task in (TASK, REFERENCE):
        play = CE._cfg(task.replace("-v0", "-Play-v0"))
        assert play.pushes is False and EM.build_block(play.events, play.sim.dt, play.episode_length_s) == b
    full = CE._cfg(REFERENCE)
    for blk in ("rewards", "observations", "events", "commands", "terminations", "actions"):
        assert getattr(full, blk) is not None, blk
    assert full.scene.robot is not None and EM.build_block(full.events, full.sim.dt, full.episode_length_s) == b


def test_new_terms_describe_and_are_never_called():
    EV = CE._em()[1]
    for fn in (EV.push_by_setting_velocity, EV.apply_external_force_torque):
        assert callable(fn.describe)
        with pytest.raises(TypeError, match="never called"):
            fn(None, None, *([None] * (fn.__code__.co_argcount - 2 - len(fn.__defaults__ or ()))))
    assert EV.push_by_setting_velocity.__code__.co_varnames[:4] == ("env", "env_ids", "velocity_range", "asset_cfg")
    assert EV.apply_external_force_torque.__code__.co_varnames[:5] == ("env", "env_ids", "force_range", "torque_range", "asset_cfg")


def test_block_errors_name_the_term():
    EM, EV, Term = CE._em()
    from cat_envs.shim import SceneEntityCfg
    build = lambda cfg: EM.build_block(cfg, 0.005, 10.0)                      # noqa: E731
    timed = lambda **kw: Term(func=EV.push_by_setting_velocity, mode="interval", params={"velocity_range": {}}, **kw)   # noqa: E731
    random = Term(func=EV.push_by_setting_velocity_with_random_envs, mode="interval", params={"velocity_range": {}})
    wrench = lambda mode="reset", **kw: Term(func=EV.apply_external_force_torque, mode=mode,                # noqa: E731
                                             params={"force_range": (0, 1), "torque_range": (0, 1), **kw})
    scale = {"position_range": (0.9, 1.1), "velocity_range": (0, 0)}
    with pytest.raises(ValueError, match="'shove'.*is_global_time"):
        build({"shove": timed(interval_range_s=(1.0, 2.0), is_global_time=True)})
    with pytest.raises(ValueError, match="'shove'.*interval_range_s"):
        build({"shove": timed()})
    for bad in ((0.0, 1.0), (2.0, 1.0), (-1.0, 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="'shove'.*interval_range_s.*0 < a <= b"):
            build({"shove": timed(interval_range_s=bad)})
    with pytest.raises(ValueError, match=r"'shove'.*velocity_range\['z'\]"):
        build({"shove": Term(func=EV.push_by_setting_velocity, mode="interval", interval_range_s=(1, 2),
                             params={"velocity_range": {"z": (0.0, 0.5)}})})
    with pytest.raises(ValueError, match="'late'.*'interval' event, configured as 'reset'"):
        build({"late": Term(func=EV.push_by_setting_velocity, mode="reset", params={"velocity_range": {}})})
    # at most one push term of either kind, with the message the events suite pins
    with pytest.raises(ValueError, match="'p2'.*second push.*'p1'"):
        build({"p1": random, "p2": timed(interval_range_s=(1, 2))})
    with pytest.raises(ValueError, match="'p2'.*second push.*'p1'"):
        build({"p1": timed(interval_range_s=(1, 2)), "p2": random})
    with pytest.raises(ValueError, match="'p2'.*second push.*'p1'"):
        build({"p1": timed(interval_range_s=(1, 2)), "p2": timed(interval_range_s=(1, 2))})
    with pytest.raises(ValueError, match="'p2'.*second push.*'p1'"):
        build({"p1": random, "p2": random})
    with pytest.raises(ValueError, match="'w'.*only interval event"):
        build({"w": wrench("interval")})
    with pytest.raises(ValueError, match="'w2'.*second wrench.*'w1'"):
        build({"w1": wrench(), "w2": wrench("startup")})
    with pytest.raises(ValueError, match="'w'.*body_names.*base"):
        build({"w": wrench(asset_cfg=SceneEntityCfg("robot", body_names="FL_FOOT"))})
    with pytest.raises(ValueError, match="'w'.*force_range.*lo <= hi"):
        build({"w": wrench(force_range=(1.0, 0.0))})
    with pytest.raises(ValueError, match="'w'.*force_range and torque_range are required"):
        build({"w": Term(func=EV.apply_external_force_torque, mode="reset", params={"force_range": (0, 1)})})
    for names in ("base", "base_link", ".*", ["trunk", "base.*"]):
        assert build({"w": wrench(asset_cfg=SceneEntityCfg("robot", body_names=names))})["flags_ext"] == DT.WRENCH | DT.WRENCH_RESET
    assert build({"w": wrench("startup")})["flags_ext"] == DT.WRENCH
    # the old texts still match
    with pytest.raises(ValueError, match="'timed'.*only interval event"):
        build({"timed": Term(func=EV.reset_joints_by_scale, mode="interval", params=scale)})
    with pytest.raises(ValueError, match="'custom'.*no describe"):
        build({"custom": Term(func=lambda env, env_ids: None, mode="reset")})


def _env(cfg, pushed):
    return types.SimpleNamespace(cfg=cfg, max_episode_length_s=cfg.episode_length_s,
                                 sim=types.SimpleNamespace(set_event_block=lambda w: pushed.append(w.copy())))


def test_manager_switches_and_run_state():
    EM = CE._em()[0]
    cfg, pushed = CE._cfg(TASK), []
    mgr = EM.EventManager(cfg.events, _env(cfg, pushed))
    both = DT.PUSH_TIMED | DT.WRENCH | DT.WRENCH_RESET
    flags = lambda i=-1: int(pushed[i].view(np.int32)[0])                     # noqa: E731
    assert len(pushed) == 1 and pushed[0].shape == (64,) and flags() & both == both
    assert mgr.interval_enabled and mgr.wrench_enabled
    mgr.set_wrench_enabled(True)
    assert len(pushed) == 1                                                   # nothing to copy
    mgr.set_wrench_enabled(False)
    assert len(pushed) == 2 and flags() & both == DT.PUSH_TIMED and (pushed[1][1:].view(U32) == pushed[0][1:].view(U32)).all()
    mgr.set_interval_enabled(False)
    assert flags() & both == 0 and flags() == ET.JOINT_SCALE | ET.ROOT | ET.FRICTION
    assert mgr.state_dict() == {"interval": False, "wrench": False} and "pushes off" in str(mgr) and "(off)" in str(mgr)
    fp = mgr.fingerprint()
    assert len(fp[-1]) == 64
    mgr.load_state_dict({"interval": True, "wrench": True})
    assert mgr.interval_enabled and mgr.wrench_enabled and flags() & both == both and mgr.fingerprint() == fp
    with pytest.raises(ValueError, match="wrench"):
        mgr.check_state_dict({"interval": True})
    # set_interval_enabled clears and sets both push bits: the per-step push of the reference's cfg as before
    ref, pushed_ref = CE._cfg(), []
    old = EM.EventManager(ref.events, _env(ref, pushed_ref))
    assert pushed_ref[0].shape == (32,) and old.state_dict() == {"interval": True} and len(old.fingerprint()[-1]) == 32
    assert not old.wrench_enabled
    old.load_state_dict({"interval": False})                                  # an older run state loads unchanged
    assert not pushed_ref[-1].view(np.int32)[0] & (ET.PUSH | DT.PUSH_TIMED)
    with pytest.raises(TypeError, match="apply_external_force_torque"):
        old.set_wrench_enabled(False)
    before = copy.deepcopy(old.fingerprint())
    old.set_interval_enabled(True)
    assert old.fingerprint() == before


def test_eval_env_cfg_goes_on_dropping_the_events():
    from cat_envs.tasks.utils.cleanrl import periodic_eval as EVAL
    cfg = CE._cfg(TASK)
    assert cfg.events is not None and getattr(EVAL.make_eval_env_cfg(cfg, 8), "events", None) is None


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("case", ["32 words", "64 words, flags clear", "64 words, zero-range wrench", "timed bit without a field"])
def test_nothing_on_is_the_events_twin_bit_for_bit(case):
    n = 17
    acts, ep0 = recipe(n)
    ref, ref_masks = ET.run_events_twin(ET.make_twin(CE._cfg(), n, ET.block(**CE.ALL), max_len=MAX_LEN), acts, ep0)
    words = {"32 words": ET.block(**CE.ALL),
             "64 words, flags clear": DT.block(**CE.ALL, interval=(0.5, 1.0), force=(-5.0, 5.0), torque=(-1.0, 1.0)),
             "64 words, zero-range wrench": DT.block(**dict(CE.ALL, flags=CE.ALL["flags"] | DT.WRENCH | DT.WRENCH_RESET)),
             "timed bit without a field": DT.block(**dict(CE.ALL, flags=CE.ALL["flags"] | DT.PUSH_TIMED), interval=T_RANGE)}[case]
    tw = DT.make_twin(CE._cfg(), n, words, max_len=MAX_LEN, ev_state=False)
    slabs, masks, _, clamps = DT.run_disturb_twin(tw, acts, ep0)
    assert tw.off == ET.make_twin(CE._cfg(), n, ET.block(), max_len=MAX_LEN).off
    np.testing.assert_array_equal(slabs.view(U32), ref.view(U32))
    np.testing.assert_array_equal(masks, ref_masks)
    assert not clamps.any() and ref_masks.any()
    # with the timer field in the row, everything in front of it is the same and the field stays zero
    if case != "timed bit without a field":
        tw4 = DT.make_twin(CE._cfg(), n, words, max_len=MAX_LEN)
        slabs4 = DT.run_disturb_twin(tw4, acts, ep0)[0]
        assert tw4.F == tw.F + 4 and tw4.off["ev_state"] == (tw.F, 4)
        np.testing.assert_array_equal(slabs4[:, :, :tw.F].view(U32), ref.view(U32))
        assert not slabs4[:, :, tw.F:].any()


def test_the_recipe_shows_every_case(runs):
    tw, acts, ep0, slabs, masks, resets, clamps = runs
    liveness(tw, slabs, masks, resets, clamps)
    st = tw.off["ev_state"][0]
    assert (slabs[:, :, st] > 0).all() and not slabs[:, :, st + 1:st + 4].any()     # a timer is always running
    lo, hi = F32(T_RANGE[0]), F32(T_RANGE[0]) + F32(T_RANGE[1] - T_RANGE[0])
    assert (slabs[:, :, st] <= hi).all()
    fresh = slabs[1:, :, st][masks]
    assert (fresh >= lo).all() and (fresh <= hi).all()
    assert not (masks & resets).any()                                               # a reset step runs no update


def _u0(seed, gid, ep, third, tag):
    ctr = np.array([[gid, ep, third, tag]], np.uint32)
    key = np.array([[seed & 0xFFFFFFFF, seed >> 32]], np.uint32)
    return R.uniform_open(R.philox4x32_10(ctr, key))[0, 0]


def test_pushed_column_equals_a_scalar_restatement_of_the_timer_rule(runs):
    """a plain fp32 loop per env, which knows of the run only when the env's episodes began and their numbers"""
    tw, acts, ep0, slabs, masks, resets, _ = runs
    so, st = tw.off["servo"][0], tw.off["ev_state"][0]
    lo, width = F32(T_RANGE[0]), F32(float(T_RANGE[1]) - float(T_RANGE[0]))
    step_dt = F32(F32(CE._cfg().sim.dt) * F32(CE._cfg().decimation))
    for i in range(tw.N):
        gid = int(tw.gid[i])
        tl = F32(lo + _u0(tw.seed, gid, 0, 0, DT.TAG_PUSH_TIME) * width)
        t = int(ep0[i])
        for s in range(STEPS):
            ep = int(slabs[s, i, so + 13])
            if resets[s, i]:
                tl, fire = F32(lo + _u0(tw.seed, gid, ep, 0, DT.TAG_PUSH_TIME) * width), False
            else:
                tl = F32(tl - step_dt)
                fire = bool(tl < F32(1e-6))
                if fire:
                    tl = F32(lo + _u0(tw.seed, gid, ep, t + 1, DT.TAG_PUSH_TIME) * width)
            assert fire == bool(masks[s, i]), (i, s)
            assert tl.view(U32) == slabs[s + 1, i, st].view(U32), (i, s)
            t = 0 if (t + 1 >= MAX_LEN or slabs[s + 1, i, tw.off["hard_reset"][0]] > 0.5) else t + 1


def test_a_timed_push_adds_and_a_wrench_shifts_what_the_legs_ask_for():
    n = 17
    acts, ep0 = recipe(n)
    cfg = CE._cfg()
    plain = ET.run_events_twin(ET.make_twin(cfg, n, ET.block(), max_len=MAX_LEN), acts, ep0)[0]
    # the timed push: up to the first fired step the rows are the plain ones; the fired step's velocity differs
    tw = DT.make_twin(cfg, n, DT.block(**TIMED_ALONE), max_len=MAX_LEN)
    slabs, masks, resets, _ = DT.run_disturb_twin(tw, acts, ep0)
    F = plain.shape[2]
    first = int(np.argmax(masks.any(1)))
    np.testing.assert_array_equal(slabs[:first + 1, :, :F].view(U32), plain[:first + 1].view(U32))
    so = tw.off["servo"][0]
    hit = masks[first]
    assert (slabs[first + 1, hit, so:so + 2] != plain[first + 1, hit, so:so + 2]).any()
    # the wrench per episode differs between an env's episodes, the wrench per env does not
    for words, per_episode in ((WRENCH_ALONE, True), (WRENCH_PER_ENV, False)):
        tw = DT.make_twin(cfg, n, DT.block(**words), max_len=MAX_LEN)
        seen = {}
        ep_len = np.asarray(ep0, np.int64).copy()
        slab, reset = tw.initial(ep_len), np.zeros(n, bool)
        for a in acts:
            ep = slab[:, so + 13].astype(int)
            slab = tw.step(slab, a, reset, ep_len)
            for i in range(n):
                seen.setdefault(i, {}).setdefault(int(ep[i]), set()).add(tw.wrench_stats["F"][i].tobytes())
            ep_len += 1
            reset = (ep_len >= MAX_LEN) | (slab[:, tw.off["hard_reset"][0]] > 0.5)
            ep_len[reset] = 0
        assert all(len(v) == 1 for eps in seen.values() for v in eps.values())      # constant for the episode
        across = [len(set.union(*eps.values())) for eps in seen.values() if len(eps) > 1]
        assert across and all(c > 1 for c in across) if per_episode else all(c == 1 for c in across)
    # a force of one body weight along x shifts the velocity the legs ask for by 1 m/s
    W = float(cfg.synthetic.servo_weight)
    tw = DT.make_twin(cfg, 1, DT.block(flags=DT.WRENCH, force=(W, W), torque=(0.0, 0.0)), max_len=MAX_LEN)
    add, load = tw.wrench(np.zeros(1, np.uint32), np.full(1, W, F32))
    assert add[0][0] == add[1][0] == 1.0 and add[2][0] == add[3][0] == add[4][0] == 0.0 and load[0] == 0.0


def _chain(n, events, disturb):
    """the whole chain - observations, commands, terminations, actions, the mixed robot, a drawn mass - under the plant twin
    (``disturb`` False) or the disturbance twin on top of it"""
    import servo_plant_twin as PT
    import servo_reward_twin as RT
    import test_servo_actions_twin as AC
    import test_servo_actuators_twin as UC
    import test_servo_commands_twin as CC
    import test_servo_randomize_twin as ZC
    import test_servo_terminations_twin as TC
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    kw = dict(commands=CC.words_of(CC.commands_cfg_of()), terminations=TC.entries_of(TC.liveness_cfg()),
              actions=AC.reference_perm()[0], width=12, actuators=UC.mixed_entries(), randomize=ZC.recipe_block())
    obs_table = AC.reference_blocks()[1]
    acts, ep0 = AC.recipe(n, 12)
    if disturb:
        tw = DT.make_twin(cfg, n, events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=ZC.MAX_LEN, robot=kw)
        return tw, DT.run_disturb_twin(tw, acts, ep0)[0]
    tw = PT.make_twin(cfg, n, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=ZC.MAX_LEN, **kw)
    return tw, PT.run_plant_twin(tw, acts, ep0)


def test_nothing_on_is_the_whole_chain_bit_for_bit_and_its_other_state_fields_live_on():
    """on top of commands, terminations and the robot the disturbance twin leaves every field of its parents what it was -
    ``cmd_state``, ``term_state`` and ``act_hist`` among them - with nothing on, and keeps them alive with everything on"""
    n = 5
    parent, ref = _chain(n, ET.block(**CE.ALL), False)
    tw, slabs = _chain(n, DT.block(**CE.ALL, interval=(0.5, 1.0), force=(-5.0, 5.0)), True)
    assert tw.F == parent.F + 4 and {k: v for k, v in tw.off.items() if k != "ev_state"} == parent.off
    np.testing.assert_array_equal(slabs[:, :, :parent.F].view(U32), ref.view(U32))
    assert not slabs[:, :, parent.F:].any()
    on, live = _chain(n, DT.block(**RECIPE), True)
    for name in ("cmd_state", "term_state", "act_hist", "ev_state"):
        a, w = on.off[name]
        assert live[:, :, a:a + w].any(), name
    c = on.off["cmd_state"][0]
    np.testing.assert_array_equal(live[0, :, c].view(U32), ref[0, :, c].view(U32))     # the first command timers are the parent's


@pytest.mark.parametrize("which", ["base", "robot"])
def test_the_restated_loops_are_their_parents_apart_from_the_marked_lines(which):
    """``_WrenchBaseLoop.step`` and ``_WrenchRobotLoop.step`` restate ``ServoTwin.step`` and ``_RandomizeLoop.step``; a change to
    either parent that the copy does not follow shows here: without the lines marked ``# wrench``, and with the load put back
    to the parent's weight, the copy is the parent's source line for line"""
    import inspect
    import servo_randomize_twin as ZT
    import servo_twin as T
    copy_fn, parent_fn, weight = {"base": (DT._WrenchBaseLoop.step, T.ServoTwin.step, 'p["weight"]'),
                                  "robot": (DT._WrenchRobotLoop.step, ZT._RandomizeLoop.step, 'rb["weight"]')}[which]
    mine = [ln.rstrip() for ln in inspect.getsource(copy_fn).split("\n") if not ln.rstrip().endswith("# wrench")]
    assert len(mine) + 4 == len(inspect.getsource(copy_fn).split("\n"))                  # four marked lines
    mine = "\n".join(mine).replace("(load / nsafe)", f"({weight} / nsafe)")
    theirs = "\n".join(ln.rstrip() for ln in inspect.getsource(parent_fn).split("\n"))
    if which == "base":      # the parent reads its module's names unqualified
        mine = mine.replace("T.tree16(", "tree16(").replace("T.tree4(", "tree4(")
        mine = mine.replace("        J, H, B, FOOT_BODY, DEFAULT_JOINT_POS = T.J, T.H, T.B, T.FOOT_BODY, T.DEFAULT_JOINT_POS\n", "")
    else:
        mine = mine.replace("ZT.TAG_", "TAG_")
    assert mine == theirs
