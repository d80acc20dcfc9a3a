"""The servo task's disturbances on the device (csrc/servo_sim_kernel.h: the events-on instances with an extended block;
``mdp.events.push_by_setting_velocity`` / ``apply_external_force_torque``, ``EventManager``, tasks ...-Solo12-Servo-Disturbances-v0
/ -Reference-Disturbances-v0): the kernel against ``servo_disturb_twin`` bit for bit - slabs, evaluation record and trace - with
each kind alone and with both on top of the whole chain, the identities with the 32-word launch, the switches, shards, the run
state, the entry point's refusals and the env.  DESIGN section 9, "Disturbances".

Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one); 40 steps of episodes of 12 steps and
a timer of 0.01 .. 0.05 s at a step of 0.02 s, so that every env is pushed several times, some in consecutive steps, and episodes
end by time-out and by falls (test_servo_disturb_twin.py asserts all of it on the twin's run of the same recipe)."""
import types

import numpy as np
import pytest
import torch

import servo_disturb_twin as DT
import servo_events_twin as ET
import servo_plant_twin as PT
import servo_reward_twin as RT
import test_gpu_servo_events as GE
import test_gpu_servo_sim as S
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_commands_twin as CC
import test_servo_disturb_twin as CD
import test_servo_events_twin as CE
import test_servo_randomize_twin as ZC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, CD.STEPS, CD.MAX_LEN
TASK = CD.TASK
_same_bits = GE._same_bits
_run_device = GE._run_device


def _device_sim(n, words, ev_state=True, offset=0, max_len=MAX_LEN):
    """a simulator with the event block ``words``: 32 words on a plain events simulator, 64 on one with the extended block and,
    with ``ev_state``, the timer field; its two slabs are the first ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = S._env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    ext = len(words) == DT.FLOATS_EXT
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, max_len, ep_len, reset,
                         env_offset=offset, events=True, disturbances=ext, event_timer=ext and ev_state)
    sim.set_event_block(words)
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _with_record(sim, trace_envs=0, steps=STEPS):
    sim.rec = torch.zeros(sim.N, 12, device="cuda")
    sim.set_eval_record(sim.rec)
    sim.trace = torch.zeros(steps, trace_envs, 72, device="cuda") if trace_envs else None
    if trace_envs:
        sim.set_trace(sim.trace)
    return sim


_REF = {}


def reference(n, words, ev_state=True, offset=0, total=None, switch=None, trace_envs=0):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs, masks, resets,
    clamps).  ``offset``, ``total``: envs offset .. offset + n of the recipe for ``total`` envs"""
    key = (n, words.tobytes(), ev_state, offset, total, None if switch is None else (switch[0], switch[1].tobytes()), trace_envs)
    if key not in _REF:
        kw = dict(trace_envs=trace_envs, trace_capacity=STEPS) if trace_envs else {}
        tw = DT.make_twin(S._env_cfg(), n, words, env_offset=offset, max_len=MAX_LEN, ev_state=ev_state, **kw)
        acts, ep0 = CD.recipe(total or n)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:offset + n]), ep0[offset:offset + n]
        out = DT.run_disturb_twin(tw, acts, ep0, switch=switch)
        out[0].setflags(write=False)
        _REF[key] = (tw, acts, ep0, *out)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_record_and_trace_equal_the_twin_bit_for_bit(n):
    from cat_envs import native
    words, k = DT.block(**CD.RECIPE), min(n, 16)
    tw, acts, ep0, ref, masks, resets, clamps = reference(n, words, trace_envs=k)
    if n >= 64:
        CD.liveness(tw, ref, masks, resets, clamps)
    sim = _with_record(_device_sim(n, words), trace_envs=k)
    assert sim.off == tw.off and sim.F == tw.F == 308 + 4 and sim.row_floats == sim.F
    d = sim._desc
    assert d.reserved == native.SERVO_EXT_EVENTS and d.ev.floats == 64 and d.ev.reserved == sim.off["ev_state"][0] == 308
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with the timed push and the wrench")
    _same_bits(sim.rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(sim.trace.cpu().numpy(), tw.trace, "trace")
    np.testing.assert_array_equal(sim.trace.cpu().numpy()[:, :, 14] > 0, masks[:, :k])     # float 14 is the fire mask


KINDS = {"timed push": CD.TIMED_ALONE, "wrench per episode": CD.WRENCH_ALONE, "wrench per env": CD.WRENCH_PER_ENV}


@pytest.mark.parametrize("kind", list(KINDS))
def test_each_kind_alone_at_a_ragged_workgroup(kind):
    n = 17
    words = DT.block(**KINDS[kind])
    tw, acts, ep0, ref, masks, _, clamps = reference(n, words)
    plain = reference(n, DT.block())[3]
    assert (ref != plain).any() and (masks.any() if "push" in kind else clamps.any()), "the kind changes nothing on the twin"
    _same_bits(_run_device(_device_sim(n, words), acts, ep0), ref, f"slabs with the {kind} alone")


def _chain_sim(n, events, words, robot, actions, terms, commands, obs_table, table, plant=None, steps=ZC.STEPS):
    """the extended event block on top of observations, commands, terminations, actions, actuators and randomisation"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, ZC.MAX_LEN, ep_len, reset,
                         policy_obs_dim=len(obs_table), commands=True, terminations=True, actions=True, randomize=True,
                         disturbances=True)
    sim.set_observation_table(obs_table)
    sim.set_event_block(events)
    sim.set_command_block(commands)
    sim.set_termination_table(terms)
    sim.set_reward_table(list(table))
    sim.set_action_table(*actions)
    sim.set_actuator_table(robot)
    sim.set_randomize_block(words)
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    _with_record(sim, steps=steps)
    if plant is not None:
        sim.plant = torch.from_numpy(plant.copy()).cuda()
        sim.set_fixed_plant(sim.plant)
    return sim


@pytest.mark.parametrize("pinned", [False, True])
def test_both_kinds_on_top_of_the_whole_chain_with_a_drawn_and_a_pinned_mass(pinned):
    """commands, terminations, actions, the mixed robot and a base mass drawn per episode, so that W is the env's own; then once
    more with a plant table that pins the mass of two envs in three"""
    n = 17
    words = ZC.recipe_block()
    robot = UC.mixed_entries()
    _, obs_table, _ = AC.reference_blocks()
    events = DT.block(**CD.RECIPE)
    terms = TC.entries_of(TC.liveness_cfg())
    commands = CC.words_of(CC.commands_cfg_of())
    actions = (AC.reference_perm()[0], 12)
    plant = PT.table(n, mass_scale=np.where(np.arange(n) % 3 == 0, np.nan, 0.6 + 0.05 * np.arange(n))) if pinned else None
    tw = DT.make_twin(TC.env_cfg(TC.LIVE_TILT_MAX), n, events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=ZC.MAX_LEN,
                      robot=dict(commands=commands, terminations=terms, actions=actions[0], width=12, actuators=robot,
                                 randomize=words, plant=plant))
    acts, ep0 = AC.recipe(n, 12)
    ref, masks, resets, clamps = DT.run_disturb_twin(tw, acts, ep0)
    weights = tw.wrench_stats["W"]
    assert len(set(weights.tolist())) > n // 2 and masks.any() and resets.any() and clamps.any() and not clamps.all()
    sim = _chain_sim(n, events, words, robot, actions, terms, commands, obs_table, RT.ALL_NON_EXP, plant=plant)
    assert sim.off == tw.off and sim.F == tw.F == 364 + 48 + 4
    dev = GE._run_device(sim, acts, ep0, max_len=ZC.MAX_LEN)
    _same_bits(dev, ref, "rows")
    _same_bits(sim.rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")


# ------------------------------------------------------------------------------------------ 2: identities and switches
def test_a_64_word_block_with_both_flags_clear_gives_the_bytes_of_the_32_word_launch():
    n, k = 64, 16
    acts, ep0 = CD.recipe(n)
    plain = _with_record(_device_sim(n, ET.block(**CE.ALL)), trace_envs=k)
    ext = DT.block(**CE.ALL, interval=(0.5, 1.0), force=(-5.0, 5.0), torque=(-1.0, 1.0))      # loud words behind clear bits
    wide = _with_record(_device_sim(n, ext, ev_state=False), trace_envs=k)
    assert plain._desc.ev.floats == 32 and wide._desc.ev.floats == 64 and wide._desc.ev.reserved == 0 and plain.F == wide.F
    a, b = _run_device(plain, acts, ep0), _run_device(wide, acts, ep0)
    for x, y, what in ((a, b, "slabs"), (plain.rec.cpu().numpy(), wide.rec.cpu().numpy(), "record"),
                       (plain.trace.cpu().numpy(), wide.trace.cpu().numpy(), "trace")):
        np.testing.assert_array_equal(x.view(U32), y.view(U32), err_msg=what)
    assert plain.trace[:, :, 14].sum() > 0
    # with the timer field in the row: the same bytes in front of it, zeros in it
    timed = _with_record(_device_sim(n, ext), trace_envs=k)
    c = _run_device(timed, acts, ep0)
    np.testing.assert_array_equal(c[:, :, :plain.F].view(U32), a.view(U32))
    assert not c[:, :, plain.F:].any()
    np.testing.assert_array_equal(timed.rec.cpu().numpy().view(U32), plain.rec.cpu().numpy().view(U32))


def test_clearing_the_timed_bit_mid_run_freezes_ev_state():
    n, at = 64, 20
    on = DT.block(**CD.RECIPE)
    off = on.copy()
    off.view(np.int32)[0] &= ~DT.PUSH_TIMED
    tw, acts, ep0, ref, masks, _, _ = reference(n, on, switch=(at, off))
    sim = _device_sim(n, on)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_event_block(off) if s == at else None)
    _same_bits(dev, ref, "slabs with the timed push switched off before step 20")
    st = tw.off["ev_state"][0]
    assert (dev[at:, :, st].view(U32) == dev[at, :, st].view(U32)).all() and (dev[at, :, st] > 0).all()
    all_on = reference(n, on)
    np.testing.assert_array_equal(dev[:at + 1].view(U32), all_on[3][:at + 1].view(U32))
    assert all_on[4][at:].any() and not masks[at:].any()


def _manager(sim, cfg_events, **kw):
    from cat_envs.tasks.utils.mdp import event_manager as EM
    cfg = S._env_cfg()
    env = types.SimpleNamespace(sim=sim, cfg=cfg, max_episode_length_s=cfg.episode_length_s)
    return EM.EventManager(cfg_events, env, **kw)


def _disturbance_cfg(force=(-10.0, 40.0), torque=(-1.0, 1.0)):
    from cat_envs.shim import EventTermCfg as EventTerm
    from cat_envs.tasks.utils.mdp import events as EV
    return {"push_robot": EventTerm(func=EV.push_by_setting_velocity, mode="interval", interval_range_s=CD.T_RANGE,
                                    params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5), "roll": (-20.0, 20.0),
                                                               "pitch": (-20.0, 20.0)}}),
            "wrench": EventTerm(func=EV.apply_external_force_torque, mode="reset",
                                params={"force_range": force, "torque_range": torque})}


def test_the_wrench_switched_off_gives_the_bytes_of_a_zero_range_wrench():
    n = 64
    acts, ep0 = CD.recipe(n)
    sim = _device_sim(n, DT.block())
    mgr = _manager(sim, _disturbance_cfg())
    on = _run_device(sim, acts, ep0)
    words = sim.event_words
    assert words.view(np.int32)[0] == DT.PUSH_TIMED | DT.WRENCH | DT.WRENCH_RESET
    _same_bits(on, reference(n, words)[3], "the manager's block against the twin")
    mgr.set_wrench_enabled(False)
    assert sim.event_words.view(np.int32)[0] == DT.PUSH_TIMED and (sim.event_words[1:] == words[1:]).all()
    off = _run_device(sim, acts, ep0)
    zero = _device_sim(n, DT.block())
    _manager(zero, _disturbance_cfg(force=(0.0, 0.0), torque=(0.0, 0.0)))
    assert zero.event_words.view(np.int32)[0] == words.view(np.int32)[0] and not zero.event_words[34:].any()
    np.testing.assert_array_equal(off.view(U32), _run_device(zero, acts, ep0).view(U32))
    assert (on != off).any()
    mgr.set_wrench_enabled(True)
    np.testing.assert_array_equal(_run_device(sim, acts, ep0).view(U32), on.view(U32))
    mgr.set_interval_enabled(False)                                          # clears the timed bit, too
    assert sim.event_words.view(np.int32)[0] == DT.WRENCH | DT.WRENCH_RESET


# ------------------------------------------------------------------------------------------ 3: shards and the run state
def test_two_shards_equal_the_rows_of_one_simulator():
    words = DT.block(**CD.RECIPE)
    tw, acts, ep0, ref, *_ = reference(64, words)
    whole = _run_device(_device_sim(64, words), acts, ep0)
    _same_bits(whole, ref, "the whole simulator")
    lo = _run_device(_device_sim(32, words, offset=0), np.ascontiguousarray(acts[:, :32]), ep0[:32])
    hi = _run_device(_device_sim(32, words, offset=32), np.ascontiguousarray(acts[:, 32:]), ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    st = tw.off["ev_state"][0]
    assert (lo[0, :, st] != hi[0, :, st]).any()                               # the timers follow the global env id


def _steps(sim, acts, first, last):
    """steps first .. last - 1 of the run, with the env's bookkeeping; the state buffer after each"""
    ep_len, reset, out = sim._episode_length, sim._reset, []
    for s in range(first, last):
        sim.step(acts[s])
        ep_len.add_(1)
        reset.copy_((ep_len >= MAX_LEN) | (sim.view("hard_reset")[:, 0] > 0.5))
        ep_len.masked_fill_(reset, 0)
        out.append(sim.cur.clone())
    return torch.stack(out).cpu().numpy()


def test_run_state_round_trips_mid_episode_and_the_run_continues_byte_identically():
    n, at = 64, 17
    tw, acts, ep0, ref, *_ = reference(n, DT.block(**CD.RECIPE))
    dev_acts = torch.from_numpy(acts).cuda()
    sim = _device_sim(n, DT.block())
    mgr = _manager(sim, _disturbance_cfg())
    mgr.set_wrench_enabled(False)                                             # a switch that must come back with the state
    sim._episode_length.copy_(torch.from_numpy(np.asarray(ep0, np.int64)))
    sim.step(None)
    _steps(sim, dev_acts, 0, at)
    saved = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in sim.state_dict().items()}
    counters = (sim._episode_length.clone(), sim._reset.clone())
    events = dict(mgr.state_dict())
    assert events == {"interval": True, "wrench": False} and (sim._episode_length > 0).any()      # mid-episode
    rest = _steps(sim, dev_acts, at, STEPS)
    again = _device_sim(n, DT.block())
    mgr2 = _manager(again, _disturbance_cfg())
    assert mgr2.wrench_enabled and mgr2.fingerprint() == mgr.fingerprint()
    again.load_state_dict(saved)
    again._episode_length.copy_(counters[0])
    again._reset.copy_(counters[1])
    mgr2.load_state_dict(events)
    assert not mgr2.wrench_enabled and (again.event_words == sim.event_words).all()
    np.testing.assert_array_equal(_steps(again, dev_acts, at, STEPS).view(U32), rest.view(U32))
    st = tw.off["ev_state"][0]
    assert (saved["cur"][:, st] > 0).all()                                    # the timers travel in the row


# ------------------------------------------------------------------------------------------ 4: the entry point's refusals
def test_descriptor_and_block_are_checked():
    from cat_envs import native
    sim = _device_sim(16, DT.block(**CD.RECIPE))
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    state = d.ev.reserved
    assert d.reserved == native.SERVO_EXT_EVENTS and d.ev.floats == 64 and state == sim.off["ev_state"][0]
    # every one of these raises before any launch
    for floats, reserved in ((48, state), (48, 0), (32, state), (32, 4), (32, 1), (64, 1), (64, state + 2), (64, sim.F),
                             (64, sim.off["servo"][0] // 4 * 4), (64, sim.off["obs"][0] // 4 * 4), (64, -4), (0, 0), (16, 0)):
        d.ev.floats, d.ev.reserved = floats, reserved
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.ev.floats, d.ev.reserved = 64, state
    good = d.ev.block
    for bad in (None, good + 4, d.state_in, d.state_out - 32 * 4):           # the second half of the block counts
        d.ev.block = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.ev.block = good
    sim._nat.servo_sim_step(d)
    d.ev.reserved = 0                                                         # without the field the timed bit is ignored
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    # an overlapping ev_state on a simulator with a command block: the field on cmd_state
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = S._env_cfg()
    ep_len, reset = torch.zeros(16, dtype=torch.long, device="cuda"), torch.zeros(16, dtype=torch.bool, device="cuda")
    both = Solo12ServoSim(16, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                          commands=True, disturbances=True)
    both.set_event_block(DT.block(**CD.RECIPE))
    both.set_command_block(CC.words_of(CC.commands_cfg_of()))
    b = both._desc
    b.state_out, b.action = both._slabs[0].data_ptr(), both.default_joint_pos.data_ptr()
    both._nat.servo_sim_step(b)
    b.ev.reserved = b.cmd.off_cmd_state
    with pytest.raises(RuntimeError, match="bad argument"):
        both._nat.servo_sim_step(b)
    torch.cuda.synchronize()
    # the simulator checks what the library cannot read
    w = DT.block(**CD.RECIPE)
    for at, value in ((32, 0.0), (32, -1.0), (33, -0.01), (35, -1.0), (37, -1.0), (38, 1.0), (63, 1.0), (34, float("nan")),
                      (36, float("inf"))):
        bad = w.copy()
        bad[at] = value
        with pytest.raises(ValueError, match="event block"):
            sim.set_event_block(bad)
    for flags in (256, DT.PUSH_TIMED | ET.PUSH, DT.WRENCH_RESET, ET.JOINT_SCALE | ET.JOINT_OFFSET):
        bad = w.copy()
        bad.view(np.int32)[0] = flags
        with pytest.raises(ValueError, match="event block"):
            sim.set_event_block(bad)
    with pytest.raises(ValueError, match="64 words"):
        sim.set_event_block(ET.block(**CE.ALL))
    without = _device_sim(16, DT.block(), ev_state=False)
    with pytest.raises(ValueError, match="ev_state"):
        without.set_event_block(DT.block(**CD.TIMED_ALONE))
    # an events simulator as built before refuses what it refused: the new bits, word 3, 64 words
    old = GE._device_sim(16, ET.block(**CE.ALL))
    for at, value in ((0, 32), (0, 64), (0, 128)):
        bad = ET.block(**CE.ALL)
        bad.view(np.int32)[at] |= value
        with pytest.raises(ValueError, match="event block"):
            old.set_event_block(bad)
    with pytest.raises(ValueError, match="32 words"):
        old.set_event_block(w)


# ------------------------------------------------------------------------------------------ 5: the env
def _env_cfg(task=TASK, n=64, seed=42):
    cfg = CE._cfg(task)
    cfg.synthetic.servo_resample_steps = 250
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # twelve steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    cfg.events.push_robot.interval_range_s = CD.T_RANGE
    return cfg


def test_the_task_steps_and_evaluate_policy_restores_both_switches():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    n, steps = 64, 24
    env = make(TASK, cfg=_env_cfg(n=n))
    u = env.unwrapped
    em = u.event_manager
    assert u.sim.F == 308 + 4 and u.sim._desc.ev.floats == 64 and u.sim._desc.ev.reserved == u.sim.off["ev_state"][0]
    assert em.interval_enabled and em.wrench_enabled and "push_robot" in str(em) and "base_external_force_torque" in str(em)
    assert u.state_dict()["events"] == {"interval": True, "wrench": True} and "event_terms" in u.state_fingerprint()
    obs = env.reset()[0]["policy"]
    rs = np.random.RandomState(7)
    for _ in range(6):
        obs = env.step(torch.from_numpy((rs.standard_normal((n, 12)) * 2).astype(F32)).cuda())[0]["policy"]
    assert torch.isfinite(obs).all() and (u.sim.view("ev_state")[:, 0] > 0).all() and not u.sim.view("ev_state")[:, 1:].any()
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.3).cuda()
    policy = lambda o: torch.tanh(o @ w) * 2                                  # noqa: E731
    on = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8)
    assert on.pushes and on.trace[:, :, 14].sum() > 10
    rows = on.push_recovery()                                                 # finds the timed pushes, unchanged
    assert len(rows) == int(on.trace[:, :, 14].sum()) and "push_recovery" in on.to_json()
    calm = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8, pushes=True, wrench=False)
    assert em.interval_enabled and em.wrench_enabled                          # both switches are back
    assert calm.pushes and calm.trace[:, :, 14].sum() > 10 and (calm.per_env != on.per_env).any()
    em.set_wrench_enabled(False)
    still = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8, pushes=False, wrench=True)
    assert not still.pushes and (still.trace[:, :, 14] == 0).all() and em.interval_enabled and not em.wrench_enabled
    with pytest.raises(RuntimeError, match="boom"):
        evaluate_policy(env, lambda o: (_ for _ in ()).throw(RuntimeError("boom")), 2, pushes=False, wrench=True)
    assert em.interval_enabled and not em.wrench_enabled and u.sim._desc.eval is None
    plain = make(GE.TASK, cfg=GE._env_cfg(n=16))
    with pytest.raises(TypeError, match="apply_external_force_torque"):
        evaluate_policy(plain, lambda o: torch.zeros(16, 12, device="cuda"), 2, wrench=False)
    assert plain.unwrapped.sim._desc.eval is None
    play = make(TASK.replace("-v0", "-Play-v0"), cfg=_env_cfg(TASK.replace("-v0", "-Play-v0"), n=16)).unwrapped
    assert not play.event_manager.interval_enabled and play.event_manager.wrench_enabled
    assert play.sim.event_words.view(np.int32)[0] & (DT.PUSH_TIMED | DT.WRENCH) == DT.WRENCH
