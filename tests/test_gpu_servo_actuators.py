"""The servo task's actuator table on the device (csrc/servo_sim_kernel.h: the actuators-on instances of
servo_sim_actuators.hip, ``Solo12ServoSim(actuators=True)``): the kernel against ``servo_actuators_twin`` bit for bit - slabs,
evaluation record, trace, reward record - each actuator kind alone, the identity table against the launch without one,
composition with the action block and with all six blocks, new gains between two launches, the entry point's refusals, the
env (``step`` and the fused ``step_into``) on the new tasks, ``evaluate_policy``, the run state and the trainer on
-Servo-DelayedActuators-v0.  DESIGN section 9, "Actuators".

Test cfg: the mixed robot of tests/test_servo_actuators_twin.py (a delayed group with lags 0 .. 12, an ideal-PD group with
per-joint gains and one joint of stiffness 0, a DC-motor group), episodes of 25 steps, 60 steps of N(0, 1) actions; the CPU
suite shows that every rule of the model fires in this recipe at 17 envs.  Shapes: 1 env, 17 (a ragged workgroup), 64 and
1000 (several workgroups, a ragged last one)."""
import numpy as np
import pytest
import torch

import servo_actuators_twin as UT
import servo_reward_twin as RT
import test_gpu_servo_events as GE
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, UC.STEPS, UC.MAX_LEN
_same_bits = GE._same_bits


def _device_sim(n, actuators, actions=None, terms=None, commands=None, events=None, obs_table=None, table=(), tilt_max=None):
    """a simulator with the actuator table ``actuators`` ("identity": the simulator's own; None: built without the actuator
    descriptor) behind the action table ``actions`` = (entries, width) (None: none of its own); its two slabs are the first
    ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg(tilt_max)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=0 if obs_table is None else len(obs_table), events=events is not None,
                         commands=commands is not None, terminations=terms is not None, actions=actions is not None,
                         actuators=actuators is not None)
    if obs_table is not None:
        sim.set_observation_table(obs_table)
    if events is not None:
        sim.set_event_block(events)
    if commands is not None:
        sim.set_command_block(commands)
    if terms is not None:
        sim.set_termination_table(terms)
    sim.set_reward_table(list(table))
    if actions is not None:
        sim.set_action_table(*actions)
    if actuators is not None:
        sim.set_actuator_table(sim.identity_actuator_entries() if isinstance(actuators, str) else actuators)
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    return GE._run_device(sim, actions, ep0, before_step=before_step, max_len=MAX_LEN)


_REF = {}


def reference(n, actuators, actions=None, switch=None, tilt_max=None, **kw):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs)"""
    entries, width = actions if actions is not None else (None, 12)
    key = (n, repr(actuators), repr(entries), width, None if switch is None else (switch[0], repr(switch[1])), tilt_max,
           repr(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _REF:
        tw = UT.make_twin(TC.env_cfg(tilt_max), n, actuators=actuators, actions=entries, width=width, max_len=MAX_LEN, **kw)
        acts, ep0 = AC.recipe(n, width)
        slabs = UT.run_actuators_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_records_and_trace_equal_the_twin_bit_for_bit(n):
    robot, k = UC.mixed_entries(), min(n, 16)
    tw, acts, ep0, ref = reference(n, robot, table=RT.ALL_NON_EXP, trace_envs=k, trace_capacity=STEPS)
    sim = _device_sim(n, robot, table=RT.ALL_NON_EXP)
    assert sim.off == tw.off and sim.F == tw.F == 308 + 48 and sim.off["act_hist"] == (308, 48)
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with the mixed robot")
    _same_bits(rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(trace.cpu().numpy(), tw.trace, "trace")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    # the trace's action floats are the raw, undelayed columns
    tr = trace.cpu().numpy()
    np.testing.assert_array_equal(tr[:, :, 60:72].view(U32), acts[:, :k].view(U32))
    # the evaluation launch (a record, no trace) and the training launch give the same rows
    sim2 = _device_sim(n, robot, table=RT.ALL_NON_EXP)
    sim2.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim2, acts, ep0), ref, "slabs of the evaluation launch")
    sim3 = _device_sim(n, robot, table=RT.ALL_NON_EXP)
    _same_bits(_run_device(sim3, acts, ep0), ref, "slabs of the training launch")
    _same_bits(sim3.reward_record.cpu().numpy(), tw.reward_record, "reward record of the training launch")
    # ... and without a reward table, in all three launches
    tw0, _, _, ref0 = reference(n, robot, trace_envs=k, trace_capacity=STEPS)
    _same_bits(_run_device(_device_sim(n, robot), acts, ep0), ref0, "slabs of the training launch without rewards")
    sim4 = _device_sim(n, robot)
    sim4.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim4, acts, ep0), ref0, "slabs of the evaluation launch without rewards")
    sim5 = _device_sim(n, robot)
    rec5, trace5 = torch.zeros(n, 12, device="cuda"), torch.zeros(STEPS, k, 72, device="cuda")
    sim5.set_eval_record(rec5)
    sim5.set_trace(trace5)
    _same_bits(_run_device(sim5, acts, ep0), ref0, "slabs of the step-response launch without rewards")
    _same_bits(trace5.cpu().numpy(), tw0.trace, "trace without rewards")
    _same_bits(rec5.cpu().numpy(), tw0.record, "evaluation record without rewards")


@pytest.mark.parametrize("name", ["late", "front", "motor"])
def test_each_actuator_kind_alone_at_a_ragged_workgroup(name):
    n = 17
    robot = UC.mixed_entries(name)
    tw, acts, ep0, ref = reference(n, robot)
    _same_bits(_run_device(_device_sim(n, robot), acts, ep0), ref, f"slabs with {name} alone")


# ------------------------------------------------------------------------------------------ 2: the identity table
@pytest.mark.parametrize("rewards", [False, True])
def test_identity_table_is_the_launch_without_a_table(rewards):
    from cat_envs import native
    n, k = 64, 16
    acts, ep0 = AC.recipe(n, 12)
    table = RT.ALL_NON_EXP if rewards else ()
    got = []
    for actuators in ("identity", None):
        sim = _device_sim(n, actuators, table=table, tilt_max=TC.LIVE_TILT_MAX)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        got.append((_run_device(sim, acts, ep0), rec.cpu().numpy(), trace.cpu().numpy(), sim))
    (on, rec_on, trace_on, sim), (off, rec_off, trace_off, plain) = got
    assert sim._desc.reserved == native.SERVO_EXT_ACTUATORS and plain._desc.reserved == 0 and sim.F == plain.F + 48
    assert sim.off["act_hist"] == (plain.F, 48) and sim._desc.act.table and sim.action_width == 12
    np.testing.assert_array_equal(on[:, :, :plain.F].view(U32), off.view(U32))
    np.testing.assert_array_equal(rec_on.view(U32), rec_off.view(U32))
    np.testing.assert_array_equal(trace_on.view(U32), trace_off.view(U32))
    if rewards:
        np.testing.assert_array_equal(sim.reward_record.cpu().numpy().view(U32), plain.reward_record.cpu().numpy().view(U32))
    assert (on[:, :, sim.off["hard_reset"][0]] > 0).sum() >= 5               # falls do occur
    # the history field is the twin's
    _same_bits(on, reference(n, None, table=table, tilt_max=TC.LIVE_TILT_MAX, trace_envs=k, trace_capacity=STEPS)[3], "identity rows")
    # the training launches, too
    on_t = _run_device(_device_sim(n, "identity", table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    off_t = _run_device(_device_sim(n, None, table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    np.testing.assert_array_equal(on_t[:, :, :plain.F].view(U32), off_t.view(U32))
    np.testing.assert_array_equal(on_t.view(U32), on.view(U32))


# ------------------------------------------------------------------------------------------ 3: composition
@pytest.mark.parametrize("all_six", [False, True])
def test_composition_with_the_other_blocks_is_bit_exact(all_six):
    """False: on top of the mixed action block of A = 8; True: on top of all six reference blocks, the -Reference-Actuators row"""
    n = 17
    robot = UC.mixed_entries()
    if all_six:
        _, obs_table, events = AC.reference_blocks()
        terms = TC.entries_of(TC.liveness_cfg())
        blocks = dict(commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
        actions = (AC.reference_perm()[0], 12)
        tw, acts, ep0, ref = reference(n, robot, actions, tilt_max=TC.LIVE_TILT_MAX, terminations=terms, **blocks)
        sim = _device_sim(n, robot, actions, terms=terms, tilt_max=TC.LIVE_TILT_MAX, **blocks)
        assert sim.off == tw.off and sim.F == tw.F == 364 + 48
        _same_bits(_run_device(sim, acts, ep0), ref, "rows")
        _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
        _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
        assert tw.stats["ended_by_termination"] >= 5 and tw.stats["ended_by_time_out"] >= 1
    else:
        actions = AC.entries_of(AC.mixed_cfg())
        assert actions[1] == 8
        tw, acts, ep0, ref = reference(n, robot, actions, table=RT.ALL_NON_EXP)
        sim = _device_sim(n, robot, actions, table=RT.ALL_NON_EXP)
        assert sim.off == tw.off and sim.F == tw.F and sim.action_width == 8
        _same_bits(_run_device(sim, acts, ep0), ref, "rows")
        _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")


# ------------------------------------------------------------------------------------------ 4: new gains
def test_gains_set_between_two_steps_are_in_the_very_next_launch():
    n, at = 64, 20
    before = UC.mixed_entries()
    after = [dict(e, kp=1.0, effort_limit=1.5) if j in (1, 7, 10) else e for j, e in enumerate(before)]
    tw, acts, ep0, ref = reference(n, before, switch=(at, after))
    sim = _device_sim(n, before)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_actuator_table(after) if s == at else None)
    _same_bits(dev, ref, "slabs with gains and limits moved before step 20")
    old = reference(n, before)[3]
    np.testing.assert_array_equal(ref[:at + 1].view(U32), old[:at + 1].view(U32))
    assert (ref[at + 1:] != old[at + 1:]).any()
    tau = tw.off["applied_torque"][0]
    for j in (1, 7, 10):
        assert np.abs(ref[at + 1:, :, tau + j]).max() <= 1.5 < np.abs(ref[1:at + 1, :, tau + j]).max()
    with pytest.raises(ValueError, match="fixed by the first call"):
        sim.set_actuator_table([dict(e, max_delay=4) if j >= 9 else e for j, e in enumerate(before)])
    with pytest.raises(ValueError, match="fixed by the first call"):
        sim.set_actuator_table([{k: v for k, v in e.items() if k != "dc_motor"} for e in before])


# ------------------------------------------------------------------------------------------ 5: the entry point's refusals
def _fresh():
    """a simulator with the actuator descriptor and no table yet"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg()
    return Solo12ServoSim(16, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN,
                          torch.zeros(16, dtype=torch.long, device="cuda"), torch.zeros(16, dtype=torch.bool, device="cuda"),
                          actuators=True)


def test_descriptor_and_table_are_checked():
    from cat_envs import native
    _, obs_table, events = AC.reference_blocks()
    sim = _device_sim(16, UC.mixed_entries(), AC.entries_of(AC.mixed_cfg()), terms=TC.entries_of(TC.liveness_cfg()),
                      commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    d = sim._desc
    action = torch.zeros(16, 8, device="cuda")
    d.state_out, d.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_ACTUATORS and d.actu.reserved == 0 and d.actu.off_act_hist == sim.off["act_hist"][0]
    sim.set_eval_record(torch.zeros(16, 12, device="cuda"))
    good = d.actu.table
    others = (d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, d.obs.table, d.ev.block, d.cmd.block,
              d.term.table, d.term.rec, d.act.table, d.act.table + 32, d.act.table - 32)
    for bad in (None, good + 4, good + 8, *others):                           # NULL, misaligned, aliasing
        d.actu.table = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.actu.table = good
    hist = d.actu.off_act_hist
    bad_offsets = (-4, hist + 2, hist + 4, sim.F - 44, sim.F, sim.off["joint_pos"][0], sim.off["obs"][0] - 44,
                   sim.off["policy_obs"][0], sim.off["cmd_state"][0], sim.off["term_state"][0] - 44)
    for off in bad_offsets:                                                   # outside the row, misaligned, on another field
        d.actu.off_act_hist = off
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.actu.off_act_hist = hist
    d.actu.reserved = 1
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.actu.reserved = 0
    good_act = d.act.table
    d.act.table = None                                                        # under this value the action table is never absent
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.act.table = good_act
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all()
    # every older value of `reserved` keeps its meaning: the same descriptor announced as actions runs the actions launch
    d.reserved = native.SERVO_EXT_ACTIONS
    sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_ACTUATORS
    torch.cuda.synchronize()
    # the simulator checks what the library cannot read
    ok = UC.mixed_entries()
    edit = lambda j, **kw: [dict(e, **kw) if i == j else e for i, e in enumerate(ok)]   # noqa: E731
    for bad, what in ((edit(0, kp=float("nan")), "finite"), (edit(0, kd=-0.1), "finite and >= 0"), (edit(0, inertia=0.0), "inertia"),
                      (edit(0, effort_limit=float("inf")), "finite"), (edit(6, velocity_limit=0.0), "DC motor"),
                      (edit(6, saturation_effort=None), "DC motor"), (edit(9, min_delay=5, max_delay=4), "delay"),
                      (edit(9, max_delay=13), "delay"), (edit(9, min_delay=-1), "delay"), (edit(9, max_delay=6), "share one lag"),
                      (edit(0, group=256), "group"), (edit(0, stiffness=1.0), "unknown actuator fields"), (ok[:-1], "one entry per joint")):
        with pytest.raises(ValueError, match=what):
            _fresh().set_actuator_table(bad)
    with pytest.raises(ValueError, match="without an actuator descriptor"):
        _device_sim(16, None, AC.entries_of(AC.mixed_cfg())).set_actuator_table(ok)


# ------------------------------------------------------------------------------------------ 6: the env
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Actuators-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Actuators-v0"
DELAYED = "Isaac-Velocity-CaT-Flat-Solo12-Servo-DelayedActuators-v0"


def _env_cfg(task=TASK, n=64, seed=42):
    cfg = CC._cfg(task)
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # 25 steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    return cfg


def _make_env(cfg, task=TASK):
    from cat_envs.shim import make
    return make(task, cfg=cfg)


def _free_graph(tr):
    """a trainer keeps the graph slot of its update phase for as long as the library's context lives: hand it back, so that
    the trainers of this file leave the suite the slots they found"""
    if tr._graph_id is not None:
        tr.nat.graph_destroy(tr._graph_id)
        tr._graph_id = None


def test_env_steps_equal_the_oracle_env_on_the_twin_and_the_model_speaks_isaaclab():
    import servo_twin as T
    from cat_envs.tasks.utils.mdp import actuators as UM
    n, steps, at = 64, 40, 20
    cfg = _env_cfg(DELAYED)
    env = _make_env(cfg, DELAYED).unwrapped
    am = env.actuators
    assert am.active_groups == ["legs"] and am.get_group("legs")["kind"] == "delayed_pd" and am.get_group("legs")["max_delay"] == 4
    assert am.stiffness.tolist() == [4.0] * 12 and am.effort_limit.tolist() == [10.0] * 12 and am.damping.shape == (12,)
    assert env.act_dim == 12 and env.sim.F == 308 + 48 and "actuators" in env.state_fingerprint() and "actuators" in env.state_dict()
    assert "actuators.legs.velocity_limit" in am.spec()["inert"] and am.spec()["groups"]["legs"]["max_delay"] == 4
    entries = UM.build_table(cfg.scene.robot, T.JOINTS, cfg.synthetic, cfg.decimation, T.DEFAULT_JOINT_POS)[0]
    assert am.entries == entries
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = UT.make_twin(cfg, n, actuators=entries, seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=MAX_LEN)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    for s in range(steps):
        if s == at:                                                           # new gains through the model: the next launch has them
            am.set_gains(stiffness={".*_KFE": 2.0}, damping=0.1, effort_limit=1.0, joint_names=["FL_.*", "HR_.*"])
            soft = [dict(e, kp=2.0 if j % 3 == 2 else e["kp"], kd=float(F32(0.1)), effort_limit=1.0) if j < 3 or j >= 9 else e
                    for j, e in enumerate(entries)]
            twin.set_actuators(soft)
            assert am.entries == soft
        a = torch.from_numpy(rs.standard_normal((n, 12)).astype(F32))
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(F32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(F32), f"dones after step {s}")
    assert am.get_group("legs")["stiffness"][:3] == [4.0, 4.0, 2.0] and am.stiffness.tolist()[3:9] == [4.0] * 6
    tau = env.sim.view("applied_torque").cpu().numpy()
    assert np.abs(tau[:, [0, 1, 2, 9, 10, 11]]).max() <= 1.0
    with pytest.raises(ValueError, match="'nope' not found"):
        am.get_group("nope")
    with pytest.raises(ValueError, match="match no joint"):
        am.set_gains(stiffness=1.0, joint_names="XX_.*")
    with pytest.raises(ValueError, match="finite and >= 0"):
        am.set_gains(damping=-1.0)


def test_step_and_step_into_advance_the_same_state():
    import test_gpu_servo_obs as OB
    n, num_steps = 64, 12
    got = []
    for fused in (True, False):
        cfg = _env_cfg(REFERENCE, n=n)
        cfg.synthetic.servo_tilt_max = TC.LIVE_TILT_MAX
        tr = OB._trainer(cfg, num_steps, fused=fused, task=REFERENCE)
        u = tr.envs.unwrapped
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45 and u.sim.F == 364 + 48 and u.act_dim == 12
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(F32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        got.append((tr.obs.float().cpu().numpy(), u.sim.cur.cpu().numpy(), tr.rewards.float().cpu().numpy(),
                    u.sim.view("servo")[:, 13].cpu().numpy().copy()))
        _free_graph(tr)
    for x, y in zip(*got):
        np.testing.assert_array_equal(x.view(U32), y.view(U32))
    assert got[0][3].sum() >= 5                                               # episodes did end
    assert (got[0][1][:, 364 + 12] == 1).all()                                # the history field is live


def test_a_robot_needs_the_servo_simulator_and_a_task_without_one_keeps_its_row():
    from cat_envs import native
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    parent = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Actions-v0"
    env = _make_env(_env_cfg(parent, n=16), parent).unwrapped
    assert env.sim.F == 364 and "actuators" not in env.state_fingerprint() and "actuators" not in env.state_dict()
    assert not hasattr(env, "actuators") and env.sim._desc.reserved == native.SERVO_EXT_ACTIONS
    env = _make_env(_env_cfg(n=16)).unwrapped
    assert env.sim._desc.reserved == native.SERVO_EXT_ACTUATORS and type(env.action_manager).__name__ == "_ActionManager"


# ------------------------------------------------------------------------------------------ 7: evaluation
def test_evaluate_policy_runs_on_the_tasks_and_the_periodic_evaluator_keeps_the_robot():
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    n, steps = 64, 40
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.5).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 3                              # noqa: E731
    for task in (TASK, DELAYED):
        res = evaluate_policy(_make_env(_env_cfg(task, n=n), task), policy, steps, fresh_cat_state=True)
        assert np.isfinite(res.per_env).all() and res.per_env[:, 0].min() == steps
    ecfg = make_eval_env_cfg(_env_cfg(REFERENCE, n=n), 16)
    assert ecfg.scene.robot is not None and ecfg.actions is not None and ecfg.events is None
    env = _make_env(ecfg, REFERENCE).unwrapped
    assert env.actuators.active_groups == ["legs"] and env.sim.off["act_hist"][1] == 48


# ------------------------------------------------------------------------------------------ 8: run state and trainer
def _resume_cfgs():
    import test_gpu_resume as RS
    from cat_envs.shim import load_cfg_from_registry
    cfg = CC._cfg(DELAYED)
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    agent_cfg = load_cfg_from_registry(DELAYED, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 2, 10 ** 9
    return DELAYED, cfg, agent_cfg


def test_trainer_two_iterations_finite_and_one_plus_one_equal_two(tmp_path, monkeypatch):
    """2 iterations at 64 envs x 8 steps on the delayed task; the parameters are finite and a run resumed after iteration 1
    is the same run, the history field of the simulator's state included"""
    import test_gpu_resume as RS
    seen, made = {}, []
    build = RS.build

    def recording_build(cfgs):
        env, tr = build(cfgs)
        made.append(tr)
        return env, tr
    monkeypatch.setattr(RS, "build", recording_build)

    def probe(env, tr):
        u = env.unwrapped
        seen["fp"] = u.state_fingerprint()
        seen["sd"] = u.state_dict()["actuators"]
        seen["hist"] = u.sim.view("act_hist").cpu().numpy().copy()
    try:
        a, b, tr = RS.check_case(_resume_cfgs, tmp_path, save_at=1, iters=2, probe=probe)
    finally:
        for t in made:
            _free_graph(t)
    assert len(seen["fp"]["actuators"]) == 12 and seen["fp"]["actuators"][0] == [0, False, 0, 4] and len(seen["sd"]["params"]) == 12
    assert (seen["hist"][:, 12] == 1).all() and np.abs(seen["hist"][:, :12]).max() > 0
    for it in a:
        assert np.isfinite(it["flat"]).all() and np.isfinite(it["actions"]).all() and np.isfinite(it["sim.cur"]).all()
        assert it["sim.cur"].shape[1] == 308 + 48
    assert (a[0]["flat"] != a[1]["flat"]).any()                               # the update moved the parameters


def test_a_state_without_the_robot_is_refused_through_the_fingerprint():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl import checkpoint

    def env_of(robot):
        t, cfg, _ = _resume_cfgs()
        cfg.scene.num_envs = 16
        if not robot:
            cfg.scene.robot = None
        env = make(t, cfg=cfg).unwrapped
        env.reset()
        return env
    with_r, without = env_of(True), env_of(False)
    assert "actuators" in with_r.state_fingerprint() and "actuators" not in without.state_fingerprint()
    with pytest.raises(ValueError, match="actuators"):
        checkpoint.check_fingerprint(with_r.state_fingerprint(), without.state_fingerprint())
    sd = checkpoint.to_plain(with_r.state_dict())
    with pytest.raises(ValueError, match="carries actuators"):
        without.check_state_dict(sd)
    with pytest.raises(ValueError, match="actuators"):
        with_r.check_state_dict(checkpoint.to_plain(without.state_dict()))
    with_r.actuators.set_gains(stiffness=1.0)
    with_r.load_state_dict(sd)
    assert with_r.actuators.stiffness.tolist() == [4.0] * 12                  # the saved gains are back, on the device too
    with_r.step(torch.zeros(16, 12, device="cuda"))
    torch.cuda.synchronize()
