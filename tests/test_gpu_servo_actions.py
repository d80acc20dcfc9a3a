"""The servo task's action block on the device (csrc/servo_sim_kernel.h: the actions-on instances of servo_sim_actions.hip,
``mdp.actions``, ``ActionManager``, tasks ...-Solo12-Servo-Actions-v0 / -Reference-Actions-v0): the kernel against
``servo_actions_twin`` bit for bit - slabs, evaluation record, trace, reward record - each kind alone, the identity block
against the launch without one, composition with the five other blocks, new scale and clip between two launches, the entry
point's refusals, the env (``step`` and the fused ``step_into``), ``evaluate_policy``, the run state and the trainer at
A = 12 and A = 8.  DESIGN section 9, "Actions".

Test cfg: the mixed block of tests/test_servo_actions_twin.py (all four kinds, five clips, four undriven joints, A = 8),
episodes of 25 steps, 60 steps of N(0, 1) actions; the CPU suite shows that every kind drives, clips and saturates in this
recipe at 17 envs.  Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one)."""
import numpy as np
import pytest
import torch

import servo_actions_twin as AT
import servo_reward_twin as RT
import servo_twin as T
import test_gpu_resume as RS
import test_gpu_servo_events as GE
import test_servo_actions_twin as AC
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, AC.STEPS, AC.MAX_LEN
TASK, REFERENCE = AC.TASK, AC.REFERENCE
_same_bits = GE._same_bits


def _mixed(only=None):
    return AC.entries_of(AC.mixed_cfg(only))


def _identity(cfg=None):
    cfg = cfg or TC.env_cfg()
    return AT.identity_entries(cfg.synthetic.servo_action_scale), 12


def _device_sim(n, actions, terms=None, commands=None, events=None, obs_table=None, table=(), tilt_max=None):
    """a simulator with the action table ``actions`` = (entries, width) (None: built without the action descriptor); its two
    slabs are the first ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg(tilt_max)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=0 if obs_table is None else len(obs_table), events=events is not None,
                         commands=commands is not None, terminations=terms is not None, actions=actions is not None)
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
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    return GE._run_device(sim, actions, ep0, before_step=before_step, max_len=MAX_LEN)


_REF = {}


def reference(n, actions, switch=None, tilt_max=None, **kw):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs)"""
    entries, width = actions
    key = (n, repr(entries), width, None if switch is None else (switch[0], repr(switch[1])), tilt_max,
           repr(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _REF:
        tw = AT.make_twin(TC.env_cfg(tilt_max), n, actions=entries, width=width, max_len=MAX_LEN, **kw)
        acts, ep0 = AC.recipe(n, width)
        slabs = AT.run_actions_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_records_and_trace_equal_the_twin_bit_for_bit(n):
    actions, k = _mixed(), min(n, 16)
    assert actions[1] == 8
    tw, acts, ep0, ref = reference(n, actions, table=RT.ALL_NON_EXP, trace_envs=k, trace_capacity=STEPS)
    sim = _device_sim(n, actions, table=RT.ALL_NON_EXP)
    assert sim.off == tw.off and sim.F == tw.F == 308 and sim.action_width == 8
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with the mixed block")
    _same_bits(rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(trace.cpu().numpy(), tw.trace, "trace")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    # the trace's action floats and the last-action block are the raw columns, zero past the width
    tr = trace.cpu().numpy()
    assert not tr[:, :, 68:72].any() and np.abs(tr[:, :, 60:68]).max() > 1
    a = tw.off["obs"][0] + 33
    assert not dev[:, :, a + 8:a + 12].any()
    # the evaluation launch (a record, no trace) and the training launch give the same rows
    sim2 = _device_sim(n, actions, table=RT.ALL_NON_EXP)
    sim2.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim2, acts, ep0), ref, "slabs of the evaluation launch")
    sim3 = _device_sim(n, actions, table=RT.ALL_NON_EXP)
    _same_bits(_run_device(sim3, acts, ep0), ref, "slabs of the training launch")
    _same_bits(sim3.reward_record.cpu().numpy(), tw.reward_record, "reward record of the training launch")
    # ... and without a reward table
    _, _, _, ref0 = reference(n, actions)
    _same_bits(_run_device(_device_sim(n, actions), acts, ep0), ref0, "slabs of the training launch without rewards")


@pytest.mark.parametrize("name", ["legs", "swing", "spin", "push"])
def test_each_kind_alone_at_a_ragged_workgroup(name):
    n = 17
    actions = _mixed(name)
    tw, acts, ep0, ref = reference(n, actions)
    _same_bits(_run_device(_device_sim(n, actions), acts, ep0), ref, f"slabs with {name} alone")


# ------------------------------------------------------------------------------------------ 2: the identity block
@pytest.mark.parametrize("rewards", [False, True])
def test_identity_block_is_the_launch_without_a_block(rewards):
    n, k = 64, 16
    acts, ep0 = AC.recipe(n, 12)
    table = RT.ALL_NON_EXP if rewards else ()                                 # kinds 11 and 12 among them
    assert {11, 12} <= {row[0] for row in RT.ALL_NON_EXP}
    got = []
    for actions in (_identity(), None):
        sim = _device_sim(n, actions, table=table, tilt_max=TC.LIVE_TILT_MAX)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        got.append((_run_device(sim, acts, ep0), rec.cpu().numpy(), trace.cpu().numpy(), sim))
    (on, rec_on, trace_on, sim), (off, rec_off, trace_off, plain) = got
    from cat_envs import native
    assert sim._desc.reserved == native.SERVO_EXT_ACTIONS and plain._desc.reserved == 0 and sim.F == plain.F
    np.testing.assert_array_equal(on.view(U32), off.view(U32))
    np.testing.assert_array_equal(rec_on.view(U32), rec_off.view(U32))
    np.testing.assert_array_equal(trace_on.view(U32), trace_off.view(U32))
    if rewards:
        np.testing.assert_array_equal(sim.reward_record.cpu().numpy().view(U32), plain.reward_record.cpu().numpy().view(U32))
    assert (on[:, :, sim.off["hard_reset"][0]] > 0).sum() >= 5               # falls do occur
    # the training launches, too
    on_t = _run_device(_device_sim(n, _identity(), table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    off_t = _run_device(_device_sim(n, None, table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    np.testing.assert_array_equal(on_t.view(U32), off_t.view(U32))
    np.testing.assert_array_equal(on_t.view(U32), on.view(U32))


# ------------------------------------------------------------------------------------------ 3: composition
@pytest.mark.parametrize("with_commands,with_events,with_obs", [(True, True, True), (False, True, False), (True, False, True)])
def test_composition_with_the_other_blocks_is_bit_exact(with_commands, with_events, with_obs):
    """(True, True, True) is the -Reference-Actions row: the reference's action block on top of all five other blocks"""
    n = 17
    _, obs_table, events = AC.reference_blocks()
    commands = CC.words_of(CC.commands_cfg_of()) if with_commands else None
    events, obs_table = events if with_events else None, obs_table if with_obs else None
    terms = TC.entries_of(TC.liveness_cfg())
    actions = (AC.reference_perm()[0], 12) if with_commands and with_events and with_obs else _mixed()
    kw = dict(terminations=terms, commands=commands, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    tw, acts, ep0, ref = reference(n, actions, tilt_max=TC.LIVE_TILT_MAX, **kw)
    sim = _device_sim(n, actions, terms=terms, commands=commands, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP,
                      tilt_max=TC.LIVE_TILT_MAX)
    assert sim.off == tw.off and sim.F == tw.F
    if with_commands and with_events and with_obs:
        assert sim.F == 364                                                   # the -Reference-Terminations row: actions add no field
    _same_bits(_run_device(sim, acts, ep0), ref, "rows")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    # episodes end, so that first states are drawn; under the mixed block almost every one ends by a termination term
    assert tw.stats["ended_by_termination"] >= 5 and tw.stats["ended_by_time_out"] >= (5 if actions[1] == 12 else 1)


# ------------------------------------------------------------------------------------------ 4: new scale and clip
def test_scale_and_clip_set_between_two_steps_are_in_the_very_next_launch():
    n, at = 64, 20
    before = _mixed()
    after = ([(c, k, F32(0.5) if j == 11 else s, o, (F32(-1.0), F32(0.25)) if j == 3 else cl)
              for j, (c, k, s, o, cl) in enumerate(before[0])], 8)          # push: scale 2.5 -> 0.5; swing/FR_HAA: clip tighter
    tw, acts, ep0, ref = reference(n, before, switch=(at, after[0]))
    sim = _device_sim(n, before)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_action_table(*after) if s == at else None)
    _same_bits(dev, ref, "slabs with scale and clip moved before step 20")
    old = reference(n, before)[3]
    np.testing.assert_array_equal(ref[:at + 1].view(U32), old[:at + 1].view(U32))
    assert (ref[at + 1:] != old[at + 1:]).any()
    tau = tw.off["applied_torque"][0] + 11
    assert np.abs(ref[at + 1:, :, tau]).max() <= 2.5 < np.abs(ref[1:at + 1, :, tau]).max()   # |0.5 a + 0.5| stays below 2.5 here
    with pytest.raises(ValueError, match="fixed by the first call"):
        sim.set_action_table([(c, k, s, o, None) for c, k, s, o, _ in before[0]], 8)


# ------------------------------------------------------------------------------------------ 5: the entry point's refusals
def test_descriptor_and_table_are_checked():
    from cat_envs import native
    _, obs_table, events = AC.reference_blocks()
    sim = _device_sim(16, _mixed(), terms=TC.entries_of(TC.liveness_cfg()), commands=CC.words_of(CC.commands_cfg_of()),
                      events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    d = sim._desc
    action = torch.zeros(16, 8, device="cuda")
    d.state_out, d.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_ACTIONS and d.act.width == 8 and d.act.reserved == 0
    sim.set_eval_record(torch.zeros(16, 12, device="cuda"))
    good = d.act.table
    others = (d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, d.obs.table, d.ev.block, d.cmd.block,
              d.term.table, d.term.rec)
    for bad in (None, good + 4, good + 8, *others):                           # NULL, misaligned, aliasing
        d.act.table = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.act.table = good
    for width in (0, 13, -1):
        d.act.width = width
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.act.width = 8
    d.act.reserved = 1
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.act.reserved = 0
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all()
    # a descriptor with actions and no terminations: the termination descriptor is marked absent
    plain = _device_sim(16, _mixed())
    assert plain._desc.reserved == native.SERVO_EXT_ACTIONS and plain._desc.term.terms == 0 and not plain._desc.term.table
    # the simulator checks what the library cannot read
    fresh = _fresh()
    ok = _mixed()[0]
    edit = lambda j, **kw: [tuple(kw.get(f, v) for f, v in zip(("col", "kind", "scale", "offset", "clip"), e)) if i == j else e  # noqa: E731
                            for i, e in enumerate(ok)]
    for bad, width, what in ((edit(0, kind=5), 8, "unknown action kind"), (edit(0, col=8), 8, "column"), (edit(5, col=3), 8, "column"),
                             (edit(0, col=-1), 8, "column"), (edit(0, col=3), 8, "one joint each"), (ok, 9, "one joint each"),
                             (ok, 0, "width"), (ok, 13, "width"), (ok[:-1], 8, "one entry per joint"),
                             (edit(0, scale=float("nan")), 8, "finite"), (edit(0, offset=float("inf")), 8, "finite"),
                             (edit(2, clip=(1.0, -1.0)), 8, "lo <= hi"), (edit(2, clip=(0.0, float("nan"))), 8, "lo <= hi")):
        with pytest.raises(ValueError, match=what):
            fresh.set_action_table(bad, width)
    with pytest.raises(ValueError, match="without an action descriptor"):
        _device_sim(16, None).set_action_table(*_mixed())
    with pytest.raises(ValueError, match=r"the simulator reads\s+\[16, 8\]"):
        plain.advance(torch.zeros(16, 12, device="cuda"))


def _fresh():
    """a simulator with the action descriptor and no table yet"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg()
    return Solo12ServoSim(16, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN,
                          torch.zeros(16, dtype=torch.long, device="cuda"), torch.zeros(16, dtype=torch.bool, device="cuda"),
                          actions=True)


# ------------------------------------------------------------------------------------------ 6: the env
def _env_cfg(task=TASK, n=64, seed=42, block="keep"):
    cfg = CC._cfg(task)
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # 25 steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    if block == "mixed":
        cfg.actions = AC.mixed_cfg()
    elif block is None:
        cfg.actions = None
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


def test_env_steps_equal_the_oracle_env_on_the_twin_and_the_manager_speaks_isaaclab():
    AM = AC._am()
    n, steps, at = 64, 40, 20
    cfg = _env_cfg(block="mixed")
    env = _make_env(cfg).unwrapped
    am = env.action_manager
    assert env.act_dim == am.total_action_dim == 8 and env.single_action_space.shape == (8,)
    assert am.active_terms == ["legs", "swing", "spin", "push"] and am.action_term_dim == [3, 2, 2, 1]
    assert am.action.shape == (n, 8) and am.prev_action.shape == (n, 8)
    assert "action_terms" in env.state_fingerprint() and "actions" in env.state_dict()
    assert am.get_term("swing").joint_names == ["FR_HFE", "FR_HAA"] and am.get_term("swing").action_dim == 2
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    entries, width = _mixed()
    twin = AT.make_twin(cfg, n, actions=entries, width=width, seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=MAX_LEN)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    orc.action, orc.prev_action = np.zeros((n, 8), F32), np.zeros((n, 8), F32)     # the oracle env's action history is [N, A], too
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    softer = AM.JointEffortActionCfg(joint_names=["HR_KFE"], scale=0.5, offset=0.5, clip={"HR_KFE": (-1.0, 0.75)})
    for s in range(steps):
        if s == at:                                                           # new values through the manager: the next launch has them
            am.set_term_cfg("push", softer)
            twin.set_actions([(c, k, F32(0.5), o, (F32(-1.0), F32(0.75))) if j == 11 else (c, k, sc, o, cl)
                              for j, (c, k, sc, o, cl) in enumerate(entries)], 8)
        a = torch.from_numpy(rs.standard_normal((n, 8)).astype(F32))
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(F32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(F32), f"dones after step {s}")
    p = am.get_term("push").processed_actions.cpu().numpy()
    raw = am.get_term("push").raw_actions.cpu().numpy()
    np.testing.assert_array_equal(p, np.clip(raw * F32(0.5) + F32(0.5), F32(-1.0), F32(0.75)))
    assert am.get_term_cfg("push") is softer and am.spec()["columns"][7]["scale"] == 0.5
    with pytest.raises(ValueError, match="'push'.*fixed"):
        am.set_term_cfg("push", AM.JointEffortActionCfg(joint_names=["HR_HFE"]))
    with pytest.raises(ValueError, match="'nope' not found"):
        am.get_term("nope")


def test_step_and_step_into_advance_the_same_state():
    import test_gpu_servo_obs as OB
    n, num_steps = 64, 12
    got = []
    for fused in (True, False):
        cfg = _env_cfg(REFERENCE, n=n)
        cfg.synthetic.servo_tilt_max = TC.LIVE_TILT_MAX
        tr = OB._trainer(cfg, num_steps, fused=fused, task=REFERENCE)
        u = tr.envs.unwrapped
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45 and u.sim.F == 364 and u.act_dim == 12
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


def test_actions_need_the_servo_simulator_and_a_task_without_them_keeps_its_row():
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    env = _make_env(_env_cfg(TC.REFERENCE, n=16), TC.REFERENCE).unwrapped
    assert env.sim.F == 364 and "action_terms" not in env.state_fingerprint() and "actions" not in env.state_dict()
    assert type(env.action_manager).__name__ == "_ActionManager" and env.act_dim == 12
    from cat_envs import native
    assert env.sim._desc.reserved == native.SERVO_EXT_TERMINATIONS
    # a last_action observation term has the block's width, or its term's columns
    from cat_envs.shim import ObservationTermCfg as ObsTerm
    from cat_envs.tasks.utils.mdp import observations as O
    cfg = _env_cfg(REFERENCE, n=16, block="mixed")
    env = _make_env(cfg, REFERENCE).unwrapped
    assert env.obs_dim == 45 - 12 + 8 and env.observation_manager.group_obs_term_dim["policy"][-1] == (8,)
    cfg = _env_cfg(REFERENCE, n=16, block="mixed")
    cfg.observations.policy.actions = ObsTerm(func=O.last_action, params={"action_name": "spin"})
    env = _make_env(cfg, REFERENCE).unwrapped
    assert env.obs_dim == 45 - 12 + 2 and env.observation_manager.entries[-2][0] == 33 + 5
    cfg = _env_cfg(REFERENCE, n=16, block="mixed")
    cfg.observations.policy.actions = ObsTerm(func=O.last_action, params={"action_name": "nope"})
    with pytest.raises(ValueError, match="'actions'.*'nope'"):
        _make_env(cfg, REFERENCE)


# ------------------------------------------------------------------------------------------ 7: evaluation
def test_evaluate_policy_runs_on_the_task_and_the_periodic_evaluator_keeps_the_block():
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    n, steps = 64, 40
    for block, width in (("keep", 12), ("mixed", 8)):
        w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, width)).astype(F32) * 0.5).cuda()
        policy = lambda obs: torch.tanh(obs @ w) * 3                          # noqa: E731
        res = evaluate_policy(_make_env(_env_cfg(n=n, block=block)), policy, steps, fresh_cat_state=True)
        assert np.isfinite(res.per_env).all() and res.per_env[:, 0].min() == steps
    ecfg = make_eval_env_cfg(_env_cfg(REFERENCE, n=n), 16)
    assert ecfg.actions is not None and ecfg.events is None and ecfg.terminations is None
    env = _make_env(ecfg, REFERENCE).unwrapped
    assert type(env.action_manager).__name__ == "ActionManager" and env.action_manager.entries == AC.reference_perm()[0]


# ------------------------------------------------------------------------------------------ 8: run state and trainer
def _resume_cfgs(block="keep"):
    from cat_envs.shim import load_cfg_from_registry
    cfg = CC._cfg(TASK)
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    if block == "mixed":
        cfg.actions = AC.mixed_cfg()
    elif block is None:
        cfg.actions = None
    agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 2, 10 ** 9
    return TASK, cfg, agent_cfg


@pytest.mark.parametrize("block,width", [("keep", 12), ("mixed", 8)])
def test_trainer_two_iterations_finite_and_one_plus_one_equal_two(tmp_path, monkeypatch, block, width):
    """2 iterations at 64 envs x 8 steps; the parameters are finite and a run resumed after iteration 1 is the same run"""
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
        seen["sd"] = u.state_dict()["actions"]
        seen["width"] = (u.act_dim, tuple(tr.actions.shape))
    try:
        a, b, tr = RS.check_case(lambda: _resume_cfgs(block), tmp_path, save_at=1, iters=2, probe=probe)
    finally:
        for t in made:
            _free_graph(t)
    assert seen["width"] == (width, (8, 64, width)) and len(seen["fp"]["action_terms"]) == 12 and len(seen["sd"]["params"]) == 12
    for it in a:
        assert np.isfinite(it["flat"]).all() and np.isfinite(it["actions"]).all() and np.isfinite(it["sim.cur"]).all()
    assert (a[0]["flat"] != a[1]["flat"]).any()                               # the update moved the parameters


def test_a_state_without_the_block_is_refused_through_the_fingerprint():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl import checkpoint

    def env_of(block):
        t, cfg, _ = _resume_cfgs(block)
        cfg.scene.num_envs = 16
        env = make(t, cfg=cfg).unwrapped
        env.reset()
        return env
    with_a, without = env_of("keep"), env_of(None)
    assert "action_terms" in with_a.state_fingerprint() and "action_terms" not in without.state_fingerprint()
    with pytest.raises(ValueError, match="action_terms"):
        checkpoint.check_fingerprint(with_a.state_fingerprint(), without.state_fingerprint())
    sd = checkpoint.to_plain(with_a.state_dict())
    with pytest.raises(ValueError, match="carries actions"):
        without.check_state_dict(sd)
    with pytest.raises(ValueError, match="actions"):
        with_a.check_state_dict(checkpoint.to_plain(without.state_dict()))
    with_a.load_state_dict(sd)
    with_a.step(torch.zeros(16, 12, device="cuda"))
    torch.cuda.synchronize()
