"""The servo task's terminations on the device (csrc/servo_sim.hip: the terminations-on instances, ``mdp.terminations``,
``TerminationManager``, tasks ...-Solo12-Servo-Terminations-v0 / -Reference-Terminations-v0): the kernel against
``servo_terminations_twin`` bit for bit - slabs, ``term_state``, the record, evaluation record and trace - each kind alone,
the built-in block against the launch without one, composition with the other blocks, new params between two launches, the
entry point's refusals, the env (``step`` and the fused ``step_into``), ``evaluate_policy`` and the run state.  DESIGN
section 9, "Terminations".

Test cfg: the liveness block of tests/test_servo_terminations_twin.py (all eight kinds, tilt_max 0.21), episodes of 25 steps,
60 steps of N(0, 1) actions; the CPU suite shows that every kind decides the end of some episode in this recipe at 17 envs.
Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one)."""
import json

import numpy as np
import pytest
import torch

import servo_reward_twin as RT
import servo_terminations_twin as TT
import servo_twin as T
import test_gpu_resume as RS
import test_gpu_servo_commands as GC
import test_gpu_servo_events as GE
import test_servo_commands_twin as CC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, TC.STEPS, TC.MAX_LEN
TASK, REFERENCE = TC.TASK, TC.REFERENCE
_same_bits = GE._same_bits


def _live(only=None):
    return TC.entries_of(TC.liveness_cfg(only))


def _device_sim(n, terms, commands=None, events=None, obs_table=None, table=(), tilt_max=TC.LIVE_TILT_MAX):
    """a simulator with the termination table ``terms`` (None: built without the termination descriptor); its two slabs and
    its termination record are the first ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg(tilt_max)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=0 if obs_table is None else len(obs_table), events=events is not None,
                         commands=commands is not None, terminations=terms is not None)
    if obs_table is not None:
        sim.set_observation_table(obs_table)
    if events is not None:
        sim.set_event_block(events)
    if commands is not None:
        sim.set_command_block(commands)
    sim.set_reward_table(list(table))
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    if terms is not None:
        sim.set_termination_table(terms)
        sim._guarded_record = torch.full((n + GUARD, 16), CANARY, device="cuda")
        sim._term_record = sim._guarded_record[:n]
        sim._desc.term.rec = sim._term_record.data_ptr()
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    out = GE._run_device(sim, actions, ep0, before_step=before_step, max_len=MAX_LEN)
    if sim.termination_record is not None:
        assert (sim._guarded_record[sim.N:] == CANARY).all(), "a launch wrote behind the last row of the record"
    return out


_REF = {}


def reference(n, terms, commands=None, events=None, obs_table=None, table=(), switch=None, tilt_max=TC.LIVE_TILT_MAX, **kw):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs, bits)"""
    key = (n, tuple(terms), None if commands is None else commands.tobytes(), None if events is None else events.tobytes(),
           None if obs_table is None else tuple(obs_table), tuple(table), None if switch is None else (switch[0], tuple(switch[1])),
           tilt_max, tuple(sorted(kw.items())))
    if key not in _REF:
        tw = TT.make_twin(TC.env_cfg(tilt_max), n, terms, commands=commands, events=events, obs_table=obs_table, table=table,
                          max_len=MAX_LEN, **kw)
        acts, ep0 = CC.recipe(n)
        slabs, bits = TT.run_terminations_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs, bits)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_records_and_trace_equal_the_twin_bit_for_bit(n):
    terms, k = _live(), min(n, 16)
    tw, acts, ep0, ref, bits = reference(n, terms, trace_envs=k, trace_capacity=STEPS)
    if n == 17:
        ended = tw.term_record.sum(0)
        assert all(0 < c < ended[15] for c in ended[:8]), ended                  # the CPU suite's condition
    sim = _device_sim(n, terms)
    assert sim.off == tw.off and sim.F == tw.F == 312 and sim.off["term_state"] == (308, 4)
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with the liveness block")
    a = tw.off["term_state"][0]
    np.testing.assert_array_equal(dev[1:, :, a], bits.astype(F32))
    assert not dev[:, :, a + 1:a + 4].any() and not dev[0, :, a].any()
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    _same_bits(rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(trace.cpu().numpy(), tw.trace, "trace")
    # field 2 of both is `terminated`, not the model's flag
    terminated = (bits & ~U32(1)) != 0
    np.testing.assert_array_equal(trace[:, :, 2].cpu().numpy(), terminated[:, :k].astype(F32))
    np.testing.assert_array_equal(rec[:, 2].cpu().numpy(), terminated.sum(0).astype(F32))
    # the evaluation launch (a record, no trace) and the training launch give the same rows
    sim2 = _device_sim(n, terms)
    sim2.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim2, acts, ep0), ref, "slabs of the evaluation launch")
    sim3 = _device_sim(n, terms)
    _same_bits(_run_device(sim3, acts, ep0), ref, "slabs of the training launch")
    _same_bits(sim3.termination_record.cpu().numpy(), tw.term_record, "termination record of the training launch")


@pytest.mark.parametrize("name", list(TC.LIVE_COUNTS_17)[1:])
def test_each_kind_alone_at_a_ragged_workgroup(name):
    n = 17
    terms = _live(name)
    tw, acts, ep0, ref, bits = reference(n, terms)
    assert 0 < tw.term_record[:, 1].sum() < tw.term_record[:, 15].sum(), name
    sim = _device_sim(n, terms)
    _same_bits(_run_device(sim, acts, ep0), ref, f"slabs with {name} alone")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")


# ------------------------------------------------------------------------------------------ 2: the built-in block
@pytest.mark.parametrize("rewards", [False, True])
def test_builtin_block_is_the_launch_without_a_block(rewards):
    n, k = 64, 16
    acts, ep0 = CC.recipe(n)
    table = RT.ALL_NON_EXP if rewards else ()                                 # kinds 15 and 16 among them
    got = []
    for terms in (TC.entries_of(TC.builtin_cfg()), None):
        sim = _device_sim(n, terms, table=table)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        got.append((_run_device(sim, acts, ep0), rec.cpu().numpy(), trace.cpu().numpy(), sim))
    (on, rec_on, trace_on, sim), (off, rec_off, trace_off, plain) = got
    a = sim.off["term_state"][0]
    assert a == plain.F and sim.F == plain.F + 4
    np.testing.assert_array_equal(on[:, :, :a].view(U32), off.view(U32))
    np.testing.assert_array_equal(rec_on.view(U32), rec_off.view(U32))
    np.testing.assert_array_equal(trace_on.view(U32), trace_off.view(U32))
    if rewards:
        np.testing.assert_array_equal(sim.reward_record.cpu().numpy().view(U32), plain.reward_record.cpu().numpy().view(U32))
    h = sim.off["hard_reset"][0]
    assert (on[:, :, h] > 0).sum() >= 5                                       # falls do occur
    np.testing.assert_array_equal(on[1:, :, a] >= 2, on[1:, :, h] > 0)
    # the training launches, too
    on_t = _run_device(_device_sim(n, TC.entries_of(TC.builtin_cfg()), table=table), acts, ep0)
    off_t = _run_device(_device_sim(n, None, table=table), acts, ep0)
    np.testing.assert_array_equal(on_t[:, :, :a].view(U32), off_t.view(U32))
    np.testing.assert_array_equal(on_t.view(U32), on.view(U32))


# ------------------------------------------------------------------------------------------ 3: composition
@pytest.mark.parametrize("with_commands,with_events,with_obs", [(True, True, True), (True, False, False), (False, True, False),
                                                                (False, False, True), (False, True, True)])
def test_composition_with_the_other_blocks_is_bit_exact(with_commands, with_events, with_obs):
    n = 17
    _, obs_table, events = GC._reference_blocks()
    commands = GC._words() if with_commands else None
    events, obs_table = events if with_events else None, obs_table if with_obs else None
    terms = _live()
    tw, acts, ep0, ref, bits = reference(n, terms, commands=commands, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    sim = _device_sim(n, terms, commands=commands, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    assert sim.off == tw.off and sim.F == tw.F
    _same_bits(_run_device(sim, acts, ep0), ref, "rows")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    assert tw.stats["ended_by_termination"] >= 5 and tw.stats["ended_by_time_out"] >= 5


# ------------------------------------------------------------------------------------------ 4: new params
def test_params_set_between_two_steps_are_in_the_very_next_launch():
    n, at = 64, 20
    before = _live()
    after = [(k, m, F32(0.12) if k == 3 else p0, p1) for k, m, p0, p1 in before]      # upside_down: 0.215 -> 0.12
    tw, acts, ep0, ref, bits = reference(n, before, switch=(at, after))
    sim = _device_sim(n, before)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_termination_table(after) if s == at else None)
    _same_bits(dev, ref, "slabs with the limit moved before step 20")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    old = reference(n, before)[4]
    np.testing.assert_array_equal(bits[:at], old[:at])
    fired = (bits >> U32(2)) & 1
    assert fired[at:].sum() > 3 * max(int(fired[:at].sum()), 1)               # the tighter limit fires far more often
    with pytest.raises(ValueError, match="fixed by the first call"):
        sim.set_termination_table(before[:-1])


# ------------------------------------------------------------------------------------------ 5: the entry point's refusals
def test_descriptor_and_table_are_checked():
    from cat_envs import native
    _, obs_table, events = GC._reference_blocks()
    sim = _device_sim(16, _live(), commands=GC._words(), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_TERMINATIONS and d.term.terms == 8 and d.term.off_term_state == 360 and sim.F == 364
    rec = torch.zeros(16, 12, device="cuda")
    sim.set_eval_record(rec)
    good_table, good_rec = d.term.table, d.term.rec
    others = (d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.obs.table, d.ev.block, d.cmd.block)
    for bad in (None, good_table + 4, good_table + 8, good_rec, *others):
        d.term.table = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.term.table = good_table
    for bad in (None, good_rec + 4, good_rec + 8, good_table, *others):       # misaligned, aliasing
        d.term.rec = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.term.rec = good_rec
    for terms in (0, 16, -1):
        d.term.terms = terms
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.term.terms = 8
    # off_term_state: negative, not a multiple of 4, past the row, on cmd_state, the policy field, the raw observation, joint_pos
    for off in (-4, 361, 362, 364, 1000, 356, 308, d.off_obs, d.off_servo, 0):
        d.term.off_term_state = off
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.term.off_term_state = 360
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for g in (*sim._guarded, sim._guarded_record):
        assert (g[sim.N:] == CANARY).all()
    # the simulator checks what the library cannot read
    fresh = _fresh()
    for bad, what in ((_live() + [(9, 0, 0.0, 0.0)], "unknown termination kind"), ([], "termination terms"),
                      ([(1, 0, 0.0, 0.0)] * 16, "termination terms"), ([(2, 0, 1.0, 0.0)], "body mask"),
                      ([(2, 1 << 17, 1.0, 0.0)], "body mask"), ([(6, 0x1000, 0.0, 1.0)], "joint mask"), ([(7, 0, 1.0, 0.0)], "joint mask"),
                      ([(6, 1, 1.0, 0.0)], "p0 <= p1"), ([(3, 0, float("nan"), 0.0)], "finite")):
        with pytest.raises(ValueError, match=what):
            fresh.set_termination_table(bad)
    with pytest.raises(ValueError, match="without a termination descriptor"):
        _device_sim(16, None).set_termination_table(_live())


def _fresh():
    """a simulator with the termination descriptor and no table yet"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg()
    return Solo12ServoSim(16, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN,
                          torch.zeros(16, dtype=torch.long, device="cuda"), torch.zeros(16, dtype=torch.bool, device="cuda"),
                          terminations=True)


# ------------------------------------------------------------------------------------------ 6: the env
def _env_cfg(task=TASK, n=64, seed=42, block=True):
    cfg = CC._cfg(task)
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # 25 steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    cfg.synthetic.servo_tilt_max = TC.LIVE_TILT_MAX
    cfg.terminations = TC.liveness_cfg() if block else None
    return cfg


def _make_env(cfg, task=TASK):
    from cat_envs.shim import make
    return make(task, cfg=cfg)


def test_env_steps_masks_terms_and_log_equal_the_oracle_env_on_the_twin():
    TM, Done, _ = TC._tm()
    n, steps, at = 64, 50, 25
    cfg = _env_cfg()
    env = _make_env(cfg).unwrapped
    tm = env.termination_manager
    names = list(TC.LIVE_COUNTS_17)
    assert env.max_episode_length == MAX_LEN and env.sim.F == 312 and tm.active_terms == names
    assert "termination_terms" in env.state_fingerprint() and "terminations" in env.state_dict()
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = TT.make_twin(cfg, n, _live(), seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=MAX_LEN)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    tighter = [(k, m, F32(0.15) if k == 3 else p0, p1) for k, m, p0, p1 in _live()]
    for s in range(steps):
        if s == at:                                                           # a new limit through the manager: the next launch has it
            tm.set_term_cfg("upside_down", Done(func=TM.upside_down, params={"limit": 0.15}))
            twin.set_terminations(tighter)
        a = torch.from_numpy(rs.standard_normal((n, 12)).astype(F32))
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(F32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(F32), f"dones after step {s}")
        bits = twin.bits
        np.testing.assert_array_equal(env.reset_terminated.cpu().numpy(), (bits & ~U32(1)) != 0)
        np.testing.assert_array_equal(env.reset_time_outs.cpu().numpy(), (bits & U32(1)) != 0)
        np.testing.assert_array_equal(tm.terminated.cpu().numpy() | tm.time_outs.cpu().numpy(), tm.dones.cpu().numpy())
        for k, name in enumerate(names):
            np.testing.assert_array_equal(tm.get_term(name).cpu().numpy(), (bits >> U32(k)) & 1 == 1)
    assert tm.compute() is env.reset_buf
    sums = twin.term_record.astype(np.float64).sum(0)
    assert sums[15] > 50 and all(0 < c < sums[15] for c in sums[:8])
    log = tm.pop_log()
    assert log == {f"Episode_Termination/{name}": sums[k] / sums[15] for k, name in enumerate(names)}
    assert tm.pop_log() is None and not tm.record.any()


def _free_graph(tr):
    """a trainer keeps the graph slot of its update phase for as long as the library's context lives: hand it back, so that
    the trainers of this file leave the suite the slots they found"""
    if tr._graph_id is not None:
        tr.nat.graph_destroy(tr._graph_id)
        tr._graph_id = None


def test_step_and_step_into_advance_the_same_state_and_masks():
    import test_gpu_servo_obs as OB
    n, num_steps = 64, 12
    got = []
    for fused in (True, False):
        tr = OB._trainer(_env_cfg(REFERENCE, n=n), num_steps, fused=fused, task=REFERENCE)
        u = tr.envs.unwrapped
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45 and u.sim.F == 364
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(F32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        bits = u.sim.view("term_state")[:, 0].cpu().numpy().astype(U32)
        np.testing.assert_array_equal(u.reset_terminated.cpu().numpy(), (bits & ~U32(1)) != 0)
        np.testing.assert_array_equal(u.reset_time_outs.cpu().numpy(), (bits & U32(1)) != 0)
        got.append((tr.obs.float().cpu().numpy(), u.sim.cur.cpu().numpy(), tr.rewards.float().cpu().numpy(),
                    u.sim.view("servo")[:, 13].cpu().numpy().copy()))
        _free_graph(tr)
    for x, y in zip(*got):
        np.testing.assert_array_equal(x.view(U32), y.view(U32))
    assert got[0][3].sum() >= 5                                               # episodes did end (the iteration's log popped the record)


def test_terminations_need_the_servo_simulator_and_a_task_without_them_keeps_its_row():
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    env = _make_env(_env_cfg(CC.REFERENCE, n=16, block=False), CC.REFERENCE).unwrapped
    assert env.sim.F == 360 and "term_state" not in env.sim.off and "termination_terms" not in env.state_fingerprint()
    assert "terminations" not in env.state_dict() and not hasattr(env, "termination_manager")
    from cat_envs import native
    assert env.sim._desc.reserved == native.SERVO_EXT_COMMANDS


# ------------------------------------------------------------------------------------------ 7: evaluate_policy
def test_evaluate_policy_reports_the_termination_share_only_with_the_block():
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    n, steps = 64, 40
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.5).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 3                              # noqa: E731
    res = {}
    for block in (True, False):
        env = _make_env(_env_cfg(n=n, block=block))
        res[block] = evaluate_policy(env, policy, steps, fresh_cat_state=True)
    share = res[True].termination_share
    assert list(share) == list(TC.LIVE_COUNTS_17) and all(0.0 <= v <= 1.0 for v in share.values())
    assert max(share.values()) > 0 and json.loads(res[True].to_json())["termination_share"] == share
    assert res[False].termination_share is None and "termination_share" not in json.loads(res[False].to_json())
    assert "termination_share" not in res[False].metrics
    # the periodic evaluator's env carries no block: Eval/* means the same under every termination block
    assert make_eval_env_cfg(_env_cfg(n=n), 16).terminations is None


# ------------------------------------------------------------------------------------------ 8: run state
def _resume_cfgs(block=True):
    from cat_envs.shim import load_cfg_from_registry
    cfg = CC._cfg(TASK)
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    cfg.synthetic.servo_tilt_max = TC.LIVE_TILT_MAX
    cfg.terminations = TC.liveness_cfg() if block else None
    agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 4, 10 ** 9
    return TASK, cfg, agent_cfg


def test_two_plus_two_iterations_equal_four(tmp_path, monkeypatch):
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
        seen["sd"] = u.state_dict()["terminations"]
        seen["hard"] = float(u.termination_manager.record[:, 1:8].sum()) + float(u.sim.view("hard_reset").sum())
    try:
        a, b, tr = RS.check_case(_resume_cfgs, tmp_path, save_at=2, iters=4, probe=probe)
    finally:
        for t in made:                                                        # the four trainers of the three arms
            _free_graph(t)
    assert len(made) == 4
    assert [t[0] for t in seen["fp"]["termination_terms"]] == list(TC.LIVE_COUNTS_17)
    assert list(seen["sd"]["params"]) == list(TC.LIVE_COUNTS_17) and tuple(seen["sd"]["record"].shape) == (64, 16)
    assert tr.envs.unwrapped.sim.F == 312


def test_a_state_without_the_block_is_refused_through_the_fingerprint():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl import checkpoint

    def env_of(block):
        t, cfg, _ = _resume_cfgs(block)
        cfg.scene.num_envs = 16
        env = make(t, cfg=cfg).unwrapped
        env.reset()
        return env
    with_t, without = env_of(True), env_of(False)
    assert "termination_terms" in with_t.state_fingerprint() and "termination_terms" not in without.state_fingerprint()
    with pytest.raises(ValueError, match="termination_terms"):
        checkpoint.check_fingerprint(with_t.state_fingerprint(), without.state_fingerprint())
    with pytest.raises(ValueError, match="termination_terms"):
        checkpoint.check_fingerprint(without.state_fingerprint(), with_t.state_fingerprint())
    sd = checkpoint.to_plain(with_t.state_dict())
    with pytest.raises(ValueError, match="carries terminations"):
        without.check_state_dict(sd)
    with pytest.raises(ValueError, match="terminations"):
        with_t.check_state_dict(checkpoint.to_plain(without.state_dict()))
    with_t.load_state_dict(sd)
    with_t.step(torch.zeros(16, 12, device="cuda"))
    torch.cuda.synchronize()
    assert checkpoint.FORMAT == 1
