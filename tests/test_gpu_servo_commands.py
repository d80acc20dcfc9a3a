"""The servo task's commands on the device (csrc/servo_sim.hip: the commands-on instances, ``mdp.commands``,
``CommandManager``, tasks ...-Solo12-Servo-Commands-v0 / -Reference-v0): the kernel against ``servo_commands_twin`` bit for
bit - the dead-zone class, each rule alone, the base class, record and trace, composition with rewards, observations and
events, shards, fixed commands, ``set_ranges``, the entry point's refusals and the env.  DESIGN section 9, "Commands".

Test cfg: the dead-zone class with p_move = 0.05, p_still = 0.3, a timed resample every 0.1 .. 0.3 s, episodes of 25 steps,
60 steps of N(0, 1) actions; tests/test_servo_commands_twin.py shows on the CPU that every rule fires at least five times
in this recipe at 17 envs.  Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one)."""
import types

import numpy as np
import pytest
import torch

import servo_commands_twin as CT
import servo_reward_twin as RT
import servo_twin as T
import test_gpu_servo_events as GE
import test_gpu_servo_sim as S
import test_servo_commands_twin as CC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, CC.STEPS, CC.MAX_LEN
TASK, REFERENCE = CC.TASK, CC.REFERENCE
_same_bits = GE._same_bits


def _words(cls="deadzone", flags=None, **over):
    return CC.words_of(CC.commands_cfg_of(cls, **over), flags)


def _device_sim(n, commands, events=None, obs_table=None, table=(), offset=0, descriptor=None):
    """a simulator with the command block ``commands`` (None: built without the command descriptor, unless ``descriptor``
    says otherwise); its two slabs are the first ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = S._env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         env_offset=offset, policy_obs_dim=0 if obs_table is None else len(obs_table),
                         events=events is not None,
                         commands=commands is not None if descriptor is None else descriptor)
    if obs_table is not None:
        sim.set_observation_table(obs_table)
    if events is not None:
        sim.set_event_block(events)
    if commands is not None:
        sim.set_command_block(commands)
    sim.set_reward_table(list(table))
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    return GE._run_device(sim, actions, ep0, before_step=before_step, max_len=MAX_LEN)


_REF = {}


def reference(n, commands, events=None, obs_table=None, table=(), offset=0, switch=None, **kw):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs, marks)"""
    key = (n, commands.tobytes(), None if events is None else events.tobytes(), None if obs_table is None else tuple(obs_table),
           tuple(table), offset, None if switch is None else (switch[0], switch[1].tobytes()),
           tuple((k, np.asarray(v).tobytes()) for k, v in sorted(kw.items())))
    if key not in _REF:
        tw = CT.make_twin(S._env_cfg(), n, commands, events=events, obs_table=obs_table, table=table, env_offset=offset,
                          max_len=MAX_LEN, **kw)
        acts, ep0 = CC.recipe(n + offset)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:]), ep0[offset:]
        slabs, marks = CT.run_commands_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs, marks)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_equal_the_twin_bit_for_bit(n):
    words = _words()
    tw, acts, ep0, ref, marks = reference(n, words)
    if n >= 17:
        assert all(tw.stats[k] >= 5 for k in CT.COUNTS), tw.stats              # every rule fired (the CPU suite's condition)
    sim = _device_sim(n, words)
    assert sim.off == tw.off and sim.F == tw.F == 312 and sim.off["cmd_state"] == (308, 4)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with the dead-zone command term")
    a = tw.off["cmd_state"][0]
    assert (dev[:, :, a] > 0).all() and not dev[:, :, a + 1:a + 4].any()


ALONE = {"deadzone": dict(flags=CT.DEADZONE), "random_resample": dict(flags=CT.RANDOM_RESAMPLE), "yaw_flip": dict(flags=CT.YAW_FLIP),
         "no_flag": dict(flags=0), "base_class_standing": dict(cls="base")}


@pytest.mark.parametrize("case", list(ALONE))
def test_each_rule_alone_and_the_base_class_at_a_ragged_workgroup(case):
    n = 17
    words = _words(**ALONE[case])
    tw, acts, ep0, ref, marks = reference(n, words)
    plain = reference(n, _words(flags=0))[3]
    assert case == "no_flag" or (ref != plain).any(), "the rule changes nothing on the twin"
    counts = {"deadzone": "deadzone", "random_resample": "random_moving", "yaw_flip": "yaw_flips"}
    assert tw.stats["timed"] >= 5 and (case not in counts or tw.stats[counts[case]] >= 5), tw.stats
    dev = _run_device(_device_sim(n, words), acts, ep0)
    _same_bits(dev, ref, f"slabs with {case}")


@pytest.mark.parametrize("n,k", [(17, 17), (64, 16)])
def test_record_and_trace_with_generated_commands(n, k):
    """the step-response instance with the generator running: float 15 of a trace row is the update's mark"""
    words = _words()
    tw, acts, ep0, ref, marks = reference(n, words, trace_envs=k, trace_capacity=STEPS)
    sim = _device_sim(n, words)
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs")
    _same_bits(rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(trace.cpu().numpy(), tw.trace, "trace")
    got = trace[:, :, 15].cpu().numpy()
    np.testing.assert_array_equal(got, marks[:, :k])
    assert (got == 1).any() and (got >= 2).any() and (trace[:, :, 14] == 0).all()
    # the evaluation instance (a record, no trace) gives the same rows
    sim2 = _device_sim(n, words)
    sim2.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim2, acts, ep0), ref, "slabs of the evaluation instance")


# ------------------------------------------------------------------------------------------ 2: composition
def _reference_blocks(push_probability=0.25):
    """the four blocks of the Reference task: its rewards, observations and events (pushes raised to 0.25 so that they occur
    in 60 steps) and the commands of the test cfg (the task's own redraw every 10 s, that is never in 60 steps)"""
    from cat_envs.tasks.utils.mdp import event_manager as EM
    from cat_envs.tasks.utils.mdp import observation_manager as OM
    from cat_envs.tasks.utils.mdp import rewards as R
    cfg = CC._cfg(REFERENCE)
    push = cfg.events.push_robot
    push.params = {**push.params, "probability": push_probability}
    table = [tuple(row[1:]) for row in R.build_table(cfg.rewards, T.JOINTS, 45)[1]]
    obs_table = OM.build_table(OM.policy_group(cfg.observations), T.JOINTS, T.DEFAULT_JOINT_POS)[0]
    events = EM.pack(EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s))
    return table, obs_table, events


def test_composition_with_rewards_observations_and_events():
    """The Reference task's ``RewardsCfg`` is the two exp terms, whose device ``expf`` is allowed 3 ulp against the twin's
    correctly rounded value (tests/test_gpu_servo_reward.py).  The reward feeds nothing back, so every float of the row but
    ``reward`` - the raw observation, the policy field, ``cmd_state`` - is compared bit for bit.  Bound of the reward float:
    raw <= 1 is within 3 ulp(1) = 3.6e-7; times weight * step_dt (0.02 and 0.01): 7.2e-9 + 3.6e-9; two rounded products per
    term on values <= 0.02: 4 * 0.02 * 2^-24 = 4.8e-9; the rounded sum <= 0.03: 1.8e-9; together below 2e-8."""
    n = 17
    table, obs_table, events = _reference_blocks()
    assert [t[0] for t in table] == [1, 2]
    words = _words()
    tw, acts, ep0, ref, marks = reference(n, words, events=events, obs_table=obs_table, table=table)
    assert tw.F == 360 and tw.stats["random_moving"] >= 5 and tw.stats["falls"] + tw.stats["timeouts"] >= 5
    sim = _device_sim(n, words, events=events, obs_table=obs_table, table=table)
    assert sim.off == tw.off and sim.F == 360
    dev = _run_device(sim, acts, ep0)
    o = tw.off["reward"][0]
    keep = np.arange(tw.F) != o
    _same_bits(dev[:, :, keep], ref[:, :, keep], "rows (reward apart): raw row, policy field and cmd_state")
    assert np.abs(dev[:, :, o].astype(np.float64) - ref[:, :, o]).max() <= 2e-8
    without = reference(n, words, obs_table=obs_table, table=table)[3]
    assert (ref != without).any()                                            # the events do act in this run


@pytest.mark.parametrize("with_events,with_obs", [(True, True), (True, False), (False, True)])
def test_composition_is_bit_exact_with_the_non_exp_reward_terms(with_events, with_obs):
    """the remaining combinations of the kernel's pack, reward float included"""
    n = 17
    _, obs_table, events = _reference_blocks()
    events, obs_table = events if with_events else None, obs_table if with_obs else None
    words = _words()
    tw, acts, ep0, ref, marks = reference(n, words, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    dev = _run_device(_device_sim(n, words, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP), acts, ep0)
    _same_bits(dev, ref, "rows")


# ------------------------------------------------------------------------------------------ 3: shards
def test_two_shards_equal_the_rows_of_one_simulator():
    words = _words()
    tw, acts, ep0, ref, marks = reference(64, words)
    whole = _run_device(_device_sim(64, words), acts, ep0)
    lo = _run_device(_device_sim(32, words, offset=0), np.ascontiguousarray(acts[:, :32]), ep0[:32])
    hi = _run_device(_device_sim(32, words, offset=32), np.ascontiguousarray(acts[:, 32:]), ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    _same_bits(hi, reference(32, words, offset=32)[3], "the upper shard against its own twin")
    c = tw.off["command"][0]
    assert (lo[0, :, c:c + 3] != hi[0, :, c:c + 3]).any()                     # commands follow the global env id


# ------------------------------------------------------------------------------------------ 4: fixed commands
def test_fixed_commands_win_and_record_and_trace_are_the_bytes_without_commands():
    n, k = 64, 17
    words = _words()
    acts, ep0 = CC.recipe(n)
    table = torch.from_numpy(np.random.RandomState(2).uniform(-0.5, 0.5, (n, 3)).astype(F32)).cuda()
    got = []
    for commands in (words, None):
        sim = _device_sim(n, commands)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_fixed_command(table)
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        got.append((_run_device(sim, acts, ep0), rec.cpu().numpy(), trace.cpu().numpy(), sim))
    (on, rec_on, trace_on, sim), (off, rec_off, trace_off, _) = got
    c, s = sim.off["command"][0], sim.off["cmd_state"][0]
    assert (on[:, :, c:c + 3] == table.cpu().numpy()).all() and not on[:, :, s:s + 4].any()
    np.testing.assert_array_equal(on[:, :, :s].view(U32), off.view(U32))
    np.testing.assert_array_equal(rec_on.view(U32), rec_off.view(U32))
    np.testing.assert_array_equal(trace_on.view(U32), trace_off.view(U32))
    assert rec_on[:, 0].min() == STEPS and (trace_on[:, :, 15] == 0).all()
    tw = reference(n, words, fixed_command=table.cpu().numpy())
    _same_bits(on, tw[3], "slabs under a fixed table against the twin")
    # without the table the generator runs again, from the row as it stands
    sim.set_fixed_command(None)
    sim.set_trace(None)
    sim.set_eval_record(None)
    _same_bits(_run_device(sim, acts, ep0), reference(n, words)[3], "slabs after the table was detached")


# ------------------------------------------------------------------------------------------ 5: set_ranges
def _manager(sim, commands_cfg):
    from cat_envs.tasks.utils.mdp import command_manager as KM
    cfg = S._env_cfg()
    env = types.SimpleNamespace(sim=sim, cfg=cfg, max_episode_length_s=cfg.episode_length_s)
    return KM.CommandManager(commands_cfg, env)


def test_ranges_set_between_two_steps_are_in_the_very_next_launch():
    n, at = 64, 20
    new = dict(lin_vel_x=(0.5, 0.8), ang_vel_z=(-1.0, -0.6))                  # disjoint from the old ranges
    C = CC._km()[1]
    after = _words(ranges=C.Ranges(**{**CC.TEST_RANGES, **new}))
    before = _words()
    tw, acts, ep0, ref, marks = reference(n, before, switch=(at, after))
    sim = _device_sim(n, None, descriptor=True)                               # the manager writes the block
    mgr = _manager(sim, CC.commands_cfg_of())
    np.testing.assert_array_equal(sim.command_words.view(U32), before.view(U32))
    assert mgr.get_command("base_velocity").data_ptr() == sim.view("command").data_ptr()
    dev = _run_device(sim, acts, ep0, before_step=lambda s: mgr.set_ranges(**new) if s == at else None)
    np.testing.assert_array_equal(sim.command_words.view(U32), after.view(U32))
    _same_bits(dev, ref, "slabs with the ranges moved before step 20")
    old = reference(n, before)[3]
    np.testing.assert_array_equal(dev[:at + 1].view(U32), old[:at + 1].view(U32))              # nothing before it changed
    c = tw.off["command"][0]
    cmd = dev[1:, :, c:c + 3]
    redrawn = (marks == 1) | (marks == 3)
    late = redrawn[at:] & (marks[at:] < 2)                                    # redrawn at or after the switch, yaw not flipped
    assert late.sum() > 50 and redrawn[:at].sum() > 50
    assert (cmd[at:][late][:, 0] >= F32(0.5)).all() and (cmd[at:][late][:, 0] <= F32(0.8)).all()
    assert (cmd[at:][late][:, 2] >= F32(-1.0)).all() and (cmd[at:][late][:, 2] <= F32(-0.6)).all()
    assert (cmd[:at][redrawn[:at]][:, 0] <= F32(0.3)).all()


# ------------------------------------------------------------------------------------------ 6: the entry point's refusals
def test_descriptor_and_block_are_checked():
    from cat_envs import native
    _, obs_table, events = _reference_blocks()
    words = _words()
    sim = _device_sim(16, words, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_COMMANDS and d.cmd.floats == 16 and d.cmd.off_cmd_state == 356 and d.ev.floats == 32
    good = d.cmd.block
    rec = torch.zeros(16, 12, device="cuda")
    sim.set_eval_record(rec)
    for bad in (None, good + 4, good + 8, d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.obs.table, d.ev.block):
        d.cmd.block = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.cmd.block = good
    for floats in (0, 15, 32):
        d.cmd.floats = floats
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.cmd.floats = 16
    # off_cmd_state: negative, not a multiple of 4, past the row, on the policy field, on the raw observation, on joint_pos
    for off in (-4, 357, 358, 360, 1000, 352, 308, d.off_obs, d.off_servo, 0):
        d.cmd.off_cmd_state = off
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.cmd.off_cmd_state = 356
    d.max_episode_length = 2 ** 27                                           # the step index would not fit the counter word
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.max_episode_length = MAX_LEN
    d.ev.floats = 0                                                          # floats 0 goes with a NULL block only
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.ev.floats = 32
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all()
    # the simulator checks what the library cannot read
    for at, value in ((1, -0.1), (2, 1.5), (3, -0.5), (5, -1.0), (10, 2.0), (11, 0.0), (12, -0.1), (13, 1.0), (4, float("nan")),
                      (9, float("inf"))):
        bad = words.copy()
        bad[at] = value
        with pytest.raises(ValueError, match="command block"):
            sim.set_command_block(bad)
    bad = words.copy()
    bad.view(np.int32)[0] = 16
    with pytest.raises(ValueError, match="command block"):
        sim.set_command_block(bad)
    with pytest.raises(ValueError, match="without a command descriptor"):
        _device_sim(16, None).set_command_block(words)


# ------------------------------------------------------------------------------------------ 7: the env
def _env_cfg(task=TASK, n=64, seed=42):
    cfg = CC._cfg(task)
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # 25 steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    cfg.commands = CC.commands_cfg_of()
    return cfg


def _make_env(cfg, task=TASK):
    from cat_envs.shim import make
    return make(task, cfg=cfg)


def test_env_steps_equal_the_oracle_env_on_the_commands_twin():
    n, steps = 64, 40
    cfg = _env_cfg()
    env = _make_env(cfg).unwrapped
    km = env.command_manager
    assert env.max_episode_length == MAX_LEN and env.obs_dim == 45 and env.sim.F == 312
    assert km.active_terms == ["base_velocity"] and km.inert == ["base_velocity.rel_standing_envs", "base_velocity.rel_heading_envs"]
    assert "base_velocity" in str(km) and km.get_command("base_velocity").data_ptr() == env.sim.view("command").data_ptr()
    words = env.sim.command_words
    np.testing.assert_array_equal(words.view(U32), _words().view(U32))
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = CT.make_twin(cfg, n, words, seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=MAX_LEN)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    for s in range(steps):
        a = torch.from_numpy(rs.standard_normal((n, 12)).astype(F32))
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(obs["policy"].cpu().numpy(), o_obs["policy"].numpy(), f"observation after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(F32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(F32), f"dones after step {s}")
    assert all(twin.stats[k] >= 5 for k in CT.COUNTS), twin.stats
    assert "command_terms" in env.state_fingerprint() and env.state_dict()["commands"]["ranges"][0] == [-0.2, 0.3]


def test_step_and_step_into_advance_the_same_state():
    import test_gpu_servo_obs as OB
    n, num_steps = 64, 6
    got = []
    for fused in (True, False):
        tr = OB._trainer(_env_cfg(REFERENCE, n=n), num_steps, fused=fused, task=REFERENCE)
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45 and tr.envs.unwrapped.sim.F == 360
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(F32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        got.append((tr.obs.float().cpu().numpy(), tr.envs.unwrapped.sim.cur.cpu().numpy(), tr.rewards.float().cpu().numpy()))
    for x, y in zip(*got):
        np.testing.assert_array_equal(x.view(U32), y.view(U32))
    assert got[0][0].std() > 0


def test_evaluate_policy_on_a_fixed_grid_is_the_same_with_and_without_commands():
    """fixed commands win at the env's level, too: record and trace of an evaluation do not depend on ``cfg.commands``"""
    from cat_envs.tasks.utils.cleanrl.evaluate import COMMAND_RANGES, command_grid, evaluate_policy
    n, steps = 64, 30
    grid = command_grid(*[(lo, hi, 2) for lo, hi in COMMAND_RANGES], num_envs=n)[0]
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.3).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 2                              # noqa: E731
    got = {}
    for commands in (True, False):
        cfg = _env_cfg(n=n)
        if not commands:
            cfg.commands = None
        env = _make_env(cfg)
        got[commands] = (evaluate_policy(env, policy, steps, commands=grid, fresh_cat_state=True, trace_envs=8),
                         evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8))
        assert env.unwrapped.sim._desc.eval is None and env.unwrapped.sim._desc.fixed_command is None
    (fixed_on, free_on), (fixed_off, free_off) = got[True], got[False]
    np.testing.assert_array_equal(fixed_on.per_env.view(U32), fixed_off.per_env.view(U32))
    np.testing.assert_array_equal(fixed_on.trace.view(U32), fixed_off.trace.view(U32))
    assert (fixed_on.trace[:, :, 4:7] == grid[:8]).all() and (fixed_on.trace[:, :, 15] == 0).all()
    # without a grid the env's own command term runs: redraws and flips show in the trace, the built-in generator's do not
    assert (free_on.trace[:, :, 15] > 0).any() and (free_off.trace[:, :, 15] == 0).all()
    assert (free_on.per_env != free_off.per_env).any()


def test_commands_need_the_servo_simulator_and_a_task_without_them_keeps_its_row():
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    full = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Full-v0"
    fcfg = CC._cfg(full)
    fcfg.scene.num_envs = 16
    env = _make_env(fcfg, full).unwrapped
    assert env.sim.F == 356 and "cmd_state" not in env.sim.off and "command_terms" not in env.state_fingerprint()
    assert "commands" not in env.state_dict() and not hasattr(env.command_manager, "set_ranges")
