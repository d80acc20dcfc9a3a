"""The servo task's events on the device (csrc/servo_sim.hip: the events-on instances, ``mdp.events``, ``EventManager``, tasks
...-Solo12-Servo-Events-v0 / -Full-v0): the kernel against ``servo_events_twin`` bit for bit - all four kinds, each kind alone,
neutral blocks, the interval switch, composition with rewards, observations, record, schedule and trace, shards, the entry
point's refusals and the env.  DESIGN section 9, "Events".

Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one); 40 steps of episodes of 12 steps,
so that time-outs, falls and post-reset observations all occur; push probability 0.25."""
import types

import numpy as np
import pytest
import torch

import servo_events_twin as ET
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T
import test_gpu_servo_sim as S
import test_servo_events_twin as CE

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = 12345.0, 8, CE.STEPS, CE.MAX_LEN
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Events-v0"
ALL = CE.ALL


def _same_bits(dev, ref, what):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    diff = np.ascontiguousarray(dev).view(U32) != np.ascontiguousarray(ref).view(U32)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {at}: device {dev[at]!r} twin {ref[at]!r}")


def _device_sim(n, events, obs_table=None, table=(), offset=0, max_len=MAX_LEN):
    """a simulator with the event block ``events`` (None: built without the event descriptor); its two slabs are the first
    ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = S._env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, max_len, ep_len, reset,
                         env_offset=offset, policy_obs_dim=0 if obs_table is None else len(obs_table), events=events is not None)
    if obs_table is not None:
        sim.set_observation_table(obs_table)
    if events is not None:
        sim.set_event_block(events)
    sim.set_reward_table(list(table))
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None, max_len=MAX_LEN):
    ep_len, reset = sim._episode_length, sim._reset
    ep_len.copy_(torch.from_numpy(np.asarray(ep0, np.int64)))
    reset.zero_()
    sim.step(None)
    slabs = [sim.cur.clone()]
    acts = torch.from_numpy(actions).cuda()
    for s in range(len(actions)):
        if before_step is not None:
            before_step(s)
        sim.step(acts[s])
        ep_len.add_(1)
        reset.copy_((ep_len >= max_len) | (sim.view("hard_reset")[:, 0] > 0.5))
        ep_len.masked_fill_(reset, 0)
        slabs.append(sim.cur.clone())
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all(), "a launch wrote behind the last row"
    return torch.stack(slabs).cpu().numpy()


_REF = {}


def reference(n, events, obs_table=None, table=(), offset=0, switch=None):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs, push masks)"""
    key = (n, events.tobytes(), None if obs_table is None else tuple(obs_table), tuple(table), offset,
           None if switch is None else (switch[0], switch[1].tobytes()))
    if key not in _REF:
        tw = ET.make_twin(S._env_cfg(), n, events, obs_table=obs_table, table=table, env_offset=offset, max_len=MAX_LEN)
        acts, ep0 = CE.recipe(n + offset)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:]), ep0[offset:]
        slabs, masks = ET.run_events_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs, masks)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_equal_the_twin_bit_for_bit(n):
    words = ET.block(**ALL)
    tw, acts, ep0, ref, masks = reference(n, words)
    h, so = tw.off["hard_reset"][0], tw.off["servo"][0]
    if n >= 17:
        falls = int((ref[1:, :, h] > 0).sum())
        episodes = ref[-1, :, so + 13]
        assert falls > 0 and episodes.sum() > falls and masks.any()             # falls, time-outs and pushes
    if n == 64:                                                               # a push ends an episode in a fall
        assert CE.pushed_falls(S._env_cfg(), n, acts, ep0, (tw, ref, masks)) > 0
    sim = _device_sim(n, words)
    assert sim.off == tw.off and sim.F == tw.F == 308
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs with all four event kinds")


KINDS = {"push": dict(flags=ET.PUSH, p=0.25, push=ALL["push"]),
         "push_with_yaw": dict(flags=ET.PUSH, p=0.25, push=[(-0.3, 0.6), (0.0, 0.0), (-1.0, 1.0), (0.0, 0.0), (-5.0, 5.0)]),
         "joints_by_scale": dict(flags=ET.JOINT_SCALE, joint_pos=[(0.95, 1.05)]),
         "joints_by_offset": dict(flags=ET.JOINT_OFFSET, joint_pos=[(-0.1, 0.2)], joint_vel=[(-0.5, 0.5)]),
         "root": dict(flags=ET.ROOT, root_pos=ALL["root_pos"], root_vel=ALL["root_vel"]),
         "friction_1": dict(flags=ET.FRICTION, num_buckets=1, friction=[(0.5, 1.25)]),
         "friction_3": dict(flags=ET.FRICTION, num_buckets=3, friction=[(0.5, 1.25)]),
         "friction_100": dict(flags=ET.FRICTION, num_buckets=100, friction=[(0.5, 1.25)])}


@pytest.mark.parametrize("kind", list(KINDS))
def test_each_kind_alone_at_a_ragged_workgroup(kind):
    n = 17
    words = ET.block(**KINDS[kind])
    tw, acts, ep0, ref, masks = reference(n, words)
    _, _, _, plain, _ = reference(n, ET.block())
    assert (ref != plain).any(), "the kind changes nothing on the twin"
    dev = _run_device(_device_sim(n, words), acts, ep0)
    _same_bits(dev, ref, f"slabs with {kind} alone")


# ------------------------------------------------------------------------------------------ 2: neutral cases and the switch
def _manager(sim, cfg_events, **kw):
    from cat_envs.tasks.utils.mdp import event_manager as EM
    cfg = S._env_cfg()
    env = types.SimpleNamespace(sim=sim, cfg=cfg, max_episode_length_s=cfg.episode_length_s)
    return EM.EventManager(cfg_events, env, **kw)


def _push_only_cfg():
    from cat_envs.shim import EventTermCfg as EventTerm
    from cat_envs.tasks.utils.mdp import events as EV
    return {"push_robot": EventTerm(func=EV.push_by_setting_velocity_with_random_envs, mode="interval",
                                    params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5), "roll": (-20.0, 20.0),
                                                               "pitch": (-20.0, 20.0)}, "probability": 0.25})}


def test_neutral_blocks_give_the_bytes_of_a_simulator_without_events():
    n = 64
    acts, ep0 = CE.recipe(n)
    without = _run_device(_device_sim(n, None), acts, ep0)
    zeros = _run_device(_device_sim(n, ET.block()), acts, ep0)
    np.testing.assert_array_equal(without.view(U32), zeros.view(U32))
    sim = _device_sim(n, ET.block())
    mgr = _manager(sim, _push_only_cfg())
    mgr.set_interval_enabled(False)
    switched_off = _run_device(sim, acts, ep0)
    np.testing.assert_array_equal(without.view(U32), switched_off.view(U32))
    mgr.set_interval_enabled(True)
    on = _run_device(sim, acts, ep0)
    tw, _, _, ref, masks = reference(n, ET.block(**KINDS["push"]))
    _same_bits(on, ref, "pushes switched on again")
    assert masks.any() and (on != without).any()


def test_a_switch_flipped_between_two_steps_is_in_the_very_next_launch():
    n, at = 64, 20
    on, off = ET.block(**ALL), ET.block(**dict(ALL, flags=ALL["flags"] & ~ET.PUSH))
    tw, acts, ep0, ref, masks = reference(n, on, switch=(at, off))
    sim = _device_sim(n, on)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_event_block(off) if s == at else None)
    _same_bits(dev, ref, "slabs with the pushes switched off before step 20")
    _, _, _, all_on, masks_on = reference(n, on)
    np.testing.assert_array_equal(dev[:at + 1].view(U32), all_on[:at + 1].view(U32))          # nothing before it changed
    assert masks_on[at].any() and not masks[at:].any() and (dev[at + 1] != all_on[at + 1]).any()


# ------------------------------------------------------------------------------------------ 3: composition
def _shaped_table():
    from cat_envs.tasks.locomotion.velocity.config.solo12.cat_flat_env_cfg import ShapedRewardsCfg
    from cat_envs.tasks.utils.mdp import rewards as R
    return [tuple(row[1:]) for row in R.build_table(ShapedRewardsCfg(), T.JOINTS, 45)[1]]


def _obs_table():
    import test_gpu_servo_obs as OB
    return OB.reference_table()


def _composed(n, k, words, table, obs_table):
    """(device, twin) results with rewards, observations, record, schedule and trace attached: slabs, reward record,
    evaluation record, trace"""
    L = 2
    acts, ep0 = CE.recipe(n)
    rs = np.random.RandomState(11)
    sched = rs.uniform(-0.5, 0.5, (3, n, 3)).astype(F32)
    sim = _device_sim(n, words, obs_table=obs_table, table=table)
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_fixed_command(torch.from_numpy(sched).cuda(), L)
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    slabs = _run_device(sim, acts, ep0)
    dev = (slabs, sim.reward_record.cpu().numpy(), rec.cpu().numpy(), trace.cpu().numpy())
    if words is None:
        tw = OT.make_twin(S._env_cfg(), n, obs_table, table=table, max_len=MAX_LEN, schedule=sched, segment_steps=L,
                          trace_envs=k, trace_capacity=STEPS)
        ref_slabs, masks = OT.run_obs_twin(tw, acts, ep0), None
    else:
        tw = ET.make_twin(S._env_cfg(), n, words, obs_table=obs_table, table=table, max_len=MAX_LEN, schedule=sched,
                          segment_steps=L, trace_envs=k, trace_capacity=STEPS)
        ref_slabs, masks = ET.run_events_twin(tw, acts, ep0)
    return dev, (ref_slabs, tw.reward_record, tw.record, tw.trace), tw, masks


@pytest.mark.parametrize("n,k", [(17, 1), (17, 16), (17, 17), (64, 1), (64, 16), (64, 17)])
def test_composition_with_rewards_observations_record_schedule_and_trace(n, k):
    """``ShapedRewardsCfg`` has the two exp terms, whose device ``expf`` is allowed 3 ulp against the twin's correctly
    rounded value (tests/test_gpu_servo_reward.py).  The reward feeds nothing back, so everything but the row's ``reward``
    float and the two exp terms' sums is compared bit for bit.  Bounds of the rest: each exp value (at most 0.02) is within
    3 ulp + 3 ulp = 1.2e-8; each of the eight following adds of the sum rounds a partial sum below 1 that may already differ:
    8 * 2^-24 = 4.8e-7; together 5e-7.  A record sum adds up to 40 values below 0.02 with partial sums below 1:
    40 * (5.6e-9 + 6e-8) = 2.7e-6."""
    table, obs_table = _shaped_table(), _obs_table()
    assert [t[0] for t in table][:2] == [1, 2] and all(t[0] > 2 for t in table[2:]) and len(table) == 9
    (slabs, rrec, rec, trace), (r_slabs, r_rrec, r_rec, r_trace), tw, masks = _composed(n, k, ET.block(**ALL), table, obs_table)
    o = tw.off["reward"][0]
    keep = np.arange(tw.F) != o
    _same_bits(slabs[:, :, keep], r_slabs[:, :, keep], "rows (reward apart), policy field included")
    assert np.abs(slabs[:, :, o].astype(np.float64) - r_slabs[:, :, o]).max() <= 5e-7
    exact = [c for c in range(32) if c not in (0, 1, 16, 17)]
    _same_bits(rrec[:, exact], r_rrec[:, exact], "reward record: the non-exp terms and the episode count")
    assert np.abs(rrec.astype(np.float64) - r_rrec).max() <= 2.7e-6
    _same_bits(rec, r_rec, "evaluation record")
    _same_bits(trace, r_trace, "trace")
    np.testing.assert_array_equal(trace[:, :, 14], masks[:, :k].astype(F32))
    assert (trace[:, :, 15] == 0).all() and (masks[:, :k].any() or k == 1)


def test_composition_is_bit_exact_with_the_non_exp_terms_and_events_off_keeps_todays_bytes():
    n, k = 64, 17
    obs_table = _obs_table()
    dev, ref, tw, masks = _composed(n, k, ET.block(**ALL), RT.ALL_NON_EXP, obs_table)
    for what, x, y in zip(("slabs", "reward record", "evaluation record", "trace"), dev, ref):
        _same_bits(x, y, what)
    assert masks[:, :k].any() and (dev[3][:, :, 14] == masks[:, :k]).all()
    # events off (a simulator built without them, and a zero block): record and trace bytes are today's
    plain, plain_ref, _, _ = _composed(n, k, None, RT.ALL_NON_EXP, obs_table)
    zero, _, _, _ = _composed(n, k, ET.block(), RT.ALL_NON_EXP, obs_table)
    for what, x, y, z in zip(("slabs", "reward record", "evaluation record", "trace"), plain, plain_ref, zero):
        _same_bits(x, y, what + " without events")
        np.testing.assert_array_equal(x.view(U32), z.view(U32), err_msg=what)
    assert (plain[3][:, :, 14:16] == 0).all()


# ------------------------------------------------------------------------------------------ 4: shards
def test_two_shards_equal_the_rows_of_one_simulator():
    words = ET.block(**ALL)
    tw, acts, ep0, ref, masks = reference(64, words)
    whole = _run_device(_device_sim(64, words), acts, ep0)
    lo = _run_device(_device_sim(32, words, offset=0), np.ascontiguousarray(acts[:, :32]), ep0[:32])
    hi = _run_device(_device_sim(32, words, offset=32), np.ascontiguousarray(acts[:, 32:]), ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    _same_bits(hi, reference(32, words, offset=32)[3], "the upper shard against its own twin")
    jp = tw.off["joint_pos"][0]
    assert (lo[0, :, jp:jp + 12] != hi[0, :, jp:jp + 12]).any()               # first states follow the global env id


# ------------------------------------------------------------------------------------------ 5: the entry point's refusals
def test_descriptor_and_block_are_checked():
    from cat_envs import native
    sim = _device_sim(16, ET.block(**ALL), obs_table=_obs_table(), table=RT.ALL_NON_EXP)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_EVENTS and d.ev.floats == 32 and d.obs.width == 45
    good = d.ev.block
    rec = torch.zeros(16, 12, device="cuda")
    sim.set_eval_record(rec)
    for bad in (None, good + 4, good + 8, d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.obs.table):
        d.ev.block = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.ev.block = good
    for floats, reserved in ((16, 0), (0, 0), (32, 1)):
        d.ev.floats, d.ev.reserved = floats, reserved
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.ev.floats, d.ev.reserved = 32, 0
    d.max_episode_length = 2 ** 27                                           # the step index would not fit the counter word
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.max_episode_length = MAX_LEN
    d.reserved = 2                                                           # neither 0 nor an announcement
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_EVENTS
    d.obs.width = 0                                                          # width 0 goes with a NULL table only
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.obs.width = 45
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    short = native.ServoSimObs()
    short.reserved = native.SERVO_EXT_EVENTS
    with pytest.raises(TypeError, match="ServoSimEvents"):
        sim._nat.servo_sim_step(short)
    # the simulator checks what the library cannot read
    w = ET.block(**ALL)
    for at, value in ((1, 1.5), (1, -0.1), (5, -1.0), (28, float("nan")), (3, 1.0), (29, float("inf"))):
        bad = w.copy()
        bad[at] = value
        with pytest.raises(ValueError, match="event block"):
            sim.set_event_block(bad)
    for at, value in ((0, 32), (0, ET.JOINT_SCALE | ET.JOINT_OFFSET), (2, 0)):
        bad = w.copy()
        bad.view(np.int32)[at] = value
        with pytest.raises(ValueError, match="event block"):
            sim.set_event_block(bad)
    with pytest.raises(ValueError, match="without an event descriptor"):
        _device_sim(16, None).set_event_block(w)


# ------------------------------------------------------------------------------------------ 6: the env
def _env_cfg(task=TASK, n=64, seed=42):
    cfg = CE._cfg(task)
    cfg.synthetic.servo_resample_steps = 250
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # twelve steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    push = cfg.events.push_robot
    push.params = {**push.params, "probability": 0.25,
                   "velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5), "roll": (-20.0, 20.0), "pitch": (-20.0, 20.0)}}
    return cfg


def _make_env(cfg, task=TASK):
    from cat_envs.shim import make
    return make(task, cfg=cfg)


def test_env_steps_equal_the_oracle_env_on_the_events_twin_and_the_switch_reaches_replayed_launches():
    n, steps, at = 64, 30, 14
    cfg = _env_cfg()
    env = _make_env(cfg).unwrapped
    em = env.event_manager
    assert env.max_episode_length == MAX_LEN and env.obs_dim == 45 and env.sim.F == 308 and em.interval_enabled
    assert em.block["p"] == 0.25 and list(em.active_terms) == ["startup", "reset", "interval"] and "push_robot" in str(em)
    words = env.sim.event_words
    off = words.copy()
    off.view(np.int32)[0] &= ~ET.PUSH
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = ET.make_twin(cfg, n, words, seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=MAX_LEN)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    pushes = 0
    for s in range(steps):
        if s == at:
            env.set_pushes(False)
            twin.set_events(off)
        a = torch.from_numpy((rs.standard_normal((n, 12)) * 2).astype(F32))
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        pushes += int(twin.pushed.sum())
        assert s < at or not twin.pushed.any()
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(obs["policy"].cpu().numpy(), o_obs["policy"].numpy(), f"observation after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(F32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(F32), f"dones after step {s}")
    assert pushes > 100 and not em.interval_enabled and env.state_dict()["events"] == {"interval": False}
    assert (orc.stream[0][:, twin.off["servo"][0] + 13] >= 2).all()
    assert "event_terms" in env.state_fingerprint()


def test_step_and_step_into_advance_the_same_state():
    import test_gpu_servo_obs as OB
    n, num_steps = 64, 6
    got = []
    for fused in (True, False):
        tr = OB._trainer(_env_cfg(n=n), num_steps, fused=fused, task=TASK)
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(F32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        got.append((tr.obs.float().cpu().numpy(), tr.envs.unwrapped.sim.cur.cpu().numpy(), tr.rewards.float().cpu().numpy()))
    for x, y in zip(*got):
        np.testing.assert_array_equal(x.view(U32), y.view(U32))
    assert got[0][0].std() > 0


def test_events_need_the_servo_simulator_and_play_runs_without_pushes():
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    play = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Events-Play-v0"
    env = _make_env(_env_cfg(play, n=16), play).unwrapped
    em = env.event_manager
    assert em.interval_enabled is False and list(em.active_terms) == ["startup", "reset", "interval"]
    assert env.sim.event_words.view(np.int32)[0] == ET.JOINT_SCALE | ET.ROOT | ET.FRICTION


def test_evaluate_policy_sets_the_pushes_for_the_call_and_restores_them():
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    n, steps = 64, 24
    env = _make_env(_env_cfg(n=n))
    em = env.unwrapped.event_manager
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.3).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 2                              # noqa: E731
    on = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8)
    assert on.pushes and on.trace[:, :, 14].sum() > 10 and em.interval_enabled
    rows = on.push_recovery()
    assert len(rows) == int(on.trace[:, :, 14].sum()) and "push_recovery" in on.to_json()
    off = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8, pushes=False)
    assert not off.pushes and (off.trace[:, :, 14] == 0).all() and em.interval_enabled and "push_recovery" not in off.to_json()
    assert (off.per_env != on.per_env).any()
    again = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=8, pushes=True)
    np.testing.assert_array_equal(again.trace.view(U32), on.trace.view(U32))
    with pytest.raises(RuntimeError, match="boom"):
        evaluate_policy(env, lambda o: (_ for _ in ()).throw(RuntimeError("boom")), 2, pushes=False)
    assert em.interval_enabled and env.unwrapped.sim._desc.eval is None        # restored in the same finally as the record
    plain_cfg = CE._cfg(T.TASK)
    plain_cfg.scene.num_envs = 16
    plain = _make_env(plain_cfg, T.TASK)
    with pytest.raises(TypeError, match="cfg.events"):
        evaluate_policy(plain, lambda o: torch.zeros(plain.unwrapped.num_envs, 12, device="cuda"), 2, pushes=False)
    assert plain.unwrapped.sim._desc.eval is None
