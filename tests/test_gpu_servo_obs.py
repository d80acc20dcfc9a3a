"""The servo task's observation terms on the device (csrc/servo_sim.hip: the obs-on instances, ``mdp.observations``,
``ObservationManager``, task ...-Solo12-Servo-Obs-v0): the kernel against ``servo_obs_twin`` bit for bit - raw row and policy
field, noise on and off -, no side effect on anything else, shards, the noise keys of init launches and of steps that end
an episode, the corruption switch, the env and the trainer's observation plane, descriptor checks, run state and
``evaluate_policy(corruption=...)``.  DESIGN section 9, "Observations".

Shapes: 1 env, 17 (a ragged workgroup), 64 and 1000 (several workgroups, a ragged last one); 40 steps of episodes of 7
steps, so that time-outs and post-reset observations occur, with actions large enough for falls."""
import ctypes

import numpy as np
import pytest
import torch

import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T
import test_gpu_servo_sim as S

pytestmark = pytest.mark.gpu

U32 = np.uint32
CANARY, GUARD, STEPS = 12345.0, 8, 40
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-v0"
PLAY = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-Play-v0"
assert S.MAX_LEN == RT.MAX_LEN


def _same_bits(dev, ref, what):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    diff = np.ascontiguousarray(dev).view(U32) != np.ascontiguousarray(ref).view(U32)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {at}: device {dev[at]!r} twin {ref[at]!r}")


def _om():
    from cat_envs.tasks.utils.mdp import observation_manager as OM
    return OM


def _task_cfg(task=TASK):
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    return load_cfg_from_registry(task, "env_cfg_entry_point")


_TABLE = []


def reference_table():
    """the entries of the task's own ``ObservationsCfg`` (the reference's six terms), noise bits set"""
    if not _TABLE:
        OM = _om()
        _TABLE.append(OM.build_table(OM.policy_group(_task_cfg().observations), T.JOINTS, T.DEFAULT_JOINT_POS)[0])
    return _TABLE[0]


def recipe(n):
    acts, ep0 = RT.recipe(n)
    return np.ascontiguousarray(acts[:STEPS]), ep0


def _device_sim(n, obs_table, table=(), offset=0):
    """a simulator with a policy field of ``len(obs_table)`` floats (``obs_table`` None: none at all); its two slabs are the
    first ``n`` rows of buffers with canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = S._env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, S.MAX_LEN, ep_len, reset,
                         env_offset=offset, policy_obs_dim=0 if obs_table is None else len(obs_table))
    if obs_table is not None:
        sim.set_observation_table(obs_table)
    sim.set_reward_table(list(table))
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    """``test_gpu_servo_sim._run_device`` with a hook: ``before_step(s)`` runs on the host before step ``s`` is enqueued"""
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
        reset.copy_((ep_len >= S.MAX_LEN) | (sim.view("hard_reset")[:, 0] > 0.5))
        ep_len.masked_fill_(reset, 0)
        slabs.append(sim.cur.clone())
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all(), "a launch wrote behind the last row"
    return torch.stack(slabs).cpu().numpy()


_REF = {}


def reference(n, obs_table, table=(), offset=0, switch=None):
    """the twin's run of the recipe (computed once per case and left unchanged)"""
    key = (n, tuple(obs_table), tuple(table), offset, None if switch is None else (switch[0], tuple(switch[1])))
    if key not in _REF:
        tw = OT.make_twin(S._env_cfg(), n, obs_table, table=table, env_offset=offset)
        acts, ep0 = recipe(n + offset)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:]), ep0[offset:]
        slabs = OT.run_obs_twin(tw, acts, ep0, switch=switch)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("corruption", [True, False], ids=["noise", "clean"])
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_rows_and_policy_field_equal_the_twin_bit_for_bit(n, corruption):
    table = OT.with_corruption(reference_table(), corruption)
    tw, acts, ep0, ref = reference(n, table)
    falls = int((ref[:, :, tw.off["hard_reset"][0]] > 0).sum())
    episodes = ref[-1, :, tw.off["servo"][0] + 13]
    assert (falls > 0 or n == 1) and episodes.min() >= 5 and episodes.sum() > falls          # falls and time-outs
    sim = _device_sim(n, table)
    assert sim.off == tw.off and sim.F == tw.F == 356 and sim.off["policy_obs"] == (308, 45)
    dev = _run_device(sim, acts, ep0)
    p = tw.off["policy_obs"][0]
    _same_bits(dev[:, :, :p], ref[:, :, :p], "the row up to the policy field")
    _same_bits(dev[:, :, p:], ref[:, :, p:], "policy field")
    a = tw.off["obs"][0]
    noisy = (dev[:, :, p:p + 3] != dev[:, :, a:a + 3] * np.float32(0.25)).mean()
    assert (noisy > 0.9) if corruption else (noisy == 0)


def _stress_tables():
    from cat_envs.shim import AdditiveUniformNoiseCfg as Unoise
    from cat_envs.shim import ObservationTermCfg as ObsTerm
    from cat_envs.shim import SceneEntityCfg
    from cat_envs.tasks.utils.mdp import observations as O
    sub5 = SceneEntityCfg("robot", joint_names=["HR_KFE", "FL_HAA", "FR_HFE", "HL_HFE", "FL_KFE"], preserve_order=True)
    sub7 = SceneEntityCfg("robot", joint_names=[".*_HAA", "F._KFE", "HR_HFE"])
    ref_order = SceneEntityCfg("robot", joint_names=["FL_HAA", "FL_HFE", "FL_KFE", "FR_HAA", "FR_HFE", "FR_KFE", "HR_HAA",
                                                     "HR_HFE", "HR_KFE", "HL_HAA", "HL_HFE", "HL_KFE"], preserve_order=True)
    permuted = {
        "actions": ObsTerm(func=O.last_action, clip=(-0.5, 0.5), scale=tuple(0.5 + 0.125 * k for k in range(12))),
        "some_vel": ObsTerm(func=O.joint_vel_rel, params={"asset_cfg": sub5}, noise=Unoise(n_min=-0.2, n_max=0.3), scale=0.05),
        "gravity": ObsTerm(func=O.projected_gravity, noise=Unoise(n_min=-0.05, n_max=0.05), clip=(-0.02, 0.02)),
        "commands": ObsTerm(func=O.generated_commands, params={"command_name": "base_velocity"}, scale=(2.0, -2.0, 0.25)),
        "joint_pos": ObsTerm(func=O.joint_pos, params={"asset_cfg": ref_order}, noise=Unoise(n_min=0.0, n_max=0.0)),
        "ang_vel": ObsTerm(func=O.base_ang_vel, scale=0.25),
        "some_pos": ObsTerm(func=O.joint_pos_rel, params={"asset_cfg": sub7}, clip=(-0.1, 10.0), scale=3.0)}
    p45 = _om().build_table(permuted, T.JOINTS, T.DEFAULT_JOINT_POS)[0]
    assert len(p45) == 45 and [e[0] for e in p45] != list(range(45))
    f = lambda x: float(np.float32(x))                                       # noqa: E731
    p64 = [((7 * j) % 45, j % 8, f(0.1 * j - 3), f(-0.3), f(0.6), -1.0, 1.0, f(1 + 0.01 * j)) for j in range(64)]
    p1 = [(44, 7, 0.5, f(-0.1), f(0.2), -0.25, 0.25, 3.0)]
    return {"P64": p64, "P1": p1, "P45_permuted": p45}


@pytest.mark.parametrize("which", ["P64", "P1", "P45_permuted"])
def test_stress_tables_at_a_ragged_workgroup(which):
    """every flag combination, a clip that binds (gravity +- 0.05 noise against +- 0.02; actions of size 2 against +- 0.5),
    per-element scales, joint subsets in cfg order and in robot order, widths 1, 45 and 64 (the field then ends the row)"""
    n = 17
    table = _stress_tables()[which]
    tw, acts, ep0, ref = reference(n, table)
    p, w = tw.off["policy_obs"]
    assert tw.F == 308 + (w + 3) // 4 * 4
    if which == "P45_permuted":
        assert (np.abs(ref[:, :, p:p + 12]) == np.float32(0.5) * np.float32([0.5 + 0.125 * k for k in range(12)])).mean() > 0.3
        assert (np.abs(ref[:, :, p + 17:p + 20]) == np.float32(0.02)).any()
    dev = _run_device(_device_sim(n, table), acts, ep0)
    _same_bits(dev, ref, f"slabs with table {which}")
    assert (dev[:, :, p + w:] == 0).all()                                    # the padding of the field


# ------------------------------------------------------------------------------------------ 2: nothing else moves
def test_observations_change_the_policy_field_only():
    """rows, reward record, evaluation record and trace with everything attached: byte-identical with and without the
    observation table - reward kind 11 (action_rate_l2) keeps reading the RAW last action"""
    n, k, L = 64, 17, 2
    acts, ep0 = recipe(n)
    rs = np.random.RandomState(11)
    sched = torch.from_numpy(rs.uniform(-0.5, 0.5, (3, n, 3)).astype(np.float32)).cuda()
    # the policy observation's last-action block is scaled and clipped: were kind 11 to read it, the reward would move
    table = [(*e[:7], 0.5) for e in _stress_tables()["P45_permuted"]]
    got = []
    for obs_table in (None, table):
        sim = _device_sim(n, obs_table, table=RT.ALL_NON_EXP)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_fixed_command(sched, L)
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        slabs = _run_device(sim, acts, ep0)
        got.append((slabs, sim.reward_record.cpu().numpy(), rec.cpu().numpy(), trace.cpu().numpy()))
    (s0, w0, r0, t0), (s1, w1, r1, t1) = got
    assert s0.shape[2] == 308 and s1.shape[2] == 356
    np.testing.assert_array_equal(s0.view(U32), s1[:, :, :308].view(U32))
    np.testing.assert_array_equal(w0.view(U32), w1.view(U32))
    np.testing.assert_array_equal(r0.view(U32), r1.view(U32))
    np.testing.assert_array_equal(t0.view(U32), t1.view(U32))
    assert (w0[:, 16 + 8] != 0).any() and (r0[:, 0] == STEPS).all() and (t0[:, :, 3] != 0).any()     # slot 8 is kind 11
    tw = OT.make_twin(S._env_cfg(), n, table, table=RT.ALL_NON_EXP, schedule=sched.cpu().numpy(), segment_steps=L,
                      trace_envs=k, trace_capacity=STEPS)
    ref = OT.run_obs_twin(tw, acts, ep0)
    _same_bits(s1, ref, "slabs under a schedule, with rewards and observations")
    _same_bits(w1, tw.reward_record, "reward record")
    # the training instance without rewards, too
    plain = _run_device(_device_sim(n, None), acts, ep0)
    both = _run_device(_device_sim(n, reference_table()), acts, ep0)
    np.testing.assert_array_equal(plain.view(U32), both[:, :, :308].view(U32))


# ------------------------------------------------------------------------------------------ 3: shards
def test_two_shards_equal_the_rows_of_one_simulator():
    table = reference_table()
    tw, acts, ep0, ref = reference(64, table)
    whole = _run_device(_device_sim(64, table), acts, ep0)
    lo = _run_device(_device_sim(32, table, offset=0), np.ascontiguousarray(acts[:, :32]), ep0[:32])
    hi = _run_device(_device_sim(32, table, offset=32), np.ascontiguousarray(acts[:, 32:]), ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    p = tw.off["policy_obs"][0]
    assert (lo[:, :, p:p + 3] != hi[:, :, p:p + 3]).any()                    # the noise is keyed on the global env id


# ------------------------------------------------------------------------------------------ 4: the keys of the noise
def test_init_and_episode_end_key_their_noise_on_the_next_episode_at_zero():
    """one env, zero actions (no fall), first episode length 0: steps 1 .. 6 observe (episode 0, t' = 1 .. 6), step 7 ends the
    episode by time-out and observes (episode 1, 0), the init launch (0, 0)"""
    table = OT.identity_table(noise=(-1.0, 2.0))                             # policy float j = (raw_j + 2 u_j) - 1
    acts = np.zeros((9, 1, 12), np.float32)
    dev = _run_device(_device_sim(1, table), acts, [0])
    tw = OT.make_twin(S._env_cfg(), 1, table)
    a, p = tw.off["obs"][0], tw.off["policy_obs"][0]
    assert (dev[:, 0, tw.off["hard_reset"][0]] == 0).all()
    keys = [(0, 0)] + [(0, t) for t in range(1, 7)] + [(1, 0), (1, 1), (1, 2)]
    assert [int(x) for x in dev[:, 0, tw.off["servo"][0] + 13]] == [k[0] for k in keys]
    for s, (ep, t) in enumerate(keys):
        want = tw.policy(dev[s, :, a:a + 45], np.array([ep], np.uint32), np.array([t], np.int64))
        _same_bits(dev[s, :, p:p + 45], want, f"slab {s}: noise of (episode {ep}, t' {t})")
    wrong = tw.policy(dev[7, :, a:a + 45], np.array([0], np.uint32), np.array([7], np.int64))
    assert (wrong != dev[7, :, p:p + 45]).all()                              # not the key of the step that just ended
    u = np.stack([tw.uniforms(np.array([ep], np.uint32), np.array([t], np.int64))[0] for ep, t in keys])
    assert len(np.unique(u)) > 0.999 * u.size


def test_corruption_switched_off_between_two_steps():
    n, at = 64, 20
    noisy = reference_table()
    clean = OT.with_corruption(noisy, False)
    tw, acts, ep0, ref = reference(n, noisy, switch=(at, clean))
    sim = _device_sim(n, noisy)
    dev = _run_device(sim, acts, ep0, before_step=lambda s: sim.set_observation_table(clean) if s == at else None)
    _same_bits(dev, ref, "slabs with the table rewritten before step 20")
    _, _, _, all_noisy = reference(n, noisy)
    _, _, _, all_clean = reference(n, clean)
    p = tw.off["policy_obs"][0]
    np.testing.assert_array_equal(dev[:at + 1].view(U32), all_noisy[:at + 1].view(U32))        # nothing before it changed
    np.testing.assert_array_equal(dev[at + 1:].view(U32), all_clean[at + 1:].view(U32))        # the next step's is noise-free
    assert (all_noisy[at + 1:, :, p:p + 3] != all_clean[at + 1:, :, p:p + 3]).mean() > 0.9


# ------------------------------------------------------------------------------------------ 5: descriptor checks
def test_descriptor_and_table_are_checked():
    from cat_envs import native
    sim = _device_sim(16, reference_table())
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    o = d.obs
    good = (o.width, o.off_policy_obs, o.table)
    assert good[:2] == (45, 308) and d.reserved == native.SERVO_EXT_OBS
    obs_at = sim.off["obs"][0]
    bad = [(0, good[1], good[2]), (65, good[1], good[2]), (-1, good[1], good[2]),            # width
           (good[0], good[1] + 2, good[2]), (good[0], -4, good[2]),                          # unaligned / negative offset
           (good[0], good[1] + 4, good[2]),                                                  # the padded field leaves the row
           (good[0], obs_at // 4 * 4, good[2]), (4, (obs_at + 40) // 4 * 4, good[2]),        # overlaps the raw observation
           (good[0], good[1], None), (good[0], good[1], good[2] + 4),                        # NULL / unaligned table
           (good[0], good[1], d.state_out), (good[0], good[1], d.state_in)]                  # the table aliases a slab
    for width, off, table in bad:
        o.width, o.off_policy_obs, o.table = width, off, table
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    o.width, o.off_policy_obs, o.table = good
    sim._nat.servo_sim_step(d)
    d.reserved = 1                                                           # neither 0 nor the announcement
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_OBS
    d.max_episode_length = 2 ** 27                                           # t' would not fit the counter word
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.max_episode_length = S.MAX_LEN
    d.obs_dim = 44                                                           # the raw observation must be the 45 floats
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.obs_dim = 45
    sim.set_reward_table(RT.ALL_NON_EXP)
    o.table = d.reward_table                                                 # the table may not alias the reward table
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    o.table = good[2]
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    # the simulator checks what the library cannot read
    for entries in (reference_table()[:44], [(45, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)] * 45, [(0, 8, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)] * 45,
                    [(0, 0, 0.0, 0.0, -1.0, 0.0, 0.0, 1.0)] * 45, [(0, 4, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0)] * 45,
                    [(0, 0, float("nan"), 0.0, 0.0, 0.0, 0.0, 1.0)] * 45):
        with pytest.raises(ValueError):
            sim.set_observation_table(entries)
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    with pytest.raises(ValueError, match="policy_obs_dim = 0"):
        _device_sim(16, None).set_observation_table(reference_table())
    cfg = S._env_cfg()
    for obs_dim, width in ((44, 45), (45, 65)):
        with pytest.raises(ValueError, match="policy observation"):
            Solo12ServoSim(16, obs_dim, "cuda", 1, cfg.synthetic, cfg.sim.dt, cfg.decimation, 7, sim._episode_length, sim._reset,
                           policy_obs_dim=width)
    assert ctypes.sizeof(d) == 384


# ------------------------------------------------------------------------------------------ 6: the env
def _env_cfg(task=TASK, n=64, seed=42):
    cfg = _task_cfg(task)
    cfg.episode_length_s = 7 * cfg.sim.dt * cfg.decimation - 1e-9            # seven steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    return cfg


def _make_env(cfg, task=TASK):
    from cat_envs.shim import make
    return make(task, cfg=cfg)


def test_env_observations_equal_the_oracle_env_fed_the_policy_field():
    n, steps = 64, 40
    cfg = _env_cfg()
    env = _make_env(cfg).unwrapped
    assert env.max_episode_length == 7 and env.obs_dim == 45 and env.single_observation_space["policy"].shape == (45,)
    assert env.sim.D == 45 and env.sim.F == 356 and env.observation_manager.corruption is True
    assert env.obs_buf["policy"].data_ptr() == env.sim.view("policy_obs").data_ptr()
    assert "joint_pos" in str(env.observation_manager)
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = OT.make_twin(cfg, n, reference_table(), seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=7)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    orc.off = {**twin.off, "obs": twin.off["policy_obs"]}                    # the oracle env observes the policy field
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    for s in range(steps):
        a = torch.from_numpy((rs.standard_normal((n, 12)) * 2).astype(np.float32))     # large enough to fall
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(obs["policy"].cpu().numpy(), o_obs["policy"].numpy(), f"policy observation after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(np.float32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(np.float32), f"dones after step {s}")
    assert (orc.stream[0][:, twin.off["servo"][0] + 13] >= 4).all()


def _trainer(cfg, num_steps, fused=True, hidden=(64, 64), task=TASK):
    """64 envs x ``num_steps`` steps, one epoch of two minibatches; hidden (64, 64) is the smallest shape the MLP kernels take"""
    from cat_envs.shim import load_cfg_from_registry
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    n = cfg.scene.num_envs
    agent_cfg = load_cfg_from_registry(task, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.updates_epochs = num_steps, n * num_steps // 2, 1
    agent_cfg.hidden, agent_cfg.save_interval, agent_cfg.fused_rollout = tuple(hidden), 10 ** 9, fused
    env = _make_env(cfg, task)
    torch.manual_seed(int(cfg.seed))
    return PPOTrainer(env, agent_cfg)


def test_step_and_step_into_fill_the_same_observation_plane():
    n, num_steps = 64, 4
    planes = []
    for fused in (True, False):
        tr = _trainer(_env_cfg(n=n), num_steps, fused=fused)
        assert (tr.sink is not None) == fused and tr.agent.obs_dim == 45
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(np.float32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        sim = tr.envs.unwrapped.sim
        planes.append((tr.obs.float().cpu().numpy(), sim.cur.cpu().numpy(), tr.agent.obs_rms.running_mean.cpu().numpy()))
    for x, y in zip(*planes):
        np.testing.assert_array_equal(x.view(U32), y.view(U32))
    assert planes[0][0].std() > 0
    # the plane is the normalised POLICY field, not the raw one: the command block is scaled by (2, 2, 0.25)
    p, a = sim.off["policy_obs"][0], sim.off["obs"][0]
    cur = planes[0][1]
    np.testing.assert_array_equal(cur[:, p + 3:p + 6], cur[:, a + 6:a + 9] * np.float32([2.0, 2.0, 0.25]))


def test_observations_need_the_servo_simulator_and_the_raw_45_floats():
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg)
    cfg = _env_cfg(n=16)
    cfg.synthetic.obs_dim = 48
    with pytest.raises(ValueError, match="obs_dim"):
        _make_env(cfg)


# ------------------------------------------------------------------------------------------ 7: run state
def test_two_plus_two_iterations_equal_four(tmp_path):
    """64 envs x 8 steps, hidden (64, 64): parameters, optimiser, normalisers, rollout, CaT state, simulator state (the
    policy field is part of it) of iterations 3 and 4, bytes against the uninterrupted run; new env + new trainer in this
    process, like the resume tests this one borrows its arms from"""
    import test_gpu_resume as RS

    def cfgs():
        cfg = _task_cfg()
        RS._shape_env(cfg)
        cfg.scene.num_envs, cfg.seed = 64, 42
        from cat_envs.shim import load_cfg_from_registry
        agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
        agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
        agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 4, 10 ** 9
        return TASK, cfg, agent_cfg
    seen = {}

    def probe(env, tr):
        u = env.unwrapped
        seen["fp"] = u.state_fingerprint()
        seen["sd"] = u.state_dict()["observations"]
    a, b, tr = RS.check_case(cfgs, tmp_path, save_at=2, iters=4, probe=probe)
    assert seen["sd"] == {"corruption": True} and len(seen["fp"]["observation_terms"]) == 6
    p = tr.envs.unwrapped.sim.off["policy_obs"][0]
    assert (a[-1]["sim.cur"][:, p:p + 45] != 0).any()
    # a state saved with the switch off comes back with the switch off, on the device too
    from cat_envs.tasks.utils.cleanrl import checkpoint
    env = _make_env(_env_cfg(n=16)).unwrapped
    env.reset()
    env.set_observation_corruption(False)
    sd = checkpoint.to_plain(env.state_dict())
    other = _make_env(_env_cfg(n=16)).unwrapped
    other.reset()
    other.load_state_dict(sd)
    assert other.observation_manager.corruption is False
    act = torch.zeros(16, 12, device="cuda")
    other.step(act)
    raw, pol = other.sim.view("obs"), other.sim.view("policy_obs")
    assert torch.equal(pol[:, 0:3], raw[:, 0:3] * 0.25)                      # base_ang_vel: scaled, no noise
    with pytest.raises(ValueError, match="observations"):
        bad = dict(sd)
        del bad["observations"]
        other.check_state_dict(bad)


# ------------------------------------------------------------------------------------------ 8: evaluation
def test_evaluate_policy_without_corruption_equals_a_play_env():
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    n, steps = 64, 20
    noisy_env = _make_env(_env_cfg(TASK, n))
    play_env = _make_env(_env_cfg(PLAY, n), PLAY)
    assert noisy_env.unwrapped.observation_manager.corruption and not play_env.unwrapped.observation_manager.corruption
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(np.float32) * 0.3).cuda()
    seen = []

    def policy(obs):
        seen.append(obs.clone())
        return torch.tanh(obs @ w) * 2

    def run(env, **kw):
        seen.clear()
        res = evaluate_policy(env, policy, steps, fresh_cat_state=True, trace_envs=4, **kw)
        return res, torch.stack(seen).cpu().numpy()
    clean, obs_clean = run(noisy_env, corruption=False)
    assert noisy_env.unwrapped.observation_manager.corruption is True        # left as it was found
    play, obs_play = run(play_env)
    for what, x, y in (("record", clean.per_env, play.per_env), ("trace", clean.trace, play.trace),
                       ("cat reward", clean.cat_reward, play.cat_reward), ("observations", obs_clean, obs_play)):
        np.testing.assert_array_equal(x.view(U32), y.view(U32), err_msg=what)
    noisy, obs_noisy = run(noisy_env)                                        # None: the env's own switch, noise on
    assert (obs_noisy != obs_clean).mean() > 0.5 and (noisy.per_env != clean.per_env).any()
    on_play, obs_on = run(play_env, corruption=True)
    np.testing.assert_array_equal(obs_on.view(U32), obs_noisy.view(U32))
    assert play_env.unwrapped.observation_manager.corruption is False
    with pytest.raises(RuntimeError, match="boom"):
        evaluate_policy(noisy_env, lambda o: (_ for _ in ()).throw(RuntimeError("boom")), 2, corruption=False)
    assert noisy_env.unwrapped.observation_manager.corruption is True        # restored in the same finally as the record
    assert noisy_env.unwrapped.sim._desc.eval is None
    import servo_twin
    plain = _make_env_plain(servo_twin.TASK, 16)
    with pytest.raises(TypeError, match="cfg.observations"):
        evaluate_policy(plain, lambda o: torch.zeros(16, 12, device="cuda"), 2, corruption=False)
    assert plain.unwrapped.sim._desc.eval is None
    # the periodic evaluator's env measures without noise
    cfg = _env_cfg(TASK, n)
    ecfg = make_eval_env_cfg(cfg, 16)
    assert ecfg.observations.policy.enable_corruption is False and cfg.observations.policy.enable_corruption is True


def _make_env_plain(task, n):
    cfg = _task_cfg(task)
    cfg.scene.num_envs = n
    return _make_env(cfg, task)
