"""The servo task's reward terms on the device (csrc/servo_sim.hip ``reward_terms`` / ``reward_rec`` / ``reward_table``,
``mdp.rewards``, ``RewardManager``, task ...-Solo12-Servo-Rewards-v0): the kernel against ``servo_reward_twin`` bit for bit,
the exp kinds within their ulp bound, no side effect on anything else, shards, the env, run state and the trainer's log.
DESIGN section 9, "Rewards"."""
import numpy as np
import pytest
import torch

import servo_reward_twin as RT
import servo_twin as T
import test_gpu_servo_sim as S

pytestmark = pytest.mark.gpu

U32 = np.uint32
CANARY, GUARD = 12345.0, 8
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-v0"
assert S.MAX_LEN == RT.MAX_LEN


def _same_bits(dev, ref, what):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    diff = np.ascontiguousarray(dev).view(U32) != np.ascontiguousarray(ref).view(U32)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {at}: device {dev[at]!r} twin {ref[at]!r}")


def _device_sim(n, table, offset=0, guard=True):
    """a simulator with the reward table and (``guard``) a record of the test's own with canary rows behind it"""
    sim = S._device_sim(n, offset=offset, seed=RT.SEED)
    sim.set_reward_table(table)
    buf = None
    if table and guard:
        buf = torch.full((n + GUARD, RT.REC_FLOATS), CANARY, device="cuda")
        sim._desc.reward_rec = buf.data_ptr()
    return sim, buf


def _run(n, table, offset=0, acts=None, ep0=None):
    if acts is None:
        acts, ep0 = RT.recipe(n)
    sim, buf = _device_sim(n, table, offset)
    slabs = S._run_device(sim, np.ascontiguousarray(acts, np.float32), ep0)
    return slabs, (None if buf is None else buf.cpu().numpy())


_REF = {}


def reference(n, table=None):
    """the twin's run of the recipe at ``n`` envs (computed once per size and table)"""
    key = (n, None if table is None else tuple(table))
    if key not in _REF:
        tw = RT.make_twin(S._env_cfg(), n, RT.ALL_NON_EXP if table is None else table)
        acts, ep0 = RT.recipe(n)
        slabs, rec, values = RT.run_reward_twin(tw, acts, ep0)
        for a in (acts, slabs, rec, values):
            a.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs, rec, values)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_rows_and_record_equal_the_twin_bit_for_bit(n):
    """every non-exp kind with distinct weights, an HAA-only mask on kind 10; n = 1 and 17 leave spare lane groups in the
    last workgroup, 1000 is many workgroups with a ragged last one"""
    tw, acts, ep0, ref_slabs, ref_rec, values = reference(n)
    assert tw.stats["falls"] > 0 and tw.stats["timeouts"] > 0 and tw.stats["touch_air"] > 0
    assert (values != 0).any(axis=(0, 1)).all(), "a configured term is zero in every step"
    slabs, buf = _run(n, RT.ALL_NON_EXP)
    _same_bits(slabs, ref_slabs, "slabs")
    _same_bits(buf[:n], ref_rec, "reward record")
    assert (buf[n:] == np.float32(CANARY)).all(), "a launch wrote behind the record"


# ------------------------------------------------------------------------------------------ 2: the exp kinds
def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", [17, 64])
def test_exp_kinds_within_three_ulp(n, kind):
    """3 ulp: 2 for a device expf within 1 ulp of the true value against the correctly rounded reference, 1 for the rounded
    product with step_dt (the weight is 1.0).  Everything but ``reward`` is bit-exact; the record is the fp32 sequential sum
    of the device's own rewards"""
    table = [(kind, 0, 1.0, 0.25)]
    tw, acts, ep0, ref_slabs, ref_rec, values = reference(n, table)
    assert (values != 0).any()
    slabs, buf = _run(n, table)
    o = tw.off["reward"][0]
    keep = np.arange(tw.F) != o
    _same_bits(slabs[:, :, keep], ref_slabs[:, :, keep], "row fields other than reward")
    dist = _ulps(slabs[1:, :, o], ref_slabs[1:, :, o])
    print(f"exp kind {kind}, n = {n}: max distance {int(dist.max())} ulp, {int((dist > 0).sum())} of {dist.size} differ")
    import parity_record
    parity_record.record(f"servo_reward_exp_kind{kind}_n{n}", dict(max_ulp=int(dist.max()), differing=int((dist > 0).sum())),
                         sizes=dict(num_envs=n, steps=RT.STEPS), seed=RT.SEED, note="device expf against fp64 exp rounded")
    assert dist.max() <= 3, f"reward of exp kind {kind} is {int(dist.max())} ulp from the correctly rounded reference"
    own = RT.recount_record(tw, slabs, slabs[1:, :, o:o + 1], ep0)
    _same_bits(buf[:n], own, "record against the sequential sum of the device's own rewards")


# ------------------------------------------------------------------------------------------ 3: nothing else moves
def test_rewards_change_the_reward_field_only():
    n = 64
    tw, acts, ep0, ref_slabs, ref_rec, values = reference(n)
    on, _ = _run(n, RT.ALL_NON_EXP)
    off, _ = _run(n, [])
    o = tw.off["reward"][0]
    keep = np.arange(tw.F) != o
    np.testing.assert_array_equal(on[:, :, keep].view(U32), off[:, :, keep].view(U32))
    assert (on[1:, :, o] != off[1:, :, o]).any()
    _same_bits(off, T.run_twin(T.ServoTwin(n, tw.D, tw.p, RT.SEED, RT.MAX_LEN, tw.dt, tw.dec), acts, ep0), "rewards off")
    # a descriptor with T = 0 computes the parent's bytes whatever the rest of the tail holds
    sim, buf = _device_sim(n, RT.ALL_NON_EXP)
    sim._desc.reward_terms = 0
    zero = S._run_device(sim, np.array(acts), ep0)
    np.testing.assert_array_equal(zero.view(U32), off.view(U32))
    assert (buf.cpu().numpy() == np.float32(CANARY)).all()                  # and touches no record


def test_eval_record_and_trace_keep_the_builtin_reward():
    """the yardstick property: evaluation record and trace are byte-identical with rewards on and off"""
    n, k, L = 64, 17, 2
    acts, ep0 = RT.recipe(n)
    rs = np.random.RandomState(11)
    sched = torch.from_numpy(rs.uniform(-0.5, 0.5, (3, n, 3)).astype(np.float32)).cuda()
    got = []
    for table in ([], RT.ALL_NON_EXP):
        sim, _ = _device_sim(n, table, guard=False)
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(RT.STEPS, k, 72, device="cuda")
        sim.set_fixed_command(sched, L)
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        slabs = S._run_device(sim, np.array(acts), ep0)
        got.append((slabs, rec.cpu().numpy(), trace.cpu().numpy()))
    (s0, r0, t0), (s1, r1, t1) = got
    np.testing.assert_array_equal(r0.view(U32), r1.view(U32))
    np.testing.assert_array_equal(t0.view(U32), t1.view(U32))
    assert (r0[:, 0] == RT.STEPS).all() and (t0[:, :, 3] != 0).any()
    tw = RT.make_twin(S._env_cfg(), n, RT.ALL_NON_EXP, schedule=sched.cpu().numpy(), segment_steps=L, trace_envs=k,
                      trace_capacity=RT.STEPS)
    ref_slabs, ref_rec, _ = RT.run_reward_twin(tw, acts, ep0)
    _same_bits(s1, ref_slabs, "slabs under a schedule, with rewards")
    _same_bits(r1, tw.record, "evaluation record")
    _same_bits(t1, tw.trace, "trace")


# ------------------------------------------------------------------------------------------ 4: shards
def test_two_shards_equal_the_rows_of_one_simulator():
    n = 64
    tw, acts, ep0, ref_slabs, ref_rec, values = reference(n)
    whole, rec = _run(n, RT.ALL_NON_EXP)
    lo, rec_lo = _run(32, RT.ALL_NON_EXP, offset=0, acts=acts[:, :32], ep0=ep0[:32])
    hi, rec_hi = _run(32, RT.ALL_NON_EXP, offset=32, acts=acts[:, 32:], ep0=ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    np.testing.assert_array_equal(rec[:32].view(U32), rec_lo[:32].view(U32))
    np.testing.assert_array_equal(rec[32:64].view(U32), rec_hi[:32].view(U32))


def test_descriptor_and_table_are_checked():
    sim, buf = _device_sim(16, RT.ALL_NON_EXP)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    good = (d.reward_terms, d.reward_rec, d.reward_table)
    for terms, rec, table in ((16, good[1], good[2]), (-1, good[1], good[2]), (good[0], None, good[2]),
                              (good[0], good[1] + 4, good[2]), (good[0], d.state_out, good[2]),
                              (good[0], d.state_in, good[2]), (good[0], good[1], None), (good[0], good[1], good[2] + 4)):
        d.reward_terms, d.reward_rec, d.reward_table = terms, rec, table
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.reward_terms, d.reward_rec, d.reward_table = good
    rec = torch.zeros(16, 12, device="cuda")
    sim.set_eval_record(rec)
    d.reward_rec = rec.data_ptr()                                            # the record may not alias the evaluation record
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for bad in ([(0, 0, 1.0, 0.0)], [(17, 0, 1.0, 0.0)], [(1, 0, 1.0, 0.0)], [(4, 0, 1.0, -1.0)], [(7, 0, 1.0, 0.0)],
                [(10, 0x1000, 1.0, 0.0)], [(12, 0, 1.0, 0.0)] * 16):
        with pytest.raises(ValueError):
            sim.set_reward_table(bad)
    with pytest.raises(ValueError, match="obs_dim"):
        S._device_sim(16, obs_dim=44).set_reward_table([(11, 0, 1.0, 0.0)])


# ------------------------------------------------------------------------------------------ 5: the env
def _shaped_cfg():
    """the rewards task with a block of non-exp terms (bit-exact against the twin): rational tracking plus penalties"""
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import RewardTermCfg as RewTerm
    from cat_envs.shim import SceneEntityCfg, load_cfg_from_registry
    from cat_envs.tasks.utils.mdp import rewards as R
    cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")
    cfg.rewards = {
        "track_lin": RewTerm(func=R.track_lin_vel_xy_rational, weight=1.0, params={"scale": 0.25}),
        "track_yaw": RewTerm(func=R.track_ang_vel_z_rational, weight=0.5, params={"scale": 0.25}),
        "unused": RewTerm(func=R.action_l2, weight=0.0),
        "torques": RewTerm(func=R.joint_torques_l2, weight=-1.0e-3, params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*"])}),
        "action_rate": RewTerm(func=R.action_rate_l2, weight=-0.01),
        "hips": RewTerm(func=R.joint_deviation_l1, weight=-0.1,
                        params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*_HAA"])}),
        "air_time": RewTerm(func=R.feet_air_time, weight=0.5, params={"command_name": "base_velocity", "threshold": 0.01,
                                                                     "sensor_cfg": SceneEntityCfg("contact_forces", body_names=".*_FOOT")}),
        "fell": RewTerm(func=R.is_terminated, weight=-5.0)}
    cfg.episode_length_s = 7 * cfg.sim.dt * cfg.decimation - 1e-9            # seven steps: episodes end by time-out, too
    return cfg


def _table_of(cfg):
    from cat_envs.tasks.utils.mdp import rewards as R
    return [row[1:] for row in R.build_table(cfg.rewards, T.JOINTS, int(cfg.synthetic.obs_dim))[1]]


def _make_env(cfg, n, seed=42):
    from cat_envs.shim import make
    cfg.scene.num_envs, cfg.seed = n, seed
    return make(TASK, cfg=cfg)


def test_env_rewards_and_dones_equal_the_oracle_env():
    n, steps = 64, 40
    cfg = _shaped_cfg()
    env = _make_env(cfg, n).unwrapped
    assert env.max_episode_length == 7 and env.reward_manager.active_terms[2] == "unused"
    assert "unused" in str(env.reward_manager) and len(env.sim._reward_entries) == 7
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    twin = RT.make_twin(cfg, n, _table_of(cfg), seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=7)
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    env.reset()
    rs = np.random.RandomState(7)
    for s in range(steps):
        a = torch.from_numpy((rs.standard_normal((n, 12)) * 2).astype(np.float32))     # large enough to fall
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(env.sim.cur.cpu().numpy(), orc.stream[0], f"simulator state after step {s}")
        _same_bits(env.reward_manager.compute(None).cpu().numpy(), twin._f(orc.stream[0], "reward")[:, 0], f"raw reward {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(np.float32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(np.float32), f"dones after step {s}")
        np.testing.assert_array_equal(time_outs.cpu().numpy(), o_time_outs.numpy())
    _same_bits(env.reward_manager.record.cpu().numpy(), twin.reward_record, "reward record")
    assert twin.stats["falls"] > 0 and twin.stats["timeouts"] > 0
    # pop_log: the ended sums over the count over the episode length, then floats 16..31 are zero
    rec = twin.reward_record.astype(np.float64)
    log = env.reward_manager.pop_log()
    names = [r for r in env.reward_manager.active_terms if r != "unused"]
    for k, name in enumerate(names):
        assert log[f"Episode_Reward/{name}"] == pytest.approx(rec[:, 16 + k].sum() / rec[:, 31].sum() / env.max_episode_length_s,
                                                              rel=1e-12, abs=1e-300)
    assert log["Episode_Reward/unused"] == 0.0 and len(log) == 8
    after = env.reward_manager.record.cpu().numpy()
    assert (after[:, 16:] == 0).all()
    _same_bits(after[:, :16], twin.reward_record[:, :16], "running sums after pop_log")
    assert env.reward_manager.pop_log() is None


def _trainer(cfg, n, num_steps, fused=True, writer=None, hidden=(64, 64), seed=42):
    """64 envs x 8 steps, one epoch of two minibatches; hidden (64, 64) is the smallest shape the MLP kernels take (widths
    are multiples of 64: ``native.layout_of`` refuses (32, 32))"""
    from cat_envs.shim import load_cfg_from_registry
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.updates_epochs = num_steps, n * num_steps // 2, 1
    agent_cfg.hidden, agent_cfg.save_interval, agent_cfg.fused_rollout = tuple(hidden), 10 ** 9, fused
    env = _make_env(cfg, n, seed)
    torch.manual_seed(seed)
    return PPOTrainer(env, agent_cfg, writer=writer)


def test_step_and_step_into_fill_the_same_reward_plane():
    n, num_steps = 64, 8
    planes = []
    for fused in (True, False):
        tr = _trainer(_shaped_cfg(), n, num_steps, fused=fused)
        assert (tr.sink is not None) == fused
        rs = np.random.RandomState(1)
        eps = torch.from_numpy(rs.standard_normal((num_steps, n, 12)).astype(np.float32)).cuda()
        perm = torch.from_numpy(rs.permutation(n * num_steps).astype(np.int64)).cuda()
        tr.run_iteration(eps_fn=lambda s: eps[s], perm_fn=lambda e: perm)
        torch.cuda.synchronize()
        planes.append((tr.rewards.float().cpu().numpy(), tr.envs.unwrapped.sim.cur.cpu().numpy()))
    np.testing.assert_array_equal(planes[0][0].view(U32), planes[1][0].view(U32))
    np.testing.assert_array_equal(planes[0][1].view(U32), planes[1][1].view(U32))
    assert planes[0][0].std() > 0


def test_rewards_need_the_servo_simulator():
    cfg = _shaped_cfg()
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        _make_env(cfg, 16)


# ------------------------------------------------------------------------------------------ 6: run state
def test_run_state_round_trip_and_refusals():
    from cat_envs.tasks.utils.cleanrl import checkpoint
    n = 64
    rs = np.random.RandomState(5)
    acts = torch.from_numpy(rs.standard_normal((20, n, 12)).astype(np.float32)).cuda()
    a = _make_env(_shaped_cfg(), n).unwrapped
    a.reset()
    for s in range(10):
        a.step(acts[s])
    fp = a.state_fingerprint()
    assert [r[0] for r in fp["reward_terms"]] == ["track_lin", "track_yaw", "torques", "action_rate", "hips", "air_time", "fell"]
    sd = checkpoint.to_plain(a.state_dict())
    assert tuple(sd["rewards"]["record"].shape) == (n, 32) and sd["rewards"]["weights"]["fell"] == -5.0
    b = _make_env(_shaped_cfg(), n).unwrapped
    b.reset()
    rec_ptr = b.reward_manager.record.data_ptr()
    b.load_state_dict(sd)
    assert b.reward_manager.record.data_ptr() == rec_ptr == b.sim._desc.reward_rec         # in place
    for s in range(10, 20):
        ra = a.step(acts[s])[1]
        rb = b.step(acts[s])[1]
    torch.cuda.synchronize()
    for what, x, y in (("state", a.sim.cur, b.sim.cur), ("record", a.reward_manager.record, b.reward_manager.record),
                       ("reward_buf", ra, rb)):
        np.testing.assert_array_equal(x.cpu().numpy().view(U32), y.cpu().numpy().view(U32), err_msg=what)
    assert (a.reward_manager.record[:, 31] > 0).any()
    # a state saved without rewards is refused by an env with them, and the reverse
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry, make
    plain_cfg = load_cfg_from_registry(T.TASK, "env_cfg_entry_point")
    plain_cfg.scene.num_envs, plain_cfg.seed = n, 42
    plain_cfg.episode_length_s = _shaped_cfg().episode_length_s
    plain = make(T.TASK, cfg=plain_cfg).unwrapped
    plain.reset()
    assert "reward_terms" not in plain.state_fingerprint() and "rewards" not in plain.state_dict()
    with pytest.raises(ValueError, match="reward_terms"):
        checkpoint.check_fingerprint(fp, plain.state_fingerprint())
    with pytest.raises(ValueError, match="reward_terms"):
        checkpoint.check_fingerprint(plain.state_fingerprint(), fp)
    with pytest.raises(ValueError, match="reward"):
        plain.check_state_dict(sd)
    with pytest.raises(ValueError, match="rewards"):
        b.check_state_dict(checkpoint.to_plain(plain.state_dict()))


# ------------------------------------------------------------------------------------------ 7: the trainer
class _Scalars:
    def __init__(self):
        self.rows = []

    def add_scalar(self, key, value, step):
        self.rows.append((key, float(value), int(step)))


def test_trainer_logs_episode_reward_per_term():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(TASK, "env_cfg_entry_point")                # the task's own RewardsCfg: the two exp terms
    cfg.episode_length_s = _shaped_cfg().episode_length_s
    w = _Scalars()
    tr = _trainer(cfg, 64, 8, writer=w)
    for _ in range(2):
        tr.run_iteration()
    torch.cuda.synchronize()
    for name in ("track_lin_vel_xy_exp", "track_ang_vel_z_exp"):
        got = [(v, it) for k, v, it in w.rows if k == f"Episode_Reward/{name}"]
        assert len(got) == 2 and got[1][1] == got[0][1] + 1, (name, w.rows)          # once per iteration
        assert all(np.isfinite(v) and v > 0 for v, _ in got)
    shaped = _trainer(_shaped_cfg(), 64, 8, writer=(w2 := _Scalars()))
    shaped.run_iteration()
    assert {k for k, _, _ in w2.rows if k.startswith("Episode_Reward/")} == {
        f"Episode_Reward/{n}" for n in shaped.envs.unwrapped.reward_manager.active_terms}


def test_a_new_weight_is_in_the_next_step_and_in_nothing_before():
    n = 64
    rs = np.random.RandomState(9)
    acts = torch.from_numpy(rs.standard_normal((4, n, 12)).astype(np.float32)).cuda()
    a, b = _make_env(_shaped_cfg(), n).unwrapped, _make_env(_shaped_cfg(), n).unwrapped
    o = a.sim.off["reward"][0]
    for env in (a, b):
        env.reset()
    for s in range(3):
        a.step(acts[s])
        b.step(acts[s])
        np.testing.assert_array_equal(a.sim.cur.cpu().numpy().view(U32), b.sim.cur.cpu().numpy().view(U32))
    term = b.reward_manager.get_term_cfg("track_lin")
    term.weight = 2.0
    b.reward_manager.set_term_cfg("track_lin", term)
    before = b.sim.cur.clone()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(before.cpu().numpy().view(U32), a.sim.cur.cpu().numpy().view(U32))   # nothing before it
    a.step(acts[3])
    b.step(acts[3])
    ra, rb = a.sim.cur.cpu().numpy(), b.sim.cur.cpu().numpy()
    keep = np.arange(a.sim.F) != o
    np.testing.assert_array_equal(ra[:, keep].view(U32), rb[:, keep].view(U32))
    assert (rb[:, o] > ra[:, o]).all()                                       # the tracking term is positive: twice of it is more
    with pytest.raises(ValueError, match="weight 0 when the env was built"):
        unused = b.reward_manager.get_term_cfg("unused")
        unused.weight = 1.0
        b.reward_manager.set_term_cfg("unused", unused)
