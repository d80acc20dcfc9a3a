"""The servo task's randomisation block on the device (csrc/servo_sim_kernel.h: the randomisation-on instances of
servo_sim_randomize.hip, ``Solo12ServoSim(randomize=True)``): the kernel against ``servo_randomize_twin`` bit for bit - slabs,
evaluation record, trace, reward record - each term alone and in each mode, a block with nothing on against the launch without
the pack, composition with all six blocks and the reference's robot, the switch and new gains between two launches, env
shards, the entry point's refusals, the env and the trainer on -Servo-Randomized-v0.  DESIGN section 9, "Randomisation".

Test cfg: the recipe of tests/test_servo_randomize_twin.py (gains scaled per env, friction and an absolute armature per
episode, mass added per episode, on the mixed robot of the actuator suite), episodes of 25 steps, 60 steps of N(0, 1) actions;
the CPU suite shows that every rule of the model fires in this recipe at 17 envs.  Shapes: 1 env, 17 (a ragged workgroup), 64
and 1000 (several workgroups, a ragged last one)."""
import numpy as np
import pytest
import torch

import servo_randomize_twin as ZT
import servo_reward_twin as RT
import test_gpu_servo_actuators as GA
import test_gpu_servo_events as GE
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_commands_twin as CC
import test_servo_randomize_twin as ZC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, STEPS, MAX_LEN = GE.CANARY, GE.GUARD, ZC.STEPS, ZC.MAX_LEN
_same_bits = GE._same_bits


def _device_sim(n, words, actuators="mixed", actions=None, terms=None, commands=None, events=None, obs_table=None, table=(),
                tilt_max=None, env_offset=0):
    """a simulator with the randomisation block ``words`` behind the actuator table ``actuators`` ("mixed": the mixed robot;
    None: the identity table the block's writer installs); its two slabs are the first ``n`` rows of buffers with canary
    rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg(tilt_max)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=0 if obs_table is None else len(obs_table), events=events is not None,
                         commands=commands is not None, terminations=terms is not None, actions=actions is not None,
                         randomize=True, env_offset=env_offset)
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
        sim.set_actuator_table(UC.mixed_entries() if isinstance(actuators, str) else actuators)
    sim.set_randomize_block(words)
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, actions, ep0, before_step=None):
    return GE._run_device(sim, actions, ep0, before_step=before_step, max_len=MAX_LEN)


_REF = {}


def reference(n, words, actuators="mixed", actions=None, switch=None, gains=None, tilt_max=None, offset=0, total=None, **kw):
    """the twin's run of the recipe (computed once per case and left unchanged): (twin, actions, ep0, slabs).  ``offset``,
    ``total``: envs offset .. offset + n of the recipe for ``total`` envs"""
    entries, width = actions if actions is not None else (None, 12)
    robot = UC.mixed_entries() if isinstance(actuators, str) else actuators
    key = (n, words.tobytes(), repr(robot), repr(entries), width, None if switch is None else (switch[0], switch[1].tobytes()),
           None if gains is None else (gains[0], repr(gains[1])), tilt_max, offset, total,
           repr(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in kw.items())))
    if key not in _REF:
        tw = ZT.make_twin(TC.env_cfg(tilt_max), n, randomize=words, actuators=robot, actions=entries, width=width,
                          max_len=MAX_LEN, env_offset=offset, **kw)
        acts, ep0 = AC.recipe(total or n, width)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:offset + n]), ep0[offset:offset + n]
        slabs = ZT.run_randomize_twin(tw, acts, ep0, switch=switch, gains=gains)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_records_and_trace_equal_the_twin_bit_for_bit(n):
    words, k = ZC.recipe_block(), min(n, 16)
    tw, acts, ep0, ref = reference(n, words, table=RT.ALL_NON_EXP, trace_envs=k, trace_capacity=STEPS)
    sim = _device_sim(n, words, table=RT.ALL_NON_EXP)
    assert sim.off == tw.off and sim.F == tw.F == 308 + 48                    # the row is the actuators' row
    rec = torch.zeros(n, 12, device="cuda")
    trace = torch.zeros(STEPS, k, 72, device="cuda")
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs of the recipe")
    _same_bits(rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(trace.cpu().numpy(), tw.trace, "trace")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    # the evaluation launch (a record, no trace) and the training launch give the same rows
    sim2 = _device_sim(n, words, table=RT.ALL_NON_EXP)
    sim2.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim2, acts, ep0), ref, "slabs of the evaluation launch")
    sim3 = _device_sim(n, words, table=RT.ALL_NON_EXP)
    _same_bits(_run_device(sim3, acts, ep0), ref, "slabs of the training launch")
    _same_bits(sim3.reward_record.cpu().numpy(), tw.reward_record, "reward record of the training launch")
    # ... and without a reward table, in all three launches
    tw0, _, _, ref0 = reference(n, words, trace_envs=k, trace_capacity=STEPS)
    _same_bits(_run_device(_device_sim(n, words), acts, ep0), ref0, "slabs of the training launch without rewards")
    sim4 = _device_sim(n, words)
    sim4.set_eval_record(torch.zeros(n, 12, device="cuda"))
    _same_bits(_run_device(sim4, acts, ep0), ref0, "slabs of the evaluation launch without rewards")
    sim5 = _device_sim(n, words)
    rec5, trace5 = torch.zeros(n, 12, device="cuda"), torch.zeros(STEPS, k, 72, device="cuda")
    sim5.set_eval_record(rec5)
    sim5.set_trace(trace5)
    _same_bits(_run_device(sim5, acts, ep0), ref0, "slabs of the step-response launch without rewards")
    _same_bits(trace5.cpu().numpy(), tw0.trace, "trace without rewards")
    _same_bits(rec5.cpu().numpy(), tw0.record, "evaluation record without rewards")


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("only", ["gains", "joint", "mass"])
def test_each_term_alone_in_each_mode_at_a_ragged_workgroup(only, reset):
    n = 17
    words = ZC.recipe_block(only=only, reset=reset)
    tw, acts, ep0, ref = reference(n, words)
    _same_bits(_run_device(_device_sim(n, words), acts, ep0), ref, f"slabs with {only} alone, reset mode {reset}")
    nominal = reference(n, ZC.recipe_block(enabled=False))[3]
    assert (ref != nominal).any()


def test_on_top_of_all_six_reference_blocks_and_the_reference_robot():
    from cat_envs.assets.odri import SOLO12_MINIMAL_CFG
    from cat_envs.tasks.utils.mdp import actuators as UM
    import servo_twin as T
    n = 17
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    robot = UM.build_table(SOLO12_MINIMAL_CFG, T.JOINTS, cfg.synthetic, cfg.decimation, T.DEFAULT_JOINT_POS)[0]
    words = ZC.recipe_block()
    _, obs_table, events = AC.reference_blocks()
    terms = TC.entries_of(TC.liveness_cfg())
    blocks = dict(commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    actions = (AC.reference_perm()[0], 12)
    tw, acts, ep0, ref = reference(n, words, robot, actions, tilt_max=TC.LIVE_TILT_MAX, terminations=terms, **blocks)
    sim = _device_sim(n, words, robot, actions, terms=terms, tilt_max=TC.LIVE_TILT_MAX, **blocks)
    assert sim.off == tw.off and sim.F == tw.F == 364 + 48
    _same_bits(_run_device(sim, acts, ep0), ref, "rows")
    _same_bits(sim.termination_record.cpu().numpy(), tw.term_record, "termination record")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    assert tw.stats["ended_by_termination"] >= 1 and tw.stats["ended_by_time_out"] >= 1


# ------------------------------------------------------------------------------------------ 2: nothing on
@pytest.mark.parametrize("which", ["no quantity", "switch off"])
@pytest.mark.parametrize("rewards", [False, True])
def test_nothing_on_is_the_actuators_launch_without_the_pack(rewards, which):
    from cat_envs import native
    n, k = 64, 16
    acts, ep0 = AC.recipe(n, 12)
    table = RT.ALL_NON_EXP if rewards else ()
    words = ZC._off_blocks()[which]
    got = []
    for sim in (_device_sim(n, words, table=table, tilt_max=TC.LIVE_TILT_MAX),
                GA._device_sim(n, UC.mixed_entries(), table=table, tilt_max=TC.LIVE_TILT_MAX)):
        rec = torch.zeros(n, 12, device="cuda")
        trace = torch.zeros(STEPS, k, 72, device="cuda")
        sim.set_eval_record(rec)
        sim.set_trace(trace)
        got.append((_run_device(sim, acts, ep0), rec.cpu().numpy(), trace.cpu().numpy(), sim))
    (on, rec_on, trace_on, sim), (off, rec_off, trace_off, plain) = got
    assert sim._desc.reserved == native.SERVO_EXT_RANDOMIZE and plain._desc.reserved == native.SERVO_EXT_ACTUATORS
    assert sim.F == plain.F and sim.off == plain.off
    np.testing.assert_array_equal(on.view(U32), off.view(U32))
    np.testing.assert_array_equal(rec_on.view(U32), rec_off.view(U32))
    np.testing.assert_array_equal(trace_on.view(U32), trace_off.view(U32))
    if rewards:
        np.testing.assert_array_equal(sim.reward_record.cpu().numpy().view(U32), plain.reward_record.cpu().numpy().view(U32))
    assert (on[:, :, sim.off["hard_reset"][0]] > 0).sum() >= 5               # falls do occur
    # the training launches, too; and a simulator without a robot gets the identity tables
    on_t = _run_device(_device_sim(n, words, table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    np.testing.assert_array_equal(on_t.view(U32), on.view(U32))
    bare = _run_device(_device_sim(n, words, actuators=None, table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    ident = _run_device(GA._device_sim(n, "identity", table=table, tilt_max=TC.LIVE_TILT_MAX), acts, ep0)
    np.testing.assert_array_equal(bare.view(U32), ident.view(U32))


# ------------------------------------------------------------------------------------------ 3: between two launches
def test_the_switch_and_new_gains_are_in_the_very_next_launch():
    n, at, at2 = 64, 20, 35
    on, off = ZC.recipe_block(), ZC.recipe_block(enabled=False)
    before = UC.mixed_entries()
    after = [dict(e, kp=1.0, effort_limit=1.5) if j in (1, 7, 10) else e for j, e in enumerate(before)]
    tw, acts, ep0, ref = reference(n, on, switch=(at, off), gains=(at2, after))
    sim = _device_sim(n, on)

    def before_step(s):
        if s == at:
            sim.set_randomize_block(off)                                     # the flag word alone is copied
        if s == at2:
            sim.set_actuator_table(after)
    dev = _run_device(sim, acts, ep0, before_step=before_step)
    _same_bits(dev, ref, "slabs with the switch off before step 20 and new gains before step 35")
    old = reference(n, on)[3]
    np.testing.assert_array_equal(ref[:at + 1].view(U32), old[:at + 1].view(U32))
    assert (ref[at + 1] != old[at + 1]).any()
    # ... and back on, with the gains scaled from the new table
    tw2, _, _, ref2 = reference(n, off, switch=(at, on), gains=(at, after))
    sim2 = _device_sim(n, off)

    def before_step2(s):
        if s == at:
            sim2.set_randomize_block(on)
            sim2.set_actuator_table(after)
    _same_bits(_run_device(sim2, acts, ep0, before_step=before_step2), ref2, "slabs with the switch on before step 20")
    tau = tw2.off["applied_torque"][0]
    for j in (1, 7, 10):
        assert np.abs(ref2[at + 1:, :, tau + j]).max() <= 1.5 < np.abs(ref2[1:at + 1, :, tau + j]).max()


def test_shards_reproduce_the_rows_of_one_simulator():
    words = ZC.recipe_block()
    whole = reference(64, words)
    dev = _run_device(_device_sim(64, words), whole[1], whole[2])
    _same_bits(dev, whole[3], "one simulator of 64 envs")
    for off in (0, 32):
        tw, acts, ep0, ref = reference(32, words, offset=off, total=64)
        np.testing.assert_array_equal(ref.view(U32), whole[3][:, off:off + 32].view(U32))
        shard = _run_device(_device_sim(32, words, env_offset=off), acts, ep0)
        _same_bits(shard, whole[3][:, off:off + 32], f"the shard at env_offset {off}")


# ------------------------------------------------------------------------------------------ 4: the entry point's refusals
def test_descriptor_and_block_are_checked():
    from cat_envs import native
    _, obs_table, events = AC.reference_blocks()
    sim = _device_sim(16, ZC.recipe_block(), "mixed", AC.entries_of(AC.mixed_cfg()), terms=TC.entries_of(TC.liveness_cfg()),
                      commands=CC.words_of(CC.commands_cfg_of()), events=events, obs_table=obs_table, table=RT.ALL_NON_EXP)
    d = sim._desc
    action = torch.zeros(16, 8, device="cuda")
    d.state_out, d.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_RANDOMIZE and list(d.rnd.reserved) == [0, 0]
    sim.set_eval_record(torch.zeros(16, 12, device="cuda"))
    good = d.rnd.block
    others = (d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, d.obs.table, d.ev.block, d.cmd.block,
              d.term.table, d.term.rec, d.act.table, d.actu.table, d.actu.table + 32, d.actu.table - 64, d.ev.block + 64,
              d.cmd.block - 64)
    for bad in (None, good + 4, good + 8, *others):                           # NULL, misaligned, aliasing
        d.rnd.block = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.rnd.block = good
    for i in (0, 1):
        d.rnd.reserved[i] = 1
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
        d.rnd.reserved[i] = 0
    good_actu = d.actu.table
    d.actu.table = None                                                      # under this value the actuator table is never absent
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.actu.table = good_actu
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all()
    # every older value of `reserved` keeps its meaning: the same descriptor announced as actuators runs that launch
    d.reserved = native.SERVO_EXT_ACTUATORS
    sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_RANDOMIZE
    torch.cuda.synchronize()
    # the simulator checks what the library cannot read
    ok = ZC.recipe_block()

    def edit(word, value, as_int=False):
        w = ok.copy()
        (w.view(np.int32) if as_int else w)[word] = value
        return w
    W = ZT.WORDS
    for bad, what in ((edit(W["flags"], 0x40, True), "unknown bits"), (edit(W["ops"], 3, True), "operations"),
                      (edit(W["gains_mask"], 0x1000, True), "masks"), (edit(W["stiffness"], float("nan")), "finite"),
                      (edit(W["friction"] + 1, -0.1), "width"), (edit(W["m0"], 0.0), "m0"), (edit(5, 1.0), "spare"),
                      (edit(W["ops"], 0, True), "friction cannot be scaled"), (ok[:-1], "32 words")):
        with pytest.raises(ValueError, match=what):
            sim.set_randomize_block(bad)
    with pytest.raises(ValueError, match="without a randomisation descriptor"):
        GA._device_sim(16, UC.mixed_entries()).set_randomize_block(ok)


# ------------------------------------------------------------------------------------------ 5: the env and the trainer
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Randomized-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-Randomized-v0"


def _env_cfg(task=TASK, n=64, seed=42):
    cfg = CC._cfg(task)
    cfg.episode_length_s = MAX_LEN * cfg.sim.dt * cfg.decimation - 1e-9      # 25 steps: episodes end by time-out, too
    cfg.scene.num_envs, cfg.seed = n, seed
    return cfg


def test_the_env_launches_the_pack_and_its_managers_speak_isaaclab():
    from cat_envs import native
    from cat_envs.shim import make
    from cat_envs.tasks.utils.mdp import randomization as RZ
    env = make(TASK, cfg=_env_cfg(n=16)).unwrapped
    em, sim = env.event_manager, env.sim
    assert sim._desc.reserved == native.SERVO_EXT_RANDOMIZE and sim._event_block is None and not sim._desc.ev.block   # no event pack
    assert em.active_terms == {"startup": ["actuator_gains", "add_base_mass"], "reset": ["joint_parameters"]}
    assert em.inert == ["add_base_mass.recompute_inertia"] and sorted(em.randomization["terms"]) == sorted(sum(em.active_terms.values(), []))
    assert "randomization" in env.state_dict()["events"] and em.randomization_enabled
    flag = lambda: int(sim._randomize_block.cpu().numpy().view(np.int32)[0])   # noqa: E731
    np.testing.assert_array_equal(sim._randomize_block.cpu().numpy().view(U32), RZ.pack(env._randomization).view(U32))
    assert flag() & 1
    env.reset()
    env.step(torch.zeros(16, 12, device="cuda"))
    env.set_randomization(False)
    assert not flag() & 1 and (flag() | 1) == int(RZ.pack(env._randomization).view(np.int32)[0])
    env.step(torch.zeros(16, 12, device="cuda"))
    sd = env.state_dict()
    assert sd["events"]["randomization"] is False
    env.set_randomization(True)
    env.load_state_dict(sd)
    assert not flag() & 1 and not em.randomization_enabled
    # set_gains repeats the stability check at the worst corner of the ranges: 2 a + b < 4 with dt 0.005, inertia 0.00436207
    env.actuators.set_gains(damping=1.0)
    with pytest.raises(ValueError, match="'actuator_gains'.*unstable"):
        env.actuators.set_gains(damping=1.5)                                 # 1.2 * 1.5 * 0.005 / 0.00436 = 2.06: 2 a > 4
    assert env.actuators.damping.tolist() == [1.0] * 12
    torch.cuda.synchronize()
    # all six blocks: the event pack and the randomisation pack together
    ref = make(REFERENCE, cfg=_env_cfg(REFERENCE, n=16)).unwrapped
    assert ref.sim._desc.reserved == native.SERVO_EXT_RANDOMIZE and ref.sim._desc.ev.block and ref.sim.F == 364 + 48
    assert ref.event_manager.active_terms["interval"] == ["push_robot"]
    ref.reset()
    ref.step(torch.zeros(16, 12, device="cuda"))
    assert torch.isfinite(ref.sim.cur).all()
    cfg = _env_cfg(n=16)
    cfg.synthetic.kind = "stream"
    with pytest.raises(TypeError, match="closed-loop simulator"):
        make(TASK, cfg=cfg)


def test_evaluate_policy_sets_the_switch_for_the_call_and_restores_it():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    n, steps = 64, 30
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((45, 12)).astype(F32) * 0.5).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 3                              # noqa: E731
    env = make(TASK, cfg=_env_cfg(n=n))
    em = env.unwrapped.event_manager
    on = evaluate_policy(env, policy, steps, fresh_cat_state=True)
    off = evaluate_policy(env, policy, steps, fresh_cat_state=True, randomization=False)
    assert em.randomization_enabled and int(env.unwrapped.sim._randomize_block.cpu().numpy().view(np.int32)[0]) & 1
    again = evaluate_policy(env, policy, steps, fresh_cat_state=True, randomization=True)
    assert np.isfinite(on.per_env).all() and on.per_env[:, 0].min() == steps
    np.testing.assert_array_equal(on.per_env.view(U32), again.per_env.view(U32))
    assert (on.per_env != off.per_env).any()                                 # the nominal robot is another robot
    # the nominal robot is the -Servo-Actuators task's
    plain = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Actuators-v0"
    nominal = evaluate_policy(make(plain, cfg=_env_cfg(plain, n=n)), policy, steps, fresh_cat_state=True)
    np.testing.assert_array_equal(off.per_env.view(U32), nominal.per_env.view(U32))
    with pytest.raises(TypeError, match="randomises the robot"):
        evaluate_policy(make(plain, cfg=_env_cfg(plain, n=n)), policy, steps, randomization=False)


def _resume_cfgs():
    import test_gpu_resume as RS
    from cat_envs.shim import load_cfg_from_registry
    cfg = CC._cfg(TASK)
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 3, 10 ** 9
    return TASK, cfg, agent_cfg


def test_trainer_three_iterations_finite_and_two_plus_one_equal_three(tmp_path, monkeypatch):
    """3 iterations at 64 envs x 8 steps on the randomised task; the losses are finite and a run resumed after iteration 2 is
    the same run"""
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
        seen["sd"] = u.state_dict()["events"]
    try:
        a, b, tr = RS.check_case(_resume_cfgs, tmp_path, save_at=2, iters=3, probe=probe)
    finally:
        for t in made:
            GA._free_graph(t)
    assert seen["sd"] == {"interval": True, "randomization": True} and len(seen["fp"]["event_terms"][-1]) == 32
    for it in a:
        assert np.isfinite(it["flat"]).all() and np.isfinite(it["actions"]).all() and np.isfinite(it["sim.cur"]).all()
        assert np.isfinite(np.asarray(it["stats"], np.float64)).all()
        assert it["sim.cur"].shape[1] == 308 + 48
    assert (a[0]["flat"] != a[1]["flat"]).any()                               # the update moved the parameters
