"""The servo task's pinned plants on the device (csrc/servo_sim_kernel.h: the plant-on instances of servo_sim_plant.hip,
``Solo12ServoSim.set_fixed_plant``): the kernel against ``servo_plant_twin`` bit for bit - slabs, evaluation record, trace,
reward record - with another plant in every row and with each pin alone, an all-clear table against the launch without the
level on the randomise and on the history pack, a pinned table against the existing randomise launch at zero-width ranges,
composition with all six reference blocks, the reference robot and a depth-3 history, canary rows around the table, env
shards, the entry point's refusals, and ``evaluate_policy(plant=...)``.  DESIGN section 9, "Robustness".

The recipes are the case modules' own (test_gpu_servo_randomize.py: 60 steps, episodes of 25; test_gpu_servo_history.py: 12
steps, episodes of 5), so episodes end inside every run.  Shapes: 1 env (one lane group), 17 (a ragged workgroup), 64 (whole
workgroups) and 1000 (many workgroups and a ragged tail)."""
import numpy as np
import pytest
import torch

import servo_history_twin as HT
import servo_plant_twin as PT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import test_gpu_servo_events as GE
import test_gpu_servo_history as HG
import test_gpu_servo_randomize as ZG
import test_servo_actions_twin as AC
import test_servo_actuators_twin as UC
import test_servo_commands_twin as CC
import test_servo_plant_twin as PC
import test_servo_randomize_twin as ZC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
CANARY, GUARD, STEPS, MAX_LEN = ZG.CANARY, ZG.GUARD, ZG.STEPS, ZG.MAX_LEN
_same_bits = GE._same_bits


def _attach(sim, table, trace_envs=0, steps=STEPS, canary=CANARY):
    """the evaluation record (and a trace of the first ``trace_envs`` envs) and the plant table ``table``, which lies between
    ``GUARD`` canary rows on either side"""
    n = sim.N
    sim.rec = torch.zeros(n, 12, device="cuda")
    sim.set_eval_record(sim.rec)
    sim.trace = torch.zeros(steps, trace_envs, 72, device="cuda") if trace_envs else None
    if trace_envs:
        sim.set_trace(sim.trace)
    sim.plant_guarded = torch.full((GUARD + n + GUARD, 8), canary, device="cuda")
    sim.plant_guarded[GUARD:GUARD + n].copy_(torch.from_numpy(np.ascontiguousarray(table, F32)))
    sim.set_fixed_plant(sim.plant_guarded[GUARD:GUARD + n])
    return sim


def _canaries_intact(sim, canary=CANARY):
    g, n = sim.plant_guarded, sim.N
    return bool((g[:GUARD] == canary).all() and (g[GUARD + n:] == canary).all())


_REF = {}


def reference(n, plant, words=None, actuators="mixed", table=(), trace_envs=0, offset=0, total=None):
    """the plant twin's run of the randomise suite's recipe (computed once per case and left unchanged)"""
    words = ZC.recipe_block() if words is None else words
    robot = UC.mixed_entries() if isinstance(actuators, str) else actuators
    key = (n, plant.tobytes(), words.tobytes(), repr(robot), repr(table), trace_envs, offset, total)
    if key not in _REF:
        tw = PT.make_twin(TC.env_cfg(), n, plant=plant, randomize=words, actuators=robot, max_len=MAX_LEN, env_offset=offset,
                          table=table, **(dict(trace_envs=trace_envs, trace_capacity=STEPS) if trace_envs else {}))
        acts, ep0 = AC.recipe(total or n, 12)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:offset + n]), ep0[offset:offset + n]
        slabs = PT.run_plant_twin(tw, acts, ep0)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_record_and_trace_equal_the_twin_bit_for_bit(n):
    from cat_envs import native
    plant, k = PT.mixed_table(n), min(n, 16)
    assert len({r.tobytes() for r in plant}) == n                             # every row another plant
    tw, acts, ep0, ref = reference(n, plant, table=RT.ALL_NON_EXP, trace_envs=k)
    sim = _attach(ZG._device_sim(n, ZC.recipe_block(), table=RT.ALL_NON_EXP), plant, trace_envs=k)
    assert sim.off == tw.off and sim.F == tw.F == 308 + 48                    # the row gets no new state
    assert sim._desc.reserved == native.SERVO_EXT_PLANT and isinstance(sim._desc, native.ServoSimPlant)
    dev = ZG._run_device(sim, acts, ep0)
    _same_bits(dev, ref, "slabs")
    _same_bits(sim.rec.cpu().numpy(), tw.record, "evaluation record")
    _same_bits(sim.trace.cpu().numpy(), tw.trace, "trace")
    _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    assert _canaries_intact(sim)
    # the launch with a record and no trace, and without a reward table
    tw0, _, _, ref0 = reference(n, plant)
    sim0 = _attach(ZG._device_sim(n, ZC.recipe_block()), plant)
    _same_bits(ZG._run_device(sim0, acts, ep0), ref0, "slabs without rewards and trace")
    _same_bits(sim0.rec.cpu().numpy(), tw0.record, "evaluation record without rewards and trace")
    if n >= 2:
        unpinned = ZG.reference(n, ZC.recipe_block())[3]
        np.testing.assert_array_equal(ref0[:, 0].view(U32), unpinned[:, 0].view(U32))   # row 0 pins nothing
        assert (ref0[:, 1] != unpinned[:, 1]).any()                                      # row 1 pins everything


@pytest.mark.parametrize("rewards", [False, True])
@pytest.mark.parametrize("only", PT.QUANTITIES)
def test_each_pin_alone_at_a_ragged_workgroup(only, rewards):
    n = 17
    plant = PT.mixed_table(n)
    plant.view(np.int32)[:, 0] = np.where(np.arange(n) % 3 == 0, 0, PT.BITS[only])   # a third of the envs keep their draws
    table = RT.ALL_NON_EXP if rewards else ()
    tw, acts, ep0, ref = reference(n, plant, table=table)
    sim = _attach(ZG._device_sim(n, ZC.recipe_block(), table=table), plant)
    _same_bits(ZG._run_device(sim, acts, ep0), ref, f"slabs with {only} alone")
    _same_bits(sim.rec.cpu().numpy(), tw.record, "evaluation record")
    if rewards:
        _same_bits(sim.reward_record.cpu().numpy(), tw.reward_record, "reward record")
    unpinned = ZG.reference(n, ZC.recipe_block(), table=table)[3]
    assert (ref[:, 1::3] != unpinned[:, 1::3]).any()
    np.testing.assert_array_equal(ref[:, 0::3].view(U32), unpinned[:, 0::3].view(U32))


# ------------------------------------------------------------------------------------------ 2: device against device
def _with_record(sim, trace_envs=0, steps=STEPS):
    sim.rec = torch.zeros(sim.N, 12, device="cuda")
    sim.set_eval_record(sim.rec)
    sim.trace = torch.zeros(steps, trace_envs, 72, device="cuda") if trace_envs else None
    if trace_envs:
        sim.set_trace(sim.trace)
    return sim


@pytest.mark.parametrize("rewards", [False, True])
def test_an_all_clear_table_is_the_randomise_launch_without_the_level(rewards):
    from cat_envs import native
    n, k = 64, 16
    acts, ep0 = AC.recipe(n, 12)
    table = RT.ALL_NON_EXP if rewards else ()
    loud = PT.mixed_table(n)
    loud.view(np.int32)[:, 0] = 0                                            # values behind clear bits are not read
    on = _attach(ZG._device_sim(n, ZC.recipe_block(), table=table, tilt_max=TC.LIVE_TILT_MAX), loud, trace_envs=k)
    off = _with_record(ZG._device_sim(n, ZC.recipe_block(), table=table, tilt_max=TC.LIVE_TILT_MAX), trace_envs=k)
    assert on._desc.reserved == native.SERVO_EXT_PLANT and off._desc.reserved == native.SERVO_EXT_RANDOMIZE
    a, b = ZG._run_device(on, acts, ep0), ZG._run_device(off, acts, ep0)
    np.testing.assert_array_equal(a.view(U32), b.view(U32))
    np.testing.assert_array_equal(on.rec.cpu().numpy().view(U32), off.rec.cpu().numpy().view(U32))
    np.testing.assert_array_equal(on.trace.cpu().numpy().view(U32), off.trace.cpu().numpy().view(U32))
    if rewards:
        np.testing.assert_array_equal(on.reward_record.cpu().numpy().view(U32), off.reward_record.cpu().numpy().view(U32))
    assert (a[:, :, on.off["hard_reset"][0]] > 0).sum() >= 5                  # falls do occur


def test_an_all_clear_table_is_the_history_launch_without_the_level():
    from cat_envs import native
    n = 33
    entries, words = HG.case("group3")
    acts, ep0 = HG.recipe(n)
    on = _attach(HG._device_sim(n, entries, words), np.zeros((n, 8), F32), steps=HG.STEPS)
    off = _with_record(HG._device_sim(n, entries, words))
    assert on.T == 135 and on._desc.reserved == native.SERVO_EXT_PLANT and off._desc.reserved == native.SERVO_EXT_HISTORY
    assert on._desc.hist.floats == 135 and on._desc.row_stride == off._desc.row_stride
    a, b = HG._run_device(on, acts, ep0), HG._run_device(off, acts, ep0)
    np.testing.assert_array_equal(a.view(U32), b.view(U32))
    np.testing.assert_array_equal(on.rec.cpu().numpy().view(U32), off.rec.cpu().numpy().view(U32))
    assert (a[:, :, on.row_floats:] != 0).any()


@pytest.mark.parametrize("only", [None, "lag", "mass_scale"])
def test_a_pinned_table_is_the_existing_randomise_launch_at_zero_width_ranges(only):
    n = 64
    acts, ep0 = AC.recipe(n, 12)
    words, robot = PC.zero_width_reference(only)
    under = ZC.recipe_block(enabled=only is None)                            # all six pinned: on top of the recipe's draws
    pinned = _attach(ZG._device_sim(n, under, table=RT.ALL_NON_EXP), PC.pinned_table(n, only), trace_envs=16)
    plain = _with_record(ZG._device_sim(n, words, actuators=robot, table=RT.ALL_NON_EXP), trace_envs=16)
    a, b = ZG._run_device(pinned, acts, ep0), ZG._run_device(plain, acts, ep0)
    np.testing.assert_array_equal(a.view(U32), b.view(U32))
    np.testing.assert_array_equal(pinned.rec.cpu().numpy().view(U32), plain.rec.cpu().numpy().view(U32))
    np.testing.assert_array_equal(pinned.trace.cpu().numpy().view(U32), plain.trace.cpu().numpy().view(U32))
    np.testing.assert_array_equal(pinned.reward_record.cpu().numpy().view(U32), plain.reward_record.cpu().numpy().view(U32))


# ------------------------------------------------------------------------------------------ 3: composition
def test_on_top_of_all_six_reference_blocks_the_reference_robot_and_a_depth_3_history():
    from cat_envs import native
    from cat_envs.assets.odri import SOLO12_MINIMAL_CFG
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    from cat_envs.tasks.utils.mdp import actuators as UM
    import servo_twin as T
    n = 17
    cfg = TC.env_cfg(TC.LIVE_TILT_MAX)
    robot = UM.build_table(SOLO12_MINIMAL_CFG, T.JOINTS, cfg.synthetic, cfg.decimation, T.DEFAULT_JOINT_POS)[0]
    words = ZC.recipe_block()
    _, obs_table, events = AC.reference_blocks()
    terms = TC.entries_of(TC.liveness_cfg())
    commands = CC.words_of(CC.commands_cfg_of())
    actions = (AC.reference_perm()[0], 12)
    hist = HT.history_map([len(obs_table)], [3])
    plant = PT.mixed_table(n)
    plant[:, PT.WORDS["kd_scale"]] = np.minimum(plant[:, PT.WORDS["kd_scale"]], F32(1.1))   # the reference robot's stable range
    inner = PT.make_twin(cfg, n, plant=plant, randomize=words, actuators=robot, actions=actions[0], width=12, terminations=terms,
                         commands=commands, events=events, obs_table=obs_table, table=RT.ALL_NON_EXP, max_len=MAX_LEN)
    tw = HT.ServoHistoryTwin(inner, hist)
    acts, ep0 = AC.recipe(n, 12)
    ref = HT.run_history_twin(tw, acts, ep0)
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=len(obs_table), events=True, commands=True, terminations=True, actions=True,
                         randomize=True, history_floats=len(hist))
    sim.set_observation_table(obs_table)
    sim.set_event_block(events)
    sim.set_command_block(commands)
    sim.set_termination_table(terms)
    sim.set_reward_table(list(RT.ALL_NON_EXP))
    sim.set_action_table(*actions)
    sim.set_actuator_table(robot)
    sim.set_randomize_block(words)
    sim.set_history_table(hist)
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    _attach(sim, plant)
    assert sim.off == tw.off and sim.F == tw.stride == 364 + 48 + 136 and sim._desc.reserved == native.SERVO_EXT_PLANT
    assert sim._desc.ev.block and sim._desc.cmd.block and sim._desc.term.table and sim._desc.hist.map
    _same_bits(GE._run_device(sim, acts, ep0, max_len=MAX_LEN), ref, "rows")
    _same_bits(sim.rec.cpu().numpy(), inner.record, "evaluation record")
    _same_bits(sim.termination_record.cpu().numpy(), inner.term_record, "termination record")
    _same_bits(sim.reward_record.cpu().numpy(), inner.reward_record, "reward record")
    assert inner.stats["ended_by_termination"] >= 1 and inner.stats["ended_by_time_out"] >= 1 and _canaries_intact(sim)


# ------------------------------------------------------------------------------------------ 4: containment
def test_rows_around_the_table_are_neither_written_nor_read():
    n = 17                                                                   # the spare lane groups of the workgroup recompute env 16
    plant = PT.mixed_table(n)
    tw, acts, ep0, ref = reference(n, plant)
    runs = []
    for canary in (CANARY, float("nan")):                                    # rows >= N hold something else: no output moves
        sim = _attach(ZG._device_sim(n, ZC.recipe_block()), plant, canary=canary)
        runs.append((ZG._run_device(sim, acts, ep0), sim.rec.cpu().numpy()))
        g = sim.plant_guarded.cpu().numpy()
        want = np.full((GUARD, 8), canary, F32)
        np.testing.assert_array_equal(g[:GUARD].view(U32), want.view(U32))
        np.testing.assert_array_equal(g[GUARD + n:].view(U32), want.view(U32))
        np.testing.assert_array_equal(g[GUARD:GUARD + n].view(U32), plant.view(U32))
    _same_bits(runs[0][0], ref, "slabs between canary rows")
    np.testing.assert_array_equal(runs[0][0].view(U32), runs[1][0].view(U32))
    np.testing.assert_array_equal(runs[0][1].view(U32), runs[1][1].view(U32))


def test_shards_reproduce_the_rows_of_one_simulator():
    plant = PT.mixed_table(64)
    whole = reference(64, plant)
    dev = ZG._run_device(_attach(ZG._device_sim(64, ZC.recipe_block()), plant), whole[1], whole[2])
    _same_bits(dev, whole[3], "one simulator of 64 envs")
    for off in (0, 32):
        half = np.ascontiguousarray(plant[off:off + 32])
        tw, acts, ep0, ref = reference(32, half, offset=off, total=64)
        np.testing.assert_array_equal(ref.view(U32), whole[3][:, off:off + 32].view(U32))
        shard = ZG._run_device(_attach(ZG._device_sim(32, ZC.recipe_block(), env_offset=off), half), acts, ep0)
        _same_bits(shard, whole[3][:, off:off + 32], f"the shard at env_offset {off}")


# ------------------------------------------------------------------------------------------ 5: the entry point's refusals
def test_descriptor_and_table_are_checked():
    from cat_envs import native
    n = 16
    entries, words = HG.case("group3")
    sim = _attach(HG._device_sim(n, entries, words), PT.mixed_table(n), steps=HG.STEPS)
    d = sim._desc
    action = torch.zeros(n, 12, device="cuda")
    d.state_out, d.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_PLANT and list(d.plant.reserved) == [0, 0] and list(d.rnd.reserved) == [0, 0]
    # a wrong class: the library would read behind it
    short = native.ServoSimHistory()
    short.reserved = native.SERVO_EXT_PLANT
    with pytest.raises(TypeError, match="ServoSimPlant"):
        sim._nat.servo_sim_step(short)
    good = d.plant.table
    others = (d.state_in, d.state_out, d.state_out + 4 * sim.F, d.eval, d.action, d.obs.table, d.term.table, d.term.rec,
              d.act.table, d.actu.table, d.rnd.block, d.hist.map, d.hist.map + 64, d.act.table + 32)
    for bad in (None, good + 4, good + 8, *others):                           # NULL, misaligned, aliasing
        d.plant.table = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.plant.table = good
    for i in (0, 1):
        d.plant.reserved[i] = 1
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
        d.plant.reserved[i] = 0
    rec = d.eval
    d.eval = None                                                            # no evaluation pointer: a plant table is an evaluation input
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.eval = rec
    table, width = d.obs.table, d.obs.width
    d.obs.table, d.obs.width = None, 0                                        # a history that is present needs its observations
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.obs.table, d.obs.width = table, width
    block = d.rnd.block
    d.rnd.block = None                                                       # the randomisation block is never absent
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.rnd.block = block
    sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_HISTORY                                    # every older value of `reserved` keeps its meaning
    sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_PLANT
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all() and (g[:sim.N, sim.row_end:] == CANARY).all()
    assert _canaries_intact(sim)
    # the simulator checks what the library cannot read, and names the row and the quantity
    bad = PT.mixed_table(n)
    bad[5, PT.WORDS["mass_scale"]], bad.view(np.int32)[5, 0] = -1.0, PT.MASS
    with pytest.raises(ValueError, match="row 5: mass_scale must be > 0"):
        sim.set_fixed_plant(torch.from_numpy(bad).cuda())
    with pytest.raises(ValueError, match=r"shape \(16, 8\)"):
        sim.set_fixed_plant(torch.zeros(n + 1, 8, device="cuda"))
    assert sim._desc.plant.table == good                                     # a refused table leaves the attached one
    # detaching gives back exactly the descriptor the simulator had
    sim.set_fixed_plant(None)
    assert type(sim._desc) is native.ServoSimHistory and sim._desc.reserved == native.SERVO_EXT_HISTORY
    assert sim._desc.row_stride == sim.F and sim._desc.eval == rec
    sim._desc.state_out, sim._desc.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(sim._desc)
    with pytest.raises(RuntimeError, match="a plant table is attached"):
        _attach(HG._device_sim(n, entries, words), PT.mixed_table(n), steps=HG.STEPS).state_dict()
    with pytest.raises(ValueError, match="act_hist"):
        GE._device_sim(n, None).set_fixed_plant(torch.zeros(n, 8, device="cuda"))
    torch.cuda.synchronize()


def test_a_simulator_without_a_robot_gets_the_identity_tables_for_the_tables_time():
    import test_gpu_servo_actuators as GA
    from cat_envs import native
    n = 17
    acts, ep0 = AC.recipe(n, 12)
    sim = GA._device_sim(n, UC.mixed_entries())                              # actuators, no randomisation block
    assert type(sim._desc) is native.ServoSimActuators and sim._randomize_block is None
    _attach(sim, np.zeros((n, 8), F32))
    assert sim._desc.reserved == native.SERVO_EXT_PLANT and sim._desc.rnd.block
    on = ZG._run_device(sim, acts, ep0)
    sim.set_fixed_plant(None)
    assert type(sim._desc) is native.ServoSimActuators and sim._desc.reserved == native.SERVO_EXT_ACTUATORS
    assert sim._randomize_block is None and sim._randomize_words is None
    off = ZG._run_device(sim, acts, ep0)                                     # the record is still attached: the evaluation launch
    np.testing.assert_array_equal(on.view(U32), off.view(U32))


# ------------------------------------------------------------------------------------------ 6: evaluate_policy
REFERENCE = ZG.REFERENCE


def test_evaluate_policy_attaches_the_table_for_the_call_and_restores_the_descriptor():
    from cat_envs import native
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy, plant_grid
    n, steps = 48, 30
    env = make(REFERENCE, cfg=ZG._env_cfg(REFERENCE, n=n))
    u = env.unwrapped
    w = torch.from_numpy(np.random.RandomState(3).standard_normal((u.obs_dim, u.act_dim)).astype(F32) * 0.5).cuda()
    policy = lambda obs: torch.tanh(obs @ w) * 3                              # noqa: E731
    plants = plant_grid(kp_scale=(0.6, 1.3, 2), mass_scale=(0.4, 1.5, 2), lag=(0, 8, 2), num_envs=n)
    cls, reserved = type(u.sim._desc), u.sim._desc.reserved
    flag = lambda: int(u.sim._randomize_block.cpu().numpy().view(np.int32)[0])   # noqa: E731
    before = flag()
    assert cls is native.ServoSimRandomize and reserved == native.SERVO_EXT_RANDOMIZE
    res = evaluate_policy(env, policy, steps, fresh_cat_state=True, plant=plants)
    assert type(u.sim._desc) is cls and u.sim._desc.reserved == reserved and flag() == before
    assert u.sim._plant_table is None and not u.sim._desc.eval and not u.sim._desc.fixed_command
    np.testing.assert_array_equal(res.plant.view(U32), plants["packed"].view(U32))
    groups = res.by_plant()
    assert len(groups) == 8 and [g["envs"] for g in groups] == [6] * 8
    assert [g["plant"]["lag"] for g in groups] == [0, 8] * 4 and np.isfinite(res.per_env).all()
    assert len({g["metrics"]["reward_per_step"] for g in groups}) == 8        # another plant, another outcome
    rb = res.robustness()
    assert sorted(rb["by_quantity"]) == ["kp_scale", "lag", "mass_scale"] and rb["groups"] == 8 and rb["spread"] > 0
    # two such calls agree bit for bit; the pins are orthogonal to the switch
    again = evaluate_policy(env, policy, steps, fresh_cat_state=True, plant=plants["packed"])
    np.testing.assert_array_equal(res.per_env.view(U32), again.per_env.view(U32))
    nominal = evaluate_policy(env, policy, steps, fresh_cat_state=True, plant=plants, randomization=False)
    assert (nominal.per_env != res.per_env).any() and flag() == before       # friction and armature keep their draws, or not
    unpinned = evaluate_policy(env, policy, steps, fresh_cat_state=True)
    assert (unpinned.per_env != res.per_env).any() and unpinned.plant is None

    # ... also after a policy that raises, and after a table the writer refuses
    def failing(obs):
        raise RuntimeError("policy failed")
    with pytest.raises(RuntimeError, match="policy failed"):
        evaluate_policy(env, failing, steps, fresh_cat_state=True, plant=plants)
    assert type(u.sim._desc) is cls and u.sim._desc.reserved == reserved and u.sim._plant_table is None and not u.sim._desc.eval
    with pytest.raises(ValueError, match="row 0: lag must be in"):
        evaluate_policy(env, policy, steps, plant=plant_grid(lag=99, num_envs=n))
    assert type(u.sim._desc) is cls and u.sim._desc.reserved == reserved and not u.sim._desc.eval
    with pytest.raises(ValueError, match="48 envs"):
        evaluate_policy(env, policy, steps, plant=plant_grid(lag=1, num_envs=n - 1))
    after = evaluate_policy(env, policy, steps, fresh_cat_state=True, plant=plants)
    np.testing.assert_array_equal(res.per_env.view(U32), after.per_env.view(U32))


# ------------------------------------------------------------------------------------------ 7: play.py
def test_play_sweeps_commands_and_plants_and_writes_the_robustness_file(tmp_path, monkeypatch, capsys):
    """play.py in this process (its own command line; it looks for logs/ under the working directory): --eval_plant with
    --eval_grid gives every (command, plant) pair its envs, the [EVAL] line carries by_plant and robustness, and the two blocks
    are <run>/eval/<checkpoint>_robustness.json"""
    import json
    import os
    import sys
    from cat_envs.shim import load_cfg_from_registry, make
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    agent_cfg = load_cfg_from_registry(REFERENCE, "clean_rl_cfg_entry_point")
    run = tmp_path / "logs" / "clean_rl" / agent_cfg.experiment_name / "run0"
    os.makedirs(run)
    torch.manual_seed(0)
    torch.save(Agent(make(REFERENCE, cfg=ZG._env_cfg(REFERENCE, n=16)), hidden=tuple(agent_cfg.hidden)).state_dict(), run / "model_0.pt")
    sys.path.insert(0, os.path.join(PC.ROOT, "scripts", "clean_rl"))
    try:
        import play
    finally:
        sys.path.pop(0)
    monkeypatch.chdir(tmp_path)
    play.main([f"--task={REFERENCE}", "--headless", "--num_envs", "16", "--video_length", "2", "--eval_steps", "8",
               "--eval_grid", "2", "1", "1", "--eval_plant", "kp_scale=0.8:1.2:2", "lag=0:8:2", "mass_scale=1.3"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("[EVAL] ")]
    assert len(lines) == 1 and "2 commands x 4 plants x 2 on 16 envs" in out
    d = json.loads(lines[0][len("[EVAL] "):])
    assert d["metrics"]["steps"] == 16 * 8 and [g["envs"] for g in d["by_command"]] == [8, 8]
    mass = float(F32(1.3))
    assert [g["plant"] for g in d["by_plant"]] == [{"kp_scale": float(F32(kp)), "mass_scale": mass, "lag": lag}
                                                   for kp in (0.8, 1.2) for lag in (0, 8)]
    assert [g["envs"] for g in d["by_plant"]] == [4] * 4
    rb = d["robustness"]
    assert rb["metric"] == "reward_per_step" and rb["groups"] == 4 and sorted(rb["by_quantity"]) == ["kp_scale", "lag", "mass_scale"]
    with open(run / "eval" / "model_0_robustness.json") as f:
        assert json.load(f) == {"by_plant": d["by_plant"], "robustness": rb}
    with open(run / "eval" / "model_0.json") as f:
        assert json.load(f) == d
    with pytest.raises(SystemExit):
        play.main([f"--task={REFERENCE}", "--headless", "--eval_steps", "8", "--eval_plant", "stiffness=1"])
