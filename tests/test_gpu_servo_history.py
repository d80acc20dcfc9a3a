"""The servo task's observation history on the device (csrc/servo_sim_kernel.h: the history-on instances of
servo_sim_history.hip, ``Solo12ServoSim(history_floats=T)``): the kernel against ``servo_history_twin`` bit for bit over the
whole stride of both slabs - group depths 2, 3 and 5 on the reference's terms, mixed per-term depths and a field of exactly 512
floats, noise on and off, a recipe that rolls the robot over before the time-out - containment of the launch (the row below
the field, canary floats behind it inside the stride, canary rows past N), env shards, the entry point's and the map writer's
refusals.  DESIGN section 9, "History".

Shapes: 1 env, 17 and 33 (16 envs per workgroup: a ragged last one, whose spare lane groups must write nothing); episodes of
5 steps, 12 steps, so every env ends two episodes by time-out.  The pack is the one with the built-in termination table, the
identity action and actuator tables and the switched-off randomisation block, which is also what the twin chain restates."""
import numpy as np
import pytest
import torch

import servo_history_twin as HT
import servo_obs_twin as OT
import servo_randomize_twin as ZT
import servo_reward_twin as RT
import test_gpu_servo_events as GE
import test_servo_history_twin as HC
import test_servo_terminations_twin as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
F32 = np.float32
CANARY, GUARD, TAIL = GE.CANARY, GE.GUARD, 8
STEPS, MAX_LEN = 12, 5
_same_bits = GE._same_bits


def case(name):
    """(entries of the current frame, map words) of a depth case"""
    group = {"group2": lambda: HC.group_with(group_depth=2), "group3": lambda: HC.group_with(group_depth=3),
             "group5": lambda: HC.group_with(group_depth=5), "mixed": lambda: HC.group_with(depths=[3, 1, 5, 2, 1, 4]),
             "t512": HC.group_of_512}[name]()
    table = HC.table_of(group)
    return table[0], np.asarray(table.history, U32)


FLOATS = {"group2": 90, "group3": 135, "group5": 225, "mixed": 3 * 3 + 3 + 3 * 5 + 12 * 2 + 12 + 12 * 4, "t512": 512}


def recipe(n, roll=False):
    """12 steps of N(0, 1) actions, first episode lengths in 0 .. 4; ``roll``: +4 on the left HFE columns, -4 on the right"""
    rs = np.random.RandomState(11)
    acts, ep0 = rs.standard_normal((STEPS, n, 12)).astype(F32), rs.randint(0, MAX_LEN, n)
    if roll:
        acts[:, :, [1, 7]] += 4
        acts[:, :, [4, 10]] -= 4
    return acts, ep0


def _terms():
    return TC.entries_of(TC.builtin_cfg())


def _device_sim(n, entries, words, env_offset=0, history=True):
    """a simulator with the observation table ``entries`` and the history map ``words`` (``history`` False: the same pack
    without the history descriptor); its state buffer and its two slabs are ``TAIL`` floats wider than its row, canaries, and
    the slabs have canary rows behind them"""
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    sim = Solo12ServoSim(n, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                         policy_obs_dim=len(entries), terminations=True, randomize=True, env_offset=env_offset,
                         history_floats=len(words) if history else 0)
    sim.set_observation_table(entries)
    sim.set_termination_table(_terms())
    if history:
        sim.set_history_table(words)
    else:
        sim.set_randomize_block(sim.neutral_randomize_words())
    # widen the stride: the kernel takes it from the descriptor, the views from ``F``
    sim.row_end = sim.F
    sim.F += TAIL
    sim.cur = torch.full((n, sim.F), CANARY, device="cuda")
    sim._desc.state_in, sim._desc.row_stride = sim.cur.data_ptr(), sim.F
    sim._build_scene()
    sim._guarded = [torch.full((n + GUARD, sim.F), CANARY, device="cuda") for _ in range(2)]
    sim._slabs = [g[:n] for g in sim._guarded]
    return sim


def _run_device(sim, acts, ep0):
    """slabs [steps + 1, N, row_end] and the canary tail checked after every launch"""
    dev = GE._run_device(sim, acts, ep0, max_len=MAX_LEN)
    assert (dev[:, :, sim.row_end:] == CANARY).all(), "a launch wrote behind the padded field inside the stride"
    return dev[:, :, :sim.row_end]


_REF = {}


def reference(n, name, noise=True, roll=False, offset=0, total=None):
    """the twin's run (computed once per case and left unchanged): (twin, actions, ep0, slabs)"""
    key = (n, name, noise, roll, offset, total)
    if key not in _REF:
        entries, words = case(name)
        entries = OT.with_corruption(entries, noise)
        inner = ZT.make_twin(TC.env_cfg(), n, terminations=_terms(), obs_table=entries, max_len=MAX_LEN, env_offset=offset)
        tw = HT.ServoHistoryTwin(inner, words)
        acts, ep0 = recipe(total or n, roll)
        acts, ep0 = np.ascontiguousarray(acts[:, offset:offset + n]), ep0[offset:offset + n]
        slabs = HT.run_history_twin(tw, acts, ep0)
        slabs.setflags(write=False)
        _REF[key] = (tw, acts, ep0, slabs)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: the kernel against the twin
@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("name", ["group2", "group3", "group5", "mixed", "t512"])
@pytest.mark.parametrize("n", [1, 17, 33])
def test_whole_stride_of_both_slabs_equals_the_twin_bit_for_bit(n, name, noise):
    from cat_envs import native
    tw, acts, ep0, ref = reference(n, name, noise)
    entries, words = case(name)
    sim = _device_sim(n, OT.with_corruption(entries, noise), words)
    assert sim.off == tw.off and sim.row_floats == tw.row_floats and sim.row_end == tw.stride
    assert sim.T == FLOATS[name] == tw.T and sim._desc.reserved == native.SERVO_EXT_HISTORY
    assert sim._desc.row_floats == sim.row_floats < sim._desc.row_stride == sim.F
    dev = _run_device(sim, acts, ep0)
    _same_bits(dev, ref, f"slabs of {name} at {n} envs, noise {noise}")
    # every env ended two episodes by time-out; the slot before the newest one does hold another frame
    assert (ref[-1, :, tw.off["servo"][0] + 13] >= 2).all()
    a = tw.off["policy_obs_hist"][0]
    new = int(np.nonzero(words & HT.NEWEST)[0][0])                           # the first term's newest slot (its depth is above 1)
    assert (ref[3:, :, a + new] != ref[3:, :, a + new - int(words[new] >> 8 & 0xFF)]).any()


def test_an_episode_that_ends_by_a_roll_over_fills_the_history():
    n, name = 17, "group3"
    tw, acts, ep0, ref = reference(n, name, roll=True)
    # the twin first: some env has hard_reset in a step before its time-out, so the fill after a termination is compared
    hard = ref[1:, :, tw.off["hard_reset"][0]] > 0
    ep_len, early = ep0.astype(np.int64).copy(), 0
    for s in range(STEPS):
        early += int((hard[s] & (ep_len + 1 < MAX_LEN)).sum())
        ep_len = np.where(hard[s] | (ep_len + 1 >= MAX_LEN), 0, ep_len + 1)
    assert early >= 1
    # ... and the row written by such a step holds the post-reset frame in every slot
    a, p = tw.off["policy_obs_hist"][0], tw.off["policy_obs"][0]
    s, e = (int(x[0]) for x in np.nonzero(hard))
    for slot in range(3):
        np.testing.assert_array_equal(ref[s + 1, e, a + 3 * slot:a + 3 * slot + 3].view(U32), ref[s + 1, e, p:p + 3].view(U32))
    entries, words = case(name)
    dev = _run_device(_device_sim(n, entries, words), acts, ep0)
    _same_bits(dev, ref, "slabs of the roll-over recipe")


# ------------------------------------------------------------------------------------------ 2: containment
@pytest.mark.parametrize("n", [17, 33])
def test_the_row_below_the_field_is_the_launch_without_the_history_descriptor(n):
    from cat_envs import native
    entries, words = case("group3")
    acts, ep0 = recipe(n)
    with_h = _device_sim(n, entries, words)
    without = _device_sim(n, entries, words, history=False)
    assert without._desc.reserved == native.SERVO_EXT_RANDOMIZE and without.row_end == without.row_floats == with_h.row_floats
    assert with_h.row_end == with_h.row_floats + 136
    on, off = _run_device(with_h, acts, ep0), _run_device(without, acts, ep0)
    np.testing.assert_array_equal(on[:, :, :with_h.row_floats].view(U32), off.view(U32))
    assert (on[:, :, with_h.row_floats:] != 0).any()


def test_shards_reproduce_the_rows_of_one_simulator():
    name = "group3"
    entries, words = case(name)
    whole = reference(32, name)
    _same_bits(_run_device(_device_sim(32, entries, words), whole[1], whole[2]), whole[3], "one simulator of 32 envs")
    for off in (0, 16):
        tw, acts, ep0, ref = reference(16, name, offset=off, total=32)
        np.testing.assert_array_equal(ref.view(U32), whole[3][:, off:off + 16].view(U32))
        shard = _run_device(_device_sim(16, entries, words, env_offset=off), acts, ep0)
        _same_bits(shard, whole[3][:, off:off + 16], f"the shard at env_offset {off}")


# ------------------------------------------------------------------------------------------ 3: refusals
def test_descriptor_and_map_are_checked():
    from cat_envs import native
    entries, words = case("group3")
    sim = _device_sim(16, entries, words)
    d = sim._desc
    action = torch.zeros(16, 12, device="cuda")
    d.state_out, d.action = sim._slabs[0].data_ptr(), action.data_ptr()
    sim._nat.servo_sim_step(d)                                               # the descriptor as it stands is fine
    assert d.reserved == native.SERVO_EXT_HISTORY and d.hist.floats == 135 and d.hist.off_hist == sim.row_floats
    good = d.hist.map
    others = (d.state_in, d.state_out, d.state_in + 64, d.state_out + 4 * sim.F, d.action, d.obs.table, d.obs.table + 32,
              d.term.table, d.term.rec, d.act.table, d.actu.table, d.rnd.block, d.rnd.block + 64, d.act.table + 32)
    for bad in (None, good + 4, good + 8, *others):                           # NULL, misaligned, aliasing
        d.hist.map = bad
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.hist.map = good
    for floats in (0, -4, 513, 135 + TAIL + 4):                               # T out of range, or past the stride
        d.hist.floats = floats
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.hist.floats = 135
    for off in (sim.row_floats - 4, sim.row_floats + 2, sim.row_floats + TAIL + 4, 0, -4):   # inside the LDS part, misaligned, past
        d.hist.off_hist = off
        with pytest.raises(RuntimeError, match="bad argument"):
            sim._nat.servo_sim_step(d)
    d.hist.off_hist = sim.row_floats
    table, width = d.obs.table, d.obs.width
    d.obs.table, d.obs.width = None, 0                                        # under this value the observations are never absent
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.obs.table, d.obs.width = table, width
    sim._nat.servo_sim_step(d)
    # every older value of `reserved` keeps its meaning: the same descriptor announced as randomisation runs that launch
    d.reserved = native.SERVO_EXT_RANDOMIZE
    sim._nat.servo_sim_step(d)
    d.reserved = native.SERVO_EXT_HISTORY
    torch.cuda.synchronize()
    for g in sim._guarded:
        assert (g[sim.N:] == CANARY).all() and (g[:sim.N, sim.row_end:] == CANARY).all()
    # the simulator checks what the library cannot read

    def edit(i, value):
        w = words.copy()
        w[i] = value
        return w
    unfinished = words.copy()
    unfinished[6:9] &= 0xFFFF                                                # the first term's last slot is not the newest
    seventeen = np.concatenate([np.asarray([1 << 8 | (HT.NEWEST if s == 16 else 0) for s in range(17)], U32), words[17:]])
    for bad, what in ((edit(4, 0x300 | 5), "not one slot"), (edit(0, 0x400), "not one slot"), (edit(2, 0x10302), "not one slot"),
                      (unfinished, "no newest"), (edit(0, 0x20300), "bits above 16"), (edit(0, 0), "frame width"),
                      (edit(0, 46 << 8), "frame width"), (edit(134, 45 | 12 << 8 | 1 << 16), "not one slot"),
                      (seventeen, "17 slots"), (words[:-1], "one word per float")):
        with pytest.raises(ValueError, match=what):
            sim.set_history_table(bad)
    sim.set_history_table(words)
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = TC.env_cfg()
    args = (16, 45, "cuda", RT.SEED, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, sim._episode_length, sim._reset)
    with pytest.raises(ValueError, match="needs a policy observation"):
        Solo12ServoSim(*args, history_floats=135)
    with pytest.raises(ValueError, match="needs a policy observation"):
        Solo12ServoSim(*args, policy_obs_dim=45, history_floats=513)
    with pytest.raises(ValueError, match="without a history field"):
        Solo12ServoSim(*args, policy_obs_dim=45).set_history_table(words)
    with pytest.raises(ValueError, match="set_observation_table comes first"):
        Solo12ServoSim(*args, policy_obs_dim=45, history_floats=135).set_history_table(words)
