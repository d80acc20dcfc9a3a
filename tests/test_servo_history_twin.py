"""The servo task's observation history without a device ("History"): the history descriptor, and the numpy
twin against an independent, naive restatement of the rule of IsaacLab's ObservationManager and CircularBuffer - one ``deque``
per env and term, filled by the first push after a reset, flattened oldest first (PARITY UNPINNED: restated from their
published form).  The device test compares the kernel with this twin, so what the twin is checked against here is what the
kernel is held to."""
import ctypes
from collections import deque

import numpy as np
import pytest

import servo_history_twin as HT
import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T
import test_servo_obs_twin as OC

F32 = np.float32
U32 = np.uint32
N = 17
#: the reference's six terms: frame widths in table order
WIDTHS = [3, 3, 3, 12, 12, 12]


def _om():
    return OC._om()


def group_with(depths=None, group_depth=None):
    """the reference's policy group as a dict cfg; ``depths``: per-term ``history_length``s, ``group_depth``: the group's"""
    OM, O, ObsTerm, Unoise, Entity = _om()
    ref = OM.policy_group(OC._cfg().observations)
    group = {}
    for k, (name, term) in enumerate(OM.group_items(ref)):
        group[name] = ObsTerm(func=term.func, params=term.params, noise=term.noise, clip=term.clip, scale=term.scale,
                              history_length=0 if depths is None else depths[k])
    group["enable_corruption"] = True
    if group_depth is not None:
        group["history_length"] = group_depth
    return group


def group_of_512():
    """a group whose history is exactly the 512 floats the row keeps: 12 x 16 + 12 x 16 + 12 x 10 + 2 x 4, 38 floats per frame"""
    OM, O, ObsTerm, Unoise, Entity = _om()
    noise = Unoise(n_min=-0.01, n_max=0.01)
    return {"q": ObsTerm(func=O.joint_pos, noise=noise, history_length=16),
            "qd": ObsTerm(func=O.joint_vel, noise=noise, scale=0.05, history_length=16),
            "a": ObsTerm(func=O.last_action, history_length=10),
            "haa": ObsTerm(func=O.joint_pos, noise=noise, history_length=4,
                           params={"asset_cfg": Entity("robot", joint_names=["FL_HAA", "HR_HAA"])}),
            "enable_corruption": True}


def table_of(group):
    OM = _om()[0]
    return OM.build_table(group, T.JOINTS, T.DEFAULT_JOINT_POS)


def naive_history(frames, first, widths, depths):
    """[steps + 1, N, T] from the frames [steps + 1, N, P]: ``first`` [steps + 1, N] marks a frame that is the first of an
    episode.  One deque per env and term: a first frame clears it and fills every slot, any other is appended"""
    steps, n, _ = frames.shape
    out = np.zeros((steps, n, sum(w * h for w, h in zip(widths, depths))), F32)
    rings = [[deque(maxlen=h) for h in depths] for _ in range(n)]
    for s in range(steps):
        for e in range(n):
            at, col = 0, 0
            for k, (w, h) in enumerate(zip(widths, depths)):
                ring, frame = rings[e][k], frames[s, e, at:at + w].copy()
                if first[s, e]:
                    ring.clear()
                    ring.extend([frame] * h)
                else:
                    ring.append(frame)
                out[s, e, col:col + w * h] = np.concatenate(list(ring))
                at, col = at + w, col + w * h
    return out


def run(depths, table=None, switch=None, n=N):
    """(twin, slabs, first): the obs twin under the history twin on the reward suite's recipe (50 steps, episodes of 7)"""
    table = table_of(group_with())[0] if table is None else table
    acts, ep0 = RT.recipe(n)
    tw = HT.ServoHistoryTwin(OT.make_twin(OC._cfg(), n, table), HT.history_map(WIDTHS, depths))
    slabs = HT.run_history_twin(tw, acts, ep0, switch=switch)
    # frame s is the first of an episode: the initial one, or the one written by a step that ended its episode
    ep_len = np.asarray(ep0, np.int64).copy()
    first = [np.ones(n, bool)]
    for s in range(len(acts)):
        ep_len += 1
        ended = (ep_len >= tw.max_len) | (tw._f(slabs[s + 1], "hard_reset")[:, 0] > 0.5)
        ep_len[ended] = 0
        first.append(ended)
    return tw, slabs, np.stack(first)


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert [f[0] for f in native.ServoHistory._fields_] == ["map", "off_hist", "floats"]
    assert ctypes.sizeof(native.ServoHistory) == 16 and native.ServoHistory.off_hist.offset == 8
    assert native.ServoSimHistory.rnd.offset == 472 and native.ServoSimHistory.hist.offset == 488
    assert ctypes.sizeof(native.ServoSimHistory) == 504 and issubclass(native.ServoSimHistory, native.ServoSimRandomize)
    assert native.SERVO_EXT_HISTORY == int.from_bytes(b"HST1", "big") and native.SERVO_HISTORY_NEWEST == HT.NEWEST
    assert (native.SERVO_OBS_HISTORY_MAX_FLOATS, native.SERVO_OBS_HISTORY_MAX_DEPTH) == (HT.MAX_FLOATS, HT.MAX_DEPTH) == (512, 16)
    known = [getattr(native, n) for n in dir(native) if n.startswith("SERVO_EXT_")]
    assert len(set(known)) == len(known) == 8


def test_servo_sim_step_refuses_a_descriptor_without_the_history_tail():
    from cat_envs import native
    d = native.ServoSimRandomize()
    d.reserved = native.SERVO_EXT_HISTORY
    with pytest.raises(TypeError, match="ServoSimHistory"):
        native.Native.servo_sim_step(None, d)


def test_the_map_of_the_twin_is_the_map_of_the_manager():
    OM = _om()[0]
    for depths in ([3] * 6, [3, 1, 5, 2, 1, 4], [1] * 6):
        np.testing.assert_array_equal(HT.history_map(WIDTHS, depths), np.asarray(OM.history_map(WIDTHS, depths), U32))


# ------------------------------------------------------------------------------------------ the twin against the deques
@pytest.mark.parametrize("depths", [[3] * 6, [2] * 6, [5] * 6, [3, 1, 5, 2, 1, 4], [16, 1, 1, 1, 1, 1]])
def test_twin_equals_one_deque_per_env_and_term_over_many_episodes_with_noise_on(depths):
    tw, slabs, first = run(depths)
    a, T_ = tw.off["policy_obs_hist"]
    assert T_ == sum(w * h for w, h in zip(WIDTHS, depths)) and tw.stride == tw.row_floats + (T_ + 3) // 4 * 4
    p, P = tw.off["policy_obs"]
    want = naive_history(slabs[:, :, p:p + P], first, WIDTHS, depths)
    np.testing.assert_array_equal(slabs[:, :, a:a + T_].view(U32), want.view(U32))
    assert (slabs[:, :, a + T_:] == 0).all()                                 # the padding
    # the comparison is not vacuous: at least three episodes per env, ended by falls and by time-outs; noise is on (two frames
    # of one episode differ in the command term only through it), and a newest slot does differ from the one before it
    episodes = slabs[-1, :, tw.off["servo"][0] + 13]
    falls = int((slabs[:, :, tw.off["hard_reset"][0]] > 0).sum())
    assert episodes.min() >= 3 and falls > 0 and first[1:].sum() > falls
    k = int(np.argmax(np.asarray(depths) > 1))
    last = a + sum(w * h for w, h in zip(WIDTHS[:k + 1], depths[:k + 1])) - WIDTHS[k]      # the term's newest slot
    assert (slabs[5:, :, last:last + WIDTHS[k]] != slabs[5:, :, last - WIDTHS[k]:last]).any()


def test_the_row_below_the_field_is_the_inner_twins_row():
    tw, slabs, _ = run([3] * 6)
    acts, ep0 = RT.recipe(N)
    plain = OT.run_obs_twin(OT.make_twin(OC._cfg(), N, table_of(group_with())[0]), acts, ep0)
    assert plain.shape[2] == tw.row_floats
    np.testing.assert_array_equal(slabs[:, :, :tw.row_floats].view(U32), plain.view(U32))


def test_a_group_depth_overrides_the_term_depths():
    OM = _om()[0]
    table = table_of(group_with(depths=[5, 0, 1, 7, 2, 3], group_depth=2))
    assert list(table.depths.values()) == [2] * 6 and table.history_floats == 90
    assert table[1]["joint_pos"] == (24,) and table[0] == table_of(group_with())[0]
    np.testing.assert_array_equal(np.asarray(table.history, U32), HT.history_map(WIDTHS, [2] * 6))
    # a group value of 0 or 1 is an override, too: the current frame only
    for g in (0, 1):
        assert list(table_of(group_with(depths=[5] * 6, group_depth=g)).depths.values()) == [1] * 6
    # None leaves the terms their own
    mixed = table_of(group_with(depths=[3, 1, 5, 2, 0, 4]))
    assert list(mixed.depths.values()) == [3, 1, 5, 2, 1, 4] and not table_of(group_with()).has_history and mixed.has_history
    assert OM.term_depth({"history_length": None}, "t", group_with()["joint_pos"]) == 1


def test_all_depths_one_the_field_is_the_policy_observation_bit_for_bit():
    tw, slabs, _ = run([1] * 6)
    a, T_ = tw.off["policy_obs_hist"]
    p, P = tw.off["policy_obs"]
    assert T_ == P == 45
    np.testing.assert_array_equal(slabs[:, :, a:a + T_].view(U32), slabs[:, :, p:p + P].view(U32))


def test_a_stored_frame_keeps_its_noise_when_the_switch_goes_off():
    at = 20
    built = table_of(group_with())[0]
    tw, slabs, first = run([3] * 6, switch=(at, OT.with_corruption(built, False)))
    on = run([3] * 6)[1]
    a, T_ = tw.off["policy_obs_hist"]
    p, P = tw.off["policy_obs"]
    np.testing.assert_array_equal(slabs[:at + 1].view(U32), on[:at + 1].view(U32))
    assert (slabs[at + 1, :, p:p + P] != on[at + 1, :, p:p + P]).any()      # the new frame is clean
    # ... and the two older slots of the row written by step `at` are the noisy frames of the two steps before, for every env
    # whose episode began before them
    keep = ~first[at + 1] & ~first[at]
    assert keep.sum() >= 5
    want = naive_history(slabs[:, :, p:p + P], first, WIDTHS, [3] * 6)
    np.testing.assert_array_equal(slabs[:, :, a:a + T_].view(U32), want.view(U32))
    base = slabs[at + 1, keep, a:a + 9].reshape(-1, 3, 3)                    # base_ang_vel: slots of 3 floats
    np.testing.assert_array_equal(base[:, 0].view(U32), on[at - 1, keep, p:p + 3].view(U32))
    np.testing.assert_array_equal(base[:, 1].view(U32), on[at, keep, p:p + 3].view(U32))


def test_clamps_keep_a_wild_map_inside_the_row():
    words = HT.history_map(WIDTHS, [3] * 6)
    words[7] = 0xFF | 0xFF << 8                                              # cur 255, the next slot 255 floats on
    words[100] = 0xFF | 0xFF << 8 | HT.NEWEST
    acts, ep0 = RT.recipe(N)
    tw = HT.ServoHistoryTwin(OT.make_twin(OC._cfg(), N, table_of(group_with())[0]), words)
    slabs = HT.run_history_twin(tw, acts[:10], ep0)
    a, T_ = tw.off["policy_obs_hist"]
    p, P = tw.off["policy_obs"]
    np.testing.assert_array_equal(slabs[1:, :, a + 100].view(U32), slabs[1:, :, p + P - 1].view(U32))
    keep = slabs[2, :, tw.off["servo"][0] + 13] == slabs[1, :, tw.off["servo"][0] + 13]
    np.testing.assert_array_equal(slabs[2, keep, a + 7].view(U32), slabs[1, keep, a + T_ - 1].view(U32))
