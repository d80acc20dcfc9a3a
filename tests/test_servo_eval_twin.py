"""The servo surrogate's evaluation mode on the CPU: the eval twin (tests/servo_eval_twin.py) leaves the state rows alone,
its record is what a plain recount of the slabs gives, fixed commands are the command everywhere, and the evaluator's
numpy side (aggregation, command grid) is right.  No GPU needed.  DESIGN section 9, "Evaluation"."""
import json

import numpy as np
import pytest

import servo_eval_twin as E
import servo_twin as T

MAX_LEN, RESAMPLE, STEPS = 7, 3, 50
F32 = np.float32


def _cfg():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(T.TASK, "env_cfg_entry_point")
    cfg.synthetic.servo_resample_steps = RESAMPLE
    return cfg


def eval_twin(n, fixed=None, offset=0, seed=5, obs_dim=45, max_len=MAX_LEN):
    cfg = _cfg()
    return E.ServoEvalTwin(n, obs_dim, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, offset,
                           fixed_command=fixed)


def inputs(n, steps=STEPS):
    """actions of twice unit variance: falls occur at every n down to 1 (unit variance gives none below n = 1000)"""
    rs = np.random.RandomState(0)
    return (rs.standard_normal((steps, n, 12)) * 2).astype(F32), rs.randint(0, MAX_LEN, n)


def fixed_table(n):
    """commands over the whole range, with rows inside the dead zone (|c| <= 0.1) that a draw would have zeroed"""
    rs = np.random.RandomState(11)
    tab = (T.CMD_LO + rs.random_sample((n, 3)).astype(F32) * T.CMD_RANGE).astype(F32)
    tab[::3] = np.array([0.03, -0.02, 0.04], F32)
    return tab


def assert_falls_and_timeouts(twin, slabs, ep0):
    """the run must contain an episode that ended by a fall and one that ended by the time limit"""
    c = E.recount(twin, slabs, ep0)
    assert c[:, 2].sum() >= 1 and (c[:, 1] - c[:, 2]).sum() >= 1, (c[:, 1].sum(), c[:, 2].sum())


@pytest.fixture(scope="module")
def run17():
    acts, ep0 = inputs(17)
    tw = eval_twin(17)
    slabs, rec = E.run_eval_twin(tw, acts, ep0)
    return tw, acts, ep0, slabs, rec


def test_the_record_leaves_the_rows_alone(run17):
    tw, acts, ep0, slabs, rec = run17
    cfg = _cfg()
    plain = T.ServoTwin(17, 45, T.params_from_cfg(cfg.synthetic), 5, MAX_LEN, cfg.sim.dt, cfg.decimation)
    ref = T.run_twin(plain, acts, ep0)
    np.testing.assert_array_equal(slabs.view(np.uint32), ref.view(np.uint32))
    assert rec.shape == (17, 12) and rec.dtype == F32 and len(E.FIELDS) == 12


def test_the_record_is_a_recount_of_the_slabs(run17):
    tw, acts, ep0, slabs, rec = run17
    assert_falls_and_timeouts(tw, slabs, ep0)
    c = E.recount(tw, slabs, ep0)
    k = {name: i for i, name in enumerate(E.FIELDS)}
    assert (rec[:, k["steps"]] == STEPS).all()
    np.testing.assert_array_equal(rec[:, k["episodes"]], slabs[-1, :, tw.off["servo"][0] + 13])
    np.testing.assert_array_equal(rec[:, k["episodes"]], c[:, 1])
    hard = slabs[1:, :, tw.off["hard_reset"][0]] > 0.5
    np.testing.assert_array_equal(rec[:, k["falls"]], hard.sum(0))
    np.testing.assert_array_equal(rec[:, k["falls"]], c[:, 2])
    np.testing.assert_array_equal(rec[:, k["done_return"]], c[:, 3].astype(F32))
    np.testing.assert_array_equal(rec[:, k["done_length"]], c[:, 4])
    # the raw reward sum in step order, and the return of the episode that is still running
    rew = slabs[1:, :, tw.off["reward"][0]]
    total = np.zeros(17, F32)
    for t in range(STEPS):
        total = total + rew[t]
    np.testing.assert_array_equal(rec[:, k["reward"]], total)
    assert (rec[:, k["feet"]] <= 4 * STEPS).all() and (rec[:, k["torque2"]] > 0).all()
    # steps = lengths of the ended episodes + length of the running one - what the first episode had before the run
    running = STEPS + ep0 - rec[:, k["done_length"]]
    assert ((running >= 0) & (running < MAX_LEN)).all()


def test_fixed_commands_are_the_command_everywhere():
    n = 17
    acts, ep0 = inputs(n)
    tab = fixed_table(n)
    tw = eval_twin(n, fixed=tab)
    slabs, rec = E.run_eval_twin(tw, acts, ep0)
    assert_falls_and_timeouts(tw, slabs, ep0)
    c0, o0, s0, r0 = (tw.off[k][0] for k in ("command", "obs", "servo", "reward"))
    for t in range(STEPS + 1):                                   # every row, post-reset observations included
        np.testing.assert_array_equal(slabs[t, :, c0:c0 + 3].view(np.uint32), tab.view(np.uint32))
        np.testing.assert_array_equal(slabs[t, :, o0 + 6:o0 + 9].view(np.uint32), tab.view(np.uint32))
    assert (np.abs(tab[0]) > 0).all() and float((tab[0] ** 2).sum()) < 0.01      # inside the dead zone, and kept
    s = T.params_from_cfg(_cfg().synthetic)["reward_scale"]
    for t in range(1, STEPS + 1):
        v = slabs[t, :, s0:s0 + 3]
        ex, ey, ew = tab[:, 0] - v[:, 0], tab[:, 1] - v[:, 1], tab[:, 2] - v[:, 2]
        want = F32(1) / (F32(1) + (ex * ex + ey * ey) / s) + F32(0.5) / (F32(1) + (ew * ew) / s)
        np.testing.assert_array_equal(slabs[t, :, r0].view(np.uint32), want.astype(F32).view(np.uint32))
    # the dynamics do not read the command: joints and base are those of the run with drawn commands
    free, _ = E.run_eval_twin(eval_twin(n), acts, ep0)
    np.testing.assert_array_equal(slabs[:, :, :48], free[:, :, :48])
    assert (slabs[:, :, r0] != free[:, :, r0]).any()


def test_aggregate_on_a_hand_made_table():
    from cat_envs.tasks.utils.cleanrl.evaluate import FIELDS, aggregate
    assert tuple(FIELDS) == E.FIELDS
    rec = np.zeros((2, 12), F32)
    #          steps ep falls reward lin2 yaw2 tilt2 tq2 feet ep_ret done_ret done_len
    rec[0] = [10, 2, 1, 5.0, 2.5, 0.9, 0.1, 40.0, 30, 0.5, 4.5, 9]
    rec[1] = [10, 2, 0, 7.0, 1.5, 0.1, 0.3, 20.0, 38, 0.0, 7.0, 10]
    m = aggregate(rec, cat_reward=[4.0, 6.0], termination_prob=[1.0, 0.0], violations=[[3, 0, 3], [1, 2, 2]],
                  term_names=("a", "b"))
    assert m["steps"] == 20 and m["episodes"] == 4 and m["fall_rate"] == 0.25
    assert m["reward_per_step"] == 0.6 and m["cat_reward_per_step"] == 0.5
    assert m["rms_err_lin"] == pytest.approx(np.sqrt(0.2), rel=1e-12) and m["rms_err_yaw"] == pytest.approx(np.sqrt(0.05), rel=1e-7)
    assert m["mean_tilt2"] == pytest.approx(0.02, rel=1e-6) and m["mean_torque2"] == 3.0 and m["mean_feet"] == 3.4
    assert m["episode_return_mean"] == 11.5 / 4 and m["episode_length_mean"] == 19 / 4
    assert m["termination_prob_mean"] == 0.05
    assert m["violation_share/a"] == 0.2 and m["violation_share/b"] == 0.1 and m["violation_share/any"] == 0.25
    # no episode ended: the per-episode ratios are None, everything else stands
    rec[:, [1, 2, 10, 11]] = 0
    m = aggregate(rec)
    assert m["episodes"] == 0 and m["fall_rate"] is None
    assert m["episode_return_mean"] is None and m["episode_length_mean"] is None
    assert m["reward_per_step"] == 0.6 and m["cat_reward_per_step"] is None and "violation_share/any" not in m
    json.dumps(m)


def test_eval_result_groups_by_command():
    from cat_envs.tasks.utils.cleanrl.evaluate import EvalResult, aggregate
    rec = np.zeros((5, 12), F32)
    rec[:, 0], rec[:, 3] = 4, [1, 2, 3, 4, 5]
    cmds = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], F32)
    res = EvalResult(per_env=rec, commands=cmds, cat_reward=np.ones(5, F32), termination_prob=np.zeros(5, F32),
                     violations=np.zeros((5, 1), F32))
    res.metrics = res._aggregate()
    groups = res.by_command()
    assert [g["command"] for g in groups] == [[1, 0, 0], [0, 1, 0]] and [g["envs"] for g in groups] == [3, 2]
    assert groups[0]["metrics"]["reward_per_step"] == 9 / 12 and groups[1]["metrics"]["reward_per_step"] == 6 / 8
    assert res.metrics == aggregate(rec, np.ones(5), np.zeros(5), np.zeros((5, 1)))
    d = json.loads(res.to_json())
    assert d["metrics"]["steps"] == 20 and len(d["by_command"]) == 2 and d["num_envs"] == 5


def test_command_grid_with_a_ragged_env_count():
    from cat_envs.tasks.utils.cleanrl.evaluate import command_grid
    cmds, idx = command_grid(vx=(-0.3, 1.0, 3), vy=(-0.7, 0.7, 2), wz=(-0.78, 0.78, 1), num_envs=8)
    assert cmds.shape == (8, 3) and cmds.dtype == F32 and idx.tolist() == [0, 1, 2, 3, 4, 5, 0, 1]
    pts = [[-0.3, -0.7, 0], [-0.3, 0.7, 0], [0.35, -0.7, 0], [0.35, 0.7, 0], [1.0, -0.7, 0], [1.0, 0.7, 0]]
    np.testing.assert_array_equal(cmds[:6], np.array(pts, F32))
    np.testing.assert_array_equal(cmds[6:], cmds[:2])
    one, idx = command_grid(num_envs=3)
    assert idx.tolist() == [0, 0, 0] and np.allclose(one, [[0.35, 0.0, 0.0]] * 3)
    with pytest.raises(ValueError):
        command_grid(vx=(0, 1, 0), num_envs=2)


def test_the_native_descriptor_carries_the_two_fields_last():
    from cat_envs import native
    names = [f[0] for f in native.ServoSim._fields_]
    assert names[-2:] == ["fixed_command", "eval"] and names[-3] == "command_deadzone"
    assert native.ServoSim.eval.offset % 8 == 0 and len(native.SERVO_EVAL_FIELDS) == 12
