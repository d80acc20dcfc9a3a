"""Step responses on the CPU: the trace twin (tests/servo_trace_twin.py) follows a command schedule keyed on the episode
length, its trace rows are the named fields of the slab rows, neither changes slabs or record, and the evaluator's numpy
side (``step_response``, ``command_sequence``, argument checks) is right.  No GPU needed.  DESIGN section 9, "Step responses"."""
import json

import numpy as np
import pytest

import servo_eval_twin as E
import servo_trace_twin as R
import servo_twin as T
import test_servo_eval_twin as C

F32, U32 = np.float32, np.uint32
MAX_LEN, STEPS = C.MAX_LEN, C.STEPS
SEGMENT_STEPS = 2                                    # t // 2 reaches 3 at MAX_LEN 7 and is clamped to row 2


def schedule(n, segments=3):
    """``segments`` different tables over the whole command range, rows inside the dead zone included"""
    rs = np.random.RandomState(23)
    tab = (T.CMD_LO + rs.random_sample((segments, n, 3)).astype(F32) * T.CMD_RANGE).astype(F32)
    tab[1, ::3] = np.array([0.03, -0.02, 0.04], F32)
    return tab


def trace_twin(n, sched=None, segment_steps=None, k=0, capacity=0, fixed=None, offset=0, seed=5, obs_dim=45):
    cfg = C._cfg()
    return R.ServoTraceTwin(n, obs_dim, T.params_from_cfg(cfg.synthetic), seed, MAX_LEN, cfg.sim.dt, cfg.decimation, offset,
                            fixed_command=fixed, schedule=sched, segment_steps=segment_steps, trace_envs=k,
                            trace_capacity=capacity)


def expected_commands(sched, segment_steps, t):
    """[steps, N, 3]: row min(t // L, S - 1) of every env for the episode lengths ``t`` [steps, N]"""
    seg = np.minimum(t // segment_steps, len(sched) - 1)
    return sched[seg, np.arange(sched.shape[1])[None, :]]


def assert_traced_envs_fall_and_time_out(twin, slabs, ep0, k):
    """a fall and a time-out inside the traced envs 0 .. k - 1, not only somewhere in N"""
    c = E.recount(twin, slabs, ep0)[:k]
    assert c[:, 2].sum() >= 1 and (c[:, 1] - c[:, 2]).sum() >= 1, (k, c[:, 1].sum(), c[:, 2].sum())


@pytest.fixture(scope="module")
def run17():
    n = 17
    acts, ep0 = C.inputs(n)
    sched = schedule(n)
    tw = trace_twin(n, sched, SEGMENT_STEPS, k=n, capacity=STEPS)
    slabs, rec, trace = R.run_trace_twin(tw, acts, ep0)
    return tw, acts, ep0, sched, slabs, rec, trace


def test_a_schedule_of_one_segment_is_the_fixed_table():
    n = 17
    acts, ep0 = C.inputs(n)
    tab = C.fixed_table(n)
    ref_slabs, ref_rec = E.run_eval_twin(C.eval_twin(n, fixed=tab), acts, ep0)
    slabs, rec, _ = R.run_trace_twin(trace_twin(n, tab[None], 4), acts, ep0)
    np.testing.assert_array_equal(slabs.view(U32), ref_slabs.view(U32))
    np.testing.assert_array_equal(rec.view(U32), ref_rec.view(U32))
    # and the trace twin without a schedule is the eval twin
    slabs, rec, trace = R.run_trace_twin(trace_twin(n, fixed=tab), acts, ep0)
    np.testing.assert_array_equal(slabs.view(U32), ref_slabs.view(U32))
    assert trace is None


def test_the_schedule_follows_the_episode_length_and_restarts(run17):
    tw, acts, ep0, sched, slabs, rec, trace = run17
    C.assert_falls_and_timeouts(tw, slabs, ep0)
    t = R.episode_lengths(tw, slabs, ep0)
    assert t.max() == MAX_LEN - 1 and (t // SEGMENT_STEPS).max() == 3 and len(sched) == 3       # the clamp is exercised
    c0, o0 = tw.off["command"][0], tw.off["obs"][0]
    want = expected_commands(sched, SEGMENT_STEPS, t)
    np.testing.assert_array_equal(slabs[1:, :, c0:c0 + 3].view(U32), want.view(U32))
    first = expected_commands(sched, SEGMENT_STEPS, np.asarray(ep0, np.int64)[None])[0]
    np.testing.assert_array_equal(slabs[0, :, c0:c0 + 3].view(U32), first.view(U32))              # the init row
    np.testing.assert_array_equal(slabs[0, :, o0 + 6:o0 + 9].view(U32), first.view(U32))
    # the observation of a step that ends an episode shows segment 0; every other one the step's own command
    ends = np.zeros_like(t, bool)
    ends[:-1] = t[1:] == 0
    ends[-1] = (t[-1] + 1 >= MAX_LEN) | (slabs[-1, :, tw.off["hard_reset"][0]] > 0.5)
    assert ends.sum() >= 17 * 6
    obs_cmd = slabs[1:, :, o0 + 6:o0 + 9]
    seg0 = np.broadcast_to(sched[0], obs_cmd.shape)
    np.testing.assert_array_equal(obs_cmd[ends].view(U32), seg0[ends].view(U32))
    np.testing.assert_array_equal(obs_cmd[~ends].view(U32), want[~ends].view(U32))
    assert (want[ends] != seg0[ends]).any()
    # after a reset the schedule starts again: the first step of every episode uses segment 0
    np.testing.assert_array_equal(want[t == 0].view(U32), np.broadcast_to(sched[0], want.shape)[t == 0].view(U32))
    # rows inside the dead zone are kept as they stand
    assert (np.abs(sched[1, 0]) > 0).all() and float((sched[1, 0] ** 2).sum()) < 0.01


def test_the_trace_changes_neither_slabs_nor_record(run17):
    tw, acts, ep0, sched, slabs, rec, trace = run17
    plain_slabs, plain_rec, none = R.run_trace_twin(trace_twin(17, sched, SEGMENT_STEPS), acts, ep0)
    assert none is None
    np.testing.assert_array_equal(slabs.view(U32), plain_slabs.view(U32))
    np.testing.assert_array_equal(rec.view(U32), plain_rec.view(U32))


def test_every_trace_field_is_the_named_field_of_the_slab_row(run17):
    from cat_envs import native
    tw, acts, ep0, sched, slabs, rec, trace = run17
    assert native.SERVO_TRACE_FIELDS == R.TRACE_FIELDS and native.SERVO_TRACE_FLOATS == R.TRACE_FLOATS == 72
    assert [a for _, a, _ in R.TRACE_FIELDS] == list(np.cumsum([0] + [w for _, _, w in R.TRACE_FIELDS])[:-1])
    assert sum(w for _, _, w in R.TRACE_FIELDS) == 72
    assert_traced_envs_fall_and_time_out(tw, slabs, ep0, 17)
    assert trace.shape == (STEPS, 17, 72) and trace.dtype == F32
    t = R.episode_lengths(tw, slabs, ep0)
    rows, col = slabs[1:], R.COL

    def field(name):
        a, w = tw.off[name]
        return rows[:, :, a:a + w]
    x = field("servo")
    hard = field("hard_reset")[:, :, 0] > 0.5
    pairs = {"t": t.astype(F32)[..., None], "ends": ((t + 1 >= MAX_LEN) | hard).astype(F32)[..., None],
             "fallen": hard.astype(F32)[..., None], "reward": field("reward"), "command": field("command"), "v": x[..., 0:3],
             "roll": x[..., 3:4], "pitch": x[..., 4:5], "z": field("root_pos_w")[..., 2:3],
             "ncon": ((x[..., 9] + x[..., 10]) + (x[..., 11] + x[..., 12]))[..., None], "zero": np.zeros((STEPS, 17, 2), F32),
             "contact": x[..., 9:13],
             "fz": field("forces").reshape(STEPS, 17, T.H, T.B, 3)[:, :, 0, T.FOOT_BODY, 2],
             "q": field("joint_pos"), "qd": field("joint_vel"), "tau_w": field("applied_torque"), "action": acts}
    assert set(pairs) == set(col)
    for name, want in pairs.items():
        np.testing.assert_array_equal(trace[:, :, col[name]].view(U32), np.ascontiguousarray(want, F32).view(U32), err_msg=name)
    assert (trace[:, :, col["fz"]] > 0).any() and (trace[:, :, col["contact"]] == 0).any()
    # the reward column summed in step order is field 3 of the record
    total = np.zeros(17, F32)
    for s in range(STEPS):
        total = total + trace[s, :, 3]
    np.testing.assert_array_equal(total.view(U32), rec[:, 3].view(U32))


def test_rows_past_the_capacity_are_dropped_and_a_prefix_of_envs_is_traced(run17):
    tw, acts, ep0, sched, slabs, rec, full = run17
    small = trace_twin(17, sched, SEGMENT_STEPS, k=5, capacity=20)
    _, rec2, trace = R.run_trace_twin(small, acts, ep0)
    assert trace.shape == (20, 5, 72)
    np.testing.assert_array_equal(trace.view(U32), full[:20, :5].view(U32))
    np.testing.assert_array_equal(rec2.view(U32), rec.view(U32))
    assert (rec2[:, 0] == STEPS).all()                                  # the steps went on being counted


# ---------------------------------------------------------------------------------------------- step_response
def _trace_of(v, cmd, t0=0, ends_at=None):
    """a one-env trace [T, 1, 72] with the given vx series and command series (vy, wz and their commands zero)"""
    from cat_envs import native
    steps = len(v)
    tr = np.zeros((steps, 1, native.SERVO_TRACE_FLOATS), F32)
    tr[:, 0, 0] = np.arange(t0, t0 + steps)
    tr[:, 0, 4], tr[:, 0, 7] = cmd, v
    if ends_at is not None:
        tr[ends_at, 0, 1] = 1
        tr[ends_at + 1:, 0, 0] = np.arange(steps - ends_at - 1)
    return tr


def test_step_response_of_a_first_order_lag():
    from cat_envs.tasks.utils.cleanrl.evaluate import step_response
    L, c_old, c_new = 8, 0.25, 0.75                                      # dyadic: every e_k = -0.5 * 2^-k is exact
    cmd = np.array([c_old] * L + [c_new] * L, F32)
    v = np.zeros(2 * L, F32)
    v[:L] = c_old
    x = c_old
    for k in range(L):
        x = x + 0.5 * (c_new - x)
        v[L + k] = x
    np.testing.assert_array_equal(np.abs(v[L:] - c_new), 0.5 * 2.0 ** -np.arange(1, L + 1))
    got = step_response(_trace_of(v, cmd), L)
    assert len(got) == 1                                                 # vy and wz did not change: no entry
    r = got[0]
    assert (r["env"], r["segment"], r["axis"], r["from"], r["to"], r["complete"]) == (0, 1, "vx", 0.25, 0.75, True)
    assert r["rise_steps"] == 4 and r["settle_steps"] == 4 and r["overshoot"] == 0.0
    assert r["steady_error"] < 0.1 * 0.5 and r["steady_error"] == pytest.approx(0.5 * (2.0 ** -7 + 2.0 ** -8) / 2)
    # a tighter tolerance moves both: 2^-k <= 0.01 first at k = 7
    r = step_response(_trace_of(v, cmd), L, tolerance=0.01)[0]
    assert r["rise_steps"] == r["settle_steps"] == 7
    # a step down mirrors it
    r = step_response(_trace_of(1.0 - v, 1.0 - cmd), L)[0]
    assert (r["from"], r["to"], r["rise_steps"], r["settle_steps"], r["overshoot"]) == (0.75, 0.25, 4, 4, 0.0)


def test_step_response_with_overshoot_a_late_excursion_and_a_cut_segment():
    from cat_envs.tasks.utils.cleanrl.evaluate import step_response, summarise_step_response
    L = 8
    cmd = np.array([0.0] * L + [1.0] * L + [0.5] * L, F32)
    #                      k = 1    2     3     4    5     6     7    8
    seg1 = np.array([0.5, 0.95, 1.25, 1.05, 1.0, 0.85, 1.0, 1.0], F32)          # delta +1: band [0.9, 1.1]
    seg2 = np.array([0.75, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5], F32)             # delta -0.5: band [0.45, 0.55]
    v = np.concatenate([np.zeros(L, F32), seg1, seg2])
    got = step_response(_trace_of(v, cmd), L)
    assert [(r["segment"], r["axis"]) for r in got] == [(1, "vx"), (2, "vx")]
    a, b = got
    assert a["rise_steps"] == 2 and a["settle_steps"] == 7                        # the excursion at k = 6 moves settling only
    assert a["overshoot"] == pytest.approx(0.25) and a["steady_error"] == 0.0
    assert b["rise_steps"] == 2 and b["settle_steps"] == 2 and b["overshoot"] == 0.0 and b["steady_error"] == 0.0
    # never inside the band: no rise, no settling; last step outside: no settling
    far = step_response(_trace_of(np.concatenate([np.zeros(L, F32), np.full(L, 0.5, F32)]), cmd[:2 * L]), L)[0]
    assert far["rise_steps"] is None and far["settle_steps"] is None and far["steady_error"] == 0.5
    late = seg1.copy()
    late[-1] = 0.8
    r = step_response(_trace_of(np.concatenate([np.zeros(L, F32), late]), cmd[:2 * L]), L)[0]
    assert r["rise_steps"] == 2 and r["settle_steps"] is None
    # the episode ends at the fourth step of segment 2: that response is incomplete, and what follows is another episode
    cut = step_response(_trace_of(v, cmd, ends_at=2 * L + 3), L)
    assert [(r["segment"], r["complete"]) for r in cut] == [(1, True), (2, False)]
    assert "rise_steps" not in cut[1] and cut[0] == a
    s = summarise_step_response(cut)
    assert s["incomplete"] == 1 and s["vx"]["responses"] == 1 and s["vx"]["rise_steps"] == 2.0 and s["vx"]["settle_steps"] == 7.0
    assert s["vy"] == {"responses": 0, "rise_steps": None, "settle_steps": None, "overshoot": None, "steady_error": None}
    json.dumps(s)
    with pytest.raises(ValueError):
        step_response(np.zeros((4, 1, 71), F32), L)
    with pytest.raises(ValueError):
        step_response(_trace_of(v, cmd), 0)


def test_eval_result_carries_the_step_response():
    from cat_envs.tasks.utils.cleanrl.evaluate import EvalResult, command_sequence
    L = 4
    cmds = command_sequence([[0, 0, 0], [1, 0, 0.5]], 3)
    tr = np.zeros((2 * L, 2, 72), F32)
    tr[:, :, 0] = np.arange(2 * L)[:, None]
    tr[L:, :, 4], tr[L:, :, 6] = 1.0, 0.5
    tr[L:, :, 7], tr[L:, :, 9] = 1.0, 0.25
    rec = np.zeros((3, 12), F32)
    rec[:, 0] = 2 * L
    res = EvalResult(per_env=rec, commands=cmds, trace=tr, segment_steps=L)
    res.metrics = res._aggregate()
    got = res.step_response()
    assert [(r["env"], r["axis"]) for r in got] == [(0, "vx"), (0, "wz"), (1, "vx"), (1, "wz")]
    assert got[0]["rise_steps"] == 1 and got[1]["rise_steps"] is None and got[1]["steady_error"] == 0.25
    d = json.loads(res.to_json())
    assert d["segment_steps"] == L and d["step_response"]["responses"] == got
    assert d["step_response"]["summary"]["vx"]["responses"] == 2 and d["step_response"]["summary"]["incomplete"] == 0
    assert len(d["by_command"]) == 1 and d["by_command"][0]["envs"] == 3
    assert [name for name, _, _ in res.trace_fields][:4] == ["t", "ends", "fallen", "reward"]
    with pytest.raises(ValueError):
        EvalResult(per_env=rec, commands=cmds).step_response()
    assert "step_response" not in json.loads(EvalResult(per_env=rec, commands=cmds[0], metrics=res.metrics).to_json())


# ---------------------------------------------------------------------------------------------- arguments
def test_command_sequence():
    from cat_envs.tasks.utils.cleanrl.evaluate import command_sequence
    pts = [[0, 0, 0], [0.6, 0, 0], [0.6, 0, 0.5]]
    seq = command_sequence(pts, 5)
    assert seq.shape == (3, 5, 3) and seq.dtype == F32 and seq.flags["C_CONTIGUOUS"]
    for i in range(5):
        np.testing.assert_array_equal(seq[:, i], np.array(pts, F32))
    for bad in ([0, 0, 0], [[0, 0]], np.zeros((0, 3))):
        with pytest.raises(ValueError):
            command_sequence(bad, 4)
    with pytest.raises(ValueError):
        command_sequence(pts, 0)


def test_evaluate_policy_checks_its_arguments_before_any_device_use():
    import types
    from cat_envs.tasks.utils.cleanrl.evaluate import command_sequence, evaluate_policy
    touched = []
    u = types.SimpleNamespace(num_envs=4, device="cpu", set_eval_record=lambda t: touched.append(t))
    env = types.SimpleNamespace(unwrapped=u)
    seq = command_sequence([[0, 0, 0], [1, 0, 0]], 4)
    for kw in (dict(commands=seq), dict(commands=seq, segment_steps=0), dict(commands=seq[0], segment_steps=3),
               dict(segment_steps=3), dict(trace_envs=5), dict(trace_envs=-1)):
        with pytest.raises(ValueError):
            evaluate_policy(env, lambda obs: obs, 8, **kw)
    with pytest.raises(TypeError):
        evaluate_policy(types.SimpleNamespace(unwrapped=types.SimpleNamespace()), lambda obs: obs, 8, trace_envs=1)
    assert touched == []


def test_the_native_descriptor_carries_the_step_response_tail():
    import ctypes
    from cat_envs import native
    assert issubclass(native.ServoSimStep, native.ServoSim)
    assert [f[0] for f in native.ServoSimStep._fields_] == ["fixed_segments", "fixed_segment_steps", "trace", "trace_envs",
                                                            "trace_capacity"]
    assert native.ServoSimStep.fixed_segments.offset == ctypes.sizeof(native.ServoSim)      # the tail starts where it ended
    assert native.ServoSimStep.trace.offset % 8 == 0
    assert ctypes.sizeof(native.ServoSimStep) == ctypes.sizeof(native.ServoSim) + 24
    d = native.ServoSimStep()
    assert (d.fixed_segments, d.fixed_segment_steps, d.trace, d.trace_envs, d.trace_capacity) == (0, 0, None, 0, 0)
