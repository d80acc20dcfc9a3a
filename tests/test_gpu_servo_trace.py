"""Step responses on the device: the command schedule and the step trace of csrc/servo_sim.hip against the trace twin
(tests/servo_trace_twin.py) bit for bit, the descriptor checks, the evaluator with a schedule and a trace on a CaTEnv, and
play.py's flags.  DESIGN section 9, "Step responses"."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import servo_eval_twin as E
import servo_trace_twin as R
import servo_twin as T
import test_gpu_servo_eval as G
import test_gpu_servo_sim as S
import test_servo_eval_twin as C
import test_servo_trace_twin as W

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
U32 = np.uint32
K = G.K
L = W.SEGMENT_STEPS
CANARY, GUARD = 1234.5, 8


@functools.lru_cache(maxsize=None)
def reference(n, segments=3):
    """the twin's run of C.inputs(n) under W.schedule(n) with every env traced for all 50 steps, computed once per n and
    left unchanged; a trace of K < n envs and T < 50 steps is its corner [:T, :K] (test_servo_trace_twin, CPU)"""
    acts, ep0 = C.inputs(n)
    sched = W.schedule(n, segments)
    tw = W.trace_twin(n, sched, L, k=n, capacity=C.STEPS)
    slabs, rec, trace = R.run_trace_twin(tw, acts, ep0)
    for a in (acts, sched, slabs, rec, trace):
        a.setflags(write=False)
    return tw, acts, ep0, sched, slabs, rec, trace


def _device_sim(n, sched=None, segment_steps=None, k=0, capacity=0, offset=0, record=True):
    """(sim, record, trace, whole buffer): the trace is the first ``capacity`` rows of a buffer whose last GUARD rows hold
    a canary pattern that no step may touch"""
    sim = S._device_sim(n, offset=offset)
    rec = torch.full((n, 12), 7.0, device="cuda") if record else None
    sim.set_eval_record(rec)
    if sched is not None:
        sim.set_fixed_command(torch.from_numpy(np.array(sched, np.float32)).cuda(), segment_steps)   # a copy: the reference is read-only
    trace = buf = None
    if k:
        buf = torch.zeros(capacity + GUARD, k, 72, device="cuda")
        buf[capacity:] = CANARY
        trace = buf[:capacity]
        sim.set_trace(trace)
    return sim, rec, trace, buf


def _run(n, sched=None, segment_steps=None, k=0, capacity=0, offset=0, acts=None, ep0=None):
    if acts is None:
        acts, ep0 = C.inputs(n)
    sim, rec, trace, buf = _device_sim(n, sched, segment_steps, k, capacity, offset)
    slabs = S._run_device(sim, np.array(acts, np.float32), ep0)
    return slabs, rec.cpu().numpy(), (None if trace is None else buf.cpu().numpy())


def _same_bits(dev, ref, what):
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    diff = np.ascontiguousarray(dev).view(U32) != np.ascontiguousarray(ref).view(U32)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {at}: device {dev[at]!r} twin {ref[at]!r}")


# ------------------------------------------------------------------------------------------ the kernel against the twin
@pytest.mark.parametrize("capacity", [50, 20])
@pytest.mark.parametrize("n,k", [(1, 1), (17, 1), (17, 16), (17, 17), (64, 16), (64, 17), (64, 64), (1000, 17), (1000, 1000)])
def test_slabs_record_and_trace_equal_the_twin_bit_for_bit(n, k, capacity):
    """50 steps under a schedule of three segments of two steps (MAX_LEN 7: t // 2 reaches 3 and is clamped).  k = 16
    against 17 is the workgroup edge; n = 1 and 17 leave spare lane groups in the last workgroup; capacity 20 drops the
    last 30 steps, and the eight canary rows behind the buffer survive"""
    tw, acts, ep0, sched, ref_slabs, ref_rec, ref_trace = reference(n)
    C.assert_falls_and_timeouts(tw, ref_slabs, ep0)
    W.assert_traced_envs_fall_and_time_out(tw, ref_slabs, ep0, k)
    slabs, rec, buf = _run(n, sched, L, k, capacity)
    _same_bits(slabs, ref_slabs, "slabs")
    _same_bits(rec, ref_rec, "record")
    assert (rec[:, K["steps"]] == C.STEPS).all()
    assert buf.shape == (capacity + GUARD, k, 72)
    _same_bits(buf[:capacity], ref_trace[:capacity, :k], "trace")
    assert (buf[capacity:] == np.float32(CANARY)).all(), "a step wrote behind the trace's capacity"
    t = R.episode_lengths(tw, ref_slabs, ep0)
    _same_bits(buf[:capacity, :, 4:7], W.expected_commands(sched, L, t)[:capacity, :k], "command columns")


def test_the_trace_has_no_side_effect_and_one_segment_is_the_fixed_table():
    n = 64
    tw, acts, ep0, sched, ref_slabs, ref_rec, ref_trace = reference(n)
    plain, rec_plain, _ = _run(n, sched, L)
    traced, rec_traced, _ = _run(n, sched, L, k=n, capacity=C.STEPS)
    np.testing.assert_array_equal(traced.view(U32), plain.view(U32))
    np.testing.assert_array_equal(rec_traced.view(U32), rec_plain.view(U32))
    _same_bits(plain, ref_slabs, "slabs without a trace")
    tab = C.fixed_table(n)
    fixed, rec_fixed = G._run(n, tab)
    one, rec_one, buf = _run(n, tab[None], 4, k=5, capacity=C.STEPS)
    np.testing.assert_array_equal(one.view(U32), fixed.view(U32))
    np.testing.assert_array_equal(rec_one.view(U32), rec_fixed.view(U32))
    _same_bits(buf[:C.STEPS, :, 4:7], np.broadcast_to(tab[:5], (C.STEPS, 5, 3)).copy(), "command columns of a fixed table")
    # init mode writes no row: a reset leaves the (caller-zeroed) trace alone and zeroes the record
    sim, rec, trace, _ = _device_sim(n, sched, L, k=3, capacity=4)
    trace.fill_(5.0)
    sim.reset()
    torch.cuda.synchronize()
    assert (trace.cpu().numpy() == 5.0).all() and (rec.cpu().numpy() == 0).all()


def test_two_shards_trace_the_rows_of_one_simulator():
    n = 64
    tw, acts, ep0, sched, ref_slabs, ref_rec, ref_trace = reference(n)
    whole, rec, buf = _run(n, sched, L, k=n, capacity=C.STEPS)
    lo, rec_lo, buf_lo = _run(32, sched[:, :32], L, k=32, capacity=C.STEPS, offset=0, acts=acts[:, :32], ep0=ep0[:32])
    hi, rec_hi, buf_hi = _run(32, sched[:, 32:], L, k=20, capacity=C.STEPS, offset=32, acts=acts[:, 32:], ep0=ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    np.testing.assert_array_equal(rec[:32].view(U32), rec_lo.view(U32))
    np.testing.assert_array_equal(rec[32:].view(U32), rec_hi.view(U32))
    _same_bits(buf_lo[:C.STEPS], buf[:C.STEPS, :32], "rows traced by shard 0")
    _same_bits(buf_hi[:C.STEPS], buf[:C.STEPS, 32:52], "rows traced by shard 1")
    _same_bits(buf[:C.STEPS], ref_trace, "trace of the whole simulator")


def test_descriptor_checks_the_step_response_fields():
    n = 16
    sched = W.schedule(n)
    sim, rec, trace, buf = _device_sim(n, sched, L, k=4, capacity=6)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    step = sim._nat.servo_sim_step

    def refused(**fields):
        """the descriptor with these fields is refused; afterwards it is what it was"""
        old = {k: getattr(d, k) for k in fields}
        for k, v in fields.items():
            setattr(d, k, v)
        with pytest.raises(RuntimeError, match="bad argument"):
            step(d)
        for k, v in old.items():
            setattr(d, k, v)
    step(d)                                                           # the descriptor as it stands is accepted
    refused(fixed_segment_steps=0)
    refused(fixed_segment_steps=-3)
    refused(fixed_command=None)                                       # a schedule without a table
    refused(fixed_segments=-1)
    refused(eval=None)                                                # a trace without the record
    refused(trace=trace.data_ptr() + 4)                               # misaligned
    refused(trace_envs=0)
    refused(trace_envs=n + 1)
    refused(trace_capacity=0)
    refused(trace_capacity=-1)
    for other in ("state_in", "state_out", "eval", "fixed_command"):
        refused(trace=getattr(d, other))
    step(d)                                                           # and afterwards
    # a zero tail with garbage in the trace's sizes is today's descriptor
    sim.set_trace(None)
    d.trace_envs, d.trace_capacity = -5, -5
    step(d)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy()[6:] == np.float32(CANARY)).all()
    # the wrapper's own checks
    for bad in (torch.zeros(6, 4, 71, device="cuda"), torch.zeros(6, n + 1, 72, device="cuda"), torch.zeros(0, 4, 72, device="cuda"),
                torch.zeros(6, 4, 72, device="cuda", dtype=torch.float64), torch.zeros(6, 4, 72), torch.zeros(6, 8, 72, device="cuda")[:, :4]):
        with pytest.raises(ValueError):
            sim.set_trace(bad)
    cmd = torch.zeros(3, n, 3, device="cuda")
    for args in ((cmd,), (cmd, 0), (cmd[0], 2), (torch.zeros(3, n + 1, 3, device="cuda"), 2), (cmd.double(), 2)):
        with pytest.raises(ValueError):
            sim.set_fixed_command(*args)
    sim.set_fixed_command(None)
    sim.set_eval_record(None)
    sim.state_dict()
    sim.set_eval_record(rec)
    sim.set_trace(trace)
    with pytest.raises(RuntimeError, match="run state"):
        sim.state_dict()
    sim.set_eval_record(None)
    with pytest.raises(RuntimeError, match="run state"):               # the trace alone still refuses
        sim.state_dict()


# ------------------------------------------------------------------------------------------ the evaluator
def test_evaluator_with_a_schedule_and_a_trace():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import command_sequence, evaluate_policy
    n, steps, k, seg = 64, 40, 8, 2
    cfg = G._eval_env_cfg(n)
    env = make(T.TASK, cfg=cfg)
    u = env.unwrapped
    assert u.max_episode_length == 7
    acts = (np.random.RandomState(1).standard_normal((steps, n, 12)) * 2).astype(np.float32)
    acts_d, calls = torch.from_numpy(acts).cuda(), [0]
    points = np.array([[0, 0, 0], [0.6, 0, 0], [0.6, 0, 0.5], [0, -0.3, 0]], np.float32)
    sched = command_sequence(points, n)

    def replay(obs):
        calls[0] += 1
        return acts_d[calls[0] - 1]
    res = evaluate_policy(env, replay, steps, commands=sched, segment_steps=seg, trace_envs=k)
    d = u.sim._desc
    assert calls[0] == steps and d.eval is None and d.fixed_command is None and d.trace is None
    assert (d.fixed_segments, d.fixed_segment_steps, d.trace_envs, d.trace_capacity) == (0, 0, 0, 0)
    u.sim.state_dict()                                                 # detached: the env can be saved again
    assert res.trace.shape == (steps, k, 72) and res.segment_steps == seg and res.commands.shape == (4, n, 3)
    assert tuple(res.trace_fields) == R.TRACE_FIELDS
    tr, rec = res.trace, res.per_env
    # ---- what the trace says about itself
    ends = tr[:, :, 1] > 0.5
    t = np.zeros((steps, k), np.int64)
    for s in range(1, steps):
        t[s] = np.where(ends[s - 1], 0, t[s - 1] + 1)
    np.testing.assert_array_equal(tr[:, :, 0], t)                      # t restarts after every ends
    np.testing.assert_array_equal(ends, (t + 1 >= 7) | (tr[:, :, 2] > 0.5))
    np.testing.assert_array_equal(tr[:, :, 4:7], points[np.minimum(t // seg, 3)])
    assert (t // seg).max() == 3 and ends.sum() >= k * 5
    np.testing.assert_array_equal(rec[:k, K["steps"]], np.full(k, steps))
    np.testing.assert_array_equal(rec[:k, K["episodes"]], ends.sum(0))
    np.testing.assert_array_equal(rec[:k, K["falls"]], (tr[:, :, 2] > 0.5).sum(0))
    np.testing.assert_array_equal(rec[:k, K["feet"]], tr[:, :, 13].sum(0))
    total = np.zeros(k, np.float32)
    for s in range(steps):
        total = total + tr[s, :, 3]
    _same_bits(total, rec[:k, K["reward"]], "sum of the traced rewards in step order")
    np.testing.assert_array_equal(tr[:, :, 60:72], acts[:, :k])
    # ---- against the twin, which plays the same action table
    syn = cfg.synthetic
    tw = R.ServoTraceTwin(n, int(syn.obs_dim), T.params_from_cfg(syn), int(cfg.seed) + int(syn.seed_offset), 7, cfg.sim.dt,
                          cfg.decimation, 0, schedule=sched, segment_steps=seg, trace_envs=k, trace_capacity=steps)
    ref_slabs, ref_rec, ref_trace = R.run_trace_twin(tw, acts, np.zeros(n, np.int64))
    W.assert_traced_envs_fall_and_time_out(tw, ref_slabs, np.zeros(n, np.int64), k)
    _same_bits(rec, ref_rec, "record")
    _same_bits(tr, ref_trace, "trace")
    _same_bits(u.sim.cur.cpu().numpy(), ref_slabs[-1], "last state")
    # ---- the step responses are those of the trace, and the JSON carries them
    from cat_envs.tasks.utils.cleanrl.evaluate import step_response
    assert res.step_response() == step_response(ref_trace, seg)
    doc = json.loads(res.to_json())
    assert doc["segment_steps"] == seg and len(doc["step_response"]["responses"]) == len(res.step_response()) > 0
    assert set(doc["step_response"]["summary"]) == {"incomplete", "vx", "vy", "wz"}
    # ---- the default call is what it was
    again = evaluate_policy(env, lambda obs: acts_d[0], 5)
    assert again.trace is None and again.segment_steps is None and again.commands is None
    with pytest.raises(ValueError):
        evaluate_policy(env, replay, steps, commands=sched)            # a schedule without its segment length


# ------------------------------------------------------------------------------------------ play.py
def test_play_prints_step_responses_and_writes_the_trace(tmp_path):
    from cat_envs.shim import load_cfg_from_registry, make
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    agent_cfg = load_cfg_from_registry(T.TASK, "clean_rl_cfg_entry_point")
    cfg = S._env_cfg()
    cfg.scene.num_envs = 64
    run = tmp_path / "logs" / "clean_rl" / agent_cfg.experiment_name / "run0"
    os.makedirs(run)
    torch.manual_seed(0)
    torch.save(Agent(make(T.TASK, cfg=cfg), hidden=tuple(agent_cfg.hidden)).state_dict(), run / "model_0.pt")
    cmd = [sys.executable, os.path.join(ROOT, "scripts/clean_rl/play.py"), f"--task={T.TASK}", "--headless", "--num_envs", "64",
           "--video_length", "2", "--eval_steps", "24", "--eval_schedule", "0", "0", "0", "0.6", "0", "0", "0.6", "0", "0.5",
           "--eval_segment_steps", "8", "--trace_envs", "4"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[EVAL] ")]
    assert len(lines) == 1
    d = json.loads(lines[0][len("[EVAL] "):])
    assert d["metrics"]["steps"] == 64 * 24 and d["segment_steps"] == 8
    sr = d["step_response"]
    assert set(sr["summary"]) == {"incomplete", "vx", "vy", "wz"} and isinstance(sr["responses"], list)
    assert {r_["axis"] for r_ in sr["responses"]} <= {"vx", "wz"} and sr["summary"]["vy"]["responses"] == 0
    with np.load(run / "eval" / "model_0_trace.npz") as z:
        assert set(z.files) == {"trace", "fields", "commands", "segment_steps"}
        assert z["trace"].shape == (24, 4, 72) and z["commands"].shape == (3, 64, 3) and int(z["segment_steps"]) == 8
        assert [str(x) for x in z["fields"]] == [name for name, _, _ in R.TRACE_FIELDS]
        np.testing.assert_array_equal(z["trace"][:8, :, 4:7], 0)
        first = z["trace"][:, 0]
        assert (first[8:16, 4] == np.float32(0.6)).all() or (first[:16, 1] > 0.5).any()      # unless the episode ended first
    with open(run / "eval" / "model_0.json") as f:
        assert json.load(f) == d
