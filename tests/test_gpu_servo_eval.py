"""Evaluation on the servo task, on the device: fixed commands and the per-env evaluation record of csrc/servo_sim.hip
against the eval twin bit for bit, the evaluator (cat_envs/tasks/utils/cleanrl/evaluate.py) against the closed-loop CPU
oracle env, learning as the evaluator sees it, and play.py's evaluation flags.  DESIGN section 9, "Evaluation"."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import servo_eval_twin as E
import servo_twin as T
import test_gpu_servo_sim as S
import test_servo_eval_twin as C

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
MAX_LEN = S.MAX_LEN
U32 = np.uint32
K = {name: i for i, name in enumerate(E.FIELDS)}


def _device_sim(n, fixed=None, record=True, offset=0):
    sim = S._device_sim(n, offset=offset)
    rec = torch.full((n, 12), 7.0, device="cuda") if record else None      # init mode must zero it
    cmd = None if fixed is None else torch.from_numpy(np.ascontiguousarray(fixed)).cuda()
    sim.set_eval_record(rec)
    sim.set_fixed_command(cmd)
    return sim, rec


def _run(n, fixed=None, record=True, offset=0, acts=None, ep0=None):
    if acts is None:
        acts, ep0 = C.inputs(n)
    sim, rec = _device_sim(n, fixed, record, offset)
    slabs = S._run_device(sim, acts, ep0)
    return slabs, (None if rec is None else rec.cpu().numpy())


def _same_bits(dev, ref, what):
    diff = dev.view(U32) != ref.view(U32)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError(f"{what}: {int(diff.sum())} words differ; first at {at}: device {dev[at]!r} twin {ref[at]!r}")


# ------------------------------------------------------------------------------------------ (a) .. (e): the kernel
@pytest.mark.parametrize("fixed", [False, True], ids=["sampled", "fixed"])
@pytest.mark.parametrize("n", [1, 17, 64, 1000])
def test_slabs_and_record_equal_the_twin_bit_for_bit(n, fixed):
    """50 steps; n = 1 and 17 leave spare lane groups in the last workgroup (a double count shows as steps == 100)"""
    acts, ep0 = C.inputs(n)
    tab = C.fixed_table(n) if fixed else None
    tw = C.eval_twin(n, fixed=tab)
    ref_slabs, ref_rec = E.run_eval_twin(tw, acts, ep0)
    C.assert_falls_and_timeouts(tw, ref_slabs, ep0)
    slabs, rec = _run(n, tab)
    assert slabs.shape == ref_slabs.shape and rec.shape == (n, 12)
    assert (rec[:, K["steps"]] == C.STEPS).all(), rec[:, K["steps"]]
    _same_bits(slabs, ref_slabs, "slabs")
    _same_bits(rec, ref_rec, "record")
    assert rec[:, K["falls"]].sum() >= 1 and (rec[:, K["episodes"]] - rec[:, K["falls"]]).sum() >= 1
    if fixed:
        c0 = tw.off["command"][0]
        _same_bits(slabs[:, :, c0:c0 + 3], np.broadcast_to(tab, (C.STEPS + 1, n, 3)).copy(), "command field")


def test_the_record_does_not_change_the_slabs():
    with_rec, rec = _run(64, record=True)
    without, _ = _run(64, record=False)
    np.testing.assert_array_equal(with_rec.view(U32), without.view(U32))
    assert (rec[:, K["steps"]] == C.STEPS).all()


def test_reset_zeroes_the_record():
    acts, ep0 = C.inputs(64, steps=5)
    sim, rec = _device_sim(64)
    S._run_device(sim, acts, ep0)
    assert (rec.cpu().numpy()[:, K["steps"]] == 5).all()
    sim.reset()
    torch.cuda.synchronize()
    assert (rec.cpu().numpy().view(U32) == 0).all()


def test_two_shards_with_their_slices_equal_one_run():
    acts, ep0 = C.inputs(64)
    tab = C.fixed_table(64)
    whole, rec = _run(64, tab)
    lo, rec_lo = _run(32, tab[:32], offset=0, acts=acts[:, :32].copy(), ep0=ep0[:32])
    hi, rec_hi = _run(32, tab[32:], offset=32, acts=acts[:, 32:].copy(), ep0=ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(U32), lo.view(U32))
    np.testing.assert_array_equal(whole[:, 32:].view(U32), hi.view(U32))
    np.testing.assert_array_equal(rec[:32].view(U32), rec_lo.view(U32))
    np.testing.assert_array_equal(rec[32:].view(U32), rec_hi.view(U32))


def test_descriptor_checks_the_two_fields():
    sim, rec = _device_sim(16)
    d = sim._desc
    d.state_out, d.action = sim._slabs[0].data_ptr(), sim.default_joint_pos.data_ptr()
    sim._nat.servo_sim_step(d)                                       # the descriptor as it stands is accepted
    d.eval = rec.data_ptr() + 4                                       # misaligned
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.eval = d.state_out                                              # the record would overwrite the row
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.eval, d.fixed_command = rec.data_ptr(), d.state_in
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.fixed_command = None
    sim._nat.servo_sim_step(d)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        sim.set_eval_record(torch.zeros(16, 11, device="cuda"))
    with pytest.raises(ValueError):
        sim.set_fixed_command(torch.zeros(16, 3, device="cuda", dtype=torch.float64))


# ------------------------------------------------------------------------------------------ (f): the fused rollout
def test_fused_rollout_carries_the_record():
    """the fused env step launches the simulator through the same ``advance``: 24 steps counted once per env, and the raw
    reward sum is at least the CaT-scaled one (reward * (1 - p), both accumulated in fp32 in step order: rounding is
    monotone, so the order of the sums is the order of the terms)"""
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    env_cfg, agent_cfg = S._cfgs(64, 24, 512, 1, 1, (512, 256, 128), 42)
    env = make(T.TASK, cfg=env_cfg)
    torch.manual_seed(42)
    trainer = PPOTrainer(env, agent_cfg)
    assert trainer.sink is not None and trainer.T == 24
    rec = torch.zeros(64, 12, device="cuda")
    env.unwrapped.set_eval_record(rec)
    trainer.rollout()
    env.unwrapped.set_eval_record(None)
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    assert (r[:, K["steps"]] == 24).all(), r[:, K["steps"]]
    scaled = trainer.rewards.float().cpu().numpy()
    total = np.zeros(64, np.float32)
    for t in range(24):
        total = total + scaled[t]
    assert (r[:, K["reward"]] >= total).all() and (r[:, K["reward"]] > total).any()
    # the open-loop stream simulator has neither
    from cat_envs.shim import load_cfg_from_registry
    stream_cfg = load_cfg_from_registry("Isaac-Velocity-CaT-Flat-Solo12-v0", "env_cfg_entry_point")
    stream_cfg.scene.num_envs = 64
    stream_env = make("Isaac-Velocity-CaT-Flat-Solo12-v0", cfg=stream_cfg).unwrapped
    with pytest.raises(TypeError):
        stream_env.set_eval_record(rec)
    with pytest.raises(TypeError):
        stream_env.set_fixed_commands(torch.zeros(64, 3, device="cuda"))


# ------------------------------------------------------------------------------------------ (g), (h): the evaluator
def _eval_env_cfg(num_envs, seed=42):
    cfg = S._env_cfg()
    cfg.scene.num_envs, cfg.seed = num_envs, seed
    cfg.episode_length_s = 6.5 * cfg.sim.dt * cfg.decimation           # ceil -> 7 control steps
    return cfg


def test_evaluator_against_the_twin_and_the_cpu_oracle_env():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import aggregate, evaluate_policy
    n, steps = 64, 40
    cfg = _eval_env_cfg(n)
    env = make(T.TASK, cfg=cfg)
    u = env.unwrapped
    assert u.max_episode_length == 7 and len(u.constraint_manager.active_terms) == 13
    acts = (np.random.RandomState(1).standard_normal((steps, n, 12)) * 2).astype(np.float32)
    tab = C.fixed_table(n)
    acts_d, calls = torch.from_numpy(acts).cuda(), [0]
    # ---- the CPU side: the oracle env of the same cfg, its twin replaced by the eval twin with the same command table
    # (built BEFORE the device env steps: the device curriculum anneals max_p in the term cfgs both sides start from)
    cm = u.constraint_manager
    orc = T.env_oracle_from_cfg(cfg, n, np.zeros(n, np.int64), tau=cm.cat.tau, min_p=cm.cat.min_p)

    def replay(obs):
        assert obs.shape == (n, u.obs_dim)
        calls[0] += 1
        return acts_d[calls[0] - 1]
    res = evaluate_policy(env, replay, steps, commands=tab)
    assert calls[0] == steps and u.sim._desc.eval is None and u.sim._desc.fixed_command is None
    tw = E.eval_twin_from_cfg(cfg, n, tab)
    assert tw.max_len == 7 and tw.off == orc.twin.off
    orc.twin = tw
    orc.stream[0] = tw.initial(np.zeros(n, np.int64))
    seen = []
    compute = orc.mgr.compute
    orc.mgr.compute = lambda vals, max_p: (seen.append({k: np.asarray(v, np.float32).reshape(n, -1) for k, v in vals.items()}),
                                           compute(vals, max_p))[1]
    names = [t["name"] for t in orc.terms]
    assert tuple(names) == tuple(res.term_names)
    cat_reward, viol = np.zeros(n, np.float32), np.zeros((n, len(names) + 1), np.float32)
    for t in range(steps):
        _, reward, _, _, _ = orc.step(torch.from_numpy(acts[t]))
        cat_reward = cat_reward + reward.numpy().astype(np.float32)
        hit = np.stack([(seen[-1][k] > 0).any(1) for k in names], 1)
        viol[:, :-1] += hit
        viol[:, -1] += hit.any(1)
    assert tw.record[:, K["falls"]].sum() >= 1 and (tw.record[:, K["episodes"]] - tw.record[:, K["falls"]]).sum() >= 1
    _same_bits(res.per_env, tw.record, "record")
    np.testing.assert_array_equal(res.violations, viol)
    assert viol[:, -1].max() > 0 and (viol[:, :-1].sum(0) > 0).sum() >= 2      # the comparison is about something
    _same_bits(res.cat_reward, cat_reward, "CaT-scaled reward sums")
    np.testing.assert_array_equal(u.sim.cur.cpu().numpy().view(U32), orc.stream[0].view(U32))
    want = aggregate(res.per_env, res.cat_reward, res.termination_prob, res.violations, res.term_names)
    assert res.metrics == want and res.metrics["steps"] == n * steps
    assert res.metrics["cat_reward_per_step"] < res.metrics["reward_per_step"]
    groups = res.by_command()
    assert sum(g["envs"] for g in groups) == n and len(groups) == len(np.unique(tab, axis=0))
    json.loads(res.to_json())
    with pytest.raises(ValueError):
        evaluate_policy(env, replay, 2 ** 24 + 1)


def test_evaluator_with_an_agent_repeats_and_leaves_the_agent_alone():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    n, steps = 64, 16
    env = make(T.TASK, cfg=_eval_env_cfg(n))
    torch.manual_seed(3)
    agent = Agent(env, hidden=(128, 128))
    with torch.no_grad():                                              # a normaliser that is not the identity
        agent.obs_rms.running_mean.add_(0.05)
        agent.obs_rms.running_var.mul_(1.5)
        agent.actor_logstd.add_(0.5)
    flat = agent.flat.clone()
    rms = [getattr(agent.obs_rms, k).clone() for k in ("running_mean", "running_var", "count")]
    a = evaluate_policy(env, agent, steps)
    b = evaluate_policy(env, agent, steps)
    np.testing.assert_array_equal(a.per_env.view(U32), b.per_env.view(U32))
    assert (a.per_env[:, K["steps"]] == steps).all() and a.commands is None
    c = evaluate_policy(env, agent, steps, deterministic=False)
    assert (c.per_env[:, K["reward"]] != a.per_env[:, K["reward"]]).any()
    assert torch.equal(agent.flat, flat)
    for k, v in zip(("running_mean", "running_var", "count"), rms):
        assert torch.equal(getattr(agent.obs_rms, k), v), k


# ------------------------------------------------------------------------------------------ (i): learning, as evaluated
def test_training_shows_in_the_evaluation():
    """the device trainer, 30 iterations of servo_twin.learning_cfgs(); its policy before and after on the fixed grid of
    tools/servo_eval_oracle.py: the gain in reward per step and the drop in rms linear tracking error are at least half
    of the CPU oracle's recorded ones (profiles/servo_eval_oracle.json; half: the seed-to-seed allowance of the learning
    tests)"""
    import parity_record
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    with open(os.path.join(ROOT, E.EVAL_PROFILE)) as f:
        rec = json.load(f)
    assert rec["reward_gain"] > 0.2 and rec["err_lin_drop"] > 0.1, "the recorded run itself must show learning"
    assert rec["eval"] == dict(E.EVAL, grid=list(E.EVAL["grid"]))
    env_cfg, agent_cfg = T.learning_cfgs()
    env = make(T.TASK, cfg=env_cfg)
    torch.manual_seed(env_cfg.seed)
    trainer = PPOTrainer(env, agent_cfg)
    eval_cfg, _ = T.learning_cfgs(num_envs=E.EVAL["num_envs"])
    eval_env = make(T.TASK, cfg=eval_cfg)
    cmds = E.eval_commands()
    before = evaluate_policy(eval_env, trainer.agent, E.EVAL["steps"], commands=cmds).metrics
    for _ in range(T.LEARNING["iterations"]):
        trainer.run_iteration()
    after = evaluate_policy(eval_env, trainer.agent, E.EVAL["steps"], commands=cmds).metrics
    got = E.eval_summary(before, after)
    print(got, before, after)
    parity_record.record("servo_eval_learning_device",
                         dict(got, **{k + "_before": before[k] for k in E.EVAL_KEYS}, **{k + "_after": after[k] for k in E.EVAL_KEYS}),
                         sizes=dict(T.LEARNING, hidden=list(T.LEARNING["hidden"]), eval=dict(E.EVAL, grid=list(E.EVAL["grid"]))),
                         seed=env_cfg.seed, note="deterministic policy on the fixed command grid, before and after training")
    assert before["steps"] == after["steps"] == E.EVAL["num_envs"] * E.EVAL["steps"]
    assert got["reward_gain"] >= 0.5 * rec["reward_gain"], (got, rec["reward_gain"])
    assert got["err_lin_drop"] >= 0.5 * rec["err_lin_drop"], (got, rec["err_lin_drop"])


# ------------------------------------------------------------------------------------------ (j): play.py
def test_play_evaluates_a_checkpoint(tmp_path):
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
           "--video_length", "4"]
    r = subprocess.run([*cmd, "--eval_steps", "16", "--eval_grid", "2", "1", "1"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean reward per step" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[EVAL] ")]
    assert len(lines) == 1
    d = json.loads(lines[0][len("[EVAL] "):])
    for key in ("steps", "episodes", "fall_rate", "reward_per_step", "cat_reward_per_step", "rms_err_lin", "rms_err_yaw",
                "mean_tilt2", "mean_torque2", "mean_feet", "episode_return_mean", "episode_length_mean",
                "termination_prob_mean", "violation_share/any"):
        assert key in d["metrics"], key
    assert d["metrics"]["steps"] == 64 * 16 and [g["envs"] for g in d["by_command"]] == [32, 32]
    assert [g["command"][0] for g in d["by_command"]] == pytest.approx([-0.3, 1.0])
    with open(run / "eval" / "model_0.json") as f:
        assert json.load(f) == d
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mean reward per step" in r.stdout and "[EVAL]" not in r.stdout
