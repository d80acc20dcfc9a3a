"""The Solo12 servo surrogate on the device (csrc/servo_sim.hip, Solo12ServoSim, task ...-Solo12-Servo-v0): the kernel
against its numpy twin bit for bit, whole CaT-PPO iterations in closed loop against PPOOracle on the twin env, learning
with the device's own randomness, and the train / play entry points.  DESIGN section 9."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import servo_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = 7          # resets, post-reset observations and command resampling all occur within 50 steps


def _env_cfg():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(T.TASK, "env_cfg_entry_point")
    cfg.synthetic.servo_resample_steps = 3
    return cfg


def _device_sim(n, offset=0, seed=5, obs_dim=45):
    from cat_envs.tasks.utils.cat.cat_env import Solo12ServoSim
    cfg = _env_cfg()
    ep_len = torch.zeros(n, dtype=torch.long, device="cuda")
    reset = torch.zeros(n, dtype=torch.bool, device="cuda")
    return Solo12ServoSim(n, obs_dim, "cuda", seed, cfg.synthetic, cfg.sim.dt, cfg.decimation, MAX_LEN, ep_len, reset,
                          env_offset=offset)


def _twin(n, offset=0, seed=5, obs_dim=45):
    cfg = _env_cfg()
    return T.ServoTwin(n, obs_dim, T.params_from_cfg(cfg.synthetic), seed, MAX_LEN, cfg.sim.dt, cfg.decimation, offset)


def _run_device(sim, actions, ep0):
    """the env's bookkeeping around the simulator, on the device: counters, time-outs, hard resets"""
    ep_len, reset = sim._episode_length, sim._reset
    ep_len.copy_(torch.from_numpy(np.asarray(ep0, np.int64)))
    reset.zero_()
    sim.step(None)
    slabs = [sim.cur.clone()]
    acts = torch.from_numpy(actions).cuda()
    for t in range(len(actions)):
        sim.step(acts[t])
        ep_len.add_(1)
        reset.copy_((ep_len >= MAX_LEN) | (sim.view("hard_reset")[:, 0] > 0.5))
        ep_len.masked_fill_(reset, 0)
        slabs.append(sim.cur.clone())
    torch.cuda.synchronize()
    return torch.stack(slabs).cpu().numpy()


def _inputs(n, steps=50, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((steps, n, 12)).astype(np.float32), rs.randint(0, MAX_LEN, n)


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_kernel_equals_the_twin_bit_for_bit(n):
    """every float of every slab of 50 steps of random actions, compared as uint32"""
    acts, ep0 = _inputs(n)
    sim = _device_sim(n)
    assert sim.off == _twin(n).off and sim.F == _twin(n).F
    dev = _run_device(sim, acts, ep0)
    ref = T.run_twin(_twin(n), acts, ep0)
    assert dev.shape == ref.shape == (51, n, sim.F)
    diff = dev.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        t, i, c = [int(x[0]) for x in np.nonzero(diff)]
        field = [k for k, (a, w) in sim.off.items() if a <= c < a + w]
        raise AssertionError(f"{int(diff.sum())} words differ; first: step {t} env {i} column {c} {field}: "
                             f"device {dev[t, i, c]!r} twin {ref[t, i, c]!r}")
    ep = ref[-1, :, sim.off["servo"][0] + 13]
    assert ep.min() >= 6                                      # at least six episodes per env in those 50 steps
    assert (ref[:, :, sim.off["hard_reset"][0]] > 0.5).any() or n < 1000


def test_kernel_observation_width_other_than_45():
    for d in (20, 48):
        acts, ep0 = _inputs(40, steps=10, seed=d)
        dev = _run_device(_device_sim(40, obs_dim=d), acts, ep0)
        ref = T.run_twin(_twin(40, obs_dim=d), acts, ep0)
        np.testing.assert_array_equal(dev.view(np.uint32), ref.view(np.uint32))


def test_two_shards_equal_the_rows_of_one_simulator_and_runs_repeat():
    acts, ep0 = _inputs(64, seed=3)
    whole = _run_device(_device_sim(64), acts, ep0)
    again = _run_device(_device_sim(64), acts, ep0)
    np.testing.assert_array_equal(whole.view(np.uint32), again.view(np.uint32))
    lo = _run_device(_device_sim(32, offset=0), acts[:, :32].copy(), ep0[:32])
    hi = _run_device(_device_sim(32, offset=32), acts[:, 32:].copy(), ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(np.uint32), lo.view(np.uint32))
    np.testing.assert_array_equal(whole[:, 32:].view(np.uint32), hi.view(np.uint32))


def test_descriptor_is_checked():
    sim = _device_sim(16)
    d = sim._desc
    d.state_out, d.action = sim.cur.data_ptr(), sim.default_joint_pos.data_ptr()       # state_out == state_in
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)
    d.state_out, d.off_obs = sim._slabs[0].data_ptr(), sim.F - 3                        # the observation leaves the row
    with pytest.raises(RuntimeError, match="bad argument"):
        sim._nat.servo_sim_step(d)


# ------------------------------------------------------------------------------------------ whole iterations, closed loop
def _cfgs(num_envs, num_steps, minibatch, epochs, iters, hidden, seed):
    from cat_envs.shim import load_cfg_from_registry
    env_cfg = _env_cfg()
    env_cfg.synthetic.servo_resample_steps = 250
    agent_cfg = load_cfg_from_registry(T.TASK, "clean_rl_cfg_entry_point")
    env_cfg.scene.num_envs, env_cfg.seed = num_envs, seed
    agent_cfg.num_steps, agent_cfg.minibatch_size = num_steps, minibatch
    agent_cfg.updates_epochs, agent_cfg.num_iterations = epochs, iters
    agent_cfg.hidden = tuple(hidden)
    agent_cfg.save_interval = 10 ** 9
    return env_cfg, agent_cfg


def servo_run_pair(num_envs=64, num_steps=24, minibatch=512, epochs=2, iters=1, hidden=(512, 256, 128), seed=42,
                   trace=False, replay_actions=True, agent_overrides=None):
    """smoke_impl.run_pair on the servo task: PPOTrainer on the device env, PPOOracle on the closed-loop twin env, the
    same injected noise and permutations; the device's actions are replayed so that both sides see identical states"""
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    from oracle import ppo_oracle
    env_cfg, agent_cfg = _cfgs(num_envs, num_steps, minibatch, epochs, iters, hidden, seed)
    for k, v in (agent_overrides or {}).items():
        setattr(agent_cfg, k, v)
    env = make(T.TASK, cfg=env_cfg)
    torch.manual_seed(seed)
    trainer = PPOTrainer(env, agent_cfg)
    sd = {k: v.detach().cpu().clone() for k, v in trainer.agent.state_dict().items()}
    mgr = env.unwrapped.constraint_manager
    cpu_env = T.env_oracle_from_cfg(env_cfg, num_envs, env.unwrapped.episode_length_buf.cpu().numpy(), tau=mgr.cat.tau,
                                    min_p=mgr.cat.min_p)
    assert cpu_env.max_episode_length == env.unwrapped.max_episode_length
    ag = ppo_oracle.AgentOracle(trainer.D, trainer.A, hidden)
    ag.load({k: v for k, v in sd.items() if not k.startswith(("obs_rms", "value_rms"))})
    cfg = {k: getattr(agent_cfg, k) for k in ppo_oracle.PPOOracle.DEFAULT_CFG}
    orc = ppo_oracle.PPOOracle(cpu_env, num_envs, trainer.D, trainer.A, cfg=cfg, hidden=hidden, agent=ag)
    rs = np.random.RandomState(seed)
    outs = []
    B = num_envs * num_steps
    if trace:
        trainer.trace_params, orc.trace = True, True
    for it in range(iters):
        eps = rs.standard_normal((num_steps, num_envs, trainer.A)).astype(np.float32)
        perms = np.stack([rs.permutation(B) for _ in range(epochs)]).astype(np.int64)
        eps_d, perms_d = torch.from_numpy(eps).cuda(), torch.from_numpy(perms).cuda()
        trainer.run_iteration(eps_fn=lambda s: eps_d[s], perm_fn=lambda e: perms_d[e])
        acts = trainer.actions.cpu()
        outs.append(orc.run_iteration(eps_fn=lambda s: torch.from_numpy(eps[s]), perm_fn=lambda e: torch.from_numpy(perms[e]),
                                      actions_fn=(lambda s: acts[s]) if replay_actions else None))
    torch.cuda.synchronize()
    return trainer, orc, outs


def _iteration(monkeypatch, name, **kw):
    """the whole-iteration check of tests/test_gpu_parity_sizes.py (bit-exact rewards / dones, BARS["default"], the
    branch-flip proof if the parameter bar is exceeded) with the servo pair in place of the stream pair"""
    import smoke_impl
    import test_gpu_parity_sizes as PS
    assert PS.BARS["default"] == dict(values=8e-6, logprobs=1.6e-5, advantages=1e-5, returns=1e-5, params=1.2e-5,
                                      actions=1e-5)
    monkeypatch.setattr(smoke_impl, "run_pair", servo_run_pair)
    return PS._iteration(name, **kw)


def _closed_loop_checks(trainer, orc):
    sim = trainer.envs.unwrapped.sim
    assert type(sim).__name__ == "Solo12ServoSim" and trainer.sink is not None          # the fused step_into path
    # both sides ended in the same simulator state, bit for bit, and resets of both kinds happened on the way
    np.testing.assert_array_equal(sim.cur.cpu().numpy().view(np.uint32), orc.env.stream[0].view(np.uint32))
    np.testing.assert_array_equal(trainer.envs.unwrapped.episode_length_buf.cpu().numpy(), orc.env.episode_length)
    assert float(trainer.true_dones.float().sum()) > 0
    # the observations the policy saw are the twin's, normalised: the raw stream is closed loop
    assert float(trainer.rewards.float().std()) > 0


def test_closed_loop_64x24_two_iterations(monkeypatch):
    trainer, orc, outs, rep = _iteration(monkeypatch, "servo_closed_loop_64x24", num_envs=64, num_steps=24, minibatch=512,
                                         epochs=5, iters=2)
    _closed_loop_checks(trainer, orc)
    assert len(trainer.envs.unwrapped.constraint_manager.active_terms) == 13


def test_closed_loop_2048x24_one_iteration(monkeypatch):
    trainer, orc, outs, rep = _iteration(monkeypatch, "servo_closed_loop_2048x24", num_envs=2048, num_steps=24,
                                         minibatch=16384, epochs=2, iters=1)
    _closed_loop_checks(trainer, orc)
    assert float((orc.env._f(orc.env.stream[0], "servo")[:, 13]).max()) >= 1       # episodes ended


def test_fused_and_plain_env_step_give_identical_bytes():
    a, _, _ = servo_run_pair(num_envs=64, num_steps=24, minibatch=512, epochs=1, iters=1)
    b, _, _ = servo_run_pair(num_envs=64, num_steps=24, minibatch=512, epochs=1, iters=1,
                             agent_overrides={"fused_rollout": False})
    assert a.sink is not None and b.sink is None
    for name in ("obs", "actions", "rewards", "dones", "true_dones", "values", "logprobs", "advantages", "returns"):
        x, y = getattr(a, name).float().cpu().numpy(), getattr(b, name).float().cpu().numpy()
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    np.testing.assert_array_equal(a.envs.unwrapped.sim.cur.cpu().numpy().view(np.uint32),
                                  b.envs.unwrapped.sim.cur.cpu().numpy().view(np.uint32))


def test_free_running_drift_is_recorded():
    """without action replay the two sides take their own actions (1e-6 apart) through the closed loop; how far rewards,
    observations and the simulator state drift apart in two iterations is recorded, not asserted"""
    import parity_record
    trainer, orc, outs = servo_run_pair(num_envs=64, num_steps=24, minibatch=512, epochs=5, iters=2, replay_actions=False)

    def err(a, b):
        return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    rec = dict(rewards=err(trainer.rewards.float().cpu(), orc.rewards), dones=err(trainer.dones[1:trainer.T].float().cpu(), orc.dones[1:]),
               actions=err(trainer.actions.cpu(), orc.actions), values=err(trainer.values.float().cpu(), orc.values),
               sim_state=err(trainer.envs.unwrapped.sim.cur.cpu(), orc.env.stream[0]))
    print("free-running drift:", rec)
    parity_record.record("servo_free_running_64x24", rec, sizes=dict(num_envs=64, num_steps=24, iters=2), seed=42,
                         note="no action replay: recorded, not asserted")
    assert all(np.isfinite(v) for v in rec.values())


# ------------------------------------------------------------------------------------------ learning on the device
def test_device_trainer_learns_on_the_servo_task():
    """device randomness (Philox noise, keyed permutations), the sizes of the CPU learning test, 30 iterations: reward
    gain and violation drop are at least half of the recorded CPU run's (profiles/servo_learning_oracle.json)"""
    import parity_record
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    with open(os.path.join(ROOT, T.LEARNING_PROFILE)) as f:
        rec = json.load(f)
    env_cfg, agent_cfg = T.learning_cfgs()
    env = make(T.TASK, cfg=env_cfg)
    torch.manual_seed(env_cfg.seed)
    trainer = PPOTrainer(env, agent_cfg)
    assert trainer.rng == "device" and trainer.sink is not None
    env_u = env.unwrapped
    cm = env_u.constraint_manager
    assert cm.active_terms == ["joint_torque", "foot_contact_force", "base_orientation"]
    viol = torch.zeros((), device="cuda")
    step_into = env_u.step_into

    def counted(action, sink):
        out = step_into(action, sink)
        viol.add_((cm._cstr_prob_buf > 0).float().mean())
        return out
    env_u.step_into = counted
    reward, violation = [], []
    for it in range(T.LEARNING["iterations"]):
        viol.zero_()
        trainer.run_iteration()
        reward.append(float(trainer.rewards.float().mean()))
        violation.append(float(viol) / trainer.T)
    got = T.learning_summary(reward, violation)
    print(got, reward, violation)
    parity_record.record("servo_learning_device", dict(got, reward_first=reward[0], reward_last=reward[-1],
                                                       violation_first=violation[0], violation_last=violation[-1]),
                         sizes=dict(T.LEARNING, hidden=list(T.LEARNING["hidden"])), seed=env_cfg.seed,
                         note="reward per step: " + " ".join(f"{r:.3f}" for r in reward) + " | violation share: "
                              + " ".join(f"{v:.3f}" for v in violation))
    assert got["reward_gain"] >= 0.5 * rec["reward_gain"], (got, rec["reward_gain"])
    assert got["violation_drop"] >= 0.5 * rec["violation_drop"], (got, rec["violation_drop"])


# ------------------------------------------------------------------------------------------ entry points
def test_train_and_play_on_the_servo_task(tmp_path):
    common = [f"--task={T.TASK}", "--headless", "--num_envs", "256"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clean_rl/train.py"), *common, "--num_iterations", "3",
                        "--seed", "3", "agent.save_interval=3", "agent.minibatch_size=2048"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Starting training for 3 steps" in r.stdout and "Saved model" in r.stdout
    runs = os.listdir(tmp_path / "logs" / "clean_rl" / "solo12_flat")
    assert len(runs) == 1
    run = tmp_path / "logs" / "clean_rl" / "solo12_flat" / runs[0]
    assert "model_2.pt" in os.listdir(run)
    sd = torch.load(run / "model_2.pt", map_location="cpu")
    assert all(torch.isfinite(v).all() for v in sd.values())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clean_rl/play.py"), *common, "--video_length", "8"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "model_2.pt" in r.stdout and "mean reward per step" in r.stdout
