"""A run that is saved, thrown away and loaded into a NEW env and a NEW trainer computes the bytes of the run that was
never interrupted (``PPOTrainer.save_state / load_state``, ``CaTEnv.state_dict / load_state_dict``).

Common shape: 40 envs (no multiple of the 16-env tile of the servo and term kernels), 6 steps, hidden (64, 64), 240 rows in
minibatches of 64 (four, the last one ragged), 2 epochs, default ``graph_update`` (the update graph is captured before the
save and again after the load), episodes of 7 steps with ``episode_length_buf = arange(N) % 7`` right after the env is
built - at least five envs end an episode in EVERY step, the last one before the save included.

Arms: A = 6 iterations in one go; A' = A once more (the control: if A' differed from A the run would not be reproducible
and B would mean nothing); B = 3 iterations, save, new env + new trainer from fresh cfgs, load, 3 iterations.  After each
of iterations 4, 5, 6: parameters, Adam moments, the device iteration state, both normalisers, the iteration's rollout,
the CaT state, the episode counters, the simulator state, every term's ``max_p`` and the returned statistics, compared
with ``assert_array_equal`` - bytes, no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, MB, EPOCHS, ITERS, SAVE_AT = 40, 6, 64, 2, 6, 3
HIDDEN = (64, 64)
EP_LEN = 7
N_KEYS = 7 + 4 * (len(HIDDEN) + 1)          # logstd, 2 x 3 normaliser buffers, weight + bias per layer and net


# ------------------------------------------------------------------------------------------------ cfgs and arms
def _shape_env(env_cfg):
    env_cfg.episode_length_s = (EP_LEN - 0.5) * env_cfg.sim.dt * env_cfg.decimation      # ceil(6.5) = 7 steps


def stream_cfgs(num_envs=N, num_steps=T, hidden=HIDDEN, seed=42, **agent_over):
    """fresh cfg objects on every call: the curriculum writes ``max_p`` INTO the term cfgs"""
    import smoke_impl
    task, env_cfg, agent_cfg = smoke_impl.make_cfgs(num_envs, num_steps, MB, EPOCHS, ITERS, hidden=hidden, six_terms=True,
                                                    seed=seed)
    _shape_env(env_cfg)
    for k, v in agent_over.items():
        setattr(agent_cfg, k, v)
    return task, env_cfg, agent_cfg


def servo_cfgs(**agent_over):
    import servo_twin
    env_cfg, agent_cfg = servo_twin.learning_cfgs(num_envs=N)
    _shape_env(env_cfg)
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = T, MB, HIDDEN
    agent_cfg.updates_epochs, agent_cfg.num_iterations = EPOCHS, ITERS
    for term in vars(env_cfg.curriculum).values():           # progress 0.25 at the save, 0.5 at the end
        term.params["num_steps"] = ITERS * T * 2
    for k, v in agent_over.items():
        setattr(agent_cfg, k, v)
    return servo_twin.TASK, env_cfg, agent_cfg


def build(cfgs):
    """(env, trainer) from fresh cfgs, seeded like smoke_impl.run_pair"""
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    task, env_cfg, agent_cfg = cfgs()
    env = make(task, cfg=env_cfg)
    n = env.unwrapped.num_envs
    assert env.unwrapped.max_episode_length == EP_LEN
    env.unwrapped.episode_length_buf.copy_(torch.arange(n, device=env.unwrapped.device) % EP_LEN)
    torch.manual_seed(int(env_cfg.seed))
    return env, PPOTrainer(env, agent_cfg)


def term_max_p(env):
    cm = env.unwrapped.constraint_manager
    return {n: float(cm.get_term_cfg(n).max_p) for n in cm.active_terms}


def snapshot(env, tr, stats):
    """everything the issue lists, as host arrays"""
    from cat_envs import native
    torch.cuda.synchronize()
    e, a, cm = env.unwrapped, tr.agent, env.unwrapped.constraint_manager
    h = lambda t: t.detach().cpu().numpy().copy()
    state = h(tr.state)
    for f in ("adam_step_size", "adam_bc2_sqrt"):            # scratch floats of the optimiser kernel
        off = getattr(native.IterState, f).offset
        state[off:off + 4] = 0
    s = {"flat": h(a.flat), "exp_avg": h(tr.exp_avg), "exp_avg_sq": h(tr.exp_avg_sq), "iter_state": state}
    for name, rms in (("obs_rms", a.obs_rms), ("value_rms", a.value_rms)):
        s[name + ".mean"], s[name + ".var"], s[name + ".count"] = h(rms.running_mean), h(rms.running_var), h(rms.count)
    for name in ("rewards", "dones", "values", "actions", "logprobs", "advantages"):
        s[name] = h(getattr(tr, name))
    s.update({"cat.p_rm": h(cm.cat._p_rm), "cat.ep_viol": h(cm._ep_viol), "cat.ep_prob": h(cm._ep_prob),
              "episode_length_buf": h(e.episode_length_buf), "sim.cur": h(e.sim.cur)})
    mp = term_max_p(env)
    s["max_p.names"], s["max_p"] = np.array(list(mp)), np.array(list(mp.values()), np.float64)
    s["stats.keys"], s["stats"] = np.array(list(stats)), np.array([float(v) for v in stats.values()], np.float64)
    s["host"] = np.array([tr.iteration, tr.adam_step, tr.global_step, e.common_step_counter, e._sim_step_counter], np.int64)
    return s


def assert_same(a, b, what):
    assert list(a) == list(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def arm_a(cfgs, iters=ITERS, probe=None):
    """uninterrupted run: snapshots after every iteration; ``probe(env, trainer)`` is called at the save point of arm B"""
    env, tr = build(cfgs)
    snaps = []
    for it in range(1, iters + 1):
        snaps.append(snapshot(env, tr, tr.run_iteration()))
        if probe is not None and it == SAVE_AT:
            probe(env, tr)
    return snaps


def arm_b(cfgs, path, save_at=SAVE_AT, iters=ITERS, at_save=None):
    """run, save, throw away; new env + new trainer from fresh cfgs, load, go on: snapshots of the iterations after it"""
    env, tr = build(cfgs)
    for _ in range(save_at):
        tr.run_iteration()
    torch.cuda.synchronize()
    if save_at > 0:
        assert bool(env.unwrapped.reset_buf.any()), "no env ended an episode in the last step before the save"
    graph_before = tr._graph_id
    if at_save is not None:
        at_save(env, tr)
    tr.save_state(str(path))
    assert os.path.isfile(path) and not os.path.exists(str(path) + ".tmp")
    del env, tr
    env, tr = build(cfgs)
    assert tr.iteration == 0 and tr.adam_step == 0
    tr.load_state(str(path))
    assert tr.iteration == save_at and tr._graph_id is None
    snaps = [snapshot(env, tr, tr.run_iteration()) for _ in range(save_at + 1, iters + 1)]
    return snaps, tr, graph_before


def check_case(cfgs, tmp_path, save_at=SAVE_AT, iters=ITERS, probe=None, expect_graph=True):
    a = arm_a(cfgs, iters, probe)
    a2 = arm_a(cfgs, iters)
    for it in range(iters):
        assert_same(a[it], a2[it], f"control A' against A (the run itself is not reproducible), iteration {it + 1}")
    b, tr_b, graph_before = arm_b(cfgs, tmp_path / f"state_{save_at}.pt", save_at, iters, at_save=probe)
    for k, it in enumerate(range(save_at, iters)):
        assert_same(a[it], b[k], f"resumed run B against A, iteration {it + 1}")
    assert int(a[-1]["host"][0]) == iters and tr_b.iteration == iters
    if expect_graph:        # captured before the save (from the first update phase on) and captured again after the load
        assert tr_b.graph_update and tr_b._graph_id is not None and (save_at == 0 or graph_before is not None)
    else:
        assert tr_b._graph_id is None and graph_before is None
    return a, b, tr_b


# ------------------------------------------------------------------------------------------------ cases 1 - 7
def test_stream_six_terms_linear_anneal(tmp_path):
    lr0 = stream_cfgs()[2].learning_rate
    assert stream_cfgs()[2].anneal_lr and stream_cfgs()[2].lr_schedule is None
    a, b, tr = check_case(stream_cfgs, tmp_path)
    keys = list(b[0]["stats.keys"])
    assert float(b[0]["stats"][keys.index("learning_rate")]) == (1 - 3 / 6) * lr0      # iteration 4 of 6, not 1 of 6
    assert tr.nat.iter_state_read(tr.state).lr == (1 - 5 / 6) * lr0                    # the device's own, iteration 6
    # the file is also a policy checkpoint: Agent.state_dict()'s keys (23 with three hidden layers, 19 with these two),
    # loadable with the safe loader
    sd = torch.load(tmp_path / "state_3.pt", map_location="cpu", weights_only=True)
    assert len(sd["trainer"]["agent"]) == N_KEYS and list(sd["trainer"]["agent"]) == list(tr.agent.state_dict())
    assert sd["trainer"]["iter_state_fields"]["iteration"] == 3 and sd["trainer"]["sizeof_iter_state"] == tr.state.numel()
    assert "stream" not in sd["env"]["sim"] and sd["fingerprint"]["stream_steps"] == 16   # regenerated, not stored


def test_servo_three_terms_curriculum_half_way(tmp_path):
    fresh = servo_cfgs()[1]
    curriculum_terms = list(vars(fresh.curriculum))
    initial = {n: float(getattr(fresh.constraints, n).max_p) for n in curriculum_terms}
    assert sorted(curriculum_terms) == ["base_orientation", "joint_torque"]
    at_save = {}

    def probe(env, tr):
        assert env.unwrapped.common_step_counter == SAVE_AT * T
        at_save.update(term_max_p(env))
    a, b, tr = check_case(servo_cfgs, tmp_path, probe=probe)
    final = dict(zip(a[-1]["max_p.names"], a[-1]["max_p"]))
    for n in curriculum_terms:       # otherwise a lost max_p would go unnoticed
        assert at_save[n] != initial[n] and at_save[n] != final[n], (n, initial[n], at_save[n], final[n])
        assert at_save[n] == 1 / (20 + 0.25 * (1 / 0.25 - 20)) and final[n] == 1 / (20 + 0.5 * (1 / 0.25 - 20))


def test_adaptive_lr_and_last_kl_come_back_from_the_state_bytes(tmp_path):
    # kl_threshold far below the KL of an epoch of four optimiser steps at lr 3e-4: the rate moves in the first epoch
    cfgs = lambda: stream_cfgs(lr_schedule="adaptive", kl_threshold=1e-6)
    lr0 = cfgs()[2].learning_rate
    seen = []

    def probe(env, tr):
        st = tr.nat.iter_state_read(tr.state)
        seen.append((float(st.lr), float(st.last_kl)))
        assert float(st.lr) != lr0 and float(st.last_kl) != 0.0, (st.lr, st.last_kl)
    check_case(cfgs, tmp_path, probe=probe)
    assert len(seen) == 2 and seen[0] == seen[1]              # arm A and arm B stood at the same point


def test_torch_rng_generator_states_are_restored(tmp_path):
    cfgs = lambda: stream_cfgs(rng="torch")
    a, b, tr = check_case(cfgs, tmp_path, expect_graph=False)     # rng="torch": no graph, by the trainer's own rule
    assert not tr.graph_update
    sd = torch.load(tmp_path / "state_3.pt", map_location="cpu", weights_only=True)
    assert set(sd["trainer"]["torch_rng"]) == {"cpu", "device"}


def test_bf16_mlp_fp16_rollout(tmp_path):
    cfgs = lambda: stream_cfgs(mlp_precision="bf16", rollout_dtype="fp16")
    a, b, tr = check_case(cfgs, tmp_path)
    assert a[-1]["rewards"].dtype == np.float16 and tr.agent.mlp_precision == "bf16"


def test_save_straight_after_construction(tmp_path):
    """(no env step has run at this save point, so no env has ended an episode yet: ``reset_buf`` is all False here)"""
    check_case(stream_cfgs, tmp_path, save_at=0, iters=2)


@pytest.mark.parametrize("over", [dict(fused_rollout=False), dict(graph_update=False)], ids=lambda o: next(iter(o)))
def test_unfused_rollout_and_eager_update(tmp_path, over):
    cfgs = lambda: stream_cfgs(**over)
    a, b, tr = check_case(cfgs, tmp_path, expect_graph="graph_update" not in over)
    assert (tr.sink is None) == ("fused_rollout" in over)


# ------------------------------------------------------------------------------------------------ case 8: refusals
@pytest.fixture(scope="module")
def saved_stream_state(tmp_path_factory):
    env, tr = build(stream_cfgs)
    tr.run_iteration()
    path = tmp_path_factory.mktemp("resume") / "state_1.pt"
    tr.save_state(str(path))
    return str(path)


def _servo_as_stream_shapes():
    return servo_cfgs()


REFUSALS = {"num_envs": lambda: stream_cfgs(num_envs=48), "hidden": lambda: stream_cfgs(hidden=(128, 64)),
            "num_steps": lambda: stream_cfgs(num_steps=5), "env_seed": lambda: stream_cfgs(seed=43),
            "task_kind": _servo_as_stream_shapes}


@pytest.mark.parametrize("field", list(REFUSALS))
def test_refused_load_names_the_field_and_touches_nothing(saved_stream_state, field):
    env, tr = build(REFUSALS[field])
    tr.run_iteration()                                        # a graph, moments and CaT state of its own
    torch.cuda.synchronize()
    e = env.unwrapped
    watched = lambda: [t.detach().cpu().numpy().copy() for t in
                       (tr.agent.flat, tr.exp_avg, e.episode_length_buf, e.constraint_manager.cat._p_rm, tr.state, e.sim.cur)]
    before, graph, max_p = watched(), tr._graph_id, term_max_p(env)
    with pytest.raises(ValueError) as err:
        tr.load_state(saved_stream_state)
    msg = str(err.value)
    assert f"{field}: saved " in msg and saved_stream_state in msg, msg
    others = [f for f in ("num_envs", "hidden", "num_steps", "env_seed") if f != field]
    if field != "task_kind":                                  # (another task differs in its terms and constants as well)
        assert not any(f"{f}: saved " in msg for f in others + ["task_kind"]), msg
    torch.cuda.synchronize()
    for x, y in zip(before, watched()):
        np.testing.assert_array_equal(x, y)
    assert tr._graph_id == graph and tr.iteration == 1 and term_max_p(env) == max_p
    tr.run_iteration()                                        # and it goes on as if nothing had been tried
    assert tr.iteration == 2


def test_save_is_refused_while_an_evaluation_is_attached(tmp_path):
    from cat_envs import native
    env, tr = build(servo_cfgs)
    tr.run_iteration()
    e = env.unwrapped
    path = str(tmp_path / "state_1.pt")
    e.set_eval_record(torch.zeros(N, len(native.SERVO_EVAL_FIELDS), device=e.device))
    with pytest.raises(RuntimeError, match="evaluation"):
        tr.save_state(path)
    e.set_eval_record(None)
    e.set_fixed_commands(torch.zeros(N, 3, device=e.device))
    with pytest.raises(RuntimeError, match="fixed-command"):
        tr.save_state(path)
    assert os.listdir(tmp_path) == []
    e.set_fixed_commands(None)
    tr.save_state(path)
    assert os.listdir(tmp_path) == ["state_1.pt"]


# ------------------------------------------------------------------------------------------------ case 9: entry point
def test_train_resume_entry_point(tmp_path):
    """train.py to the end; train.py stopped after 4 of 6 iterations (--stop_after: the anneal follows the 6 in all three
    runs); train.py --resume True from the stopped run's state_3.pt, in a new run directory: the same model_5.pt."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts/clean_rl/train.py"), "--task=Isaac-Velocity-CaT-Flat-Solo12-Servo-v0",
           "--headless", "--num_envs", "64", "--num_iterations", "6", "agent.num_iterations=6", "agent.save_interval=2",
           "agent.hidden=[64,64]", "agent.minibatch_size=256"]
    log_root = tmp_path / "logs" / "clean_rl" / "solo12_flat"

    def run(extra, n_runs):
        r = subprocess.run(cmd + extra, cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        runs = sorted(os.listdir(log_root))
        assert len(runs) == n_runs, runs
        return r.stdout, log_root / runs[-1]
    out, full = run([], 1)
    assert out.count("Saved model") == 3
    files = sorted(f for f in os.listdir(full) if f.endswith(".pt"))
    assert files == ["model_1.pt", "model_3.pt", "model_5.pt", "state_3.pt", "state_5.pt"]      # keep_states = 2
    assert not os.path.exists(full / "params" / "resumed_from.txt")
    out, stopped = run(["--stop_after", "4"], 2)
    assert sorted(f for f in os.listdir(stopped) if f.endswith(".pt")) == ["model_1.pt", "model_3.pt", "state_1.pt", "state_3.pt"]
    out, resumed = run(["--resume", "True"], 3)
    assert "Resuming from " in out and "state_3.pt at iteration 4" in out and out.count("Saved model") == 1
    named = open(resumed / "params" / "resumed_from.txt").read().strip()
    assert os.path.isabs(named) and os.path.samefile(named, stopped / "state_3.pt")
    assert sorted(f for f in os.listdir(resumed) if f.endswith(".pt")) == ["model_5.pt", "state_5.pt"]
    want = torch.load(full / "model_5.pt", map_location="cpu")
    got = torch.load(resumed / "model_5.pt", map_location="cpu")
    assert list(want) == list(got) and len(got) == N_KEYS
    for k in want:
        assert torch.equal(want[k], got[k]), k
    a = torch.load(full / "state_5.pt", map_location="cpu", weights_only=True)
    b = torch.load(resumed / "state_5.pt", map_location="cpu", weights_only=True)
    assert torch.equal(a["trainer"]["exp_avg_sq"], b["trainer"]["exp_avg_sq"])
    assert torch.equal(a["env"]["sim"]["cur"], b["env"]["sim"]["cur"]) and a["trainer"]["global_step"] == b["trainer"]["global_step"]
