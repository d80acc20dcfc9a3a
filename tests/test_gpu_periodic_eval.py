"""Evaluation inside a training run, on the device (cat_envs/tasks/utils/cleanrl/periodic_eval.py).

Common shape (servo task): training 64 envs x 8 steps, hidden (128, 128), one epoch, two minibatches of 256 rows;
evaluation 32 envs x 16 steps on the command grid (2, 2, 1); episodes of 7 control steps, so every env ends at least two
episodes inside one evaluation and at least one inside every rollout.  Everything is compared as bytes, no tolerance -
except ``device_ms`` of a history line, which is a measured time."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import servo_eval_twin as E
import servo_twin as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, MB, HIDDEN, EP_LEN = 64, 8, 256, (128, 128), 7
EVAL_ENVS, EVAL_STEPS, EVAL_GRID = 32, 16, (2, 2, 1)
U32 = np.uint32


# ------------------------------------------------------------------------------------------------ cfgs
def _short_episodes(env_cfg):
    env_cfg.episode_length_s = (EP_LEN - 0.5) * env_cfg.sim.dt * env_cfg.decimation      # ceil(6.5) = 7 control steps


def cfgs(iters=6, **agent_over):
    """fresh cfg objects on every call (the curriculum writes ``max_p`` INTO the term cfgs): the learning experiment's
    three terms and curriculum, the curriculum sped up so that ``max_p`` moves between any two evaluations"""
    env_cfg, agent_cfg = T.learning_cfgs(num_envs=N)
    _short_episodes(env_cfg)
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = STEPS, MB, HIDDEN
    agent_cfg.updates_epochs, agent_cfg.num_iterations = 1, iters
    for term in vars(env_cfg.curriculum).values():
        term.params["num_steps"] = 2 * iters * STEPS
    agent_cfg.eval_envs, agent_cfg.eval_steps, agent_cfg.eval_grid = EVAL_ENVS, EVAL_STEPS, EVAL_GRID
    for k, v in agent_over.items():
        setattr(agent_cfg, k, v)
    return env_cfg, agent_cfg


def make_envs(env_cfg, agent_cfg, episode_length=EP_LEN):
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env
    env = make(T.TASK, cfg=env_cfg)
    assert env.unwrapped.max_episode_length == episode_length
    eval_env = make_eval_env(T.TASK, env_cfg, agent_cfg.eval_envs) if agent_cfg.eval_interval > 0 else None
    return env, eval_env


def build(**agent_over):
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    run_path = agent_over.pop("run_path", None)
    env_cfg, agent_cfg = cfgs(**agent_over)
    env, eval_env = make_envs(env_cfg, agent_cfg)
    torch.manual_seed(int(env_cfg.seed))
    return env, eval_env, PPOTrainer(env, agent_cfg, run_path, eval_env=eval_env)


def term_max_p(env):
    cm = env.unwrapped.constraint_manager
    return {n: float(cm.get_term_cfg(n).max_p) for n in cm.active_terms}


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    diff = a.view(U32) != b.view(U32)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ"


def _same_result(a, b):
    _bits(a.per_env, b.per_env, "simulator record")
    _bits(a.cat_reward, b.cat_reward, "cat_reward")
    _bits(a.termination_prob, b.termination_prob, "termination_prob")
    _bits(a.violations, b.violations, "violations")
    assert a.metrics == b.metrics


def _no_device_ms(rec):
    return {k: v for k, v in rec.items() if k != "device_ms"}


# ------------------------------------------------------------------------------------------------ 1: purity
def _loud_agent(env):
    """an agent whose mean action is large behind a normaliser that is not the identity.  Last actor layer x 100: every
    term is violated in some steps, and the torques stay below their clip in most - at x 300 every env sits at the clip,
    each violation equals the column maximum, and the probabilities saturate at ``max_p`` whatever the running maxima are"""
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    torch.manual_seed(3)
    agent = Agent(env, hidden=HIDDEN)
    with torch.no_grad():
        agent.obs_rms.running_mean.add_(0.05)
        agent.obs_rms.running_var.mul_(1.5)
        agent.actor_mean[-1].weight.mul_(100.0)
    return agent


def _dirty(env, seed):
    """a few env steps of large random actions: running maxima, probability buffers, episode sums and the log ring move"""
    u = env.unwrapped
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(5):
        env.step((torch.randn(u.num_envs, 12, generator=g) * 3.0).to(u.device))


def test_an_evaluation_from_a_fresh_cat_state_is_a_pure_function():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    env_cfg, _ = cfgs()
    tab = E.eval_commands()[:EVAL_ENVS]
    results = {}
    for fresh in (True, False):
        env = make(T.TASK, cfg=make_eval_env_cfg(env_cfg, EVAL_ENVS))
        cm = env.unwrapped.constraint_manager
        agent = _loud_agent(env)
        a = evaluate_policy(env, agent, EVAL_STEPS, commands=tab, fresh_cat_state=fresh)
        rm_ptr = cm.cat._p_rm.data_ptr()
        assert a.violations[:, -1].sum() > 0 and a.termination_prob.sum() > 0      # the comparison is about something
        assert (a.per_env[:, 0] == EVAL_STEPS).all() and a.per_env[:, 1].min() >= 2   # every env ended two episodes
        _dirty(env, seed=11)
        counter, max_p = env.unwrapped.common_step_counter, term_max_p(env)
        b = evaluate_policy(env, agent, EVAL_STEPS, commands=tab, fresh_cat_state=fresh)
        assert cm.cat._p_rm.data_ptr() == rm_ptr                                    # in place: never a rebound tensor
        results[fresh] = (a, b)
        if fresh:
            assert env.unwrapped.common_step_counter == counter and term_max_p(env) == max_p   # the curriculum stood still
    a, b = results[True]
    _same_result(a, b)
    a0, b0 = results[False]
    _bits(a0.per_env, b0.per_env, "simulator record (default keyword)")              # what the evaluator always promised
    assert (a0.termination_prob.view(U32) != b0.termination_prob.view(U32)).any()   # the gap the keyword closes
    _same_result(a, a0)                                                              # a new env IS a fresh state


def test_a_fresh_cat_state_with_a_running_curriculum():
    """on an env WITH a curriculum (the training cfg itself): ``max_p`` set by the caller holds for the whole evaluation
    and the curriculum goes on afterwards from where it stood"""
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    env_cfg, _ = cfgs()
    env_cfg.scene.num_envs = EVAL_ENVS
    env = make(T.TASK, cfg=env_cfg)
    u, agent = env.unwrapped, _loud_agent(env)
    a = evaluate_policy(env, agent, EVAL_STEPS, fresh_cat_state=True)
    start = term_max_p(env)
    _dirty(env, seed=5)
    moved = term_max_p(env)
    assert u.common_step_counter == 5 and moved != start
    cm = u.constraint_manager
    for name, p in start.items():
        cfg = cm.get_term_cfg(name)
        cfg.max_p = p
        cm.set_term_cfg(name, cfg)
    b = evaluate_policy(env, agent, EVAL_STEPS, fresh_cat_state=True)
    assert term_max_p(env) == start and u.common_step_counter == 5
    _same_result(a, b)
    env.step(torch.zeros(EVAL_ENVS, 12, device=u.device))
    assert u.common_step_counter == 6 and term_max_p(env) != start


# ------------------------------------------------------------------------------------------------ 2: non-interference
def snapshot(env, tr):
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
    for name in ("obs", "actions", "logprobs", "rewards", "dones", "true_dones", "values", "advantages", "returns"):
        s[name] = h(getattr(tr, name))
    s.update({"cat.p_rm": h(cm.cat._p_rm), "cat.p_probs": h(cm.cat._p_probs), "cat.p_cstr": h(cm.cat._p_cstr),
              "cat.ep_viol": h(cm._ep_viol), "cat.ep_prob": h(cm._ep_prob), "cat.prob_buf": h(cm._cstr_prob_buf),
              "cat.log_ring": h(cm._log_ring), "episode_length_buf": h(e.episode_length_buf), "reset_buf": h(e.reset_buf),
              "sim.cur": h(e.sim.cur)})
    mp = term_max_p(env)
    s["max_p"] = np.array(list(mp.values()), np.float64)
    s["host"] = np.array([tr.iteration, tr.adam_step, tr.global_step, e.common_step_counter, cm._log_pos,
                          int(cm.cat._p_first)], np.int64)
    s["torch_rng.cpu"], s["torch_rng.device"] = h(torch.get_rng_state()), h(torch.cuda.get_rng_state(tr.device))
    return s


def run_arm(interval, iters=6, **over):
    env, eval_env, tr = build(eval_interval=interval, iters=iters, **over)
    captures = [0]
    begin = tr.nat.graph_begin

    def counting_begin():
        captures[0] += 1
        return begin()
    tr.nat.graph_begin = counting_begin
    snaps, graph_ids = [], []
    try:
        for _ in range(iters):
            tr.run_iteration()
            snaps.append(snapshot(env, tr))
            graph_ids.append(tr._graph_id)
    finally:
        del tr.nat.graph_begin                       # the instance attribute: the class's method shows again
    return snaps, tr, captures[0], graph_ids


@pytest.mark.parametrize("rng", ["device", "torch"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_evaluations_do_not_disturb_the_run(graph, rng):
    with_eval, tr, captures, graph_ids = run_arm(2, graph_update=graph, rng=rng)
    assert [it for it, _ in tr.evaluator.history] == [0, 2, 4, 6]
    reward = [m["reward_per_step"] for _, m in tr.evaluator.history]
    assert len(set(reward)) == 4, reward                     # the policy moved between any two: they were evaluated, not cached
    without, tr0, captures0, graph_ids0 = run_arm(0, graph_update=graph, rng=rng)
    assert tr0.evaluator is None
    for it, (a, b) in enumerate(zip(with_eval, without), 1):
        assert list(a) == list(b)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"iteration {it}: {k}")
    assert tr.graph_fallback is None and tr0.graph_fallback is None
    if graph and rng == "device":
        # captured once, in both runs, and the graph replayed after an evaluation is the one replayed before it
        assert tr.graph_update and captures == 1 and captures0 == 1
        assert graph_ids[0] is not None and len(set(graph_ids)) == 1 and len(set(graph_ids0)) == 1
    else:                                                    # rng="torch" has no graph, by the trainer's own rule
        assert captures == 0 and captures0 == 0 and set(graph_ids) == {None}


# ------------------------------------------------------------------------------------------------ the trainer's refusals
def test_the_trainer_refuses_what_it_cannot_evaluate():
    from cat_envs.shim import load_cfg_from_registry, make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    env_cfg, agent_cfg = cfgs(eval_interval=2)
    env = make(T.TASK, cfg=env_cfg)
    with pytest.raises(ValueError, match="eval env"):
        PPOTrainer(env, agent_cfg)
    with pytest.raises(ValueError, match="training env"):
        PPOTrainer(env, agent_cfg, eval_env=env)
    stream_cfg = load_cfg_from_registry("Isaac-Velocity-CaT-Flat-Solo12-v0", "env_cfg_entry_point")
    stream_cfg.scene.num_envs = EVAL_ENVS
    with pytest.raises(TypeError):
        PPOTrainer(env, agent_cfg, eval_env=make("Isaac-Velocity-CaT-Flat-Solo12-v0", cfg=stream_cfg))
    agent_cfg.eval_interval = 0                              # off: an eval env or none, nobody asks
    assert PPOTrainer(env, agent_cfg).evaluator is None


# ------------------------------------------------------------------------------------------------ 3, 4: one run, its files
@pytest.fixture(scope="module")
def run_of_six(tmp_path_factory):
    """PPO() for 6 iterations, evaluated after every one, a model written after every one"""
    from cat_envs.tasks.utils.cleanrl.periodic_eval import read_history
    from cat_envs.tasks.utils.cleanrl.ppo import PPO
    root = tmp_path_factory.mktemp("periodic")
    env_cfg, agent_cfg = cfgs(eval_interval=1, save_interval=1, save_state=False)
    run = root / "logs" / "clean_rl" / agent_cfg.experiment_name / "run0"
    env, eval_env = make_envs(env_cfg, agent_cfg)
    torch.manual_seed(int(env_cfg.seed))
    trainer = PPO(env, agent_cfg, str(run), eval_env=eval_env)
    return dict(root=root, run=run, history=read_history(str(run)), trainer=trainer, agent_cfg=agent_cfg)


def test_history_lines_equal_stand_alone_evaluations(run_of_six):
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.evaluate import COMMAND_RANGES, command_grid, evaluate_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import HISTORY_KEYS, make_eval_env_cfg
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    run, history = run_of_six["run"], run_of_six["history"]
    assert [h["iteration"] for h in history] == [0, 1, 2, 3, 4, 5, 6] and all(tuple(h) == HISTORY_KEYS for h in history)
    assert all(h["device_ms"] > 0 for h in history)
    assert len({json.dumps(h["max_p"]) for h in history[1:]}) == 6          # the curriculum moved between any two
    axes = [(lo, hi, n) for (lo, hi), n in zip(COMMAND_RANGES, EVAL_GRID)]
    tab = command_grid(*axes, num_envs=EVAL_ENVS)[0]
    for h in history[1:]:
        it = h["iteration"]
        env = make(T.TASK, cfg=make_eval_env_cfg(cfgs()[0], EVAL_ENVS))        # a fresh env of the same eval cfg
        agent = Agent(env, hidden=HIDDEN)
        agent.load_state_dict(torch.load(run / f"model_{it}.pt", map_location=agent.flat.device))
        cm = env.unwrapped.constraint_manager
        assert list(h["max_p"]) == list(cm.active_terms)
        for name, p in h["max_p"].items():
            cfg = cm.get_term_cfg(name)
            cfg.max_p = p
            cm.set_term_cfg(name, cfg)
        res = evaluate_policy(env, agent, EVAL_STEPS, commands=tab, deterministic=True, fresh_cat_state=True)
        want = json.loads(json.dumps(res.metrics))
        assert list(h["metrics"]) == list(want)
        for k in want:
            assert h["metrics"][k] == want[k], (it, k, h["metrics"][k], want[k])
        assert h["by_command"] == json.loads(json.dumps(res.by_command())) and len(h["by_command"]) == 4
        assert h["metrics"]["steps"] == EVAL_ENVS * EVAL_STEPS and h["metrics"]["episodes"] >= 2 * EVAL_ENVS


def test_the_writer_carries_the_eval_scalars(run_of_six):
    path = run_of_six["run"] / "scalars.jsonl"
    if not path.exists():                                    # tensorboard is installed: the scalars went to its event file
        assert any(f.startswith("events.out.tfevents") for f in os.listdir(run_of_six["run"]))
        return
    rows = [json.loads(line) for line in open(path)]
    for h in run_of_six["history"]:
        got = {r["key"]: r["value"] for r in rows if r["step"] == h["iteration"] and r["key"].startswith("Eval/")}
        want = {"Eval/" + k: v for k, v in h["metrics"].items() if v is not None}
        want["Eval/device_ms"] = h["device_ms"]
        assert got == want


def test_best_names_the_arg_max_and_play_loads_it(run_of_six, monkeypatch, capsys):
    run, history = run_of_six["run"], run_of_six["history"]
    values = [h["metrics"]["reward_per_step"] for h in history]
    arg_max = values.index(max(values))                      # the first of equals
    best = json.load(open(run / "eval" / "best.json"))
    assert best == {"iteration": arg_max, "metric": "reward_per_step", "value": values[arg_max]}
    assert run_of_six["trainer"].evaluator.tracker.summary() == \
        f"[EVAL] best reward_per_step {values[arg_max]:.6g} at iteration {arg_max}"
    assert not [f for _, _, fs in os.walk(run) for f in fs if f.endswith(".tmp")]
    got = torch.load(run / "model_best.pt", map_location="cpu")
    if arg_max > 0:                                          # (iteration 0 has no model_<it>.pt: nothing was trained yet)
        want = torch.load(run / f"model_{arg_max}.pt", map_location="cpu")
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    # play.py, in this process (its own command line; it looks for logs/ under the working directory)
    sys.path.insert(0, os.path.join(ROOT, "scripts", "clean_rl"))
    try:
        import play
    finally:
        sys.path.pop(0)
    monkeypatch.chdir(run_of_six["root"])
    parse = play.cli_args.parse_clean_rl_cfg

    def parse_with_this_runs_widths(task, args):             # play.py takes the widths from the task's cfg: no flag for them
        cfg = parse(task, args)
        cfg.hidden = HIDDEN
        return cfg
    monkeypatch.setattr(play.cli_args, "parse_clean_rl_cfg", parse_with_this_runs_widths)
    play.main([f"--task={T.TASK}", "--headless", "--num_envs", "16", "--video_length", "2", "--checkpoint", "model_best.pt"])
    out = capsys.readouterr().out
    assert "model_best.pt" in out and "mean reward per step" in out


# ------------------------------------------------------------------------------------------------ 5: resume
def test_a_resumed_run_continues_history_and_best(tmp_path):
    """save_interval = 2 writes model_3.pt / state_3.pt; one run of iterations 1..6 against 3 + resume + 3"""
    from cat_envs.tasks.utils.cleanrl.periodic_eval import read_history
    from cat_envs.tasks.utils.cleanrl.ppo import PPO

    def run(path, **kw):
        env_cfg, agent_cfg = cfgs(eval_interval=1, save_interval=2)
        env, eval_env = make_envs(env_cfg, agent_cfg)
        torch.manual_seed(int(env_cfg.seed))
        tr = PPO(env, agent_cfg, str(path), eval_env=eval_env, **kw)
        return read_history(str(path)), tr
    whole, _ = run(tmp_path / "whole")
    first, _ = run(tmp_path / "first", stop_after=3)
    assert os.path.isfile(tmp_path / "first" / "state_3.pt")
    second, tr = run(tmp_path / "second", resume_state=str(tmp_path / "first" / "state_3.pt"))
    assert [h["iteration"] for h in whole] == [0, 1, 2, 3, 4, 5, 6]
    assert [h["iteration"] for h in first] == [0, 1, 2, 3] and [h["iteration"] for h in second] == [4, 5, 6]
    for a, b in zip(whole[:4], first):
        assert _no_device_ms(a) == _no_device_ms(b)
    for a, b in zip(whole[4:], second):                      # exactly: every key but the measured time
        assert _no_device_ms(a) == _no_device_ms(b), a["iteration"]
    best = [json.load(open(tmp_path / d / "eval" / "best.json")) for d in ("whole", "second")]
    assert best[0] == best[1]
    a = torch.load(tmp_path / "whole" / "model_best.pt", map_location="cpu")
    b = torch.load(tmp_path / "second" / "model_best.pt", map_location="cpu")
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    carried = json.load(open(tmp_path / "first" / "eval" / "best.json"))
    assert carried["iteration"] <= 3 and best[1]["value"] >= carried["value"]


# ------------------------------------------------------------------------------------------------ 6: learning in the curve
def test_learning_shows_in_the_curve(tmp_path):
    """``servo_twin.learning_cfgs()`` for 30 iterations, evaluated at 0 and 30 with the size of ``servo_eval_twin.EVAL``:
    at least half of the gain in reward per step and of the drop in rms linear tracking error that the CPU oracle's
    recorded run shows (profiles/servo_eval_oracle.json; half: the seed-to-seed allowance of the learning tests)"""
    from cat_envs.tasks.utils.cleanrl.periodic_eval import read_history
    from cat_envs.tasks.utils.cleanrl.ppo import PPO
    with open(os.path.join(ROOT, E.EVAL_PROFILE)) as f:
        rec = json.load(f)
    assert rec["reward_gain"] > 0.2 and rec["err_lin_drop"] > 0.1, "the recorded run itself must show learning"
    env_cfg, agent_cfg = T.learning_cfgs()
    agent_cfg.num_iterations = T.LEARNING["iterations"]
    agent_cfg.eval_interval, agent_cfg.eval_envs = 30, E.EVAL["num_envs"]
    agent_cfg.eval_steps, agent_cfg.eval_grid = E.EVAL["steps"], tuple(E.EVAL["grid"])
    assert T.LEARNING["iterations"] == 30
    env, eval_env = make_envs(env_cfg, agent_cfg, episode_length=500)          # the task's own 10 s episodes
    assert eval_env.unwrapped.max_episode_length == env.unwrapped.max_episode_length
    torch.manual_seed(int(env_cfg.seed))
    PPO(env, agent_cfg, str(tmp_path), eval_env=eval_env)
    history = read_history(str(tmp_path))
    assert [h["iteration"] for h in history] == [0, 30]
    before, after = history[0]["metrics"], history[1]["metrics"]
    got = E.eval_summary(before, after)
    print(got, before, after, [h["device_ms"] for h in history])
    assert before["steps"] == after["steps"] == E.EVAL["num_envs"] * E.EVAL["steps"]
    assert got["reward_gain"] >= 0.5 * rec["reward_gain"], (got, rec["reward_gain"])
    assert got["err_lin_drop"] >= 0.5 * rec["err_lin_drop"], (got, rec["err_lin_drop"])
    best = json.load(open(tmp_path / "eval" / "best.json"))
    assert best["iteration"] == 30 or best["value"] == after["reward_per_step"]
