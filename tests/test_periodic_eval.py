"""The plain-Python half of the periodic evaluation (cat_envs/tasks/utils/cleanrl/periodic_eval.py):
schedule, best tracker, file formats, carry-over into a resumed run, construction errors.  No device."""
import json
import os
import types

import pytest

from cat_envs.tasks.utils.cleanrl import periodic_eval as P


# ------------------------------------------------------------------------------------------------ schedule
def test_the_module_needs_no_device_code():
    """what the module imports when it is imported: nothing of the device path (the way checkpoint.py is written)"""
    import ast
    names = []
    for node in ast.parse(open(P.__file__).read()).body:               # module level only: the device half imports lazily
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names.append("." * node.level + (node.module or ""))
    assert sorted(names) == ["__future__", "copy", "json", "math", "os", "shutil"]


def test_fresh_run_records_iteration_zero_then_the_multiples():
    assert P.scheduled(0, 6, 2) == [0, 2, 4, 6]
    assert P.scheduled(0, 7, 3) == [0, 3, 6]
    assert P.scheduled(0, 6, 1) == [0, 1, 2, 3, 4, 5, 6]
    assert P.scheduled(0, 5, 10) == [0]


def test_interval_zero_never_evaluates():
    assert P.scheduled(0, 100, 0) == []
    assert not P.due_before(0, 0) and not any(P.due_after(it, 0) for it in range(0, 50))


def test_resumed_run_keeps_the_grid_and_repeats_nothing():
    """stopped after iteration 4 (evaluated there by the first run), interval 2: the resumed run records 6, 8, ..."""
    assert P.scheduled(4, 10, 2) == [6, 8, 10]
    assert not P.due_before(4, 2)
    assert P.scheduled(0, 4, 2) + P.scheduled(4, 10, 2) == P.scheduled(0, 10, 2)
    assert P.scheduled(3, 10, 2) == [4, 6, 8, 10]             # absolute iterations, not "every second since the resume"
    assert P.scheduled(0, 3, 2) + P.scheduled(3, 10, 2) == P.scheduled(0, 10, 2)


# ------------------------------------------------------------------------------------------------ settings
def test_settings_default_to_off_and_are_checked():
    from cat_envs.tasks.utils.cleanrl.rl_cfg import CleanRlPpoActorCriticCfg
    cfg = CleanRlPpoActorCriticCfg()
    assert (cfg.eval_interval, cfg.eval_envs, cfg.eval_steps, cfg.eval_grid, cfg.eval_metric, cfg.save_best) == \
        (0, 256, 200, (4, 4, 2), "reward_per_step", True)
    s = P.EvalSettings.from_cfg(cfg)
    assert not s.on and s.interval == 0
    assert not P.EvalSettings.from_cfg(types.SimpleNamespace()).on          # a cfg from before these fields
    cfg.eval_interval, cfg.eval_grid = 5, [2, 2, 1]
    s = P.EvalSettings.from_cfg(cfg)
    assert s.on and s.grid == (2, 2, 1) and s.envs == 256 and s.steps == 200
    for bad in (dict(interval=-1), dict(interval=1, envs=0), dict(interval=1, steps=0), dict(interval=1, steps=2 ** 24 + 1),
                dict(interval=1, grid=(2, 2)), dict(interval=1, grid=(2, 0, 1)), dict(interval=1, grid=3),
                dict(interval=1, metric="reward")):
        with pytest.raises(ValueError):
            P.EvalSettings(**bad)
    P.EvalSettings(interval=1, metric="violation_share/joint_torque")
    P.EvalSettings(interval=0, grid=(0,), metric="whatever")                  # off: nothing to check


def test_metric_names_are_the_aggregators():
    import numpy as np
    from cat_envs.tasks.utils.cleanrl.evaluate import FIELDS, aggregate
    m = aggregate(np.zeros((2, len(FIELDS)), np.float32))
    assert tuple(m) == P.METRICS


def test_seed_rule():
    assert P.eval_seed(42) == 42 + 1_000_003 and P.eval_seed(2 ** 31 - 1) == 1_000_002
    assert P.eval_seed(42) != P.eval_seed(43) != 42


# ------------------------------------------------------------------------------------------------ best tracker
def _writer(payload: bytes):
    return lambda f: f.write(payload)


def test_strict_improvement_and_ties_keep_the_earlier_iteration(tmp_path):
    run = str(tmp_path)
    t = P.BestTracker(run, "reward_per_step")
    assert t.best is None and t.summary() is None
    assert t.offer(0, {"reward_per_step": 0.25}, _writer(b"zero"))
    assert not t.offer(1, {"reward_per_step": 0.25}, _writer(b"one"))       # a tie
    assert not t.offer(2, {"reward_per_step": 0.125}, _writer(b"two"))
    assert open(tmp_path / "model_best.pt", "rb").read() == b"zero"
    assert json.load(open(tmp_path / "eval" / "best.json")) == {"iteration": 0, "metric": "reward_per_step", "value": 0.25}
    assert t.offer(3, {"reward_per_step": 0.5}, _writer(b"three"))
    assert not t.offer(4, {"reward_per_step": None}, _writer(b"four"))       # no episode ended: never the best
    assert not t.offer(5, {"reward_per_step": float("nan")}, _writer(b"five"))
    assert open(tmp_path / "model_best.pt", "rb").read() == b"three"
    assert json.load(open(tmp_path / "eval" / "best.json")) == {"iteration": 3, "metric": "reward_per_step", "value": 0.5}
    assert t.summary() == "[EVAL] best reward_per_step 0.5 at iteration 3"
    with pytest.raises(KeyError):
        t.offer(6, {"rms_err_lin": 1.0}, _writer(b"six"))
    assert sorted(os.listdir(tmp_path)) == ["eval", "model_best.pt"] and os.listdir(tmp_path / "eval") == ["best.json"]


def test_a_failing_write_leaves_no_partial_file(tmp_path):
    t = P.BestTracker(str(tmp_path), "reward_per_step")
    t.offer(0, {"reward_per_step": 1.0}, _writer(b"good"))

    def dies(f):
        f.write(b"half a pol")
        raise OSError("disk full")
    with pytest.raises(OSError):
        t.offer(1, {"reward_per_step": 2.0}, dies)
    assert open(tmp_path / "model_best.pt", "rb").read() == b"good"          # the old policy, whole
    assert json.load(open(tmp_path / "eval" / "best.json"))["iteration"] == 0   # and the record that names it
    left = [f for _, _, fs in os.walk(tmp_path) for f in fs]
    assert sorted(left) == ["best.json", "model_best.pt"], left


def test_save_best_off_tracks_but_writes_nothing(tmp_path):
    t = P.BestTracker(str(tmp_path), "reward_per_step", save_best=False)
    assert t.offer(2, {"reward_per_step": 1.0}, _writer(b"x")) and t.best["iteration"] == 2
    assert os.listdir(tmp_path) == []
    assert P.BestTracker(None, "reward_per_step").offer(0, {"reward_per_step": 1.0}, _writer(b"x"))


def test_carry_over_copies_both_files_and_continues_from_the_value(tmp_path):
    old, new = tmp_path / "old", tmp_path / "new"
    os.makedirs(old)
    os.makedirs(new)
    assert P.carry_over(str(old), str(new)) is None and os.listdir(new) == []      # nothing to carry
    t = P.BestTracker(str(old), "reward_per_step")
    t.offer(2, {"reward_per_step": 0.75}, _writer(b"policy of 2"))
    assert P.carry_over(str(old), str(new), upto_iteration=1) is None and os.listdir(new) == []   # from after the save point
    best = P.carry_over(str(old), str(new), upto_iteration=3)
    assert best == {"iteration": 2, "metric": "reward_per_step", "value": 0.75}
    assert open(new / "model_best.pt", "rb").read() == b"policy of 2"
    assert json.load(open(new / "eval" / "best.json")) == best
    assert not [f for _, _, fs in os.walk(new) for f in fs if f.endswith(".tmp")]
    t2 = P.BestTracker(str(new), "reward_per_step")
    assert t2.best == best
    assert not t2.offer(4, {"reward_per_step": 0.75}, _writer(b"policy of 4"))      # a tie with the carried value
    assert open(new / "model_best.pt", "rb").read() == b"policy of 2"
    assert t2.offer(5, {"reward_per_step": 0.875}, _writer(b"policy of 5"))
    assert json.load(open(new / "eval" / "best.json"))["iteration"] == 5
    assert open(old / "model_best.pt", "rb").read() == b"policy of 2"               # the old run is left alone
    assert P.BestTracker(str(new), "rms_err_yaw").best is None                       # another metric: not comparable
    os.remove(old / "model_best.pt")
    assert P.read_best(str(old)) is None                                             # half a pair is no pair


# ------------------------------------------------------------------------------------------------ history
def test_history_lines_round_trip_through_json(tmp_path):
    metrics = {"steps": 512.0, "episodes": 0.0, "fall_rate": None, "reward_per_step": 0.1 + 0.2, "rms_err_lin": 1e-300,
               "violation_share/any": 1 / 3}
    by_command = [{"command": [0.35, 0.0, 0.0], "envs": 8, "metrics": dict(metrics)}]
    recs = [P.history_record(0, metrics, by_command, {"joint_torque": 0.05, "base_orientation": 1 / 7}, 12.625),
            P.history_record(2, dict(metrics, reward_per_step=-0.0), [], {}, 0.0)]
    for r in recs:
        P.append_history(str(tmp_path), r)
    text = open(tmp_path / "eval" / "history.jsonl").read()
    assert text.endswith("\n") and len(text.splitlines()) == 2
    for line, r in zip(text.splitlines(), recs):
        assert tuple(json.loads(line)) == P.HISTORY_KEYS
        assert json.loads(line) == r and json.loads(json.dumps(json.loads(line))) == r
    back = P.read_history(str(tmp_path))
    assert back == recs and back[0]["metrics"]["reward_per_step"] == 0.1 + 0.2 and back[0]["metrics"]["fall_rate"] is None
    assert P.read_history(str(tmp_path / "nowhere")) == []
    with pytest.raises(ValueError):
        P.append_history(str(tmp_path), {"iteration": 3})


# ------------------------------------------------------------------------------------------------ construction errors
class _FakeEnv:
    def __init__(self, kind="servo", terms=("a", "b")):
        self.kind = kind
        self.num_envs = 32
        self.constraint_manager = types.SimpleNamespace(active_terms=list(terms))

    @property
    def unwrapped(self):
        return self

    def set_eval_record(self, record):
        if self.kind != "servo":
            raise TypeError("the evaluation record needs the closed-loop simulator")


def test_construction_errors():
    on, off = P.EvalSettings(interval=2), P.EvalSettings(interval=0)
    train, ev = _FakeEnv(), _FakeEnv()
    assert P.check_setup(on, ev, train, 1) is True
    assert P.check_setup(off, None, train, 1) is False and P.check_setup(off, None, train, 4) is False   # off: no demands
    with pytest.raises(ValueError, match="eval env"):
        P.check_setup(on, None, train, 1)
    with pytest.raises(ValueError, match="training env"):
        P.check_setup(on, train, train, 1)
    with pytest.raises(TypeError):
        P.check_setup(on, _FakeEnv("stream"), train, 1)
    with pytest.raises(TypeError):
        P.check_setup(on, types.SimpleNamespace(unwrapped=object()), train, 1)
    with pytest.raises(NotImplementedError, match="world > 1"):
        P.check_setup(on, ev, train, 2)
    with pytest.raises(ValueError, match="constraint terms"):
        P.check_setup(on, _FakeEnv(terms=("a",)), train, 1)


def test_eval_env_cfg_is_a_copy_with_its_own_terms():
    import servo_twin
    env_cfg, _ = servo_twin.learning_cfgs()
    ev = P.make_eval_env_cfg(env_cfg, 32)
    assert ev.scene.num_envs == 32 and env_cfg.scene.num_envs == 256
    assert ev.seed == P.eval_seed(env_cfg.seed) and ev.curriculum is None and env_cfg.curriculum is not None
    assert list(vars(ev.constraints)) == list(vars(env_cfg.constraints))
    for name, term in vars(env_cfg.constraints).items():
        mine = getattr(ev.constraints, name)
        assert mine is not term and mine.func is term.func and mine.max_p == term.max_p
    ev.constraints.joint_torque.max_p = 0.5
    assert env_cfg.constraints.joint_torque.max_p != 0.5
    assert ev.synthetic.kind == "servo" and ev.episode_length_s == env_cfg.episode_length_s


# ------------------------------------------------------------------------------------------------ front end
def test_train_flags_reach_the_cfg_and_play_keeps_its_own(monkeypatch):
    import argparse
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "scripts", "clean_rl"))
    import cli_args
    import train
    from cat_envs.tasks.utils.cleanrl.rl_cfg import CleanRlPpoActorCriticCfg
    args, rest = train.build_parser().parse_known_args(
        ["--task=X", "--eval_interval", "5", "--eval_envs", "64", "--eval_steps", "50", "--eval_grid", "2", "3", "1",
         "--eval_metric", "rms_err_lin", "agent.hidden=[64,64]"])
    assert rest == ["agent.hidden=[64,64]"]
    cfg = cli_args.update_eval_cfg(CleanRlPpoActorCriticCfg(), args)
    assert (cfg.eval_interval, cfg.eval_envs, cfg.eval_steps, cfg.eval_grid, cfg.eval_metric) == (5, 64, 50, (2, 3, 1), "rms_err_lin")
    assert P.EvalSettings.from_cfg(cfg).on
    none, _ = train.build_parser().parse_known_args(["--task=X"])
    cfg = cli_args.update_eval_cfg(CleanRlPpoActorCriticCfg(), none)
    assert cfg.eval_interval == 0 and cfg.eval_grid == (4, 4, 2)              # no flag: the cfg's "off"
    # play.py has --eval_steps / --eval_grid of its own (one checkpoint): the shared argument group must not claim them
    parser = argparse.ArgumentParser()
    parser.add_argument("--eval_steps", type=int, default=0)
    parser.add_argument("--eval_grid", type=int, nargs=3, default=None)
    cli_args.add_clean_rl_args(parser)
    assert parser.parse_args(["--eval_steps", "7"]).eval_steps == 7
