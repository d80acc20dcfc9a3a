"""Evaluation inside a training run: ``Eval/*`` curves, ``<run>/eval/history.jsonl`` and ``model_best.pt``.

Every ``eval_interval`` iterations (and once before the first) the trainer's own ``Agent`` is rolled out, deterministic, on a
DEDICATED env for ``eval_steps`` control steps on a fixed command grid (``evaluate.evaluate_policy`` with a fresh CaT
state: a pure function of parameters, observation normaliser, ``max_p``, env cfg and seed, steps and commands).  DESIGN
section 11.

Two halves.  Schedule, best-tracking and the file formats are plain Python - no device, no ``cat_envs.native``, torch only
where a policy file is written - the way ``checkpoint.py`` is, so they run on a CPU.  ``PeriodicEvaluator`` alone touches the
device; it belongs to one ``PPOTrainer``.

Files of a run with evaluations::

    <run>/eval/history.jsonl   one line per evaluation: {"iteration", "metrics", "by_command", "max_p", "device_ms"}
    <run>/eval/best.json       {"iteration", "metric", "value"} of the best evaluation so far
    <run>/model_best.pt        ``agent.state_dict()`` of that iteration (what ``play.py --checkpoint model_best.pt`` loads)

``model_best.pt`` is written before ``best.json``, both through ``.tmp`` and a rename: ``best.json`` never names a policy
that is not there, and a killed run leaves no partial file.
"""
from __future__ import annotations

import copy
import json
import math
import os
import shutil

HISTORY = os.path.join("eval", "history.jsonl")
BEST_JSON = os.path.join("eval", "best.json")
BEST_MODEL = "model_best.pt"
HISTORY_KEYS = ("iteration", "metrics", "by_command", "max_p", "device_ms")

#: seed of the eval env = (training env seed + EVAL_SEED_OFFSET) mod 2^31: a prime far above any env count, so the eval
#: env's draws (keyed on seed and env id) never coincide with those of a training env of a neighbouring seed
EVAL_SEED_OFFSET = 1_000_003

#: the keys of ``evaluate.aggregate`` (a test holds the two together); ``violation_share/<term>`` come on top
METRICS = ("steps", "episodes", "fall_rate", "reward_per_step", "cat_reward_per_step", "rms_err_lin", "rms_err_yaw",
           "mean_tilt2", "mean_torque2", "mean_feet", "episode_return_mean", "episode_length_mean", "termination_prob_mean")

SHARDED_EVAL = ("periodic evaluation of env-sharded runs (world > 1) is not implemented: every rank would evaluate the same "
                "replicated policy, and nothing here can test more than two ranks on one device")


def eval_seed(train_seed: int) -> int:
    return (int(train_seed) + EVAL_SEED_OFFSET) % 2 ** 31


# ------------------------------------------------------------------------------------------------ settings
class EvalSettings:
    """the ``eval_*`` / ``save_best`` fields of a runner cfg, checked (``ValueError``); a cfg without them is "off" """

    def __init__(self, interval=0, envs=256, steps=200, grid=(4, 4, 2), metric="reward_per_step", save_best=True):
        self.interval, self.envs, self.steps = int(interval), int(envs), int(steps)
        try:
            self.grid = tuple(int(g) for g in grid)
        except TypeError:
            raise ValueError(f"eval_grid must be three point counts (vx, vy, wz), got {grid!r}") from None
        self.metric, self.save_best = str(metric), bool(save_best)
        if self.interval < 0:
            raise ValueError(f"eval_interval must be >= 0 (0 = never), got {self.interval}")
        if self.interval == 0:
            return
        if self.envs < 1:
            raise ValueError(f"eval_envs must be >= 1, got {self.envs}")
        if not 1 <= self.steps <= 2 ** 24:
            raise ValueError(f"eval_steps must be in [1, 2^24], got {self.steps}")
        if len(self.grid) != 3 or min(self.grid) < 1:
            raise ValueError(f"eval_grid must be three point counts >= 1 (vx, vy, wz), got {grid!r}")
        if self.metric not in METRICS and not self.metric.startswith("violation_share/"):
            raise ValueError(f"eval_metric '{self.metric}' is not a metric of the evaluator: one of {list(METRICS)} or "
                             "'violation_share/<term>'")

    @classmethod
    def from_cfg(cls, cfg) -> "EvalSettings":
        d = cls()
        return cls(getattr(cfg, "eval_interval", d.interval), getattr(cfg, "eval_envs", d.envs),
                   getattr(cfg, "eval_steps", d.steps), getattr(cfg, "eval_grid", d.grid),
                   getattr(cfg, "eval_metric", d.metric), getattr(cfg, "save_best", d.save_best))

    @property
    def on(self) -> bool:
        return self.interval > 0


# ------------------------------------------------------------------------------------------------ schedule
def due_before(iteration_done: int, interval: int) -> bool:
    """evaluate before the next iteration?  Only a run that has completed none: the record of iteration 0.  A resumed run
    stands at ``iteration_done > 0`` and does not repeat it."""
    return interval > 0 and int(iteration_done) == 0


def due_after(it: int, interval: int) -> bool:
    """evaluate after iteration ``it``?  Counted in absolute iterations, so a resumed run keeps the grid."""
    return interval > 0 and int(it) > 0 and int(it) % interval == 0


def scheduled(iteration_done: int, last: int, interval: int) -> list:
    """the iterations a run that stands at ``iteration_done`` and goes on to ``last`` records"""
    out = [0] if due_before(iteration_done, interval) else []
    return out + [it for it in range(int(iteration_done) + 1, int(last) + 1) if due_after(it, interval)]


# ------------------------------------------------------------------------------------------------ files
def _atomic(path: str, write) -> str:
    """``write(file)`` into ``path + ".tmp"``, flush, fsync, rename: ``path`` is whole or absent, never partial"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            write(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def history_record(iteration: int, metrics: dict, by_command: list, max_p: dict, device_ms: float) -> dict:
    return {"iteration": int(iteration), "metrics": dict(metrics), "by_command": list(by_command),
            "max_p": {k: float(v) for k, v in max_p.items()}, "device_ms": float(device_ms)}


def append_history(run_dir: str, record: dict) -> str:
    """one JSON line (floats by ``repr``: they come back as the same doubles; a ratio without a divisor is ``null``)"""
    missing = [k for k in HISTORY_KEYS if k not in record]
    if missing:
        raise ValueError(f"evaluation record lacks {missing}")
    path = os.path.join(run_dir, HISTORY)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    line = json.dumps(record)
    assert "\n" not in line
    with open(path, "a") as f:
        f.write(line + "\n")
        f.flush()
    return path


def read_history(run_dir: str) -> list:
    path = os.path.join(run_dir, HISTORY)
    if not os.path.isfile(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def read_best(run_dir: str):
    """``best.json`` of a run, or None unless it AND ``model_best.pt`` are there"""
    path = os.path.join(run_dir, BEST_JSON)
    if not (os.path.isfile(path) and os.path.isfile(os.path.join(run_dir, BEST_MODEL))):
        return None
    with open(path) as f:
        best = json.load(f)
    return {"iteration": int(best["iteration"]), "metric": str(best["metric"]), "value": float(best["value"])}


def carry_over(src_run: str, dst_run: str, upto_iteration: int | None = None):
    """A resumed run starts from the best of the run it continues: copy ``model_best.pt`` and ``eval/best.json`` of
    ``src_run`` into ``dst_run`` (policy first, each through ``.tmp``) and return the record; None, and nothing copied, when
    ``src_run`` has no complete pair - or when its best is from an iteration after ``upto_iteration``, the iteration the
    run state was saved at: that policy belongs to a stretch of the old run which the resumed run computes again."""
    best = read_best(src_run)
    if best is None or (upto_iteration is not None and best["iteration"] > int(upto_iteration)):
        return None
    for name in (BEST_MODEL, BEST_JSON):
        src = os.path.join(src_run, name)
        with open(src, "rb") as s:
            _atomic(os.path.join(dst_run, name), lambda f: shutil.copyfileobj(s, f))
    return best


class BestTracker:
    """The best evaluation so far by one metric: strictly greater wins, so ties keep the earlier iteration; an evaluation
    whose metric is None (no episode ended) or NaN never wins.  With ``run_dir`` and ``save_best`` it keeps the two files; it
    starts from the ``best.json`` it finds there (``carry_over``), provided that one is about the same metric."""

    def __init__(self, run_dir: str | None, metric: str, save_best: bool = True):
        self.run_dir, self.metric, self.save_best = run_dir, str(metric), bool(save_best)
        self.best = None
        self.load()

    def load(self):
        found = read_best(self.run_dir) if self.run_dir is not None else None
        if found is not None and found["metric"] == self.metric:
            self.best = found
        return self.best

    def offer(self, iteration: int, metrics: dict, write_model=None) -> bool:
        """``write_model(file)`` writes the policy of this iteration; called only when it is the new best"""
        if self.metric not in metrics:
            raise KeyError(f"eval_metric '{self.metric}' is not among the evaluator's metrics {sorted(metrics)}")
        value = metrics[self.metric]
        if value is None or math.isnan(float(value)):
            return False
        if self.best is not None and not float(value) > self.best["value"]:
            return False
        best = {"iteration": int(iteration), "metric": self.metric, "value": float(value)}
        if self.save_best and self.run_dir is not None:
            if write_model is not None:
                _atomic(os.path.join(self.run_dir, BEST_MODEL), write_model)
            text = json.dumps(best) + "\n"
            _atomic(os.path.join(self.run_dir, BEST_JSON), lambda f: f.write(text.encode()))
        self.best = best                     # only once the files say so too
        return True

    def summary(self) -> str | None:
        if self.best is None:
            return None
        return f"[EVAL] best {self.metric} {self.best['value']:.6g} at iteration {self.best['iteration']}"


# ------------------------------------------------------------------------------------------------ the eval env
def check_setup(settings: EvalSettings, eval_env, train_env=None, world: int = 1) -> bool:
    """what a trainer checks when it is constructed; True when evaluations are on"""
    if not settings.on:
        return False
    if int(world) > 1:
        raise NotImplementedError(SHARDED_EVAL)
    if eval_env is None:
        raise ValueError(f"eval_interval={settings.interval} needs an eval env: PPOTrainer(..., eval_env=...) / "
                         "PPO(..., eval_env=...), see periodic_eval.make_eval_env")
    u = eval_env.unwrapped
    if train_env is not None and u is train_env.unwrapped:
        raise ValueError("the eval env must not be the training env: an evaluation resets the env it runs on")
    if not hasattr(u, "set_eval_record"):
        raise TypeError("periodic evaluation needs a CaTEnv")
    u.set_eval_record(None)                    # TypeError on the open-loop stream simulator, like evaluate_policy
    if train_env is not None:
        have = [list(getattr(getattr(e.unwrapped, "constraint_manager", None), "active_terms", [])) for e in (train_env, eval_env)]
        if have[0] != have[1]:
            raise ValueError(f"the eval env's constraint terms {have[1]} are not the training env's {have[0]}")
    return True


def make_eval_env_cfg(env_cfg, eval_envs: int):
    """the eval env's cfg: a deep copy of the training env's (the same task, simulator constants and constraint terms - as
    objects of its own: the curriculum writes ``max_p`` INTO term cfgs) with ``eval_envs`` envs starting at global env 0, NO
    curriculum (``max_p`` comes from the training env before every evaluation) and the seed ``eval_seed(training seed)``"""
    cfg = copy.deepcopy(env_cfg)
    cfg.scene.num_envs = int(eval_envs)
    if hasattr(cfg.scene, "env_offset"):
        cfg.scene.env_offset = 0
    cfg.seed = eval_seed(int(getattr(env_cfg, "seed", 0) or 0))
    cfg.curriculum = None
    obs = getattr(cfg, "observations", None)
    if obs is not None:                          # Eval/* is measured without sensor noise: a clean, comparable yardstick
        group = obs["policy"] if isinstance(obs, dict) else obs.policy
        if isinstance(group, dict):
            group["enable_corruption"] = False
        else:
            group.enable_corruption = False
    if getattr(cfg, "events", None) is not None:  # ... and without pushes, randomised first states or traction, likewise
        cfg.events = None
    if getattr(cfg, "terminations", None) is not None:   # ... and with the built-in episode ends, whatever the block says
        cfg.terminations = None
    return cfg


def make_eval_env(task: str, env_cfg, eval_envs: int, **make_kwargs):
    """the eval env of a training env made from ``env_cfg``; torch's generator states are as before afterwards"""
    import torch
    from cat_envs.shim import make
    with torch_rng_preserved(torch.device(getattr(env_cfg.sim, "device", "cuda:0"))):
        return make(task, cfg=make_eval_env_cfg(env_cfg, eval_envs), **make_kwargs)


class torch_rng_preserved:
    """CPU and device generator states saved on entry, restored on exit (host-side state: no device synchronisation)"""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        import torch
        self._cpu = torch.get_rng_state()
        self._dev = torch.cuda.get_rng_state(self.device) if torch.cuda.is_available() else None
        return self

    def __exit__(self, *exc):
        import torch
        torch.set_rng_state(self._cpu)
        if self._dev is not None:
            torch.cuda.set_rng_state(self._dev, self.device)
        return False


def copy_max_p(train_env, eval_env) -> dict:
    """every term's current ``max_p`` of the training env into the eval env (through ``set_term_cfg``: the next launch
    carries it); returns it by term name"""
    src, dst = train_env.unwrapped.constraint_manager, eval_env.unwrapped.constraint_manager
    out = {}
    for name in src.active_terms:
        cfg = dst.get_term_cfg(name)
        cfg.max_p = out[name] = float(src.get_term_cfg(name).max_p)
        dst.set_term_cfg(name, cfg)
    return out


# ------------------------------------------------------------------------------------------------ the device part
class PeriodicEvaluator:
    """Owned by one ``PPOTrainer``.  ``evaluate(it)`` runs on whatever stream is current - the trainer calls it on its own,
    after the update of the iteration - and costs that iteration one drain of the stream (the first copy of the results
    to the host; the later ones and the event query find the device idle).  It creates no ``Agent`` and no tensor the
    trainer reads, touches neither the training env nor the device iteration state, and leaves torch's generators as they
    were; the forward of ``rows`` rows fits the workspace the trainer reserved before its first graph capture."""

    def __init__(self, trainer, eval_env, settings: EvalSettings, run_path=None, writer=None):
        import torch
        from .evaluate import COMMAND_RANGES, command_grid
        self.trainer, self.env, self.settings = trainer, eval_env, settings
        self.run_path, self.writer = run_path, writer
        self.interval, self.steps = settings.interval, settings.steps
        self.rows = int(eval_env.unwrapped.num_envs)
        axes = [(lo, hi, n) for (lo, hi), n in zip(COMMAND_RANGES, settings.grid)]
        self.commands = torch.from_numpy(command_grid(*axes, num_envs=self.rows)[0]).to(eval_env.unwrapped.device)
        self.tracker = BestTracker(run_path, settings.metric, settings.save_best)
        self.history = []                       # this process's evaluations: (iteration, metrics)
        self.device_ms = []                     # ... and what each of them took on the device

    def carry_over_from(self, src_run: str):
        """a resumed run: the best of the run it continues, up to the iteration the trainer stands at"""
        best = None
        if self.run_path is not None and self.settings.save_best:
            best = carry_over(src_run, self.run_path, upto_iteration=self.trainer.iteration)
            self.tracker.load()
        return best

    def evaluate(self, it: int) -> dict:
        import torch
        from .evaluate import evaluate_policy
        t = self.trainer
        with torch_rng_preserved(t.device):
            max_p = copy_max_p(t.envs, self.env)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            res = evaluate_policy(self.env, t.agent, self.steps, commands=self.commands, deterministic=True,
                                  fresh_cat_state=True)
            end.record()
            end.synchronize()
            device_ms = float(start.elapsed_time(end))
        rec = history_record(it, res.metrics, res.by_command(), max_p, device_ms)
        self.history.append((int(it), rec["metrics"]))
        self.device_ms.append(device_ms)
        if self.run_path is not None:
            append_history(self.run_path, rec)
        if self.writer is not None:
            for key, value in rec["metrics"].items():
                if isinstance(value, (int, float)) and not isinstance(value, bool):
                    self.writer.add_scalar("Eval/" + key, value, it)
            self.writer.add_scalar("Eval/device_ms", device_ms, it)
        self.tracker.offer(it, rec["metrics"], lambda f: torch.save(t.agent.state_dict(), f))
        return rec
