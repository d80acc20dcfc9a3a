"""What the periodic evaluation costs inside a run  ->  profiles/periodic_eval.json

    python tools/periodic_eval_cost.py --parent TREE [--rounds 7] [--iters 30] [--limit 120]

(a) ``device_ms`` of one evaluation at 256 envs x 200 steps (the HIP event pair of ``PeriodicEvaluator.evaluate``).
(b) wall milliseconds per training iteration of the learning configuration (``servo_twin.learning_cfgs()``), three arms
    alternating in one session: ``parent`` = the Python tree of the parent commit at ``TREE`` (a plain checkout; it runs on
    THIS tree's library - the tool refuses unless csrc/ and include/ of the two trees are byte-identical, which they are
    for a change that adds no kernel), ``off`` = this tree with ``eval_interval = 0``, ``on`` = this tree with
    ``eval_interval = 10``, its evaluations amortised over the iterations.

One long-lived worker process per arm (three processes hold the device, one works at a time); the driver hands out one
round at a time - ``iters`` iterations between two device synchronisations - in the order parent, off, on, parent, ...
Every round has a time limit of its own; a worker that misses it, dies or reports an error ends the session: the others
are stopped, nothing further is started, and the file records what was measured up to there under ``"aborted"``.
"""
import argparse
import hashlib
import json
import os
import queue
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "constraints-as-terminations_amd"
MARK = "@@periodic_eval_cost "
EVAL = dict(eval_envs=256, eval_steps=200, eval_grid=(4, 4, 2))


# ------------------------------------------------------------------------------------------------ worker
def worker(tree: str, interval: int, warmup: int):
    for p in (tree, os.path.join(tree, "tests"), os.path.join(tree, PKG)):
        sys.path.insert(0, p)
    import torch
    import servo_twin as T
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    env_cfg, agent_cfg = T.learning_cfgs()
    agent_cfg.num_iterations = 10 ** 6                       # the anneal does not end inside the measurement
    env = make(T.TASK, cfg=env_cfg)
    kw = {}
    if interval > 0:
        from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env
        agent_cfg.eval_interval = interval
        for k, v in EVAL.items():
            setattr(agent_cfg, k, v)
        kw["eval_env"] = make_eval_env(T.TASK, env_cfg, EVAL["eval_envs"])
    torch.manual_seed(int(env_cfg.seed))
    tr = PPOTrainer(env, agent_cfg, **kw)
    for _ in range(warmup):                                  # graph capture, the evaluation of iteration 0, lazy loads
        tr.run_iteration()
    torch.cuda.synchronize()
    print(MARK + json.dumps({"ready": True, "iteration": tr.iteration}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        n = int(cmd[1])
        seen = len(tr.evaluator.device_ms) if interval > 0 else 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.run_iteration()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = {"ms_per_iteration": 1e3 * dt / n, "iterations": n, "iteration": tr.iteration}
        if interval > 0:
            out["device_ms"] = tr.evaluator.device_ms[seen:]
        print(MARK + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ driver
def _tree_digest(tree: str) -> str:
    h = hashlib.sha256()
    for sub in (os.path.join(PKG, "csrc"), "include"):
        for base, dirs, files in os.walk(os.path.join(tree, sub)):
            dirs.sort()
            for f in sorted(files):
                if f.endswith((".o", ".bc", ".hipfb")):
                    continue
                path = os.path.join(base, f)
                h.update(os.path.relpath(path, tree).encode())
                with open(path, "rb") as fh:
                    h.update(fh.read())
    return h.hexdigest()


class Worker:
    def __init__(self, name, tree, interval, warmup, lib):
        self.name = name
        env = dict(os.environ, CATPPO_LIB=lib, PYTHONUNBUFFERED="1")
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--interval",
                                      str(interval), "--warmup", str(warmup)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, text=True, env=env, cwd=tree)
        self.lines, self.tail = queue.Queue(), []
        threading.Thread(target=self._read, daemon=True).start()

    def _read(self):
        for line in self.proc.stdout:
            self.tail = (self.tail + [line.rstrip()])[-30:]
            if line.startswith(MARK):
                self.lines.put(json.loads(line[len(MARK):]))
        self.lines.put(None)                                 # the process ended

    def answer(self, limit: float):
        try:
            got = self.lines.get(timeout=limit)
        except queue.Empty:
            raise RuntimeError(f"arm '{self.name}' wrote nothing for {limit:.0f} s") from None
        if got is None:
            raise RuntimeError(f"arm '{self.name}' ended (exit {self.proc.wait()}): " + " | ".join(self.tail[-8:]))
        return got

    def ask(self, text: str):
        self.proc.stdin.write(text + "\n")
        self.proc.stdin.flush()

    def stop(self):
        if self.proc.poll() is None:
            try:
                self.ask("quit")
                self.proc.wait(timeout=20)
            except Exception:
                self.proc.kill()
                self.proc.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--interval", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30, help="iterations per round (a multiple of 10: three evaluations in 30)")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a worker may take to start, and for one round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_eval.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.tree, a.interval, a.warmup)
    if a.parent is None or not os.path.isdir(os.path.join(a.parent, PKG)):
        sys.exit("--parent TREE: a checkout of the parent commit is needed for the first arm")
    if a.iters % 10:
        sys.exit("--iters must be a multiple of the evaluation interval (10)")
    parent = os.path.abspath(a.parent)
    if _tree_digest(parent) != _tree_digest(ROOT):
        sys.exit("csrc/ or include/ differ between the two trees: the parent arm needs a library of its own")
    lib = os.path.join(ROOT, PKG, "lib", "libcatppo.so")
    arms = [("parent", parent, 0), ("off", ROOT, 0), ("on", ROOT, 10)]
    rec = {"device": "MI355X", "configuration": "servo_twin.learning_cfgs(): 256 envs x 24 steps, hidden (128, 128)",
           "evaluation": dict(EVAL, eval_grid=list(EVAL["eval_grid"]), eval_interval=10),
           "rounds": a.rounds, "iterations_per_round": a.iters, "warmup_iterations": a.warmup,
           "clock": "host wall clock between two device synchronisations, per round",
           "ms_per_iteration": {name: [] for name, _, _ in arms}, "eval_device_ms": []}
    workers = []
    try:
        for name, tree, interval in arms:                    # started one after the other: a start that fails ends it here
            w = Worker(name, tree, interval, a.warmup, lib)
            workers.append(w)
            w.answer(a.limit)
        for _ in range(a.rounds):
            for w in workers:
                w.ask(f"run {a.iters}")
                got = w.answer(a.limit)
                rec["ms_per_iteration"][w.name].append(got["ms_per_iteration"])
                rec["eval_device_ms"] += got.get("device_ms", [])
    except RuntimeError as e:
        rec["aborted"] = str(e)
        for w in workers:
            if w.proc.poll() is None:
                w.proc.kill()
    finally:
        for w in workers:
            w.stop()
    ms = rec["ms_per_iteration"]
    if "aborted" not in rec:
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec["median_ms_per_iteration"] = med
        rec["parent_spread_ms"] = max(ms["parent"]) - min(ms["parent"])
        rec["off_minus_parent_ms"] = med["off"] - med["parent"]
        rec["amortised_eval_overhead_ms_per_iteration"] = med["on"] - med["off"]
        rec["eval_device_ms_median"] = statistics.median(rec["eval_device_ms"])
        rec["accepted"] = bool(rec["off_minus_parent_ms"] <= rec["parent_spread_ms"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in rec.items() if k not in ("ms_per_iteration", "eval_device_ms")}, indent=1))
    if "aborted" in rec or not rec["accepted"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
