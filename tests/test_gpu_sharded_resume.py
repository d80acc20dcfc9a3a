"""An env-sharded run that is stopped and resumed computes the bytes of the run that was never interrupted, on every rank
(``PPOTrainer.save_state / load_state`` with ``world > 1``): one file per rank, committed as a set.

Two ranks share ``cuda:0`` and exchange through gloo (tests/dist_resume_worker.py, the harness of
tests/test_gpu_two_rank_trainer.py).  A case is three launches of fresh processes, 6 iterations with the save after
iteration 3: A1 with run states on, A2 with run states off (the control: a sharded run repeats itself and saving disturbs
nothing), B = new processes, new env, new trainer, load A1's ``state_3.pt`` set, iterations 4 - 6.  Every rank snapshots
after each of iterations 4, 5, 6; per rank A1 = A2 = B with ``assert_array_equal`` - bytes, no tolerance - and inside every
arm the two ranks hold the same parameters and moments.

Shapes: stream task, 65 envs = shards of 33 / 32 (ragged: the minibatch plan gives 2 minibatches of 132 / 128 rows and
scaled losses), T = 8, hidden (64, 64), 2 epochs, episodes of 7 steps, six terms, linear anneal, fused env step; servo task,
2 x 32 envs with env offsets 0 / 32, three terms with the curriculum a quarter of its way at the save, KL-adaptive rate;
stream once more with ``rng="torch"``, the unfused env step and the eager update."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import dist_resume_worker as D
import test_gpu_resume as R
from dist_trainer_worker import shard_sizes

pytestmark = pytest.mark.gpu

WORLD = 2
#: seconds one two-process launch may take before it counts as hung.  Observed on an MI355X: 2.3 - 3.9 s per launch (process
#: start dominates), 8 - 10 s per resume case, 7.6 s for the three train.py pairs; the limit leaves room for a cold file cache
LAUNCH_LIMIT_S = 120
SAVE_AT, ITERS = D.SAVE_AT, D.ITERS


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(out_dir, spec):
    """two fresh rank processes; every one joined under the limit, a non-zero exit code fails the test"""
    ctx = mp.get_context("spawn")
    port = _free_port()
    t0 = time.monotonic()
    procs = [ctx.Process(target=D.rank_main, args=(r, WORLD, port, str(out_dir), spec)) for r in range(WORLD)]
    for p in procs:
        p.start()
    deadline = t0 + LAUNCH_LIMIT_S
    for p in procs:
        p.join(timeout=max(deadline - time.monotonic(), 0.0))
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert not hung, f"ranks {hung} were still running after {LAUNCH_LIMIT_S} s ({spec})"
    for r, p in enumerate(procs):
        assert p.exitcode == 0, f"rank {r} exited with {p.exitcode} ({spec})"
    print(f"[sharded resume] launch {spec.get('arm', spec['mode'])} {spec.get('case', '')}: {time.monotonic() - t0:.1f} s")


def _snaps(npz, it):
    pre = f"{it}/"
    return {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}


# ------------------------------------------------------------------------------------------------ A1 = A2 = B
@pytest.mark.parametrize("case", D.CASES)
def test_sharded_resume_equals_the_uninterrupted_run(tmp_path, case):
    arms = {}
    for arm in ("A1", "A2", "B"):
        spec = dict(mode="arm", arm=arm, case=case, state=str(tmp_path / "run_A1" / f"state_{SAVE_AT}.pt"))
        launch(tmp_path, spec)
        arms[arm] = [np.load(tmp_path / f"{arm}_rank{r}.npz") for r in range(WORLD)]
    # what the launches wrote: the set in rank 0's directory and nowhere else; no state where run states are off
    pts = lambda d: sorted(f for f in os.listdir(tmp_path / d) if f.endswith(".pt"))
    assert pts("run_A1") == [f"model_{SAVE_AT}.pt", f"state_{SAVE_AT}.pt", f"state_{SAVE_AT}.rank1.pt"]
    assert pts("run_A2") == [f"model_{SAVE_AT}.pt"] and pts("run_B") == []
    assert not [d for d in os.listdir(tmp_path) if d.startswith("unused_")]
    assert not [f for f in os.listdir(tmp_path / "run_A1") if f.endswith(".tmp")]
    files = [torch.load(tmp_path / "run_A1" / n, map_location="cpu", weights_only=True)
             for n in (f"state_{SAVE_AT}.pt", f"state_{SAVE_AT}.rank1.pt")]
    sets = [f["trainer"]["set"] for f in files]
    assert [s["rank"] for s in sets] == [0, 1] and all(s["world"] == WORLD for s in sets)
    assert sets[0]["token"] == sets[1]["token"] and len(sets[0]["token"]) == 32
    assert [f["fingerprint"]["rank"] for f in files] == [0, 1] and all(f["fingerprint"]["world"] == WORLD for f in files)
    assert list(files[0]["trainer"]["agent"]) == list(torch.load(tmp_path / "run_A1" / f"model_{SAVE_AT}.pt", map_location="cpu"))
    assert ("torch_rng" in files[1]["trainer"]) == (case == "stream_torch")

    # the paths the case is about were taken
    for r in range(WORLD):
        M, n_mb, fused, graph, last = (int(x) for x in arms["A1"][r]["meta"])
        assert last == ITERS and all(int(arms[a][r]["meta"][4]) == ITERS for a in arms)
        if case == "servo":
            assert (M, n_mb) == (R.MB, R.T * D.N_SERVO // R.MB)
        else:
            n = shard_sizes(D.N_STREAM, WORLD)[r]
            assert (M, n_mb) == ((n * D.T_STREAM + 1) // 2, 2) and fused == int(case == "stream")
            assert list(arms["A1"][r]["mb_rows"]) == [M, n * D.T_STREAM - M]
    assert [int(arms["A1"][r]["meta"][0]) for r in range(WORLD)] == ([R.MB, R.MB] if case == "servo" else [132, 128])

    for r in range(WORLD):
        for it in range(SAVE_AT + 1, ITERS + 1):
            a1, a2, b = (_snaps(arms[a][r], it) for a in ("A1", "A2", "B"))
            assert "cm.host" in a1 and "rollout.obs" in a1 and int(a1["host"][0]) == it
            R.assert_same(a1, a2, f"{case} rank {r}: control A2 against A1 (the sharded run itself is not reproducible, or "
                                  f"saving disturbed it), iteration {it}")
            R.assert_same(a1, b, f"{case} rank {r}: resumed run B against A1, iteration {it}")
    for arm, ranks in arms.items():                              # the replicas never part, resumed or not
        for it in range(SAVE_AT + 1, ITERS + 1):
            for k in ("flat", "exp_avg", "exp_avg_sq", "obs_rms.mean", "obs_rms.var", "value_rms.mean", "value_rms.var"):
                np.testing.assert_array_equal(ranks[0][f"{it}/{k}"], ranks[1][f"{it}/{k}"], err_msg=f"{case} {arm} it {it}: {k}")
    # ... while their shards differ (otherwise rank 1 loading rank 0's shard would go unnoticed)
    assert not np.array_equal(arms["B"][0][f"{ITERS}/rewards"][:, :32], arms["B"][1][f"{ITERS}/rewards"][:, :32])

    # where the schedules stood at the save is where B stood after the load, on every rank
    for r in range(WORLD):
        for k in ("probe/lr", "probe/last_kl", "probe/max_p", "probe/max_p.names"):
            np.testing.assert_array_equal(arms["A1"][r][k], arms["B"][r][k], err_msg=f"{case} rank {r}: {k}")
    p = arms["A1"][0]
    if case == "servo":
        fresh = R.servo_cfgs()
        lr0 = float(fresh[2].learning_rate)
        assert float(p["probe/lr"]) != lr0 and float(p["probe/last_kl"]) != 0.0, (p["probe/lr"], p["probe/last_kl"])
        at_save = dict(zip(p["probe/max_p.names"], p["probe/max_p"]))
        final = dict(zip(arms["B"][0][f"{ITERS}/max_p.names"], arms["B"][0][f"{ITERS}/max_p"]))
        for n in vars(fresh[1].curriculum):                      # max_p has moved by the save, and goes on moving after it
            initial = float(getattr(fresh[1].constraints, n).max_p)
            assert at_save[n] != initial and at_save[n] != final[n], (n, initial, at_save[n], final[n])
            assert at_save[n] == 1 / (20 + 0.25 * (1 / 0.25 - 20)) and final[n] == 1 / (20 + 0.5 * (1 / 0.25 - 20))
    else:
        lr0 = float(R.stream_cfgs()[2].learning_rate)
        assert float(p["probe/lr"]) == pytest.approx((1 - (SAVE_AT - 1) / ITERS) * lr0, rel=1e-6)      # linear anneal, iteration 3 of 6


# ------------------------------------------------------------------------------------------------ save failure, refusals
@pytest.fixture(scope="module")
def guards(tmp_path_factory):
    out = tmp_path_factory.mktemp("sharded_guards")
    launch(out, dict(mode="guards"))
    return out, [json.load(open(out / f"guards_rank{r}.json")) for r in range(WORLD)]


def test_a_save_that_one_rank_cannot_write_fails_on_every_rank_and_leaves_no_file(guards):
    _, res = guards
    for r in range(WORLD):
        msg = res[r]["save_failure"]
        assert msg is not None, f"rank {r} did not raise"
        assert "rank 1: OSError" in msg or "rank 1: PermissionError" in msg, msg
        assert "Permission denied" in msg and "rank 0:" not in msg and "state_1.pt" in msg, msg
        assert res[r]["files_after_failure"] == ["model_1.pt"]                      # no state_1.pt, no sibling, no .tmp
        # the run saves again at the next save iteration
        assert res[r]["files_after_next_save"] == ["model_1.pt", "model_3.pt", "state_3.pt", "state_3.rank1.pt"]


def test_refused_sets_are_refused_by_both_ranks_and_nothing_is_written(guards):
    out, res = guards
    s1, s2 = res[0]["sets"], res[1]["sets"]
    assert s1[0]["token"] == s2[0]["token"] and s1[1]["token"] == s2[1]["token"]      # per save: one token on both ranks
    assert s1[0]["token"] != s1[1]["token"]                                          # per save: a new one
    assert res[1]["second_save_returned"].endswith("state_3.rank1.pt") and res[0]["second_save_returned"].endswith("state_3.pt")
    for r in range(WORLD):
        for attempt, x in res[r]["refusals"].items():
            assert x["raised"] == "ValueError", (r, attempt, x)
            assert "rank 1:" in x["message"] and "rank 0:" not in x["message"], (r, attempt, x["message"])
            assert "nothing was loaded" in x["message"] and os.path.join("attempt_" + attempt, "state_3.pt") in x["message"]
            assert x["changed"] == [], (r, attempt, x["changed"])
        assert res[r]["loaded_iteration"] == SAVE_AT and res[r]["iteration_after_load"] == SAVE_AT + 1
    own = res[1]["refusals"]                                      # the offending rank says what it found
    for field in ("rank: saved 0, this run 1", "num_envs: saved 33, this run 32", "env_seed: saved 42, this run 43"):
        assert field in own["copy_of_rank0"]["message"], own["copy_of_rank0"]["message"]
    assert "state_3.rank1.pt does not exist" in own["deleted"]["message"]
    for r in range(WORLD):                                        # the token: every rank can tell, no rank's own check could
        m = res[r]["refusals"]["other_save"]["message"]
        assert s1[0]["token"] in m and s1[1]["token"] in m and "different saves" in m, m
        assert "state_3.rank1.pt does not exist" in res[r]["refusals"]["deleted"]["message"]


def test_single_process_trainer_refuses_the_sharded_state(guards):
    out, _ = guards
    path = str(out / "run_guards" / "state_3.pt")
    # rank 0's shard as a run of its own: the same env count, seed and shapes - only the world differs
    env, tr = R.build(lambda: D.case_cfgs("stream", 0, WORLD, save_state=True))
    tr.run_iteration()
    torch.cuda.synchronize()
    before = tr.agent.flat.detach().cpu().numpy().copy()
    with pytest.raises(ValueError) as e:
        tr.load_state(path)
    msg = str(e.value)
    assert "world: saved 2, this run 1" in msg and "rank: saved 0, this run '<absent>'" in msg and "2 field(s) differ" in msg, msg
    np.testing.assert_array_equal(before, tr.agent.flat.detach().cpu().numpy())
    assert tr.iteration == 1


# ------------------------------------------------------------------------------------------------ entry point
def test_train_resume_entry_point_two_ranks(tmp_path):
    """two ``train.py`` processes (RANK 0 / 1 of WORLD_SIZE 2 on one device) to the end; stopped after 4 of 6 iterations;
    ``--resume True`` from the stopped pair's ``state_3.pt`` set, in ONE new run directory: the same ``model_5.pt`` and
    the same ``state_5`` set"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "scripts/clean_rl/train.py"), "--task=Isaac-Velocity-CaT-Flat-Solo12-Servo-v0",
           "--headless", "--num_envs", "32", "--num_iterations", "6", "agent.num_iterations=6", "agent.save_interval=2",
           "agent.hidden=[64,64]", "agent.minibatch_size=256"]
    log_root = tmp_path / "logs" / "clean_rl" / "solo12_flat"

    def run(extra, n_runs):
        env = dict(os.environ, WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
                   CATPPO_NATIVE_COMM="0", CATPPO_RANKS_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        t0 = time.monotonic()
        n_pair = len(os.listdir(log_root)) if os.path.isdir(log_root) else 0
        logs = [[tmp_path / f"pair{n_pair}_rank{r}.{s}" for s in ("out", "err")] for r in range(WORLD)]
        procs = []
        for r in range(WORLD):                                    # into files: nobody waits on a full pipe
            with open(logs[r][0], "w") as so, open(logs[r][1], "w") as se:
                procs.append(subprocess.Popen(cmd + extra, cwd=tmp_path, env=dict(env, RANK=str(r)), stdout=so, stderr=se))
        try:
            for p in procs:
                p.wait(timeout=max(t0 + LAUNCH_LIMIT_S - time.monotonic(), 0.1))
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
        outs = [(open(o).read(), open(e).read()) for o, e in logs]
        for r, (p, (so, se)) in enumerate(zip(procs, outs)):
            assert p.returncode == 0, f"rank {r}: " + so[-2000:] + se[-3000:]
        print(f"[sharded resume] train.py pair {extra}: {time.monotonic() - t0:.1f} s")
        runs = sorted(os.listdir(log_root))
        assert len(runs) == n_runs, runs                          # ONE run directory per pair: rank 0's
        return [o[0] for o in outs], log_root / runs[-1]
    pts = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".pt"))
    outs, full = run([], 1)
    assert outs[0].count("Saved model") == 3 and outs[1].count("Saved model") == 0
    assert pts(full) == ["model_1.pt", "model_3.pt", "model_5.pt", "state_3.pt", "state_3.rank1.pt", "state_5.pt",
                         "state_5.rank1.pt"]                                          # keep_states = 2, whole sets
    assert not os.path.exists(full / "params" / "resumed_from.txt")
    outs, stopped = run(["--stop_after", "4"], 2)
    assert pts(stopped) == ["model_1.pt", "model_3.pt", "state_1.pt", "state_1.rank1.pt", "state_3.pt", "state_3.rank1.pt"]
    outs, resumed = run(["--resume", "True"], 3)
    assert "Resuming from " in outs[0] and "state_3.pt at iteration 4" in outs[0] and outs[0].count("Saved model") == 1
    named = open(resumed / "params" / "resumed_from.txt").read().strip()
    assert os.path.isabs(named) and os.path.samefile(named, stopped / "state_3.pt")
    assert pts(resumed) == ["model_5.pt", "state_5.pt", "state_5.rank1.pt"]
    want = torch.load(full / "model_5.pt", map_location="cpu")
    got = torch.load(resumed / "model_5.pt", map_location="cpu")
    assert list(want) == list(got) and len(got) == R.N_KEYS
    for k in want:
        assert torch.equal(want[k], got[k]), k
    for name in ("state_5.pt", "state_5.rank1.pt"):
        a = torch.load(full / name, map_location="cpu", weights_only=True)
        b = torch.load(resumed / name, map_location="cpu", weights_only=True)
        assert torch.equal(a["trainer"]["exp_avg_sq"], b["trainer"]["exp_avg_sq"]), name
        assert torch.equal(a["env"]["sim"]["cur"], b["env"]["sim"]["cur"]), name
        assert a["trainer"]["global_step"] == b["trainer"]["global_step"] and a["fingerprint"] == b["fingerprint"]
    r0 = torch.load(resumed / "state_5.pt", map_location="cpu", weights_only=True)
    r1 = torch.load(resumed / "state_5.rank1.pt", map_location="cpu", weights_only=True)
    assert r0["trainer"]["set"]["token"] == r1["trainer"]["set"]["token"]
    assert (r0["fingerprint"]["env_offset"], r1["fingerprint"]["env_offset"]) == (0, 32)
    assert not torch.equal(r0["env"]["sim"]["cur"], r1["env"]["sim"]["cur"])
