"""Ranks of the env-sharded ``PPOTrainer`` that save, load and refuse run states (tests/test_gpu_sharded_resume.py).

Same harness as ``dist_trainer_worker.rank_main``: the ranks are processes that share ``cuda:0`` and exchange through a gloo
group with host-staged device operands.  ``rank_main`` (spawned per rank) runs one of two bodies:

``arm``     one arm of a resume case - A1 (6 iterations, run states on), A2 (the same, run states off), B (new processes:
            load A1's ``state_3.pt`` set, iterations 4 - 6) - and dumps ``test_gpu_resume.snapshot`` plus the rest of the
            constraint manager's state and of the rollout after each of iterations 4, 5, 6 into ``<arm>_rank<r>.npz``.
``guards``  a save whose rank 1 cannot write, the next save, and three sets that must be refused by both ranks without a
            byte written; what happened goes into ``guards_rank<r>.json``.
Test infrastructure only."""
from __future__ import annotations

import datetime
import json
import os
import shutil

import numpy as np

import dist_trainer_worker as W

N_STREAM, T_STREAM, MB_STREAM = 65, 8, 128       # shards of 33 / 32 envs: 264 / 256 rows, planned as 2 minibatches of 132 / 128
N_SERVO = 32                                     # per rank, env_offset 0 and 32
ITERS, SAVE_AT = 6, 3
CASES = ("stream", "servo", "stream_torch")
#: seconds a rank waits in a gloo collective for its peer before it raises (a peer that died must not cost the join limit)
GROUP_TIMEOUT_S = 60


def rank_main(rank: int, world: int, port: int, out_dir: str, spec: dict):
    W._paths()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CATPPO_NATIVE_COMM="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))
    try:
        {"arm": _arm, "guards": _guards}[spec["mode"]](rank, world, out_dir, spec)
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ cfgs
def case_cfgs(case: str, rank: int, world: int, save_state: bool, save_interval: int = SAVE_AT + 1):
    """fresh (task, env_cfg, agent_cfg) of rank ``rank``: the cfg helpers of tests/test_gpu_resume.py at the sharded shapes"""
    import test_gpu_resume as R
    if case == "servo":
        # ThreeConstraintsCfg, the curriculum a quarter of its way at the save; KL-adaptive rate with a threshold far below
        # the KL of an epoch, so the rate has moved by then
        task, env_cfg, agent_cfg = R.servo_cfgs(lr_schedule="adaptive", kl_threshold=1e-6)
        env_cfg.scene.num_envs, env_cfg.scene.env_offset = N_SERVO, N_SERVO * rank
    else:
        over = dict(minibatch_size=MB_STREAM)
        if case == "stream_torch":
            over.update(rng="torch", fused_rollout=False, graph_update=False)
        task, env_cfg, agent_cfg = R.stream_cfgs(num_envs=W.shard_sizes(N_STREAM, world)[rank], num_steps=T_STREAM,
                                                 seed=42 + rank, **over)
    agent_cfg.save_interval, agent_cfg.save_state = save_interval, save_state
    return task, env_cfg, agent_cfg


def build(cfgs, run_path):
    """(env, trainer) like ``test_gpu_resume.build``, with a run directory"""
    import test_gpu_resume as R
    import torch
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    task, env_cfg, agent_cfg = cfgs
    env = make(task, cfg=env_cfg)
    e = env.unwrapped
    assert e.max_episode_length == R.EP_LEN
    e.episode_length_buf.copy_(torch.arange(e.num_envs, device=e.device) % R.EP_LEN)
    torch.manual_seed(int(env_cfg.seed))
    return env, PPOTrainer(env, agent_cfg, run_path)


def full_snapshot(env, tr, stats) -> dict:
    """``test_gpu_resume.snapshot`` and what it leaves out: the rest of the rollout, and every tensor of the constraint
    manager's state (tiles, episode sums, the log ring and its position)"""
    import test_gpu_resume as R
    import torch
    s = R.snapshot(env, tr, stats)
    h = lambda t: t.detach().cpu().numpy().copy()
    for name in ("obs", "returns", "true_dones", "kl_buf"):
        s["rollout." + name] = h(getattr(tr, name))
    sd = env.unwrapped.constraint_manager.state_dict()
    for k, v in sd.items():
        if isinstance(v, torch.Tensor):
            s["cm." + k] = h(v)
    s["cm.host"] = np.array([int(sd["log_pos"]), int(sd["log_ring_slots"]), int(sd["p_first"])], np.int64)
    return s


def _probe(env, tr) -> dict:
    """where the schedules stand: the device-side rate and last KL, every term's ``max_p``"""
    import test_gpu_resume as R
    import torch
    torch.cuda.synchronize()
    st = tr.nat.iter_state_read(tr.state)
    mp = R.term_max_p(env)
    return {"probe/lr": np.float64(st.lr), "probe/last_kl": np.float64(st.last_kl), "probe/max_p.names": np.array(list(mp)),
            "probe/max_p": np.array(list(mp.values()), np.float64)}


# ------------------------------------------------------------------------------------------------ arms A1, A2, B
def _arm(rank, world, out_dir, spec):
    arm, case = spec["arm"], spec["case"]
    # rank 0's directory is everybody's; the others name one of their own, which must stay unused
    run_dir = os.path.join(out_dir, "run_" + arm) if rank == 0 else os.path.join(out_dir, f"unused_{arm}_rank{rank}")
    if rank == 0:
        os.makedirs(run_dir)
    env, tr = build(case_cfgs(case, rank, world, save_state=arm != "A2"), run_dir)
    assert tr.world == world and tr.rank == rank and tr._state_plan[0] == os.path.join(out_dir, "run_" + arm)
    out, first = {}, 1
    if arm == "B":
        assert tr.iteration == 0 and tr.adam_step == 0
        tr.load_state(spec["state"])                             # rank 0's path, on every rank
        assert tr.iteration == SAVE_AT and tr._graph_id is None
        out.update(_probe(env, tr))
        first = SAVE_AT + 1
    for it in range(first, ITERS + 1):
        stats = tr.run_iteration()
        if it == SAVE_AT:
            out.update(_probe(env, tr))
            assert bool(env.unwrapped.reset_buf.any()), "no env ended an episode in the last step before the save"
        if it > SAVE_AT:
            for k, v in full_snapshot(env, tr, stats).items():
                out[f"{it}/{k}"] = v
    out["meta"] = np.array([tr.M, tr.n_mb, int(tr.sink is not None), int(tr.graph_update), tr.iteration], np.int64)
    out["mb_rows"] = np.asarray(tr._mb_rows, np.int64)
    np.savez(os.path.join(out_dir, f"{arm}_rank{rank}.npz"), **out)


# ------------------------------------------------------------------------------------------------ save failure, refusals
def _guards(rank, world, out_dir, spec):
    import torch.distributed as dist
    from cat_envs.tasks.utils.cleanrl import checkpoint
    run_dir = os.path.join(out_dir, "run_guards")
    if rank == 0:
        os.makedirs(run_dir)
    env, tr = build(case_cfgs("stream", rank, world, save_state=True, save_interval=2), run_dir if rank == 0 else None)
    res = {}
    listing = lambda: (dist.barrier(), sorted(os.listdir(run_dir)), dist.barrier())[1]

    # -- a save whose rank 1 cannot write (iteration 1), then the next save (iteration 3)
    real = checkpoint.write_state
    if rank == 1:
        def refusing(path, payload):
            raise OSError(13, "Permission denied", path)
        checkpoint.write_state = refusing
    try:
        tr.run_iteration()
        res["save_failure"] = None
    except RuntimeError as e:
        res["save_failure"] = str(e)
    finally:
        checkpoint.write_state = real
    res["files_after_failure"] = listing()
    tr.run_iteration()
    tr.run_iteration()
    res["files_after_next_save"] = listing()
    s1 = os.path.join(run_dir, f"state_{SAVE_AT}.pt")

    # -- a second save of the same iteration: same contents, another token
    second = os.path.join(out_dir, "second")
    if rank == 0:
        os.makedirs(second)
    dist.barrier()
    s2 = os.path.join(second, f"state_{SAVE_AT}.pt")
    res["second_save_returned"] = tr.save_state(s2)
    dist.barrier()
    tokens = [checkpoint.read_state(checkpoint.sibling_path(p, rank))["trainer"]["set"] for p in (s1, s2)]
    res["sets"] = tokens

    # -- the sets to refuse, made by rank 0
    attempts = {k: os.path.join(out_dir, "attempt_" + k, f"state_{SAVE_AT}.pt") for k in ("copy_of_rank0", "deleted", "other_save")}
    if rank == 0:
        for k, head in attempts.items():
            os.makedirs(os.path.dirname(head))
            shutil.copy(s1, head)
        shutil.copy(s1, checkpoint.sibling_path(attempts["copy_of_rank0"], 1))
        shutil.copy(checkpoint.sibling_path(s2, 1), checkpoint.sibling_path(attempts["other_save"], 1))
    dist.barrier()

    stats = tr.run_iteration()                                   # iteration 4: nothing here equals the files any more
    before = full_snapshot(env, tr, stats)
    res["refusals"] = {}
    for k, head in attempts.items():
        r = {"raised": None, "message": "", "changed": []}
        try:
            tr.load_state(head)
        except Exception as e:
            r["raised"], r["message"] = type(e).__name__, str(e)
        after = full_snapshot(env, tr, stats)
        r["changed"] = [key for key in before if not np.array_equal(before[key], after[key])] + \
            ([] if list(before) == list(after) else ["<keys>"])
        res["refusals"][k] = r
        dist.barrier()
    # and a whole set still loads afterwards
    tr.load_state(s2)
    res["loaded_iteration"] = int(tr.iteration)
    tr.run_iteration()
    res["iteration_after_load"] = int(tr.iteration)
    with open(os.path.join(out_dir, f"guards_rank{rank}.json"), "w") as f:
        json.dump(res, f)
