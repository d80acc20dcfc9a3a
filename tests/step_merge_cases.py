"""Worker of tests/test_gpu_step_merge.py: every case runs the merged env step (catppo_rollout_defer_tail mode 2: the post
launch rides in the next policy forward) against the separate launches IN THIS PROCESS and records whether every buffer
came out bit-identical.  Started with the 32-row rollout window pinned open (CATPPO_FUSED_FWD_MIN_ROWS=17,
CATPPO_FUSED_FWD_MAX_ROWS=4096, CATPPO_STEP16_FWD=0) so that batches of 17 rows and more take rows_fwd_kernel<32> /
step_fwd_kernel.

    python step_merge_cases.py OUT.json
"""
import json
import sys
import traceback

import numpy as np
import torch

import smoke_impl
from cat_envs.shim import make
from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer

MERGED = "step_fwd_kernel"


def make_trainer(num_envs, num_steps, merge, minibatch=None, epochs=1):
    # (a fresh config per env: the curriculum edits the terms' max_p in place)
    task, env_cfg, agent_cfg = smoke_impl.make_cfgs(num_envs, num_steps, minibatch or num_envs * num_steps, epochs, 5,
                                                    (256, 256, 256), True, obs_dim=48, seed=11)
    env_cfg.episode_length_s = 2 * env_cfg.sim.dt * env_cfg.decimation      # max_episode_length = 2: time-outs every step
    torch.manual_seed(7)
    env = make(task, cfg=env_cfg)
    assert env.unwrapped.max_episode_length == 2
    tr = PPOTrainer(env, agent_cfg)
    assert tr.sink is not None and tr.defer_tail
    tr.step_merge = merge
    return tr, env


def state_of(tr, env):
    eu = env.unwrapped
    cm, rms = eu.constraint_manager, tr.agent.obs_rms
    return dict(mean=rms.running_mean, var=rms.running_var, count=rms.count, rm=cm.cat._p_rm, ep_viol=cm._ep_viol,
                ep_prob=cm._ep_prob, ep_len=eu.episode_length_buf, ring=cm._log_ring)


def buffers_of(tr):
    return dict(obs=tr.obs, actions=tr.actions, logprobs=tr.logprobs, values=tr.values, rewards=tr.rewards,
                dones=tr.dones, true_dones=tr.true_dones)


def snap(d):
    return {k: v.clone() for k, v in d.items()}


def rollout_with_snapshots(num_envs, merge, supplied_eps):
    """four env steps through PPOTrainer.rollout; a snapshot of every buffer and every piece of state in front of and
    behind every env step (in stream order: both arms defer the tail, so both see the same things at the same points),
    and one behind the flush of the rollout's `finally`"""
    T = 4
    tr, env = make_trainer(num_envs, T, merge)
    eu = env.unwrapped
    snaps = []
    real = eu.step_into

    def step_into(action, sink):
        snaps.append(snap({**buffers_of(tr), **state_of(tr, env)}))          # behind policy step s: step s - 1 is complete
        out = real(action, sink)
        # behind the env step only what the deferred tail publishes (in the NEXT step's first launch) is comparable: the
        # step's own outputs exist once the next policy step has carried it - the snapshot above, one step later
        snaps.append(snap({k: v for k, v in state_of(tr, env).items() if k in ("mean", "var", "count", "rm", "ring")}))
        return out
    eu.step_into = step_into
    eps_fn = None
    if supplied_eps:
        g = torch.Generator(device="cpu").manual_seed(5)
        eps = torch.randn(T, num_envs, tr.A, generator=g).to(tr.device)
        eps_fn = lambda s: eps[s]                                             # noqa: E731
    tr.nat.plan_log(1)
    tr.rollout(eps_fn=eps_fn)
    plan = tr.nat.plan_log(0)
    snaps.append(snap({**buffers_of(tr), **state_of(tr, env)}))              # behind the flush
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in s.items()} for s in snaps], plan


def compare(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys()
        for k in x:
            xb, yb = (np.ascontiguousarray(np.atleast_1d(v)).view(np.uint8) for v in (x[k], y[k]))
            np.testing.assert_array_equal(xb, yb, err_msg=f"snapshot {i}: {k}")


def case_steps(num_envs, supplied_eps):
    sep, plan_s = rollout_with_snapshots(num_envs, False, supplied_eps)
    mer, plan_m = rollout_with_snapshots(num_envs, True, supplied_eps)
    assert MERGED not in plan_s, plan_s
    assert plan_m.count(MERGED) == 3, plan_m              # steps 1..3 carry the post of steps 0..2; the last one is flushed
    assert plan_m.count("rollout_post_kernel as a launch of its own") == 1, plan_m
    compare(sep, mer)
    last = mer[-1]
    assert last["true_dones"].max() == 1 and last["dones"].max() == 1 and np.abs(last["ring"]).sum() > 0
    assert float(last["count"]) > 4 * num_envs


def case_iteration():
    res = []
    for merge in (False, True):
        tr, env = make_trainer(64, 24, merge, minibatch=512, epochs=2)
        tr.nat.plan_log(1)
        tr.run_iteration(log=False)
        plan = tr.nat.plan_log(0)
        torch.cuda.synchronize()
        assert (MERGED in plan) == merge, plan
        res.append({**{k: v.cpu().numpy() for k, v in state_of(tr, env).items()}, "flat": tr.agent.flat.cpu().numpy(),
                    "adv": tr.advantages.float().cpu().numpy()})
    compare([res[0]], [res[1]])


def case_outside_window():
    """16 rows: rows_fwd_kernel<32>'s plan takes them only inside the window; here the window is pinned to start at 17"""
    res = []
    for merge in (False, True):
        tr, env = make_trainer(16, 4, merge)
        tr.nat.plan_log(1)
        tr.rollout()
        plan = tr.nat.plan_log(0)
        torch.cuda.synchronize()
        assert MERGED not in plan, plan
        if merge:
            assert plan.count("rollout_post_kernel as a launch of its own") == 4, plan
        res.append({k: v.cpu().numpy() for k, v in {**buffers_of(tr), **state_of(tr, env)}.items()})
    compare([res[0]], [res[1]])


def case_other_rows():
    """a policy step on ANOTHER number of rows while a post step is recorded: the step is flushed first"""
    res = []
    for merge in (False, True):
        tr, env = make_trainer(64, 4, merge)
        tr.run_iteration(log=False)                        # fills the argument block of the fused step
        torch.cuda.synchronize()
        eu, nat, a = env.unwrapped, tr.nat, tr.agent
        nat.rollout_defer_tail(True, merge=merge)
        assert nat.lib.catppo_rollout_pre(nat.h, eu._rstep_ref, nat._stream()) == 0
        assert nat.lib.catppo_rollout_post(nat.h, eu._rstep_ref, nat._stream()) == 0
        nat.plan_log(1)
        val = torch.zeros(63, device=tr.device)
        x = tr.obs[tr.sink.step + 1]                       # the rows that post step writes
        nat.value_ex(a.shape, a.flat, x, 63, val)
        plan = nat.plan_log(0)
        assert MERGED not in plan, plan
        assert ("rollout_post_kernel as a launch of its own" in plan) == merge, plan
        nat.rollout_defer_tail(False)
        torch.cuda.synchronize()
        res.append({**{k: v.cpu().numpy() for k, v in {**buffers_of(tr), **state_of(tr, env)}.items()},
                    "val": val.cpu().numpy()})
    compare([res[0]], [res[1]])


def case_checkpoint():
    """an armed rollout, then a checkpoint read: nothing is pending behind the `finally`, the state is current"""
    res = []
    for merge in (False, True):
        tr, env = make_trainer(64, 4, merge)
        tr.rollout()
        nat = tr.nat
        nat.plan_log(1)
        assert nat.lib.catppo_rollout_defer_tail(nat.h, -1, nat._stream()) == 0
        assert nat.plan_log(0) == ""                       # nothing left to flush
        sd = {k: v.detach().cpu().numpy() for k, v in tr.agent.state_dict().items()}
        res.append({**sd, **{k: v.cpu().numpy() for k, v in state_of(tr, env).items()}})
    compare([res[0]], [res[1]])
    assert float(res[1]["count"]) > 4 * 64


CASES = {f"steps_{n}_{'eps' if e else 'philox'}": (lambda n=n, e=e: case_steps(n, e))
         for n in (33, 64, 300, 4096) for e in (True, False)}
CASES.update(iteration=case_iteration, outside_window=case_outside_window, other_rows=case_other_rows,
             checkpoint=case_checkpoint)


def main(out):
    results = {}
    for name, fn in CASES.items():
        try:
            fn()
            results[name] = "ok"
        except BaseException:                              # noqa: BLE001 - the parent reports it
            results[name] = traceback.format_exc()[-3000:]
            if "AssertionError" not in results[name]:      # not a mismatch: a device or library error - nothing more runs
                with open(out, "w") as f:
                    json.dump(results, f)
                sys.exit(1)
        with open(out, "w") as f:
            json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1])
