"""Rollouts only (no update phase) of the servo task, for a kernel trace of its env step:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/servo_sim_profile.py --num_envs 4096
    python tools/rocpd_stats.py DIR/.../*.db          ->  rows of profiles/servo_sim_kernel_stats.csv

Per env step the trace shows servo_sim_kernel (the simulator), the two launches of catppo_rollout_pre, the one of
catppo_rollout_post and the policy forward."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "constraints-as-terminations_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--rollouts", type=int, default=10)
    a = ap.parse_args()
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry, make
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    task = "Isaac-Velocity-CaT-Flat-Solo12-Servo-v0"
    env_cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    agent_cfg = load_cfg_from_registry(task, "clean_rl_cfg_entry_point")
    env_cfg.scene.num_envs = a.num_envs
    agent_cfg.minibatch_size = min(agent_cfg.minibatch_size, a.num_envs * agent_cfg.num_steps)
    trainer = PPOTrainer(make(task, cfg=env_cfg), agent_cfg)
    assert trainer.sink is not None
    for _ in range(a.rollouts):
        trainer.rollout()
        trainer.obs[0].copy_(trainer.obs[trainer.T])
    torch.cuda.synchronize()
    print(f"{a.rollouts} rollouts of {trainer.T} steps x {a.num_envs} envs; mean reward/step "
          f"{float(trainer.rewards.float().mean()):.4f}")


if __name__ == "__main__":
    main()
