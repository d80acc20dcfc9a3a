"""CleanRL command-line arguments (same flags as the reference scripts/clean_rl/cli_args.py)."""
from __future__ import annotations

import argparse


def add_clean_rl_args(parser: argparse.ArgumentParser):
    group = parser.add_argument_group("clean_rl", description="Arguments for CleanRL agent.")
    group.add_argument("--experiment_name", type=str, default=None,
                       help="Name of the experiment folder where logs will be stored.")
    group.add_argument("--resume", type=bool, default=None, help="Whether to resume from a checkpoint.")
    group.add_argument("--load_run", type=str, default=None, help="Name of the run folder to resume from.")
    group.add_argument("--checkpoint", type=str, default=None, help="Checkpoint file to resume from.")
    group.add_argument("--logger", type=str, default=None, choices={"wandb", "tensorboard"},
                       help="Logger module to use.")
    group.add_argument("--log_project_name", type=str, default=None,
                       help="Name of the logging project when using wandb")


def add_eval_args(parser: argparse.ArgumentParser):
    """evaluation inside the run (train.py; play.py has --eval_steps / --eval_grid of its own for one checkpoint)"""
    group = parser.add_argument_group("periodic evaluation", description="Evaluate the policy while training (servo tasks).")
    group.add_argument("--eval_interval", type=int, default=None, metavar="K",
                       help="Evaluate before the first iteration and after every K-th (0: never).")
    group.add_argument("--eval_envs", type=int, default=None, metavar="N", help="Envs of the dedicated eval env.")
    group.add_argument("--eval_steps", type=int, default=None, metavar="S", help="Control steps of one evaluation.")
    group.add_argument("--eval_grid", type=int, nargs=3, default=None, metavar=("NX", "NY", "NW"),
                       help="Fixed commands: a grid of NX x NY x NW points over the command ranges.")
    group.add_argument("--eval_metric", type=str, default=None, metavar="NAME",
                       help="The metric whose highest value selects model_best.pt.")


def parse_clean_rl_cfg(task_name: str, args_cli: argparse.Namespace):
    from cat_envs.shim import load_cfg_from_registry
    return update_clean_rl_cfg(load_cfg_from_registry(task_name, "clean_rl_cfg_entry_point"), args_cli)


def update_clean_rl_cfg(agent_cfg, args_cli: argparse.Namespace):
    """override the task's default runner configuration with CLI arguments"""
    if getattr(args_cli, "seed", None) is not None:
        agent_cfg.seed = args_cli.seed
    if args_cli.resume is not None:
        agent_cfg.resume = args_cli.resume
    if args_cli.load_run is not None:
        agent_cfg.load_run = args_cli.load_run
    if args_cli.checkpoint is not None:
        agent_cfg.load_checkpoint = args_cli.checkpoint
    if args_cli.logger is not None:
        agent_cfg.logger = args_cli.logger
    if agent_cfg.logger in {"wandb"} and args_cli.log_project_name:
        agent_cfg.wandb_project = args_cli.log_project_name
    return agent_cfg


def update_eval_cfg(agent_cfg, args_cli: argparse.Namespace):
    """the flags of ``add_eval_args`` over the task's runner configuration (all of which default to "off")"""
    for name in ("eval_interval", "eval_envs", "eval_steps", "eval_metric"):
        if getattr(args_cli, name, None) is not None:
            setattr(agent_cfg, name, getattr(args_cli, name))
    if getattr(args_cli, "eval_grid", None) is not None:
        agent_cfg.eval_grid = tuple(args_cli.eval_grid)
    return agent_cfg
