"""Load a CleanRL checkpoint into ``Agent`` and roll the policy out (reference: scripts/clean_rl/play.py).

Checkpoints written by ``PPO()`` (``model_<it>.pt``, the reference's 23-key ``state_dict``) load
here and in the reference's play.py alike.  Like the reference (play.py:107-135) the script writes
``<run>/exported/model.onnx`` and ``<run>/exported/model.pt`` (deterministic policy with the frozen
observation normaliser) before rolling the policy out on the device kernels.

``--eval_steps K`` (closed-loop servo tasks) then evaluates the deterministic policy for K control steps on a fresh env
(``cat_envs.tasks.utils.cleanrl.evaluate``): one line ``[EVAL] <json>`` and ``<run>/eval/<checkpoint name>.json``.
``--eval_grid NX NY NW`` fixes the commands to a grid over the task's command ranges (env i gets point i % (NX NY NW));
without it the simulator draws them.  ``--stochastic`` samples the actions instead of taking the mean.

``--eval_schedule VX VY WZ [VX VY WZ ...]`` (instead of ``--eval_grid``) has every env follow that sequence of commands,
``--eval_segment_steps L`` control steps each, restarting with every episode; ``--trace_envs K`` records the first K envs
step by step on the device.  With both, the ``[EVAL]`` line carries rise, settling, overshoot and steady-state error per
command change (``"step_response"``), and ``<run>/eval/<checkpoint name>_trace.npz`` holds ``trace`` [steps, K, 72],
``fields``, ``commands`` and ``segment_steps``.

``--eval_plant kp_scale=0.8:1.2:3 mass_scale=0.8:1.3:3 lag=0:8:3 ...`` (``name=value`` or ``name=lo:hi:n``; names ``kp_scale``
``kd_scale`` ``friction`` ``armature`` ``mass_scale`` ``lag``) pins the plant of every env to a point of that grid inside the
simulator's launch (``evaluate.plant_grid``), whatever the randomisation draws: the ``[EVAL]`` line then carries ``by_plant`` and
``robustness``, and ``<run>/eval/<checkpoint name>_robustness.json`` holds the two blocks.  With ``--eval_grid`` the evaluation
env has a whole multiple of (command points x plant points) envs, env i with command i % C and plant i // C (``evaluate.sweep``).
"""
import argparse
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "constraints-as-terminations_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cli_args  # noqa: E402  isort: skip


def get_checkpoint_path(log_root: str, run_dir: str = ".*", checkpoint: str = "model_.*.pt") -> str:
    """latest run matching ``run_dir`` and, inside it, the highest-numbered file matching ``checkpoint``"""
    runs = sorted(d for d in os.listdir(log_root) if os.path.isdir(os.path.join(log_root, d)) and re.match(run_dir, d))
    if not runs:
        raise ValueError(f"no run matching '{run_dir}' in {log_root}")
    run = os.path.join(log_root, runs[-1])
    files = [f for f in os.listdir(run) if re.match(checkpoint, f)]
    if not files:
        raise ValueError(f"no checkpoint matching '{checkpoint}' in {run}")
    files.sort(key=lambda f: [int(x) for x in re.findall(r"\d+", f)] or [0])
    return os.path.join(run, files[-1])


def main(argv=None):
    parser = argparse.ArgumentParser(description="Play an RL agent trained with CleanRL.")
    parser.add_argument("--video", action="store_true", default=False)
    parser.add_argument("--video_length", type=int, default=200, help="Number of roll-out steps.")
    parser.add_argument("--num_envs", type=int, default=None)
    parser.add_argument("--task", type=str, default=None)
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("--device", type=str, default=None)
    parser.add_argument("--headless", action="store_true", default=False)
    parser.add_argument("--eval_steps", type=int, default=0, help="Evaluate the policy for this many control steps (0: off).")
    parser.add_argument("--eval_grid", type=int, nargs=3, default=None, metavar=("NX", "NY", "NW"),
                        help="Fixed commands: a grid of NX x NY x NW points over the command ranges (default: sampled).")
    parser.add_argument("--eval_schedule", type=float, nargs="+", default=None, metavar="V",
                        help="Command schedule VX VY WZ [VX VY WZ ...] that every env follows (instead of --eval_grid).")
    parser.add_argument("--eval_segment_steps", type=int, default=100, help="Control steps per segment of --eval_schedule.")
    parser.add_argument("--eval_plant", type=str, nargs="+", default=None, metavar="NAME=LO:HI:N",
                        help="Pinned plants: a grid over kp_scale, kd_scale, friction, armature, mass_scale, lag (name=value or "
                             "name=lo:hi:n); combines with --eval_grid.")
    parser.add_argument("--trace_envs", type=int, default=0, help="Record the first K envs step by step (0: off).")
    parser.add_argument("--stochastic", action="store_true", default=False, help="Evaluate with sampled actions.")
    parser.add_argument("--obs_noise", choices=("on", "off"), default=None,
                        help="Observation noise of a task with cfg.observations (default: what the task's cfg says).")
    parser.add_argument("--pushes", choices=("on", "off"), default=None,
                        help="Interval events (pushes) of a task with cfg.events (default: what the task's cfg says).")
    parser.add_argument("--randomization", choices=("on", "off"), default=None,
                        help="Randomised robot of a task whose cfg.events randomises it (default: on; off: the nominal robot).")
    parser.add_argument("--wrench", choices=("on", "off"), default=None,
                        help="External force and torque of a task whose cfg.events has apply_external_force_torque (default: on).")
    parser.add_argument("--push_probability", type=float, default=None, metavar="P",
                        help="Push probability per env and control step of a task with a push term (default: the reference's).")
    cli_args.add_clean_rl_args(parser)
    args_cli = parser.parse_args(argv)
    if args_cli.eval_schedule is not None:
        if args_cli.eval_grid is not None:
            parser.error("--eval_schedule and --eval_grid are mutually exclusive")
        if len(args_cli.eval_schedule) % 3 != 0:
            parser.error("--eval_schedule takes a multiple of three values: VX VY WZ per segment")
    plant_axes = None
    if args_cli.eval_plant is not None:
        from cat_envs.tasks.utils.cleanrl.evaluate import parse_plant_axes
        try:
            plant_axes = parse_plant_axes(args_cli.eval_plant)
        except ValueError as e:
            parser.error(str(e))
    import torch

    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry, make
    from cat_envs.tasks.utils.cleanrl.ppo import Agent

    env_cfg = load_cfg_from_registry(args_cli.task, "env_cfg_entry_point")
    if args_cli.num_envs is not None:
        env_cfg.scene.num_envs = args_cli.num_envs
    if args_cli.device is not None:
        env_cfg.sim.device = args_cli.device
    if args_cli.obs_noise is not None:
        if getattr(env_cfg, "observations", None) is None:
            parser.error("--obs_noise needs a task with cfg.observations")
        env_cfg.observations.policy.enable_corruption = args_cli.obs_noise == "on"
    if args_cli.pushes is not None or args_cli.push_probability is not None:
        if getattr(env_cfg, "events", None) is None:
            parser.error("--pushes and --push_probability need a task with cfg.events")
        if args_cli.pushes is not None:
            env_cfg.pushes = args_cli.pushes == "on"
        if args_cli.push_probability is not None:
            from cat_envs.tasks.utils.mdp import events as _events
            terms = [t for t in vars(env_cfg.events).values()
                     if getattr(t, "func", None) is _events.push_by_setting_velocity_with_random_envs]
            if not terms:
                parser.error("--push_probability needs a task whose cfg.events has a push term")
            terms[0].params = {**terms[0].params, "probability": args_cli.push_probability}
    agent_cfg = cli_args.parse_clean_rl_cfg(args_cli.task, args_cli)
    log_root_path = os.path.abspath(os.path.join("logs", "clean_rl", agent_cfg.experiment_name))
    print(f"[INFO] Loading experiment from directory: {log_root_path}")
    resume_path = get_checkpoint_path(log_root_path, agent_cfg.load_run, agent_cfg.load_checkpoint)
    print(f"[INFO] Loading model: {resume_path}")

    env = make(args_cli.task, cfg=env_cfg)
    if args_cli.randomization is not None:
        em = getattr(env.unwrapped, "event_manager", None)
        if em is None or em.randomization is None:
            parser.error("--randomization needs a task whose cfg.events randomises the robot")
        em.set_randomization_enabled(args_cli.randomization == "on")
    if args_cli.wrench is not None:
        em = getattr(env.unwrapped, "event_manager", None)
        if em is None or "wrench" not in em.block:
            parser.error("--wrench needs a task whose cfg.events has apply_external_force_torque")
        em.set_wrench_enabled(args_cli.wrench == "on")
    actor = Agent(env, hidden=tuple(agent_cfg.hidden), mlp_precision=str(getattr(agent_cfg, "mlp_precision", "fp32")))
    actor.load_state_dict(torch.load(resume_path, map_location=actor.flat.device))
    actor.eval()

    from cat_envs.tasks.utils.cleanrl.export import export_policy
    om = getattr(env.unwrapped, "observation_manager", None)
    am = env.unwrapped.action_manager                   # envs with cfg.actions: the manager that knows the output contract
    um = getattr(env.unwrapped, "actuators", None)      # envs with cfg.scene.robot: gains and delay range join actions.json
    exported = export_policy(actor.state_dict(), os.path.join(os.path.dirname(resume_path), "exported"),
                             observation_spec=None if om is None else om.spec(),
                             action_spec=am.spec() if hasattr(am, "spec") else None,
                             actuator_spec=um.spec() if um is not None else None,
                             randomization_spec=getattr(getattr(env.unwrapped, "event_manager", None), "randomization", None))
    print(f"[INFO] Exported ONNX model to {exported['onnx']}")
    print(f"[INFO] Exported .pt model to {exported['jit']}")
    if om is not None:
        print(f"[INFO] Wrote the policy's input contract to {exported['observations']}")
    if "actions" in exported:
        print(f"[INFO] Wrote the policy's output contract to {exported['actions']}")

    obs = env.reset()[0]["policy"]
    ret = 0.0
    for _ in range(args_cli.video_length):
        with torch.no_grad():
            actions, _, _, _ = actor.get_action_and_value(actor.obs_rms(obs, update=False))
        obs, rewards, dones, timeouts, info = env.step(actions)
        obs = obs["policy"]
        ret += float(rewards.mean())
    print(f"[INFO] mean reward per step over {args_cli.video_length} steps: {ret / args_cli.video_length:.4f}")
    env.close()

    if args_cli.eval_steps > 0:
        import numpy as np
        from cat_envs.tasks.utils.cleanrl.evaluate import (COMMAND_RANGES, command_grid, command_sequence, evaluate_policy,
                                                           plant_grid, sweep)
        plants, swept = None, None
        if plant_axes is not None and args_cli.eval_grid is not None:
            # N = C x P envs, as often as they fit into the env count asked for: env i gets command i % C and plant i // C
            axes = [(lo, hi, n) for (lo, hi), n in zip(COMMAND_RANGES, args_cli.eval_grid)]
            points = int(np.prod(args_cli.eval_grid))
            product = points * int(np.prod([a[2] if isinstance(a, tuple) else 1 for a in plant_axes.values()]))
            reps = max(1, int(env_cfg.scene.num_envs) // product)
            cmd, table = sweep(command_grid(*axes, num_envs=points)[0],
                               plant_grid(**plant_axes, num_envs=product // points))
            swept = (np.tile(cmd, (reps, 1)), np.tile(table["packed"], (reps, 1)))
            env_cfg.scene.num_envs = product * reps
            print(f"[INFO] Evaluating {points} commands x {product // points} plants x {reps} on {product * reps} envs")
        eval_env = make(args_cli.task, cfg=env_cfg)               # a fresh env: the evaluator leaves it in the evaluated state
        commands, segment_steps = None, None
        if swept is not None:
            commands, plants = swept
        elif plant_axes is not None:
            plants = plant_grid(**plant_axes, num_envs=eval_env.unwrapped.num_envs)
        if args_cli.eval_schedule is not None:
            points = np.asarray(args_cli.eval_schedule, np.float32).reshape(-1, 3)
            commands, segment_steps = command_sequence(points, eval_env.unwrapped.num_envs), args_cli.eval_segment_steps
        elif args_cli.eval_grid is not None and swept is None:
            axes = [(lo, hi, n) for (lo, hi), n in zip(COMMAND_RANGES, args_cli.eval_grid)]
            commands = command_grid(*axes, num_envs=eval_env.unwrapped.num_envs)[0]
        result = evaluate_policy(eval_env, actor, args_cli.eval_steps, commands=commands,
                                 deterministic=not args_cli.stochastic, segment_steps=segment_steps,
                                 trace_envs=args_cli.trace_envs, plant=plants)
        text = result.to_json()
        print(f"[EVAL] {text}")
        out_dir = os.path.join(os.path.dirname(resume_path), "eval")
        os.makedirs(out_dir, exist_ok=True)
        out_path = os.path.join(out_dir, os.path.splitext(os.path.basename(resume_path))[0] + ".json")
        with open(out_path, "w") as f:
            f.write(text + "\n")
        print(f"[INFO] Wrote evaluation to {out_path}")
        if result.plant is not None:
            import json
            robust_path = os.path.splitext(out_path)[0] + "_robustness.json"
            with open(robust_path, "w") as f:
                f.write(json.dumps({"by_plant": result.by_plant(), "robustness": result.robustness()}) + "\n")
            print(f"[INFO] Wrote robustness to {robust_path}")
        if result.trace is not None:
            trace_path = os.path.splitext(out_path)[0] + "_trace.npz"
            np.savez(trace_path, trace=result.trace, fields=np.array([name for name, _, _ in result.trace_fields]),
                     commands=np.zeros((0, 3), np.float32) if result.commands is None else result.commands,
                     segment_steps=np.int64(result.segment_steps or 0))
            print(f"[INFO] Wrote trace to {trace_path}")
        eval_env.close()


if __name__ == "__main__":
    main()
