"""Which kernels does a shape get?  

    python tools/explain_plan.py [--obs 48] [--act 12] [--hidden 256,256,256] [--envs 4096] [--minibatch 16384]
                                 [--precision fp32|bf16|bf16x3]          (needs the MI355X: the plan is RECORDED, not re-derived)

Runs ONE rollout forward (catppo_policy_step on `--envs` rows) and ONE optimiser step
(catppo_ppo_minibatch_step_packed on `--minibatch` rows) on random data with catppo_plan_log switched on and prints what
the library's dispatch code wrote at its decision sites: kernel, grid, and the rule that selected it.  `--all` walks the
BASELINE shapes (profiles/r5_explain_plan.txt is this output).

    python tools/explain_plan.py --task Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-v0        (needs no device)

names the instance of the servo simulator's kernel a task's training step launches: which of ``cfg.rewards``,
``cfg.observations``, ``cfg.events``, ``cfg.commands``, ``cfg.terminations``, ``cfg.actions`` and ``cfg.scene.robot`` (``RewardsCfg``, ``ObservationsCfg``,
``EventCfg``, ``CommandsCfg``, ``TerminationsCfg``, ``ActionsCfg``) the cfg carries decides the kernel's template pack
(csrc/servo_sim_kernel.h, instantiated in servo_sim.hip, with actions in servo_sim_actions.hip and with a robot in
servo_sim_actuators.hip).
The servo tasks are ``...-Solo12-Servo-v0`` and its ``-Rewards``, ``-Obs``, ``-Events``, ``-Full``, ``-Commands``, ``-Reference``,
``-Terminations``, ``-Reference-Terminations``, ``-Actions``, ``-Reference-Actions``, ``-Actuators``, ``-Reference-Actuators``,
``-DelayedActuators``, ``-Randomized`` (servo_sim_randomize.hip), ``-Reference-Randomized``, ``-History`` (servo_sim_history.hip) and
``-Reference-History`` variants.  ``--plant`` names the instance that an evaluation with a plant table launches instead
(``evaluate_policy(plant=...)``; servo_sim_plant.hip, DESIGN section 9 "Robustness")."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "constraints-as-terminations_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def explain(obs, act, hidden, envs, mb, precision="fp32"):
    from cat_envs import native
    from cat_envs.tasks.utils.cleanrl.ppo import MLP_PRECISIONS
    nat = native.get(torch.device("cuda", 0))
    dev = nat.device
    shape = native.shape_of(obs, act, hidden, mfma_bf16=MLP_PRECISIONS[precision])
    lay = native.layout_of(shape)
    nat.mlp_reserve(shape, max(envs, mb))
    g = torch.Generator(device="cpu").manual_seed(1)
    flat = (torch.randn(lay.n_flat, generator=g) * 0.05).to(dev)
    x = torch.zeros(max(envs, mb), lay.obs_pad, device=dev)
    x[:, :obs] = torch.randn(max(envs, mb), obs, generator=g).to(dev)
    st = nat.iter_state_new(7, 3e-4)
    nat.iter_begin(st, 3e-4, 10, native.LR_FIXED)
    a, lp, v = torch.empty(envs, act, device=dev), torch.empty(envs, device=dev), torch.empty(envs, device=dev)
    out = [f"== obs {obs} (padded {lay.obs_pad}), act {act}, hidden {tuple(hidden)}, {envs} envs, minibatch {mb}, {precision}"]
    nat.plan_log(1)
    nat.policy_act_rng(shape, flat, x, envs, st, 0, a, lp, v)
    actg = torch.randn(mb, act, generator=g).to(dev)
    scal = torch.randn(4 * mb, generator=g).to(dev)
    scal[:mb] = -11.0
    parts = (mb + nat.GATHER_ROWS - 1) // nat.GATHER_ROWS
    advp = torch.zeros(2 * parts, dtype=torch.float64, device=dev)
    advp[0], advp[1] = float(scal[mb:2 * mb].double().sum()), float((scal[mb:2 * mb].double() ** 2).sum())
    hp = native.PpoHparams(0.2, 0.001, 2.0, 1, 1, 1.0 / mb, 0)
    grad, diag = torch.zeros(lay.n_flat, device=dev), torch.zeros(8, device=dev)
    m1, m2 = torch.zeros(lay.n_flat, device=dev), torch.zeros(lay.n_flat, device=dev)
    one, zero = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    nat.ppo_minibatch_step_packed(shape, hp, flat, x, actg, scal, advp, mb, zero, one, None, grad, diag, m1, m2, 1.0, 0.9,
                                  0.999, 1e-5, st)
    torch.cuda.synchronize()
    out.append(nat.plan_log(0).rstrip())
    return "\n".join(out)


def explain_task(task, plant=False):
    """the servo simulator's kernel instance of a task's training step, from its cfg alone; ``plant``: of an evaluation with a
    plant table as well"""
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    if str(getattr(cfg.synthetic, "kind", "stream")) != "servo":
        return f"== {task}: the stream simulator (no simulator kernel; the state is a pre-generated stream)"
    has = {k: getattr(cfg, k, None) is not None for k in ("rewards", "observations", "events", "commands", "terminations", "actions")}
    from cat_envs.tasks.utils.mdp import randomization as RZ
    event_terms, rnd_terms = RZ.split_events(getattr(cfg, "events", None))   # randomisation terms alone need no event pack
    packed = dict(has, events=bool(event_terms))
    pack = [name for key, name in (("observations", "catppo_servo_obs"), ("events", "catppo_servo_events"),
                                   ("commands", "catppo_servo_commands"), ("terminations", "catppo_servo_terminations"),
                                   ("actions", "catppo_servo_actions")) if packed[key]]
    robot = getattr(cfg.scene, "robot", None)
    if robot is not None or rnd_terms:           # the actuator descriptor comes behind an action descriptor, the identity one if need be
        pack += ([] if has["actions"] else ["catppo_servo_actions"]) + ["catppo_servo_actuators"]
    if rnd_terms:                                # ... and the randomisation descriptor behind an actuator descriptor, likewise
        pack += ["catppo_servo_randomize"]
    # history_length above 1 on a term or the group: the history descriptor comes last, behind the identity tables if need be
    history = None
    if has["observations"]:
        import cat_envs.tasks.utils.cat.cat_env as E
        from cat_envs.tasks.utils.mdp import observation_manager as OM
        table = OM.build_table(OM.policy_group(cfg.observations), E.SOLO12_JOINTS, E.DEFAULT_JOINT_POS)
        history = table if table.has_history else None
    if history is not None:
        pack += [n for n in ("catppo_servo_actions", "catppo_servo_actuators", "catppo_servo_randomize") if n not in pack]
        pack += ["catppo_servo_history"]
    row = 308 + (48 if has["observations"] else 0) + (4 if has["commands"] else 0) + (4 if has["terminations"] else 0)
    row += 48 if robot is not None or rnd_terms or history is not None else 0
    # a timed push or a wrench among the events: the same instance on the extended block; the timed push keeps its timer in the row
    disturb = None
    if event_terms:
        from cat_envs.tasks.utils.mdp import event_manager as EM
        block = EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s)
        disturb = block if EM.extended(block) else None
        row += 4 if disturb is not None and "interval_range" in disturb else 0
        if disturb is not None:                  # the extended block reaches the kernel as a type of its own
            pack = ["ServoEventsExt" if n == "catppo_servo_events" else n for n in pack]
    has["scene.robot"] = robot is not None
    out = [f"== {task}: " + ", ".join(f"cfg.{k} {'set' if v else 'unset'}" for k, v in has.items()),
           f"servo_sim_kernel<kTrain, {'true' if has['rewards'] else 'false'}{''.join(', ' + n for n in pack)}>: row of {row} floats "
           f"(with the reference's 45-float policy observation), {row * 64} bytes of LDS per workgroup"]
    if history is not None:
        T = history.history_floats
        out.append(f"observation history (servo_sim_history.hip): {T} floats behind the row (stride {row + (T + 3) // 4 * 4}), "
                   f"outside LDS; depths " + ", ".join(f"'{n}' {h} x {history.widths[n]}" for n, h in history.depths.items()))
    if disturb is not None:
        kinds = [k for k in ("push_timed", "wrench") if k in disturb["kinds"].values()]
        timer = disturb.get("interval_range")
        unit = "servo_sim_disturb_robot.hip" if rnd_terms or history is not None else "servo_sim_disturb.hip"
        out.append(f"disturbances ({', '.join(kinds)}; {unit}): an event block of 64 words; ServoEventsExt stands in the place of "
                   f"catppo_servo_events, a template parameter of the events path"
                   + (f"; the push fires every {timer[0]:g} .. {timer[0] + timer[1]:g} s on the env's own timer, 4 floats 'ev_state' "
                      f"at the end of the row" if timer is not None else "")
                   + (f"; wrench per {'episode' if disturb['wrench']['mode'] == 'reset' else 'env'}, force (lo, width) "
                      f"{tuple(float(f'{v:g}') for v in disturb['wrench']['force'])} N, torque "
                      f"{tuple(float(f'{v:g}') for v in disturb['wrench']['torque'])} N m" if "wrench" in disturb else ""))
    if plant:
        if robot is None and not rnd_terms and history is None:
            out.append("pinned plants: not on this task - the row has no act_hist field (the task needs cfg.scene.robot, "
                       "randomisation terms or an observation history)")
        else:
            pinned = pack + [n for n in ("catppo_servo_actions", "catppo_servo_actuators", "catppo_servo_randomize") if n not in pack]
            pinned += ["catppo_servo_plant"]
            out.append(f"pinned plants ({'servo_sim_disturb_robot.hip' if disturb is not None else 'servo_sim_plant.hip'}): an evaluation with a plant table launches servo_sim_kernel<kStepResponse, "
                       f"{'true' if has['rewards'] else 'false'}{''.join(', ' + n for n in pinned)}> on the same row; the table is "
                       f"[N, 8] fp32, 32 bytes per env beside a row of {row * 4} bytes")
    if has["commands"]:
        from cat_envs.tasks.utils.mdp import command_manager as KM
        b = KM.build_block(cfg.commands, cfg.sim.dt, cfg.episode_length_s)
        out.append(f"command term '{b['name']}' ({b['class']}): flags {b['flags']:#x}, p_still {b['p_still']:g}, p_move {b['p_move']:g}, "
                   f"ranges {b['bounds']}, resampling {b['time']} s; inert: {', '.join(b['inert']) or 'none'}")
    if has["terminations"]:
        import cat_envs.tasks.utils.cat.cat_env as E
        from cat_envs.tasks.utils.mdp import terminations as TM
        kinds = {v: k for k, v in TM.K.items()}
        for name, kind, mask, p0, p1 in TM.build_table(cfg.terminations, E.SOLO12_JOINTS, E.SOLO12_BODIES):
            out.append(f"termination term '{name}' ({kinds[kind]}{', time_out' if kind == 1 else ''}): mask {mask:#x}, p0 {p0:g}, p1 {p1:g}")
    if has["actions"]:
        import cat_envs.tasks.utils.cat.cat_env as E
        from cat_envs.tasks.utils.mdp import actions as AM
        entries, terms = AM.build_table(cfg.actions, E.SOLO12_JOINTS, E.DEFAULT_JOINT_POS)
        out.append(f"action block (servo_sim_actions.hip): {max(t['slice'][1] for t in terms.values())} columns, terms "
                   + ", ".join(f"'{n}' ({t['kind']}, columns {t['slice'][0]}..{t['slice'][1] - 1})" for n, t in terms.items()))
        for c in AM.action_spec(entries, terms, E.SOLO12_JOINTS)["columns"]:
            out.append(f"  column {c['column']:2d} -> {c['joint']:<7s} {c['kind']}: scale {c['scale']:g}, offset {c['offset']:g}, clip {c['clip']}")
    if robot is not None:
        import cat_envs.tasks.utils.cat.cat_env as E
        from cat_envs.tasks.utils.mdp import actuators as UM
        entries, spec = UM.build_table(robot, E.SOLO12_JOINTS, cfg.synthetic, cfg.decimation, E.DEFAULT_JOINT_POS)
        out.append("actuators (servo_sim_actuators.hip): groups " + ", ".join(
            f"'{n}' ({g['kind']}, {len(g['joints'])} joints, delay {g['min_delay']}..{g['max_delay']} physics steps)"
            for n, g in spec["groups"].items()) + f"; inert: {', '.join(spec['inert']) or 'none'}")
        for j in spec["joints"]:
            out.append(f"  joint {j['joint_id']:2d} {j['joint']:<7s} group '{j['group']}': stiffness {j['stiffness']:g}, damping "
                       f"{j['damping']:g}, inertia {j['inertia']:g}, effort limit {j['effort_limit']:g}")
    if rnd_terms:
        import cat_envs.tasks.utils.cat.cat_env as E
        from cat_envs.tasks.utils.mdp import actuators as UM
        entries = None if robot is None else UM.build_table(robot, E.SOLO12_JOINTS, cfg.synthetic, cfg.decimation, E.DEFAULT_JOINT_POS)[0]
        _, spec = RZ.build_randomization(cfg.events, entries, E.SOLO12_JOINTS, cfg.synthetic, cfg.sim.dt, cfg.decimation,
                                         armatures=None if robot is None else UM.armatures(robot, E.SOLO12_JOINTS))
        out.append(f"randomisation (servo_sim_randomize.hip): nominal mass {spec['nominal_mass']:g} kg, friction in "
                   f"{spec['friction_unit']}; inert: {', '.join(spec['inert']) or 'none'}")
        for n, t in spec["terms"].items():
            ranges = ", ".join(f"{q} {tuple(r)}" for q, r in t["ranges"].items() if r is not None)
            out.append(f"  {t['mode']:<7s} '{n}' ({t['func']}): {t['operation']} {ranges} on {len(t['joints'])} of "
                       f"{'the bodies' if t['kind'] == 'rigid_body_mass' else 'the joints'}")
    return "\n".join(out)


BASELINE = [
    ("cfg1: 64 envs, 2 terms, reference MLP", 48, 12, (512, 256, 128), 64, 512, "fp32"),
    ("cfg2: the bench default", 48, 12, (256, 256, 256), 4096, 16384, "fp32"),
    ("reference shapes", 45, 12, (512, 256, 128), 4096, 16384, "fp32"),
    ("cfg3: one rank's share at 8 GPUs", 45, 12, (512, 256, 128), 2048, 2048, "fp32"),
    ("cfg4: 235-d observations", 235, 12, (256, 256, 256), 4096, 16384, "fp32"),
    ("cfg5: bf16 MLP", 48, 12, (256, 256, 256), 32768, 16384, "bf16"),
    ("cfg2, split-bf16 (the secondary record)", 48, 12, (256, 256, 256), 4096, 16384, "bf16x3"),
]

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=48)
    ap.add_argument("--act", type=int, default=12)
    ap.add_argument("--hidden", default="256,256,256")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16", "bf16x3"))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--task", default=None, help="name the servo simulator's kernel instance of this task (needs no device)")
    ap.add_argument("--plant", action="store_true", help="with --task: name the instance of an evaluation with a plant table, too")
    a = ap.parse_args()
    if a.task:
        print(explain_task(a.task, plant=a.plant))
    elif a.all:
        for name, *spec in BASELINE:
            print("#", name)
            print(explain(*spec))
            print()
    else:
        print(explain(a.obs, a.act, tuple(int(h) for h in a.hidden.split(",")), a.envs, a.minibatch, a.precision))
