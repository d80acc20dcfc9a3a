"""Run state of a task with commands ("Commands"; section 10): the Reference task - rewards, observations,
events and commands together - resumed after 2 of 4 iterations equals the uninterrupted run bit for bit.  The command and
the time left travel in the simulator's row; the ranges, which a curriculum term moves before the save, travel in the env's
part.  A state saved with commands is refused by an env without them, and the reverse, through the fingerprint."""
import numpy as np
import pytest
import torch

import test_gpu_resume as RS
import test_servo_commands_twin as CC

pytestmark = pytest.mark.gpu

REFERENCE = CC.REFERENCE
NEW_RANGES = {"lin_vel_x": (0.4, 0.6), "ang_vel_z": (-0.5, 0.5)}


def _cfgs(task=REFERENCE, commands=True):
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import CurriculumTermCfg, load_cfg_from_registry
    from cat_envs.tasks.utils.cat import curriculums
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    push = cfg.events.push_robot                                             # pushes do occur in 4 x 8 steps of 64 envs
    push.params = {**push.params, "probability": 0.05}
    if commands:
        # the test cfg of the device test (resamples every few steps), and ranges that move after 10 env steps: before the save
        cfg.commands = CC.commands_cfg_of()
        cfg.curriculum.command_ranges = CurriculumTermCfg(func=curriculums.modify_command_ranges, params={
            "term_name": "base_velocity", "ranges": dict(NEW_RANGES), "num_steps": 10})
    else:
        cfg.commands = None
    agent_cfg = load_cfg_from_registry(task, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 4, 10 ** 9
    return task, cfg, agent_cfg


def test_two_plus_two_iterations_of_the_reference_task_equal_four(tmp_path):
    seen = {}

    def probe(env, tr):
        u = env.unwrapped
        seen["fp"] = u.state_fingerprint()
        seen["sd"] = u.state_dict()["commands"]
        seen["cur"] = u.sim.cur.cpu().numpy().copy()
        seen["off"] = dict(u.sim.off)
    a, b, tr = RS.check_case(_cfgs, tmp_path, save_at=2, iters=4, probe=probe)
    assert seen["sd"] == {"ranges": [[0.4, 0.6], [-0.15, 0.15], [-0.5, 0.5]]}    # the curriculum had moved them at the save
    terms = seen["fp"]["command_terms"]
    assert terms[0] == ["base_velocity", "UniformVelocityCommandWithDeadzoneCfg"] and len(terms[1]) == 16
    assert all(k in seen["fp"] for k in ("reward_terms", "observation_terms", "event_terms"))
    u = tr.envs.unwrapped
    assert u.command_manager.ranges["lin_vel_x"] == (0.4, 0.6) and u.sim.F == 360
    # the fingerprint is the configured block, the device holds the moved one
    assert u.command_manager.fingerprint() == terms and u.sim.command_words[4] == np.float32(0.4)
    c, s = seen["off"]["command"][0], seen["off"]["cmd_state"][0]
    assert (seen["cur"][:, s] > 0).all() and (seen["cur"][:, c:c + 3] != 0).any()
    # commands drawn from the moved ranges are in the state at the end: some env's x command lies above the old upper bound
    assert (a[-1]["sim.cur"][:, c] > np.float32(0.35)).any()


def test_mismatched_envs_are_refused_through_the_fingerprint():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl import checkpoint

    def env_of(commands):
        t, cfg, _ = _cfgs(commands=commands)
        cfg.scene.num_envs = 16
        env = make(t, cfg=cfg).unwrapped
        env.reset()
        return env
    with_c, without = env_of(True), env_of(False)
    assert "command_terms" in with_c.state_fingerprint() and "command_terms" not in without.state_fingerprint()
    assert "commands" not in without.state_dict() and without.sim.F == 356 and with_c.sim.F == 360
    with pytest.raises(ValueError, match="command_terms"):
        checkpoint.check_fingerprint(with_c.state_fingerprint(), without.state_fingerprint())
    with pytest.raises(ValueError, match="command_terms"):
        checkpoint.check_fingerprint(without.state_fingerprint(), with_c.state_fingerprint())
    # other ranges in the cfg are another fingerprint, too
    t, cfg, _ = _cfgs()
    cfg.scene.num_envs = 16
    cfg.commands["base_velocity"].ranges.lin_vel_y = (-0.3, 0.3)
    other = make(t, cfg=cfg).unwrapped
    with pytest.raises(ValueError, match="command_terms"):
        checkpoint.check_fingerprint(with_c.state_fingerprint(), other.state_fingerprint())
    # and the env's own part is checked as well
    sd = checkpoint.to_plain(with_c.state_dict())
    with pytest.raises(ValueError, match="carries commands"):
        without.check_state_dict(sd)
    with pytest.raises(ValueError, match="commands"):
        with_c.check_state_dict(checkpoint.to_plain(without.state_dict()))
    with_c.step(torch.zeros(16, 12, device="cuda"))
    torch.cuda.synchronize()
    assert checkpoint.FORMAT == 1
