"""Run state of a task with events ("Events"; section 10): the Full task - rewards, observations and events
together - resumed after 2 of 4 iterations equals the uninterrupted run bit for bit, the interval switch travels with the
state, and a state saved with events is refused by an env without them, and the reverse."""
import numpy as np
import pytest
import torch

import test_gpu_resume as RS

pytestmark = pytest.mark.gpu

FULL = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Full-v0"


def _cfgs(task=FULL, probability=0.05):
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    RS._shape_env(cfg)
    cfg.scene.num_envs, cfg.seed = 64, 42
    if getattr(cfg, "events", None) is not None:                             # pushes do occur in 4 x 8 steps of 64 envs
        push = cfg.events.push_robot
        push.params = {**push.params, "probability": probability}
    agent_cfg = load_cfg_from_registry(task, "clean_rl_cfg_entry_point")
    agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
    agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 4, 10 ** 9
    return task, cfg, agent_cfg


def test_two_plus_two_iterations_of_the_full_task_equal_four(tmp_path):
    seen = {}

    def probe(env, tr):
        u = env.unwrapped
        seen["fp"] = u.state_fingerprint()
        seen["sd"] = u.state_dict()["events"]
    a, b, tr = RS.check_case(_cfgs, tmp_path, save_at=2, iters=4, probe=probe)
    assert seen["sd"] == {"interval": True}
    terms = seen["fp"]["event_terms"]
    assert [t[0] for t in terms[:-1]] == ["physics_material", "reset_base", "reset_robot_joints", "push_robot"]
    assert len(terms[-1]) == 32 and "reward_terms" in seen["fp"] and "observation_terms" in seen["fp"]
    u = tr.envs.unwrapped
    assert u.event_manager.block["p"] == float(np.float32(0.05)) and (a[-1]["sim.cur"] != 0).any()


def test_the_switch_travels_with_the_state_and_mismatched_envs_are_refused():
    from cat_envs.shim import make
    from cat_envs.tasks.utils.cleanrl import checkpoint

    def env_of(task, events=True):
        t, cfg, _ = _cfgs(task)
        cfg.scene.num_envs = 16
        if not events:
            cfg.events = None                                                 # the same task without its event block
        env = make(t, cfg=cfg).unwrapped
        env.reset()
        return env
    env = env_of(FULL)
    env.set_pushes(False)
    sd = checkpoint.to_plain(env.state_dict())
    assert sd["events"] == {"interval": False}
    other = env_of(FULL)
    assert other.event_manager.interval_enabled
    other.load_state_dict(sd)
    assert other.event_manager.interval_enabled is False
    assert not other.sim.event_words.view(np.int32)[0] & 1 and other.sim.event_words.view(np.int32)[0] == 2 | 8 | 16
    other.step(torch.zeros(16, 12, device="cuda"))
    torch.cuda.synchronize()
    # a state saved with events is refused by an env without them, and the reverse
    without = env_of(FULL, events=False)
    with pytest.raises(ValueError, match="carries events"):
        without.check_state_dict(sd)
    with pytest.raises(ValueError, match="events"):
        env.check_state_dict(checkpoint.to_plain(without.state_dict()))
    assert "event_terms" not in without.state_fingerprint() and "events" not in without.state_dict()
    assert checkpoint.FORMAT == 1
