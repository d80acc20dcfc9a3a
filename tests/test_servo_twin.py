"""The Solo12 servo surrogate on the CPU: its numpy twin (tests/servo_twin.py) is deterministic, closed loop, shard
consistent and keeps the constraint terms alive; PPOOracle learns on it.  No GPU needed."""
import json
import os

import numpy as np
import torch

import servo_twin as T
from oracle import env_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-v0"

# terms the model cannot drive under white-noise actions (DESIGN section 9 names each with its reason): at most 3
EXEMPT = {"front_hfe_position"}


def _cfg():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    return load_cfg_from_registry(TASK, "env_cfg_entry_point")


def _twin(n, max_len=7, offset=0, obs_dim=45, seed=5):
    cfg = _cfg()
    return T.ServoTwin(n, obs_dim, T.params_from_cfg(cfg.synthetic), seed, max_len, cfg.sim.dt, cfg.decimation, offset)


_run = T.run_twin


def test_task_is_registered_and_the_default_simulator_is_unchanged():
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = _cfg()
    assert cfg.synthetic.kind == "servo" and len(T.oracle_terms(cfg.constraints)) == 13
    assert load_cfg_from_registry(TASK.replace("-v0", "-Play-v0"), "env_cfg_entry_point").synthetic.kind == "servo"
    assert load_cfg_from_registry("Isaac-Velocity-CaT-Flat-Solo12-v0", "env_cfg_entry_point").synthetic.kind == "stream"
    from cat_envs import native
    assert "catppo_servo_sim_step" in native.EXPORTS


def test_twin_is_deterministic_and_closed_loop():
    rs = np.random.RandomState(0)
    acts = rs.standard_normal((20, 64, 12)).astype(np.float32)
    ep0 = rs.randint(0, 7, 64)
    a, b = _run(_twin(64), acts, ep0), _run(_twin(64), acts, ep0)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(a).all()
    # another action in ONE env at step 3 changes that env's next state (joints, base, reward, observation), nobody else's
    acts2 = acts.copy()
    acts2[3, 5] += 1.0
    c = _run(_twin(64), acts2, ep0)
    np.testing.assert_array_equal(a[:4], c[:4])
    others = np.arange(64) != 5
    np.testing.assert_array_equal(a[:, others], c[:, others])
    tw = _twin(64)
    for name in ("joint_pos", "joint_vel", "applied_torque", "reward", "obs"):
        lo, w = tw.off[name]
        assert (a[4, 5, lo:lo + w] != c[4, 5, lo:lo + w]).any(), name
    # resets happened (max_episode_length = 7) and the episode counter in the row moved with them
    lo, _ = tw.off["servo"]
    assert a[-1, :, lo + 13].min() >= 2


def test_post_reset_observation_is_the_first_state_of_the_next_episode():
    rs = np.random.RandomState(1)
    acts = rs.standard_normal((16, 32, 12)).astype(np.float32)
    tw = _twin(32)
    s = _run(tw, acts, np.zeros(32, np.int64))
    lo, _ = tw.off["obs"]
    ep = s[:, :, tw.off["servo"][0] + 13]
    for t in range(1, 16):
        ended = ep[t] > ep[t - 1]
        if not ended.any():
            continue
        obs = s[t, ended, lo:lo + 45]
        assert (obs[:, :5] == 0).all() and (obs[:, 5] == -1).all() and (obs[:, 21:] == 0).all()
        q0 = tw.init_q(ep[t].astype(np.uint32))[ended]
        np.testing.assert_array_equal(obs[:, 9:21], q0 - T.DEFAULT_JOINT_POS)
        np.testing.assert_array_equal(obs[:, 6:9], tw.command(ep[t].astype(np.uint32), 0)[ended])
        # ... while the fields the terms read are the terminal state's: the joints did not jump to the new pose
        jp = s[t, ended, :12]
        assert (jp != q0).any()
        # and the next step integrates from exactly that first state: its command is the announced one
        c0, _ = tw.off["command"]
        np.testing.assert_array_equal(s[t + 1, ended, c0:c0 + 3], obs[:, 6:9])
    assert (ep[-1] >= 2).all()


def test_shards_reproduce_the_union():
    rs = np.random.RandomState(2)
    acts = rs.standard_normal((20, 64, 12)).astype(np.float32)
    ep0 = rs.randint(0, 7, 64)
    whole = _run(_twin(64), acts, ep0)
    lo = _run(_twin(32, offset=0), acts[:, :32], ep0[:32])
    hi = _run(_twin(32, offset=32), acts[:, 32:], ep0[32:])
    np.testing.assert_array_equal(whole[:, :32].view(np.uint32), lo.view(np.uint32))
    np.testing.assert_array_equal(whole[:, 32:].view(np.uint32), hi.view(np.uint32))


def test_observation_is_padded_or_truncated_to_obs_dim():
    rs = np.random.RandomState(3)
    acts = rs.standard_normal((5, 8, 12)).astype(np.float32)
    ref = _run(_twin(8), acts, np.zeros(8, np.int64))
    o45 = _twin(8).off["obs"][0]
    for d in (20, 48):
        tw = _twin(8, obs_dim=d)
        s = _run(tw, acts, np.zeros(8, np.int64))
        lo, _ = tw.off["obs"]
        w = min(d, 45)
        np.testing.assert_array_equal(s[:, :, lo:lo + w], ref[:, :, o45:o45 + w])
        assert (s[:, :, lo + w:lo + d] == 0).all()


def test_every_constraint_term_is_alive_under_white_noise_actions():
    """N(0,1) actions, 256 envs x 200 steps of the default task: every term of the full 13-term ConstraintsCfg is
    violated at least once and satisfied at least once, except the named exemptions"""
    cfg = _cfg()
    n = 256
    rs = np.random.RandomState(0)
    env = T.env_oracle_from_cfg(cfg, n, rs.randint(0, 500, n))
    seen = {t["name"]: [0, 0] for t in env.terms}
    for _ in range(200):
        env.step(torch.from_numpy(rs.standard_normal((n, 12)).astype(np.float32)))
        st = env._state(env.stream[0])
        for t in env.terms:
            v = np.asarray(EO._TERMS[t["func"]](st, t["params"], t.get("joints"), t.get("bodies")), np.float32)
            seen[t["name"]][0] += int((v > 0).sum())
            seen[t["name"]][1] += int((v <= 0).sum())
    print(seen)
    assert len(seen) == 13 and len(EXEMPT) <= 3 and EXEMPT <= set(seen)
    for name, (violated, satisfied) in seen.items():
        assert satisfied > 0, name
        if name not in EXEMPT:
            assert violated > 0, name


def test_ppo_oracle_learns_on_the_twin():
    """256 envs x 24 steps, hidden (128, 128), 30 iterations of the unchanged PPOOracle on the closed-loop twin env: the
    reward per step rises and the share of env steps with a violated constraint falls by at least half of what the
    recorded run (profiles/servo_learning_oracle.json, tools/servo_learning_oracle.py) shows - half: seed-to-seed allowance."""
    with open(os.path.join(ROOT, T.LEARNING_PROFILE)) as f:
        rec = json.load(f)
    assert rec["reward_gain"] > 0.2 and rec["violation_drop"] > 0.1, "the recorded run itself must show learning"
    torch.set_num_threads(min(8, torch.get_num_threads()))
    reward, violation = T.run_oracle_learning(seed=7)            # not the recorded seed
    got = T.learning_summary(reward, violation)
    print(got, reward, violation)
    assert got["reward_gain"] >= 0.5 * rec["reward_gain"], (got, rec["reward_gain"])
    assert got["violation_drop"] >= 0.5 * rec["violation_drop"], (got, rec["violation_drop"])
