"""The history tasks end to end on the device ("History"): ``...-Servo-History-v0`` observes 135 floats,
its ``obs_buf["policy"]`` is the row's history field and equals the twin after every step, two PPO iterations run through the
fused env step, ``evaluate_policy`` and the periodic evaluator's env keep the history, a run resumed after two iterations is
the same run, and the exported ``model.pt`` takes ``[1, 135]``."""
import json

import numpy as np
import pytest
import torch

import servo_history_twin as HT
import servo_obs_twin as OT
import servo_twin as T
import test_gpu_servo_obs as GO
import test_servo_history_twin as HC

pytestmark = pytest.mark.gpu

U32 = np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-History-v0"
PLAY = "Isaac-Velocity-CaT-Flat-Solo12-Servo-History-Play-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-History-v0"
_same_bits = GO._same_bits


def test_env_observes_the_history_field_and_it_equals_the_twin_after_every_step():
    from cat_envs import native
    n, steps = 64, 20
    cfg = GO._env_cfg(TASK, n)
    env = GO._make_env(cfg, TASK).unwrapped
    sim = env.sim
    assert env.max_episode_length == 7 and env.obs_dim == 135 and env.single_observation_space["policy"].shape == (135,)
    assert sim.P == 45 and sim.T == 135 and sim.F == sim.row_floats + 136 and sim._desc.reserved == native.SERVO_EXT_HISTORY
    assert sim.off["policy_obs_hist"] == (sim.row_floats, 135) and sim.row_floats == 356 + 48
    assert env.obs_buf["policy"].data_ptr() == sim.view("policy_obs_hist").data_ptr()
    assert env.observation_manager.group_obs_dim == {"policy": (135,)} and "history 3" in str(env.observation_manager)
    assert sim.state_dict()["cur"].shape == (n, sim.F)                       # the run state holds the whole stride
    table = HC.table_of(HC.group_with(group_depth=3))
    np.testing.assert_array_equal(sim.history_words, np.asarray(table.history, U32))
    # the oracle env on the twin: the row without a robot (identity tables change no bit), observed through the history field
    mgr = env.constraint_manager
    ep0 = env.episode_length_buf.cpu().numpy()
    inner = OT.make_twin(cfg, n, table[0], seed=int(cfg.seed) + int(cfg.synthetic.seed_offset), max_len=7)
    twin = HT.ServoHistoryTwin(inner, np.asarray(table.history, U32))
    orc = T.ServoEnvOracle(twin, T.oracle_terms(cfg.constraints), T.oracle_curriculum(cfg.curriculum), ep0,
                           cfg.sim.dt * cfg.decimation, tau=mgr.cat.tau, min_p=mgr.cat.min_p)
    orc.off = {**twin.off, "obs": twin.off["policy_obs_hist"]}
    obs = env.reset()[0]["policy"]
    _same_bits(obs.cpu().numpy(), orc.reset()[0]["policy"].numpy(), "first observation")
    rs = np.random.RandomState(7)
    for s in range(steps):
        a = torch.from_numpy((rs.standard_normal((n, 12)) * 2).astype(np.float32))     # large enough to fall
        obs, rew, dones, time_outs, _ = env.step(a.cuda())
        o_obs, o_rew, o_dones, o_time_outs, _ = orc.step(a)
        _same_bits(obs["policy"].cpu().numpy(), o_obs["policy"].numpy(), f"policy observation after step {s}")
        _same_bits(rew.cpu().numpy(), o_rew.numpy().astype(np.float32), f"reward_buf after step {s}")
        _same_bits(dones.cpu().numpy(), o_dones.numpy().astype(np.float32), f"dones after step {s}")
        # the row below the act_hist field is the twin's row, the current frame included
        _same_bits(sim.cur[:, :356].cpu().numpy(), orc.stream[0][:, :356], f"simulator row after step {s}")
    assert (orc.stream[0][:, twin.off["servo"][0] + 13] >= 2).all()
    # every depth 1: no history descriptor, the launch and the row of the -Servo-Obs task
    plain = GO._make_env(GO._env_cfg(GO.TASK, 16), GO.TASK).unwrapped
    assert plain.sim._desc.reserved == native.SERVO_EXT_OBS and plain.sim.F == plain.sim.row_floats == 356 and plain.sim.T == 0


def test_two_ppo_iterations_evaluation_and_export(tmp_path):
    from cat_envs.tasks.utils.cleanrl.evaluate import evaluate_policy
    from cat_envs.tasks.utils.cleanrl.export import export_policy
    from cat_envs.tasks.utils.cleanrl.periodic_eval import make_eval_env_cfg
    n, num_steps = 64, 8
    tr = GO._trainer(GO._env_cfg(TASK, n), num_steps, fused=True, task=TASK)
    env = tr.envs.unwrapped
    assert tr.sink is not None and tr.agent.obs_dim == 135 and env.can_step_into()
    try:
        for _ in range(2):
            tr.run_iteration(log=False)
        torch.cuda.synchronize()
        # the fused step read the history field: the rollout's observation plane is the normalised field of the last row
        st = env._rstep
        assert st.obs_raw == env.sim.view("policy_obs_hist").data_ptr() and st.obs_ld == env.sim.F and st.D == 135
        assert torch.isfinite(tr.obs.float()).all() and torch.isfinite(tr.agent.flat).all() and tr.obs.float().std() > 0
        assert torch.isfinite(env.sim.cur).all()
        # evaluate_policy: its reset fills the history, its policy sees 135 floats
        seen = []

        def policy(obs):
            seen.append(obs.clone())
            return tr.agent(obs)
        res = evaluate_policy(env, policy, 10, fresh_cat_state=True)
        assert np.isfinite(res.per_env).all() and res.per_env[:, 0].min() == 10
        first = seen[0].cpu().numpy().reshape(n, -1)
        assert first.shape == (n, 135)
        for slot in (0, 1):                                                  # the first frame of an episode fills every slot
            np.testing.assert_array_equal(first[:, 3 * slot:3 * slot + 3].view(U32), first[:, 6:9].view(U32))
            np.testing.assert_array_equal(first[:, 27 + 12 * slot:39 + 12 * slot].view(U32), first[:, 51:63].view(U32))
        second = seen[1].cpu().numpy()
        kept = (second[:, 3:6].view(U32) == first[:, 6:9].view(U32)).all(1)  # ... and the next step shifts it (unless it fell)
        assert kept.mean() > 0.9 and (second[kept, 6:9] != second[kept, 3:6]).any()
        by_agent = evaluate_policy(env, tr.agent, 10, fresh_cat_state=True)
        assert np.isfinite(by_agent.per_env).all()
        # the periodic evaluator's env keeps the observation block, so the history: a policy trained on 135 inputs is evaluated on 135
        ecfg = make_eval_env_cfg(GO._env_cfg(TASK, n), 16)
        assert ecfg.observations.policy.history_length == 3 and ecfg.observations.policy.enable_corruption is False
        eval_env = GO._make_env(ecfg, TASK).unwrapped
        assert eval_env.obs_dim == 135 and np.isfinite(evaluate_policy(eval_env, tr.agent, 5).per_env).all()
        # export: both models take 135 inputs, observations.json says whose ring it is
        out = export_policy(tr.agent.state_dict(), str(tmp_path), observation_spec=env.observation_manager.spec())
        model = torch.jit.load(out["jit"])
        assert tuple(model(torch.zeros(1, 135)).shape) == (1, 12)
        with pytest.raises(RuntimeError):
            model(torch.zeros(1, 45))
        spec = json.load(open(out["observations"]))
        assert spec["obs_dim"] == 135 and spec["frame_order"] == "oldest first" and "deployer owns" in spec["history"]
        assert [t["history_length"] for t in spec["terms"]] == [3] * 6
    finally:
        import test_gpu_servo_actuators as GA
        GA._free_graph(tr)


def test_the_reference_history_task_steps_with_all_blocks():
    from cat_envs import native
    cfg = GO._task_cfg(REFERENCE)
    cfg.scene.num_envs, cfg.seed = 16, 42
    env = GO._make_env(cfg, REFERENCE).unwrapped
    sim = env.sim
    assert env.obs_dim == 135 and sim._desc.reserved == native.SERVO_EXT_HISTORY and sim._desc.ev.block and sim._desc.cmd.block
    assert sim.row_floats == 364 + 48 and sim.F == sim.row_floats + 136 and env.event_manager.randomization_enabled
    assert int(sim.randomize_words.view(np.int32)[0]) & 1                    # the real block replaced the neutral one
    env.reset()
    for _ in range(3):
        obs = env.step(torch.zeros(16, 12, device="cuda"))[0]["policy"]
    assert obs.shape == (16, 135) and torch.isfinite(sim.cur).all()
    keep = env.episode_length_buf.cpu().numpy() >= 3
    o = obs.cpu().numpy()
    assert keep.any() and (o[keep, 0:3] != o[keep, 6:9]).any()               # three different frames of base_ang_vel


def test_two_plus_two_iterations_equal_four(tmp_path):
    """64 envs x 8 steps, hidden (64, 64): a run saved after iteration 2 and resumed is the uninterrupted run, bytes of the
    simulator state (the whole stride: the history field is part of it) included; a state made with another history is refused"""
    import test_gpu_resume as RS
    import test_gpu_servo_actuators as GA
    made = []
    build = RS.build

    def cfgs():
        from cat_envs.shim import load_cfg_from_registry
        cfg = GO._task_cfg(TASK)
        RS._shape_env(cfg)
        cfg.scene.num_envs, cfg.seed = 64, 42
        agent_cfg = load_cfg_from_registry(TASK, "clean_rl_cfg_entry_point")
        agent_cfg.num_steps, agent_cfg.minibatch_size, agent_cfg.hidden = 8, 128, (64, 64)
        agent_cfg.updates_epochs, agent_cfg.num_iterations, agent_cfg.save_interval = 1, 4, 10 ** 9
        return TASK, cfg, agent_cfg
    seen = {}

    def probe(env, tr):
        seen["fp"] = env.unwrapped.state_fingerprint()

    def recording_build(c):
        env, tr = build(c)
        made.append(tr)
        return env, tr
    RS.build = recording_build
    try:
        a, b, tr = RS.check_case(cfgs, tmp_path, save_at=2, iters=4, probe=probe)
    finally:
        RS.build = build
        for t in made:
            GA._free_graph(t)
    sim = tr.envs.unwrapped.sim
    h, T_ = sim.off["policy_obs_hist"]
    assert a[-1]["sim.cur"].shape[1] == sim.F == h + 136 and (a[-1]["sim.cur"][:, h:h + T_] != 0).any()
    assert seen["fp"]["obs_dim"] == 135 and [row[2] for row in seen["fp"]["observation_terms"]] == [3] * 6
    # a state of the -Servo-Obs task (the same terms, no history) does not fit this run, and the other way round
    from cat_envs.tasks.utils.cleanrl import checkpoint
    plain = GO._make_env(GO._env_cfg(GO.TASK, 64), GO.TASK).unwrapped.state_fingerprint()
    with pytest.raises(ValueError, match="observation_terms"):
        checkpoint.check_fingerprint(plain, seen["fp"])
    with pytest.raises(ValueError, match="obs_dim"):
        checkpoint.check_fingerprint(seen["fp"], plain)
