"""The servo task's observation terms without a device ("Observations"): the second descriptor, table
building from an ``ObservationsCfg``, the corruption switch, properties of the numpy twin and the run-state fingerprint."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import servo_obs_twin as OT
import servo_reward_twin as RT
import servo_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = np.uint32
TASK = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-v0"
PLAY = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Obs-Play-v0"
# the reference's joint order in joint_pos / joint_vel (hind right before hind left) as indices of the robot's joints
REF_JOINT_ORDER = [0, 1, 2, 3, 4, 5, 9, 10, 11, 6, 7, 8]


def _cfg(task=TASK):
    import cat_envs.tasks  # noqa: F401
    from cat_envs.shim import load_cfg_from_registry
    cfg = load_cfg_from_registry(task, "env_cfg_entry_point")
    cfg.synthetic.servo_resample_steps = 3
    return cfg


def _om():
    from cat_envs.shim import AdditiveUniformNoiseCfg as Unoise
    from cat_envs.shim import ObservationTermCfg as ObsTerm
    from cat_envs.shim import SceneEntityCfg
    from cat_envs.tasks.utils.mdp import observation_manager as OM
    from cat_envs.tasks.utils.mdp import observations as O
    return OM, O, ObsTerm, Unoise, SceneEntityCfg


def reference_table():
    OM = _om()[0]
    return OM.build_table(OM.policy_group(_cfg().observations), T.JOINTS, T.DEFAULT_JOINT_POS)


# ------------------------------------------------------------------------------------------ descriptor
def test_descriptor_layout():
    from cat_envs import native
    assert ctypes.sizeof(native.ServoObsEntry) == 32
    assert [f[0] for f in native.ServoObsEntry._fields_] == ["src", "flags", "bias", "noise_lo", "noise_width", "clip_lo",
                                                             "clip_hi", "scale"]
    assert [f[0] for f in native.ServoObs._fields_] == ["width", "off_policy_obs", "table"]
    assert native.ServoObs.table.offset == 8 and ctypes.sizeof(native.ServoObs) == 16
    # the first descriptor did not grow: the observation descriptor lies behind it, announced by ``reserved``
    assert ctypes.sizeof(native.ServoSimRewards) == 368 and issubclass(native.ServoSimObs, native.ServoSimRewards)
    assert native.ServoSimObs.obs.offset == 368 and ctypes.sizeof(native.ServoSimObs) == 384
    d = native.ServoSimObs()
    assert d.reserved == 0 and d.obs.width == 0 and d.obs.table is None
    src = open(os.path.join(ROOT, "include", "catppo.h")).read()
    assert int(re.search(r"#define CATPPO_SERVO_EXT_OBS (0x[0-9A-Fa-f]+)", src).group(1), 16) == native.SERVO_EXT_OBS
    assert int(re.search(r"#define CATPPO_SERVO_OBS_MAX_WIDTH (\d+)", src).group(1)) == native.SERVO_OBS_MAX_WIDTH == 64
    assert (native.SERVO_OBS_BIAS, native.SERVO_OBS_NOISE, native.SERVO_OBS_CLIP) == (OT.BIAS, OT.NOISE, OT.CLIP)
    assert len(native.EXPORTS) == 59                                         # no new export


def test_servo_sim_step_refuses_a_short_descriptor_that_announces_observations():
    """the library reads the observation descriptor behind the 368 bytes when ``reserved`` says so: only a ServoSimObs may"""
    from cat_envs import native
    for short in (native.ServoSim(), native.ServoSimStep()):
        short.reserved = native.SERVO_EXT_OBS
        with pytest.raises(TypeError, match="ServoSimRewards"):
            native.Native.servo_sim_step(types.SimpleNamespace(), short)
    d = native.ServoSimRewards()
    d.reserved = native.SERVO_EXT_OBS
    with pytest.raises(TypeError, match="ServoSimObs"):
        native.Native.servo_sim_step(types.SimpleNamespace(), d)


# ------------------------------------------------------------------------------------------ table building
def test_reference_cfg_builds_the_reference_table():
    OM, O = _om()[:2]
    entries, dims = reference_table()
    assert list(dims) == ["base_ang_vel", "velocity_commands", "projected_gravity", "joint_pos", "joint_vel", "actions"]
    assert list(dims.values()) == [(3,), (3,), (3,), (12,), (12,), (12,)] and len(entries) == 45
    src = [e[0] for e in entries]
    assert src == ([0, 1, 2] + [6, 7, 8] + [3, 4, 5] + [9 + j for j in REF_JOINT_ORDER] + [21 + j for j in REF_JOINT_ORDER]
                   + list(range(33, 45)))
    f = lambda x: float(F32(x))                                              # noqa: E731
    assert [e[7] for e in entries] == ([f(0.25)] * 3 + [2.0, 2.0, 0.25] + [f(0.1)] * 3 + [1.0] * 12 + [f(0.05)] * 12 + [1.0] * 12)
    assert [e[2] for e in entries[9:21]] == [float(T.DEFAULT_JOINT_POS[j]) for j in REF_JOINT_ORDER]      # joint_pos = dq + default
    assert all(e[1] == OT.BIAS | OT.NOISE for e in entries[9:21])
    assert all(e[1] == OT.NOISE for e in entries[0:3] + entries[6:9] + entries[21:33])
    assert all(e[1] == 0 for e in entries[3:6] + entries[33:45])
    lo_width = lambda a, b: (f(a), f(b - a))                                 # noqa: E731
    assert entries[0][3:5] == lo_width(-0.001, 0.001) and entries[6][3:5] == lo_width(-0.05, 0.05)
    assert entries[9][3:5] == lo_width(-0.01, 0.01) and entries[21][3:5] == lo_width(-0.2, 0.2)
    group = OM.policy_group(_cfg().observations)
    assert group.enable_corruption is True and OM.policy_group(_cfg(PLAY).observations).enable_corruption is False
    for task in ("Isaac-Velocity-CaT-Flat-Solo12-v0", T.TASK, "Isaac-Velocity-CaT-Flat-Solo12-Servo-Rewards-v0"):
        assert not hasattr(_cfg(task), "observations")


def test_terms_describe_and_are_never_called():
    OM, O, ObsTerm, Unoise, SceneEntityCfg = _om()
    env = types.SimpleNamespace(scene={"robot": types.SimpleNamespace(joint_names=list(T.JOINTS), body_names=[])},
                                default_joint_pos=[float(v) for v in T.DEFAULT_JOINT_POS])
    widths = dict(base_ang_vel=3, projected_gravity=3, generated_commands=3, joint_pos=12, joint_pos_rel=12, joint_vel=12,
                  joint_vel_rel=12, last_action=12)
    for name, w in widths.items():
        func = getattr(O, name)
        kw = {"command_name": "base_velocity"} if name == "generated_commands" else {}
        with pytest.raises(TypeError, match="inside the simulator launch"):
            func(None, **kw)
        assert len(func.describe(env, **kw)) == w
    sub = SceneEntityCfg("robot", joint_names=["HR_KFE", "FL_HAA", "FR_HFE"], preserve_order=True)
    entries, dims = OM.build_table({"q": ObsTerm(func=O.joint_pos_rel, params={"asset_cfg": sub}),
                                    "qd": ObsTerm(func=O.joint_vel_rel, params={"asset_cfg": sub}, scale=(1.0, 2.0, 3.0),
                                                  clip=(-1.0, 1.5))}, T.JOINTS, T.DEFAULT_JOINT_POS)
    assert [e[0] for e in entries] == [9 + 11, 9 + 0, 9 + 4, 21 + 11, 21 + 0, 21 + 4] and dims == {"q": (3,), "qd": (3,)}
    assert [e[7] for e in entries[3:]] == [1.0, 2.0, 3.0] and all(e[1] == OT.CLIP and e[5:7] == (-1.0, 1.5) for e in entries[3:])
    unordered = SceneEntityCfg("robot", joint_names=["HR_KFE", "FL_HAA"])
    assert [e[0] for e in OM.build_table({"q": ObsTerm(func=O.joint_pos, params={"asset_cfg": unordered})}, T.JOINTS,
                                         T.DEFAULT_JOINT_POS)[0]] == [9, 20]


def test_table_errors_name_the_term():
    OM, O, ObsTerm, Unoise, SceneEntityCfg = _om()
    build = lambda cfg: OM.build_table(cfg, T.JOINTS, T.DEFAULT_JOINT_POS)   # noqa: E731
    six = {f"t{i}": ObsTerm(func=O.last_action) for i in range(6)}
    with pytest.raises(ValueError, match="'t5'.*at most 64"):
        build(six)
    five = {k: v for k, v in six.items() if k != "t5"}
    five["g"] = ObsTerm(func=O.projected_gravity)
    five["one"] = ObsTerm(func=O.joint_vel, params={"asset_cfg": SceneEntityCfg("robot", joint_names=["FL_KFE"])})
    assert len(build(five)[0]) == 64                                         # sixty-four fit
    with pytest.raises(ValueError, match="'cmd'.*scale has 2 elements, the term has 3"):
        build({"cmd": ObsTerm(func=O.generated_commands, params={"command_name": "x"}, scale=(1.0, 2.0))})
    with pytest.raises(ValueError, match="'w'.*clip lo 1.0 > hi -1.0"):
        build({"w": ObsTerm(func=O.base_ang_vel, clip=(1.0, -1.0))})
    with pytest.raises(ValueError, match="'w'.*n_max -0.1 < n_min 0.1"):
        build({"w": ObsTerm(func=O.base_ang_vel, noise=Unoise(n_min=0.1, n_max=-0.1))})
    with pytest.raises(ValueError, match="'w'.*only additive uniform noise"):
        build({"w": ObsTerm(func=O.base_ang_vel, noise=types.SimpleNamespace(mean=0.0, std=1.0))})
    with pytest.raises(ValueError, match="'w'.*only additive uniform noise"):
        build({"w": ObsTerm(func=O.base_ang_vel, noise=Unoise(n_min=0.9, n_max=1.1, operation="scale"))})
    with pytest.raises(ValueError, match="'mine'.*describe"):
        build({"mine": ObsTerm(func=lambda env: 0.0)})
    with pytest.raises(ValueError, match="concatenate_terms"):
        build({"concatenate_terms": False, "w": ObsTerm(func=O.base_ang_vel)})
    with pytest.raises(ValueError, match="no name matches"):
        build({"q": ObsTerm(func=O.joint_pos, params={"asset_cfg": SceneEntityCfg("robot", joint_names=["nothing"])})})
    with pytest.raises(ValueError, match="exactly the group 'policy'"):
        OM.policy_group({"policy": {"w": ObsTerm(func=O.base_ang_vel)}, "critic": {"w": ObsTerm(func=O.base_ang_vel)}})


class _Sim:
    def __init__(self):
        self.pushed = []

    def set_observation_table(self, entries):
        self.pushed.append(list(entries))


def _manager(task=TASK):
    OM = _om()[0]
    sim = _Sim()
    env = types.SimpleNamespace(sim=sim, scene={"robot": types.SimpleNamespace(joint_names=list(T.JOINTS), body_names=[])})
    return OM.ObservationManager(_cfg(task).observations, env), sim


def test_set_corruption_clears_exactly_the_noise_bits():
    mgr, sim = _manager()
    built = reference_table()[0]
    assert mgr.corruption is True and sim.pushed == [built] and mgr.entries == built
    mgr.set_corruption(True)
    assert len(sim.pushed) == 1                                              # nothing to rewrite
    mgr.set_corruption(False)
    off = sim.pushed[-1]
    assert len(sim.pushed) == 2 and mgr.corruption is False
    for a, b in zip(built, off):
        assert b[1] == a[1] & ~OT.NOISE and (b[0], *b[2:]) == (a[0], *a[2:])
    assert any(a[1] != b[1] for a, b in zip(built, off))
    mgr.set_corruption(True)
    assert sim.pushed[-1] == built
    assert mgr.active_terms == {"policy": ["base_ang_vel", "velocity_commands", "projected_gravity", "joint_pos", "joint_vel", "actions"]}
    assert mgr.group_obs_dim == {"policy": (45,)} and mgr.group_obs_term_dim["policy"][3] == (12,)
    play, psim = _manager(PLAY)
    assert play.corruption is False and all(not e[1] & OT.NOISE for e in psim.pushed[0])
    assert play.fingerprint() == mgr.fingerprint()                           # the switch is state, not fingerprint
    mgr.load_state_dict(play.state_dict())
    assert mgr.corruption is False and sim.pushed[-1] == psim.pushed[0]
    spec = mgr.spec()
    assert spec["obs_dim"] == 45 and spec["terms"][3]["slice"] == [9, 21] and spec["terms"][3]["src_names"][6] == "joint_pos_rel:HR_HAA"
    assert spec["terms"][1]["scale"] == [2.0, 2.0, 0.25] and spec["terms"][1]["noise"] is None
    import json
    json.dumps(spec)


# ------------------------------------------------------------------------------------------ the twin
N, STEPS = 64, 50


@pytest.fixture(scope="module")
def runs():
    acts, ep0 = RT.recipe(N)
    built = reference_table()[0]
    out = {}
    for name, table in (("identity", OT.identity_table()), ("clean", OT.with_corruption(built, False)), ("noisy", built)):
        tw = OT.make_twin(_cfg(), N, table)
        out[name] = (tw, OT.run_obs_twin(tw, acts, ep0))
    plain = RT.run_reward_twin(RT.make_twin(_cfg(), N, []), acts, ep0)[0]
    return acts, ep0, out, plain


def test_identity_table_reproduces_the_raw_field_and_nothing_else_moves(runs):
    acts, ep0, out, plain = runs
    tw, slabs = out["identity"]
    assert slabs.shape == (STEPS + 1, N, tw.F) and tw.F == tw.F_raw + 48 and tw.off["policy_obs"] == (tw.F_raw, 45)
    a, w = tw.off["obs"]
    p = tw.off["policy_obs"][0]
    np.testing.assert_array_equal(slabs[:, :, p:p + 45].view(U32), slabs[:, :, a:a + w].view(U32))
    assert (slabs[:, :, p + 45:] == 0).all()                                 # the padding
    for name in out:
        np.testing.assert_array_equal(out[name][1][:, :, :tw.F_raw].view(U32), plain.view(U32))
    falls = int((slabs[:, :, tw.off["hard_reset"][0]] > 0).sum())
    episodes = slabs[-1, :, tw.off["servo"][0] + 13]
    assert falls > 0 and episodes.sum() > falls and episodes.min() >= 6      # falls and time-outs both end episodes


def test_noise_draws_are_distinct_from_the_command_and_init_draws(runs):
    """the counters of the three families differ in their fourth word, and within the observation family in (episode,
    t', block): every draw of an env is its own Philox block"""
    acts, ep0, out, plain = runs
    tw, slabs = out["noisy"]
    assert len({OT.TAG_OBS, T.TAG_COMMAND, T.TAG_INIT}) == 3
    ep_len = np.asarray(ep0, np.int64).copy()
    keys = [(np.zeros(N, np.int64), np.zeros(N, np.int64))]
    for s in range(STEPS):
        ep, t = tw.key_of(slabs[s + 1], ep_len)
        keys.append((ep.astype(np.int64), t))
        ep_len = np.where(t == 0, 0, ep_len + 1)
    ctr = set()
    count = 0
    for ep, t in keys[1:]:                                                   # the init key (0, 0) may recur: see below
        for b in range(12):
            for i in range(N):
                ctr.add((i, int(ep[i]), (int(t[i]) << 4) | b, OT.TAG_OBS))
                count += 1
    assert len(ctr) == count                                                 # pairwise distinct within the family
    # an env's init observation shares its key only with nothing: episode 0 at t' = 0 is never the result of a step
    assert all(not ((ep == 0) & (t == 0)).any() for ep, t in keys[1:])
    for tag in (T.TAG_COMMAND, T.TAG_INIT):
        assert all(c[3] != tag for c in ctr)
    u_obs = tw.uniforms(np.zeros(N, np.uint32), np.zeros(N, np.int64))[:, :12]
    u_cmd = tw._philox(np.zeros(N, np.uint32), 0, T.TAG_COMMAND)
    u_init = np.concatenate([tw._philox(np.zeros(N, np.uint32), b, T.TAG_INIT) for b in range(3)], 1)
    assert not np.isin(u_obs, u_cmd).any() and not np.isin(u_obs, u_init).any()


def test_noisy_values_lie_within_the_configured_range_of_the_clean_ones(runs):
    """before the scale, clean = raw + bias and noisy = ((raw + bias) + u w) + lo with u in (0, 1): they differ by a value in
    [n_min, n_max] up to the rounding of the two adds, 1 ulp of the larger magnitude each; the scale is one more rounded
    multiply of either"""
    acts, ep0, out, plain = runs
    tw, noisy = out["noisy"]
    clean = out["clean"][1]
    p, a = tw.off["policy_obs"][0], tw.off["obs"][0]
    unscaled = OT.make_twin(_cfg(), N, [(*e[:7], 1.0) for e in tw.obs_table])
    noisy1 = OT.run_obs_twin(unscaled, acts, ep0)[:, :, p:p + 45]
    unscaled.set_obs_table(OT.with_corruption(unscaled.obs_table, False))
    clean1 = OT.run_obs_twin(unscaled, acts, ep0)[:, :, p:p + 45]
    moved = 0
    for j, (src, flags, bias, nlo, nwidth, clo, chi, scale) in enumerate(tw.obs_table):
        np.testing.assert_array_equal((noisy1[:, :, j] * scale).astype(F32).view(U32), noisy[:, :, p + j].view(U32))
        np.testing.assert_array_equal((clean1[:, :, j] * scale).astype(F32).view(U32), clean[:, :, p + j].view(U32))
        if flags & OT.NOISE:
            hi = F32(nlo + nwidth)
            mag = np.maximum(np.abs(noisy1[:, :, j]), np.abs(clean1[:, :, j])) + max(abs(nlo), abs(hi))
            slack = 2 * np.spacing(mag.astype(F32)).astype(np.float64)
            d = noisy1[:, :, j].astype(np.float64) - clean1[:, :, j].astype(np.float64)
            assert (d >= np.float64(nlo) - slack).all() and (d <= np.float64(hi) + slack).all(), j
            moved += int((noisy1[:, :, j] != clean1[:, :, j]).sum())
        else:
            np.testing.assert_array_equal(noisy1[:, :, j].view(U32), clean1[:, :, j].view(U32))
    assert moved > 0.9 * 30 * (STEPS + 1) * N                                # 30 of the 45 floats are noisy
    np.testing.assert_array_equal(clean[:, :, p + 33:p + 45].view(U32), plain[:, :, a + 33:a + 45].view(U32))


def test_clip_passes_nan_and_binds():
    tw = OT.make_twin(_cfg(), 4, [(0, OT.CLIP, 0.0, 0.0, 0.0, -0.5, 0.25, 2.0)])
    raw = np.zeros((4, 45), F32)
    raw[:, 0] = [np.nan, -3.0, 0.125, 7.0]
    got = tw.policy(raw, np.zeros(4, np.uint32), np.zeros(4, np.int64))[:, 0]
    assert np.isnan(got[0]) and list(got[1:]) == [-1.0, 0.25, 0.5]


# ------------------------------------------------------------------------------------------ run state
def _fingerprint(with_observations):
    from cat_envs.tasks.utils.cat.cat_env import CaTEnv
    cfg = _cfg()
    fake = types.SimpleNamespace(cfg=cfg, sim=types.SimpleNamespace(fingerprint=lambda: {"servo": {}}), num_envs=8, obs_dim=45,
                                 act_dim=12, max_episode_length=7, exact_reset_sync=False, device="cpu")
    if with_observations:
        fake.observation_manager = _manager()[0]
    return CaTEnv.state_fingerprint(fake)


def test_fingerprint_is_unchanged_without_observations_and_extended_with_them():
    from cat_envs.tasks.utils.cleanrl import checkpoint
    plain, obs = _fingerprint(False), _fingerprint(True)
    assert sorted(plain) == sorted(["task_kind", "num_envs", "obs_dim", "act_dim", "env_seed", "seed_offset", "env_offset",
                                    "max_episode_length", "decimation", "exact_reset_sync", "constraint_terms", "servo"])
    assert sorted(obs) == sorted([*plain, "observation_terms"]) and all(obs[k] == plain[k] for k in plain)
    terms = obs["observation_terms"]
    assert [t[0] for t in terms] == ["base_ang_vel", "velocity_commands", "projected_gravity", "joint_pos", "joint_vel", "actions"]
    assert terms[1][1] == [[6, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0], [7, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0], [8, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25]]
    assert checkpoint.FORMAT == 1
    with pytest.raises(ValueError, match="observation_terms"):
        checkpoint.check_fingerprint(obs, plain)
    with pytest.raises(ValueError, match="observation_terms"):
        checkpoint.check_fingerprint(plain, obs)


# ------------------------------------------------------------------------------------------ export
def test_export_writes_the_input_contract_next_to_the_models(tmp_path):
    import json
    import torch
    from cat_envs.tasks.utils.cleanrl import export as EX
    from oracle import ppo_oracle as PO
    sd = PO.AgentOracle(45, 12).state_dict()
    spec = _manager()[0].spec()
    out = EX.export_policy(sd, str(tmp_path / "exported"), observation_spec=spec)
    assert sorted(out) == ["jit", "observations", "onnx"] and all(os.path.isfile(p) for p in out.values())
    got = json.load(open(out["observations"]))
    assert got == spec and got["obs_dim"] == 45 and [t["name"] for t in got["terms"]][:2] == ["base_ang_vel", "velocity_commands"]
    assert got["joint_order"] == T.JOINTS and got["terms"][4]["scale"] == [float(F32(0.05))] * 12 and got["terms"][3]["clip"] is None
    plain = EX.export_policy(sd, str(tmp_path / "plain"))                   # without a spec: the two models only, as before
    assert sorted(plain) == ["jit", "onnx"] and not os.path.exists(tmp_path / "plain" / "observations.json")
    assert torch.jit.load(out["jit"], map_location="cpu")(torch.zeros(1, 45)).shape == (1, 12)
