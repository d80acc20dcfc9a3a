"""``history_length`` on observation terms and groups without a device ("History"): the four cfg fields, the
dims IsaacLab's names report, the input contract, the history map's words, the errors that name the term, the run-state
fingerprint and the four tasks."""
import json
import types

import numpy as np
import pytest

import servo_twin as T
import test_servo_history_twin as HC
import test_servo_obs_twin as OC

NAMES = ["base_ang_vel", "velocity_commands", "projected_gravity", "joint_pos", "joint_vel", "actions"]
HISTORY = "Isaac-Velocity-CaT-Flat-Solo12-Servo-History-v0"
REFERENCE = "Isaac-Velocity-CaT-Flat-Solo12-Servo-Reference-History-v0"


class _Sim:
    def __init__(self):
        self.tables, self.maps = [], []

    def set_observation_table(self, entries):
        self.tables.append(list(entries))

    def set_history_table(self, words):
        self.maps.append(list(words))

    def view(self, name):
        return name


def manager_of(group):
    OM = OC._om()[0]
    sim = _Sim()
    env = types.SimpleNamespace(sim=sim, scene={"robot": types.SimpleNamespace(joint_names=list(T.JOINTS), body_names=[])})
    return OM.ObservationManager({"policy": group}, env), sim


def test_the_shim_has_the_four_fields_with_isaaclabs_defaults():
    from cat_envs.shim import ObservationGroupCfg, ObservationTermCfg
    from cat_envs.tasks.utils.mdp import observations as O
    term = ObservationTermCfg(func=O.joint_pos)
    assert term.history_length == 0 and term.flatten_history_dim is True
    assert ObservationTermCfg(func=O.joint_pos, history_length=4, flatten_history_dim=False).history_length == 4
    group = ObservationGroupCfg()
    assert group.history_length is None and group.flatten_history_dim is True


def test_a_dict_group_with_depth_three_reports_135_floats():
    """the parent accepted the group's ``history_length`` and ignored it: it reported 45"""
    mgr, sim = manager_of(HC.group_with(group_depth=3))
    assert mgr.group_obs_dim == {"policy": (135,)}
    assert mgr.group_obs_term_dim == {"policy": [(9,), (9,), (9,), (36,), (36,), (36,)]}
    assert mgr.active_terms == {"policy": NAMES} and mgr.history_lengths == dict.fromkeys(NAMES, 3) and mgr.has_history
    # the table of the current frame is the reference's 45 entries; the map went to the simulator once, behind the table
    assert sim.tables == [OC.reference_table()[0]] and len(sim.maps) == 1 and len(sim.maps[0]) == 135
    assert mgr.compute() == {"policy": "policy_obs_hist"}
    spec = mgr.spec()
    assert spec["obs_dim"] == 135 and spec["frame_dim"] == 45 and spec["frame_order"] == "oldest first"
    assert [t["slice"] for t in spec["terms"]] == [[0, 9], [9, 18], [18, 27], [27, 63], [63, 99], [99, 135]]
    assert [t["frame_slice"] for t in spec["terms"]] == [[0, 3], [3, 6], [6, 9], [9, 21], [21, 33], [33, 45]]
    assert [t["history_length"] for t in spec["terms"]] == [3] * 6 and "deployer owns" in spec["history"]
    assert spec["terms"][3]["src_names"][6] == "joint_pos_rel:HR_HAA" and len(spec["terms"][3]["scale"]) == 12
    assert json.loads(json.dumps(spec)) == spec
    assert "history 3" in str(mgr) and "135 floats" in str(mgr)
    # corruption rewrites the table and leaves the map alone
    mgr.set_corruption(False)
    assert len(sim.tables) == 2 and len(sim.maps) == 1


def test_the_class_cfg_of_the_history_tasks_is_that_group():
    OM = OC._om()[0]
    for task in (HISTORY, REFERENCE):
        table = HC.table_of(OM.policy_group(OC._cfg(task).observations))
        assert table.history_floats == 135 and list(table.depths.values()) == [3] * 6 and table[0] == OC.reference_table()[0]
    play = OC._cfg(HISTORY.replace("-v0", "-Play-v0"))
    assert play.observations.policy.enable_corruption is False and play.observations.policy.history_length == 3
    ref, rnd = OC._cfg(REFERENCE), OC._cfg(REFERENCE.replace("-History", "-Randomized"))
    assert sorted(ref.events.__dict__) == sorted(rnd.events.__dict__) and ref.scene.robot is not None
    assert all(a.max_delay == 4 and a.min_delay == 0 for a in ref.scene.robot.actuators.values())
    play = OC._cfg(REFERENCE.replace("-v0", "-Play-v0"))
    assert play.observations.policy.enable_corruption is False and play.pushes is False and play.scene.num_envs == 50


def test_per_term_depths_dims_spec_and_map():
    depths = [3, 1, 5, 0, 2, 16]
    mgr, sim = manager_of(HC.group_with(depths=depths))
    eff = [3, 1, 5, 1, 2, 16]
    want = [h * w for h, w in zip(eff, HC.WIDTHS)]
    assert mgr.group_obs_term_dim == {"policy": [(x,) for x in want]} and mgr.group_obs_dim == {"policy": (sum(want),)}
    assert sum(want) == 9 + 3 + 15 + 12 + 24 + 192
    spec = mgr.spec()
    ends = np.cumsum(want)
    assert [t["slice"] for t in spec["terms"]] == [[int(e - x), int(e)] for e, x in zip(ends, want)]
    assert [t["history_length"] for t in spec["terms"]] == eff and spec["frame_dim"] == 45
    # the map: cur | w << 8 | newest << 16, a term's slots one after the other, oldest first
    words = sim.maps[0]
    assert words[:9] == [0x300, 0x301, 0x302, 0x300, 0x301, 0x302, 0x10300, 0x10301, 0x10302]
    assert words[9:12] == [0x10303, 0x10304, 0x10305]                        # depth 1: the newest slot alone
    assert words[12:15] == [0x306, 0x307, 0x308] and words[24:27] == [0x10306, 0x10307, 0x10308]
    assert words[27] == (9 | 12 << 8 | 1 << 16) and words[39] == (21 | 12 << 8) and words[51] == (21 | 12 << 8 | 1 << 16)
    assert words[-1] == (44 | 12 << 8 | 1 << 16) and words[-13] == (44 | 12 << 8) and len(words) == sum(want)


def test_all_depths_one_attaches_no_history():
    for group in (HC.group_with(), HC.group_with(depths=[1, 0, 1, 0, 1, 0]), HC.group_with(depths=[4] * 6, group_depth=1)):
        mgr, sim = manager_of(group)
        assert not mgr.has_history and sim.maps == [] and mgr.group_obs_dim == {"policy": (45,)}
        assert mgr.compute() == {"policy": "policy_obs"} and mgr.spec()["obs_dim"] == 45


def test_errors_name_the_term():
    OM, O, ObsTerm, Unoise, Entity = OC._om()
    build = HC.table_of
    with pytest.raises(ValueError, match=r"'joint_pos'.*history_length must be >= 0, got -1"):
        build(HC.group_with(depths=[0, 0, 0, -1, 0, 0]))
    with pytest.raises(ValueError, match=r"'base_ang_vel'.*history_length must be >= 0, got -2"):
        build(HC.group_with(group_depth=-2))
    with pytest.raises(ValueError, match=r"'joint_vel'.*history_length 17 is above the 16"):
        build(HC.group_with(depths=[0, 0, 0, 0, 17, 0]))
    with pytest.raises(ValueError, match=r"'actions'.*history_length must be an int"):
        build(HC.group_with(depths=[0, 0, 0, 0, 0, 2.0]))
    # flatten_history_dim=False: on a term with H > 1, or from the group with a group depth above 1
    group = HC.group_with(depths=[0, 0, 3, 0, 0, 0])
    group["projected_gravity"].flatten_history_dim = False
    with pytest.raises(ValueError, match=r"'projected_gravity'.*flatten_history_dim=False"):
        build(group)
    group = HC.group_with(depths=[0, 0, 1, 0, 0, 0])
    group["projected_gravity"].flatten_history_dim = False
    assert not build(group).has_history                                     # at depth 1 there is nothing to flatten
    group = HC.group_with(group_depth=2)
    group["flatten_history_dim"] = False
    with pytest.raises(ValueError, match=r"'base_ang_vel'.*flatten_history_dim=False"):
        build(group)
    group = HC.group_with(depths=[3] * 6)                                    # without a group depth the group's flag is unused
    group["flatten_history_dim"] = False
    assert build(group).history_floats == 135
    # the two caps, at the term that passes them: 64 floats per frame, 512 with the history
    wide = {f"q{k}": ObsTerm(func=O.joint_pos) for k in range(6)}
    with pytest.raises(ValueError, match=r"'q5'.*reaches 72 floats.*at most 64"):
        build(wide)
    deep = {f"q{k}": ObsTerm(func=O.joint_pos, history_length=16) for k in range(3)}
    with pytest.raises(ValueError, match=r"'q2'.*reaches 576 floats.*at most 512"):
        build(deep)
    exact = HC.group_of_512()
    assert build(exact).history_floats == 512 and len(build(exact)[0]) == 38


def test_fingerprint_holds_the_depths_above_one():
    plain, _ = manager_of(HC.group_with())
    three, _ = manager_of(HC.group_with(group_depth=3))
    five, _ = manager_of(HC.group_with(group_depth=5))
    mixed, _ = manager_of(HC.group_with(depths=[1, 1, 1, 3, 1, 1]))
    fps = [m.fingerprint() for m in (plain, three, five, mixed)]
    assert all(a != b for i, a in enumerate(fps) for b in fps[i + 1:])
    # a term at depth 1 keeps the entry it had: a state made before there was a history still loads
    assert all(len(row) == 2 for row in fps[0]) and [len(row) for row in fps[3]] == [2, 2, 2, 3, 2, 2]
    assert fps[1][0][2] == 3 and fps[2][0][2] == 5 and [row[:2] for row in fps[1]] == fps[0]
    assert plain.fingerprint() == OC._manager()[0].fingerprint()
    from cat_envs.tasks.utils.cleanrl import checkpoint
    with pytest.raises(ValueError):
        checkpoint.check_fingerprint({"observation_terms": fps[0]}, {"observation_terms": fps[1]})
    with pytest.raises(ValueError):
        checkpoint.check_fingerprint({"observation_terms": fps[1]}, {"observation_terms": fps[2]})
    checkpoint.check_fingerprint({"observation_terms": fps[1]}, {"observation_terms": three.fingerprint()})
