"""Run-state files (cleanrl/checkpoint.py) on hand-made dicts: format, guards, atomic write, pruning, discovery.
No device: the module under test is plain file handling."""
import os

import pytest
import torch

from cat_envs.tasks.utils.cleanrl import checkpoint as ck


def _payload(**over):
    fp = {"task_kind": "stream", "num_envs": 40, "hidden": [64, 64], "env_seed": 42, "mlp_precision": "fp32",
          "constraint_terms": [["joint_torque", 12], ["contact", 1]], "servo": {"kp": 3.0, "kd": 0.2}}
    tr = {"agent": {"actor_logstd": torch.arange(12.0).view(1, 12)}, "exp_avg": torch.randn(7),
          "iter_state": torch.arange(64, dtype=torch.uint8), "iteration": 3, "lr": 1.5e-4, "torch_rng": None}
    env = {"episode_length_buf": torch.arange(40), "reset_buf": torch.arange(40) % 7 == 0, "common_step_counter": 18,
           "curriculum": {"state": {"Curriculum/joint_torque": 0.0625}, "max_p": {"joint_torque": 1.0 / 16.0}}}
    p = {"format": ck.FORMAT, "fingerprint": fp, "trainer": tr, "env": env}
    p.update(over)
    return p


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_round_trip_loads_with_weights_only(tmp_path):
    p = _payload()
    path = ck.write_state(str(tmp_path / "state_3.pt"), p)
    raw = torch.load(path, map_location="cpu", weights_only=True)        # the safe loader accepts the file as it is
    assert _same(raw, ck.to_plain(p))
    back = ck.read_state(path)
    assert _same(back, ck.to_plain(p))
    assert back["env"]["curriculum"]["max_p"]["joint_torque"] == 1.0 / 16.0          # doubles survive exactly
    assert back["trainer"]["iter_state"].dtype == torch.uint8 and back["env"]["reset_buf"].dtype == torch.bool


def test_to_plain_copies_tensors_and_refuses_objects():
    t = torch.arange(6.0).view(2, 3).t()                                 # a non-contiguous view
    out = ck.to_plain({"t": t, "tup": (1, 2.5, "x"), "n": None})
    assert out["t"].is_contiguous() and torch.equal(out["t"], t) and out["t"].data_ptr() != t.data_ptr()
    assert out["tup"] == [1, 2.5, "x"]
    t[0, 0] = 99.0
    assert float(out["t"][0, 0]) == 0.0                                  # a copy: later steps do not reach into it
    with pytest.raises(TypeError):
        ck.to_plain({"o": object()})
    with pytest.raises(TypeError):
        ck.to_plain({1: 2})


def test_check_fingerprint_names_every_differing_field_with_both_values():
    saved = _payload()["fingerprint"]
    ck.check_fingerprint(saved, dict(saved))                             # equal: passes
    ck.check_fingerprint(saved, dict(saved, hidden=(64, 64)))            # a tuple is the list it was saved as
    cur = dict(saved, num_envs=48, hidden=[64, 32], servo={"kp": 3.5, "kd": 0.2})
    del cur["env_seed"]
    cur["rng"] = "torch"
    with pytest.raises(ValueError) as e:
        ck.check_fingerprint(saved, cur, "/x/state_3.pt")
    msg = str(e.value)
    assert "/x/state_3.pt" in msg
    for field, a, b in (("num_envs", "40", "48"), ("hidden", "[64, 64]", "[64, 32]"), ("servo.kp", "3.0", "3.5"),
                        ("env_seed", "42", "'<absent>'"), ("rng", "'<absent>'", "'torch'")):
        assert f"{field}: saved {a}, this run {b}" in msg, (field, msg)
    assert "servo.kd" not in msg and "task_kind" not in msg and "constraint_terms" not in msg
    assert [d[0] for d in ck.fingerprint_diff(saved, cur)] == ["num_envs", "hidden", "env_seed", "servo.kp", "rng"]
    # 1 and True, 3 and 3.0: a flag is not a count, a count is a number
    assert ck.fingerprint_diff({"a": 1, "b": 3}, {"a": True, "b": 3.0}) == [("a", 1, True)]


def test_unknown_format_missing_key_and_truncated_file_give_value_error_with_the_path(tmp_path):
    path = str(tmp_path / "state_1.pt")
    torch.save(ck.to_plain(_payload(format=2)), path)
    with pytest.raises(ValueError, match="format 2") as e:
        ck.read_state(path)
    assert path in str(e.value)
    p = ck.to_plain(_payload())
    del p["env"]
    torch.save(p, path)
    with pytest.raises(ValueError, match="env") as e:
        ck.read_state(path)
    assert path in str(e.value)
    torch.save({"actor_logstd": torch.zeros(1, 12)}, path)               # a model_*.pt under the wrong name
    with pytest.raises(ValueError, match="not a run state") as e:
        ck.read_state(path)
    assert path in str(e.value)
    ck.write_state(path, _payload())
    blob = open(path, "rb").read()
    for cut in (len(blob) // 2, 10, 0):
        with open(path, "wb") as f:
            f.write(blob[:cut])
        with pytest.raises(ValueError) as e:
            ck.read_state(path)
        assert path in str(e.value)
    with pytest.raises(ValueError, match="missing") as e:                # an incomplete payload is never written
        ck.write_state(path, {"format": 1, "trainer": {}})
    with pytest.raises(ValueError, match="iteration") as e:
        ck.require({"agent": {}}, ("agent", "iteration"), path, "trainer")
    assert path in str(e.value) and "trainer" in str(e.value)


def test_atomic_write_leaves_no_tmp_and_replaces_an_existing_file(tmp_path, monkeypatch):
    path = str(tmp_path / "state_5.pt")
    ck.write_state(path, _payload())
    first = ck.read_state(path)
    p2 = _payload()
    p2["trainer"]["iteration"] = 4
    ck.write_state(path, p2)
    assert ck.read_state(path)["trainer"]["iteration"] == 4 and first["trainer"]["iteration"] == 3
    assert sorted(os.listdir(tmp_path)) == ["state_5.pt"]
    # a save that dies half way: the file of before is whole, nothing else is left behind
    real = torch.save

    def dying(obj, f, *a, **k):
        f.write(b"half a file")
        raise KeyboardInterrupt
    monkeypatch.setattr(torch, "save", dying)
    with pytest.raises(KeyboardInterrupt):
        ck.write_state(path, _payload())
    monkeypatch.setattr(torch, "save", real)
    assert sorted(os.listdir(tmp_path)) == ["state_5.pt"]
    assert ck.read_state(path)["trainer"]["iteration"] == 4
    # the replacement happens only after the data reached the disk: flush and fsync come before os.replace
    order = []
    monkeypatch.setattr(os, "fsync", lambda fd: order.append("fsync"))
    real_replace = os.replace
    monkeypatch.setattr(os, "replace", lambda a, b: (order.append(("replace", os.path.basename(a), os.path.basename(b))),
                                                      real_replace(a, b))[1])
    ck.write_state(path, _payload())
    assert order == ["fsync", ("replace", "state_5.pt.tmp", "state_5.pt")]


def test_prune_states_keeps_the_newest_by_number_and_never_touches_models(tmp_path):
    names = ["state_1.pt", "state_3.pt", "state_9.pt", "state_11.pt", "state_101.pt", "model_1.pt", "model_3.pt",
             "model_101.pt", "state_5.pt.tmp", "state_x.pt", "mystate_7.pt", "state_7.pt.bak"]
    for n in names:
        (tmp_path / n).write_bytes(b"x")
    assert ck.prune_states(str(tmp_path), 0) == []                       # 0: keep all
    assert sorted(os.listdir(tmp_path)) == sorted(names)
    removed = ck.prune_states(str(tmp_path), 2)                          # by NUMBER: 101 > 11 > 9 (not by name)
    assert sorted(os.path.basename(r) for r in removed) == ["state_1.pt", "state_3.pt", "state_9.pt"]
    left = sorted(os.listdir(tmp_path))
    assert left == sorted(n for n in names if n not in ("state_1.pt", "state_3.pt", "state_9.pt"))
    assert ck.prune_states(str(tmp_path), 2) == [] and ck.prune_states(str(tmp_path), 5) == []
    assert [os.path.basename(r) for r in ck.prune_states(str(tmp_path), 1)] == ["state_11.pt"]


def test_find_state_on_a_fake_log_tree(tmp_path):
    root = tmp_path / "logs" / "clean_rl" / "solo12_flat"
    runs = {"2026-01-01_10-00-00": ["model_1.pt", "model_3.pt", "state_1.pt", "state_3.pt"],
            "2026-01-02_09-00-00": ["model_49.pt", "model_99.pt", "model_149.pt", "state_99.pt", "state_149.pt"],
            "2025-12-31_23-59-59": ["model_999.pt", "state_999.pt"],
            "2026-01-03_00-00-00_old": ["model_49.pt", "model_99.pt"]}          # a run older than run states
    for run, files in runs.items():
        (root / run / "params").mkdir(parents=True)
        for f in files:
            (root / run / f).write_bytes(b"x")
    (root / "2026-01-04_notes.txt").write_text("a file, not a run")
    r = str(root)
    new = os.path.join(r, "2026-01-02_09-00-00")
    # latest run matching load_run, highest NUMBER in it (149 > 99), with play.py's defaults for run and checkpoint
    assert ck.find_state(r, "2026-01-0[12].*", "model_.*.pt") == os.path.join(new, "state_149.pt")
    assert ck.find_state(r, "2026-01-01.*") == os.path.join(r, "2026-01-01_10-00-00", "state_3.pt")
    assert ck.find_state(r, "2025.*") == os.path.join(r, "2025-12-31_23-59-59", "state_999.pt")
    # model_N.pt resolves to its sibling state_N.pt; state_N.pt names itself
    assert ck.find_state(r, "2026-01-02.*", "model_99.pt") == os.path.join(new, "state_99.pt")
    assert ck.find_state(r, "2026-01-02.*", "state_99.pt") == os.path.join(new, "state_99.pt")
    with pytest.raises(ValueError, match="state_49.pt does not exist") as e:       # model_49.pt is there, its state was pruned
        ck.find_state(r, "2026-01-02.*", "model_49.pt")
    assert "model_49.pt" in str(e.value) and "keep_states" in str(e.value)
    # the default run pattern picks the latest directory: the old-style run, which has policies but no state
    with pytest.raises(ValueError, match="no state_") as e:
        ck.find_state(r, ".*", "model_.*.pt")
    assert "2026-01-03_00-00-00_old" in str(e.value) and "2 model_*.pt" in str(e.value)
    with pytest.raises(ValueError, match="no run matching"):
        ck.find_state(r, "2027.*")
    with pytest.raises(ValueError, match="does not exist"):
        ck.find_state(str(tmp_path / "nowhere"))


def test_state_files_do_not_match_the_policy_checkpoint_pattern():
    """play.py looks for ``model_.*.pt`` (the task cfg's ``load_checkpoint``): a run state beside a model is never picked
    up as a policy"""
    import re

    from cat_envs.tasks.locomotion.velocity.config.solo12.agents.clean_rl_ppo_cfg import Solo12FlatPPORunnerCfg
    cfg = Solo12FlatPPORunnerCfg()
    assert not re.match(cfg.load_checkpoint, "state_149.pt") and re.match(cfg.load_checkpoint, "model_149.pt")
    assert cfg.save_state is True and cfg.keep_states == 2 and cfg.resume is False
