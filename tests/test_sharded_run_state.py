"""Run states of env-sharded runs as files (cleanrl/checkpoint.py): a set of W files is one state or none - discovery
that counts only complete sets, pruning that takes a set apart head first, the fingerprint's ``rank``, the load vote's
verdict.  No device: plain file handling in a temporary directory, hand-made payloads."""
import os

import pytest

from cat_envs.tasks.utils.cleanrl import checkpoint as ck


def _touch(d, *names):
    for n in names:
        (d / n).write_bytes(b"x")


def _set(it, world=2):
    return [f"state_{it}.pt"] + [f"state_{it}.rank{r}.pt" for r in range(1, world)]


def _heads_without_siblings(d, world=2):
    return [f for f in sorted(os.listdir(d)) if ck.state_iteration(f) is not None and ck.missing_siblings(str(d / f), world)]


# ------------------------------------------------------------------------------------------------ names
def test_sibling_names():
    assert ck.sibling_path("/r/state_12.pt", 0) == "/r/state_12.pt"
    assert ck.sibling_path("/r/state_12.pt", 3) == "/r/state_12.rank3.pt"
    assert ck.set_paths("/r/state_5.pt", 3) == ["/r/state_5.pt", "/r/state_5.rank1.pt", "/r/state_5.rank2.pt"]
    assert ck.state_iteration("/r/state_12.pt") == 12 and ck.state_iteration("/r/state_12.rank1.pt") is None
    with pytest.raises(ValueError, match="state_<iteration>.pt"):
        ck.sibling_path("/r/model_12.pt", 1)


# ------------------------------------------------------------------------------------------------ discovery
@pytest.fixture
def log_root(tmp_path):
    root = tmp_path / "logs" / "clean_rl" / "solo12_flat"
    run = root / "2026-01-02_09-00-00"
    (run / "params").mkdir(parents=True)
    _touch(run, "model_3.pt", "model_5.pt", "model_7.pt", *_set(3), *_set(5), "state_7.pt")      # state_7.rank1.pt is missing
    old = root / "2026-01-01_09-00-00"
    old.mkdir()
    _touch(old, *_set(9))
    return root, run


def test_find_state_returns_the_newest_complete_set(log_root, capsys):
    root, run = log_root
    assert ck.find_state(str(root), world=2) == str(run / "state_5.pt")
    out = capsys.readouterr().out
    assert out.count("skipping") == 1 and "state_7.pt" in out and "state_7.rank1.pt" in out      # one line per skipped iteration
    assert ck.find_state(str(root), ".*", "model_5.pt", world=2) == str(run / "state_5.pt")
    assert ck.find_state(str(root), ".*", "state_3.pt", world=2) == str(run / "state_3.pt")
    # three ranks: no set of this run is complete
    with pytest.raises(ValueError, match="all 3 ranks"):
        ck.find_state(str(root), world=3)


def test_find_state_raises_for_a_named_incomplete_set(log_root):
    root, run = log_root
    for name in ("state_7.pt", "model_7.pt"):
        with pytest.raises(ValueError) as e:
            ck.find_state(str(root), ".*", name, world=2)
        assert "state_7.rank1.pt" in str(e.value) and str(run / "state_7.pt") in str(e.value)
    with pytest.raises(ValueError) as e:
        ck.find_state(str(root), ".*", "state_5.pt", world=4)
    assert "state_5.rank2.pt" in str(e.value) and "state_5.rank3.pt" in str(e.value) and "state_5.rank1.pt" not in str(e.value)


def test_find_state_without_world_behaves_as_before(log_root, capsys):
    root, run = log_root
    assert ck.find_state(str(root)) == str(run / "state_7.pt")
    assert ck.find_state(str(root), ".*", "model_7.pt") == str(run / "state_7.pt")
    assert ck.find_state(str(root), world=1) == str(run / "state_7.pt")
    assert capsys.readouterr().out == ""


# ------------------------------------------------------------------------------------------------ pruning
@pytest.fixture
def run_dir(tmp_path):
    names = [n for it in (1, 3, 5, 7) for n in _set(it, 3)]
    orphans = ["state_2.rank1.pt", "state_2.rank2.pt"]
    others = ["model_1.pt", "model_7.pt", "state_3.rank1.pt.tmp", "state_x.rank1.pt", "mystate_1.rank1.pt", "notes.txt"]
    _touch(tmp_path, *names, *orphans, *others)
    return tmp_path, others


def test_prune_takes_whole_sets_and_orphans(run_dir):
    d, others = run_dir
    removed = ck.prune_states(str(d), 2, siblings=True)
    assert sorted(os.listdir(d)) == sorted(_set(5, 3) + _set(7, 3) + others)
    assert sorted(os.path.basename(p) for p in removed) == sorted(_set(1, 3) + _set(3, 3) + ["state_2.rank1.pt", "state_2.rank2.pt"])
    assert ck.prune_states(str(d), 2, siblings=True) == []
    assert ck.prune_states(str(d), 0, siblings=True) == []


def test_prune_leaves_siblings_newer_than_the_newest_head(tmp_path):
    _touch(tmp_path, *_set(1), *_set(3), "state_4.rank1.pt")            # iteration 4: a save that may still be under way
    ck.prune_states(str(tmp_path), 1, siblings=True)
    assert sorted(os.listdir(tmp_path)) == sorted(_set(3) + ["state_4.rank1.pt"])


def test_prune_without_sibling_handling_keeps_its_contract(run_dir):
    d, others = run_dir
    before = set(os.listdir(d))
    removed = ck.prune_states(str(d), 2)
    assert sorted(os.path.basename(p) for p in removed) == ["state_1.pt", "state_3.pt"]
    assert before - set(os.listdir(d)) == {"state_1.pt", "state_3.pt"}


def test_interrupted_pruning_leaves_nothing_that_discovery_accepts(run_dir, monkeypatch):
    d, _ = run_dir
    real = os.remove
    calls = []

    def failing(p, *a, **k):
        calls.append(os.path.basename(p))
        if ".rank" in os.path.basename(p):
            raise PermissionError(f"cannot remove {p}")
        return real(p, *a, **k)
    monkeypatch.setattr(os, "remove", failing)
    with pytest.raises(PermissionError):
        ck.prune_states(str(d), 2, siblings=True)
    monkeypatch.setattr(os, "remove", real)
    assert calls[0] == "state_1.pt" and ".rank" in calls[1]                 # head first, then its siblings
    assert not os.path.exists(d / "state_1.pt") and os.path.exists(d / "state_1.rank1.pt")
    assert _heads_without_siblings(d, 3) == []                           # no state_<it>.pt without its siblings
    root = d.parent
    assert ck.find_state(str(root), d.name, world=3) == str(d / "state_7.pt")
    with pytest.raises(ValueError, match="state_1.pt does not exist"):
        ck.find_state(str(root), d.name, "state_1.pt", world=3)
    ck.prune_states(str(d), 2, siblings=True)                            # the next pruning finishes the job
    assert sorted(f for f in os.listdir(d) if f.startswith("state_") and f.endswith(".pt") and "x" not in f) == \
        sorted(_set(5, 3) + _set(7, 3))


# ------------------------------------------------------------------------------------------------ fingerprint
def _fp(world, rank, num_envs=32):
    base = {"task_kind": "servo", "num_envs": num_envs, "env_seed": 42, "env_offset": rank * num_envs, "hidden": [64, 64]}
    return ck.rank_fingerprint(base, world, rank)


def _differing(saved, current):
    with pytest.raises(ValueError) as e:
        ck.check_fingerprint(saved, current, "/x/state_3.pt")
    assert "/x/state_3.pt" in str(e.value)
    return [d[0] for d in ck.fingerprint_diff(saved, current)], str(e.value)


def test_single_process_fingerprint_has_no_rank():
    assert "rank" not in _fp(1, 0) and _fp(1, 0)["world"] == 1
    assert _fp(2, 1)["rank"] == 1 and _fp(2, 0)["rank"] == 0 and _fp(2, 1)["world"] == 2
    ck.check_fingerprint(_fp(2, 1), _fp(2, 1))


def test_sharded_state_against_a_single_process_run_names_world_and_rank():
    fields, msg = _differing(_fp(2, 0), _fp(1, 0))
    assert fields == ["world", "rank"]
    assert "world: saved 2, this run 1" in msg and "rank: saved 0, this run '<absent>'" in msg
    fields, msg = _differing(_fp(1, 0), _fp(2, 0))                       # and the other way round
    assert fields == ["world", "rank"] and "rank: saved '<absent>', this run 0" in msg


def test_swapped_ranks_name_rank_and_env_offset():
    fields, msg = _differing(_fp(2, 0), _fp(2, 1))
    assert fields == ["env_offset", "rank"]
    assert "rank: saved 0, this run 1" in msg and "env_offset: saved 0, this run 32" in msg


def test_another_world_size_names_world_and_the_shard():
    fields, _ = _differing(_fp(2, 1, num_envs=32), _fp(4, 1, num_envs=16))
    assert fields == ["num_envs", "env_offset", "world"]


# ------------------------------------------------------------------------------------------------ the load vote
def test_load_vote_verdict():
    ok = lambda r, token="t0", it=3, step=24, world=2: (None, world, r, token, it, step)
    assert ck.check_set_votes([ok(0), ok(1)]) == []
    bad = ck.check_set_votes([ok(0), ("FileNotFoundError: state_3.rank1.pt does not exist", None, None, None, None, None)])
    assert bad == [(1, "FileNotFoundError: state_3.rank1.pt does not exist")]
    (r, why), = ck.check_set_votes([ok(0), ok(1, token="t1")])
    assert r == 1 and "t1" in why and "t0" in why and "different saves" in why
    (r, why), = ck.check_set_votes([ok(0), ok(0)])
    assert r == 1 and "written by rank 0" in why
    (r, why), = ck.check_set_votes([ok(0), ok(1, it=5, step=40)])
    assert r == 1 and "iteration 5" in why and "40 optimiser steps" in why
    both = ck.check_set_votes([ok(0, world=4), ok(1, world=4)])
    assert [r for r, _ in both] == [0, 1] and all("4 ranks" in w for _, w in both)
    # rank 0 failed: the others are compared with the first rank that did not
    bad = ck.check_set_votes([("ValueError: x", None, None, None, None, None), ok(1, world=3), ok(2, token="t9", world=3)])
    assert [r for r, _ in bad] == [0, 2]
