"""Run-state files (``state_<it>.pt``): format, guards, discovery and pruning.

A run state is everything a killed run needs to go on bit for bit: the trainer's part
(``PPOTrainer.save_state``) and the env's part (``CaTEnv.state_dict``), behind a *fingerprint* of everything that has to
match for the continuation to mean anything.  One ``torch.save`` dict::

    {"format": 1, "fingerprint": {...}, "trainer": {...}, "env": {...}}

holding only CPU tensors, ints, floats, strings, bools, lists and dicts, so it loads with ``weights_only=True``.

An env-sharded run of W ranks writes W such files, one state: ``state_<it>.pt`` (rank 0) and ``state_<it>.rank<r>.pt``
(ranks 1 ... W-1) in rank 0's run directory.  Rank 0's file is written last and removed first, so it commits the set:
where it exists, its siblings do (``sibling_path``, ``missing_siblings``, ``find_state(world=W)``, ``prune_states(siblings=True)``).

This module imports nothing from the device path (no ``cat_envs.native``): it is plain file handling and runs on a CPU.
"""
from __future__ import annotations

import os
import re

import torch

FORMAT = 1
REQUIRED_KEYS = ("format", "fingerprint", "trainer", "env")
_STATE_RE = re.compile(r"^state_(\d+)\.pt$")
_MODEL_RE = re.compile(r"^model_(\d+)\.pt$")
_SIBLING_RE = re.compile(r"^state_(\d+)\.rank(\d+)\.pt$")


# ------------------------------------------------------------------------------------------------ plain data
def to_plain(obj):
    """``obj`` with every tensor detached and copied to the CPU, tuples as lists, numpy / ctypes scalars as Python
    numbers; raises ``TypeError`` for anything a ``weights_only`` load would refuse"""
    if isinstance(obj, torch.Tensor):
        return obj.detach().to("cpu", copy=True).contiguous()
    if isinstance(obj, (bool, int, float, str)) or obj is None:
        return obj
    if isinstance(obj, dict):
        for k in obj:
            if not isinstance(k, str):
                raise TypeError(f"run state: dict keys must be strings, got {k!r}")
        return {k: to_plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_plain(v) for v in obj]
    if hasattr(obj, "item") and callable(obj.item):            # numpy scalars
        return to_plain(obj.item())
    raise TypeError(f"run state: cannot store a {type(obj).__name__}")


# ------------------------------------------------------------------------------------------------ write / read
def write_state(path: str, payload: dict) -> str:
    """atomic write: ``path + ".tmp"`` in the same directory, flush, fsync, ``os.replace`` - a killed save never leaves a
    truncated ``state_*.pt`` (at worst a ``.tmp``, which nothing reads)"""
    missing = [k for k in REQUIRED_KEYS if k not in payload]
    if missing:
        raise ValueError(f"run state for {path}: missing {missing}")
    payload = to_plain(payload)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(payload, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def read_state(path: str) -> dict:
    """the dict ``write_state`` wrote (tensors on the CPU); ``ValueError`` naming ``path`` for a file that is truncated,
    not a run state, of an unknown format or incomplete"""
    try:
        payload = torch.load(path, map_location="cpu", weights_only=True)
    except FileNotFoundError:
        raise
    except Exception as e:
        raise ValueError(f"{path}: not a readable run state (truncated or foreign file): {type(e).__name__}: {e}") from e
    if not isinstance(payload, dict) or "format" not in payload:
        raise ValueError(f"{path}: not a run state (no 'format' entry; a model_*.pt holds the policy alone)")
    if payload["format"] != FORMAT:
        raise ValueError(f"{path}: run state format {payload['format']!r} is not supported (this code reads {FORMAT})")
    missing = [k for k in REQUIRED_KEYS if k not in payload]
    if missing:
        raise ValueError(f"{path}: run state lacks {missing}")
    return payload


def require(d: dict, keys, path: str, where: str):
    """``ValueError`` naming ``path`` unless ``d`` (section ``where`` of a run state) has all ``keys``"""
    missing = [k for k in keys if k not in d]
    if missing:
        raise ValueError(f"{path}: run state section '{where}' lacks {missing}")


# ------------------------------------------------------------------------------------------------ fingerprint
def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flatten(v, f"{prefix}{k}."))
        else:
            out[prefix + k] = list(v) if isinstance(v, tuple) else v
    return out


def fingerprint_diff(saved: dict, current: dict):
    """[(field, saved value, current value)] of every field that differs (nested dicts by dotted name; a field one side
    lacks shows as ``'<absent>'``)"""
    a, b = _flatten(to_plain(saved)), _flatten(to_plain(current))
    diff = []
    for k in list(a) + [k for k in b if k not in a]:
        va, vb = a.get(k, "<absent>"), b.get(k, "<absent>")
        if type(va) is not type(vb) and not (isinstance(va, (int, float)) and isinstance(vb, (int, float))
                                             and not isinstance(va, bool) and not isinstance(vb, bool)):
            diff.append((k, va, vb))
        elif va != vb:
            diff.append((k, va, vb))
    return diff


def check_fingerprint(saved: dict, current: dict, path: str | None = None):
    """``ValueError`` naming EVERY differing field with both values"""
    diff = fingerprint_diff(saved, current)
    if diff:
        lines = "; ".join(f"{k}: saved {a!r}, this run {b!r}" for k, a, b in diff)
        raise ValueError(f"{path or 'run state'} does not fit this run ({len(diff)} field(s) differ): {lines}")


def rank_fingerprint(fp: dict, world: int, rank: int) -> dict:
    """``fp`` as rank ``rank`` of ``world`` stores it: ``world`` always, ``rank`` only in an env-sharded run (a
    single-process state keeps exactly the fields it always had)"""
    out = dict(fp, world=int(world))
    if int(world) > 1:
        out["rank"] = int(rank)
    return out


# ------------------------------------------------------------------------------------------------ sets (world > 1)
def sibling_path(path: str, rank: int) -> str:
    """the file of rank ``rank`` in the set that ``path`` (rank 0's ``state_<it>.pt``) commits: ``path`` itself for rank 0,
    ``state_<it>.rank<r>.pt`` beside it for the others"""
    if int(rank) == 0:
        return path
    d, name = os.path.split(path)
    m = _STATE_RE.match(name)
    if not m:
        raise ValueError(f"{path}: the run state of an env-sharded run is named by rank 0's file, state_<iteration>.pt")
    return os.path.join(d, f"state_{int(m.group(1))}.rank{int(rank)}.pt")


def state_iteration(path: str):
    """N of a path named ``state_N.pt`` (None for any other name)"""
    m = _STATE_RE.match(os.path.basename(path))
    return int(m.group(1)) if m else None


def check_set_votes(votes) -> list:
    """The verdict of a load vote, the same on every rank.  ``votes[r]`` is rank r's ``(error text or None, set.world,
    set.rank, set.token, iteration, adam_step)`` after it read and checked its own file.  Returns ``[(rank, why)]`` of the
    offending ranks (empty: load): a rank whose own checks failed; a file not written by a run of ``len(votes)`` ranks, or
    by another rank; a token, iteration or optimiser step count that is not rank 0's (whose file commits the set)."""
    world = len(votes)
    ref_rank = next((r for r, v in enumerate(votes) if v[0] is None), None)
    bad = []
    for r, (err, w, rk, token, it, step) in enumerate(votes):
        if err is not None:
            bad.append((r, err))
            continue
        _, _, _, token0, it0, step0 = votes[ref_rank]
        why = []
        if w != world:
            why.append(f"its file was written by a run of {w} ranks, this run has {world}")
        if rk != r:
            why.append(f"its file was written by rank {rk}")
        if token != token0:
            why.append(f"its file carries token {token}, rank {ref_rank}'s {token0}: they are of different saves")
        if it != it0:
            why.append(f"its file was saved after iteration {it}, rank {ref_rank}'s after {it0}")
        if step != step0:
            why.append(f"its file holds {step} optimiser steps, rank {ref_rank}'s {step0}")
        if why:
            bad.append((r, "; ".join(why)))
    return bad


def set_paths(path: str, world: int) -> list:
    """the ``world`` files of the set, rank order"""
    return [sibling_path(path, r) for r in range(int(world))]


def missing_siblings(path: str, world: int) -> list:
    """the files of ranks 1 ... world-1 that are not beside ``path``"""
    return [p for p in set_paths(path, world)[1:] if not os.path.isfile(p)]


def remove_siblings(run_dir: str, it: int) -> list:
    """remove every ``state_<it>.rank<r>.pt`` of ``run_dir`` (a file somebody else removed meanwhile is fine)"""
    removed = []
    for i, _, f in _siblings(run_dir):
        if i == int(it):
            try:
                os.remove(os.path.join(run_dir, f))
                removed.append(os.path.join(run_dir, f))
            except FileNotFoundError:
                pass
    return removed


# ------------------------------------------------------------------------------------------------ discovery / pruning
def _numbered(run_dir: str, pattern):
    out = []
    for f in os.listdir(run_dir):
        m = pattern.match(f)
        if m:
            out.append((int(m.group(1)), f))
    return sorted(out)


def _siblings(run_dir: str):
    """[(iteration, rank, name)] of the ``state_<it>.rank<r>.pt`` in ``run_dir``"""
    out = []
    for f in os.listdir(run_dir):
        m = _SIBLING_RE.match(f)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), f))
    return sorted(out)


def find_state(log_root: str, load_run: str = ".*", load_checkpoint: str = "model_.*.pt", world: int = 1) -> str:
    """the run state to resume from: the latest run directory under ``log_root`` matching ``load_run`` (regular expression,
    like ``play.py``) and in it the highest-numbered ``state_*.pt``.  A ``load_checkpoint`` that names one file -
    ``model_N.pt`` or ``state_N.pt`` - selects ``state_N.pt``; patterns (the default ``model_.*.pt``) mean "the latest".

    ``world`` > 1 (an env-sharded run): a ``state_<it>.pt`` counts only with the files of ranks 1 ... world-1 beside it.
    "The latest" skips incomplete sets, one printed line each; a named one that is incomplete raises, listing what is
    missing.  (Whether the files are of ONE save - their token - is compared when they are loaded.)"""
    world = int(world)
    if not os.path.isdir(log_root):
        raise ValueError(f"nothing to resume from: {log_root} does not exist")
    runs = sorted(d for d in os.listdir(log_root)
                  if os.path.isdir(os.path.join(log_root, d)) and re.match(load_run or ".*", d))
    if not runs:
        raise ValueError(f"nothing to resume from: no run matching '{load_run}' in {log_root}")
    run = os.path.join(log_root, runs[-1])
    name = os.path.basename(load_checkpoint or "")
    m = _MODEL_RE.match(name) or _STATE_RE.match(name)
    if m:
        path = os.path.join(run, f"state_{int(m.group(1))}.pt")
        if not os.path.isfile(path):
            raise ValueError(f"{path} does not exist: '{name}' has no run state beside it (the run is older than run "
                             "states, was written with save_state=False, or the file was pruned: see keep_states)")
        missing = missing_siblings(path, world)
        if missing:
            raise ValueError(f"{path} is not a complete run state of {world} ranks: "
                             f"{', '.join(os.path.basename(p) for p in missing)} missing beside it")
        return path
    states = _numbered(run, _STATE_RE)
    if not states:
        models = _numbered(run, _MODEL_RE)
        hint = (f" (it holds {len(models)} model_*.pt: policies alone, which cannot continue a run)" if models else "")
        raise ValueError(f"nothing to resume from: no state_*.pt in {run}{hint}")
    for it, f in reversed(states):
        path = os.path.join(run, f)
        missing = missing_siblings(path, world)
        if not missing:
            return path
        print(f"[catppo] skipping {path}: not a complete run state of {world} ranks "
              f"({', '.join(os.path.basename(p) for p in missing)} missing)")
    raise ValueError(f"nothing to resume from: none of the {len(states)} state_*.pt in {run} has the files of all "
                     f"{world} ranks beside it")


def prune_states(run_dir: str, keep: int, siblings: bool = False):
    """keep the ``keep`` highest-numbered ``state_*.pt`` of ``run_dir`` (0: all); returns the removed paths.  Only files
    named exactly ``state_<number>.pt`` are ever touched - and, with ``siblings`` (env-sharded runs), the
    ``state_<number>.rank<r>.pt`` that belong to them.  A set goes head first: ``state_<it>.pt``, then its siblings, so an
    interrupted pruning never leaves a ``state_<it>.pt`` without them.  Siblings without a ``state_<it>.pt`` (a killed save
    or a killed pruning) go too when they are older than the newest ``state_<it>.pt`` that stays."""
    keep = int(keep)
    if keep <= 0:
        return []
    states = _numbered(run_dir, _STATE_RE)
    removed = []
    for it, f in states[:-keep]:
        p = os.path.join(run_dir, f)
        os.remove(p)
        removed.append(p)
        if siblings:
            removed += remove_siblings(run_dir, it)
    if siblings and states:
        kept = {it for it, _ in states[-keep:]}
        for it, _, f in _siblings(run_dir):
            if it not in kept and it < max(kept) and os.path.exists(os.path.join(run_dir, f)):
                os.remove(os.path.join(run_dir, f))
                removed.append(os.path.join(run_dir, f))
    return removed


