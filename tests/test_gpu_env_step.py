"""The fused env step - rollout_pre_kernel, rollout_fold_kernel, rollout_post_kernel, rollout_post_tail_kernel
(csrc/rollout.hip, rollout_post.h) and step_fwd_kernel (csrc/step_merge.h) - and its unfused counterparts (catppo_cat_terms,
catppo_env_pre_step, catppo_cat_terms_step, catppo_cat_reset, catppo_rollout_store_ex) at the sizes where their code branches
on geometry, against the plain restatement of tests/env_step_ref.py.  tests/test_env_step_ref.py holds that restatement
against the project's pinned oracle on the CPU, shows that the cases are not vacuous and that every comparison used here
rejects a planted error and says where it is.

Every output lives in a guarded buffer (tests/env_step_cases.py drives the device); pad columns of obs_out (obs_out_ld = D + 3)
must keep the sentinel, pad columns of the raw observations hold NaN.  Every case runs with the inline tail and with the
deferred one (the tail rides in the next pre launch, a flush behind the last step), and both again in a context whose
workspace is refilled with NaN before every library call: all four runs must agree in every byte.

   N                   A   D            terms -> K                  what it reaches
   1                   1   1            1 x width 1                 smallest
   15, 16, 17          12  3            3 terms, K = 32 / 33        ragged / full / second pre tile; post constraint tile in
                                                                    registers or not (32 K <= 1024); idle moment lanes (256 % 3)
   31, 32, 33          12  64 / 65      5 terms, K = 64 / 65        post tile boundary; observation rows in registers or not
   95                  17  128 / 129    5 terms, K = 96             a wave owning two terms; OG 2 -> 1; the action shift loops
   100                 12  255/256/257  16 uneven terms, K = D      second column pass of moments and normaliser; generic
                                                                    running-maximum path (K > 256); the fold's idle columns
   40                  12  512          16 x 32, K = 512            widest table and observation; post launch above 64 KB of LDS
   512, 513            12  48           all 12 kinds, K = 70        32 / 33 pre workgroups, 16 / 17 post workgroups
   4096, 4097, 4112    12  48           16 terms, K = 81            the fold's second batch of partial rows; the reset-log fold
                                                                    past 16 rows per thread
   16384, 16400, 32784 12  48           six kinds, K = 34           grid cap: no / some / all workgroups walk a second tile
   300                 12  0            six kinds                   obs_raw = NULL: no normaliser
Options, one each at N = 300, D = 45: test_env_step_options.  The two process-wide switches (CATPPO_ROLLOUT_TREE=1; the
32-row window pinned open for step_fwd_kernel) run in one worker process each (env_step_cases.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import env_step_cases as X
import env_step_ref as E
import parity_record
from test_gpu_stat_kernels import Used

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def nat():
    from cat_envs import native
    return native.Native()


@pytest.fixture(scope="module")
def used():
    u = Used()
    u.poison()
    torch.cuda.synchronize()
    assert bool(torch.isnan(u.sums).all()) and bool(torch.isnan(u.colmax).all())
    return u


_RATIOS = {}


def _note(ratios, case):
    """largest error / bar per family, to the parity record (the cases are not vacuous)"""
    for fam, r in ratios.items():
        best = _RATIOS.setdefault(fam, {"ratio": -1.0, "case": None})
        if r > best["ratio"]:
            best["ratio"], best["case"] = float(r), str(case)
        parity_record.record("env_step_" + fam, {"largest_error_over_bar": best["ratio"]}, note=best["case"])


VARIANTS = {
    "fp16_planes": dict(run=dict(f16=True), ref=dict(f16=True)),
    "probs_null": dict(run=dict(null=("probs",))),
    "dones_null": dict(run=dict(null=("dones",))),
    "log_out_null": dict(run=dict(null=("log_out",))),
    "no_action_zeroing": dict(run=dict(zero_action=False), ref=dict(zero_action=False)),
    "strides_3": dict(case=dict(stride=3)),
    "no_env_resets": dict(case=dict(last_step="none")),
    "all_envs_reset": dict(case=dict(last_step="all")),
    "three_records": dict(records=True),
    "sim_src_rows_2048B": dict(case=dict(row_floats=512), run=dict(sim_src=True)),
    "sim_src_rows_2064B": dict(case=dict(row_floats=516), run=dict(sim_src=True)),
    "nan_and_inf": dict(case=dict(nan_inf=True)),
    "force_history_of_one": dict(case=dict(H=1)),
}


def _variant(name):
    v = VARIANTS[name]
    case = E.table_case(E.VARIANT_SHAPE, **v.get("case", {}))
    records = E.other_rank_records(case) if v.get("records") else None
    return case, records, v.get("run", {}), v.get("ref", {})


def test_the_poison_covers_the_largest_carve():
    """the NaN that Used leaves in the workspace (2 MiB from its start) reaches past everything a case of this module carves"""
    worst = max(E.carve_bytes(E.row_dims(row)) for row in E.TABLE + E.TREE_TABLE + [E.VARIANT_SHAPE])
    assert worst <= X.POISON_BYTES, (worst, X.POISON_BYTES)


def _four_runs(nat, used, case, ref, tag, **kw):
    ratios, msgs = {}, []
    inline, run = X.run_fused(nat, case, **kw)
    msgs += X.check_run(case, ref, inline, run, f"{tag}, inline tail", ratios)
    deferred, run_d = X.run_fused(nat, case, defer=1, **kw)
    msgs += X.check_run(case, ref, deferred, run_d, f"{tag}, deferred tail", ratios)
    print(f"{tag}: largest error / bar {ratios}")
    _note(ratios, tag)
    assert not msgs, "\n".join(msgs[:40])
    assert not X.differing(inline, deferred), X.differing(inline, deferred)
    del run_d, deferred
    for defer in (False, 1):
        again, _ = X.run_fused(used, case, defer=defer, **kw)
        diff = X.differing(inline, again)
        assert not diff, f"differs on a used (NaN-filled) workspace, deferred tail {bool(defer)}: {diff}"
    return inline, run


@pytest.mark.parametrize("index", range(len(E.TABLE)), ids=[f"N{r[0]}_A{r[1]}_D{r[2]}_{i}" for i, r in enumerate(E.TABLE)])
def test_fused_env_step_at_the_geometry_edges(nat, used, index):
    case = E.table_case(E.TABLE[index], index)
    ref = E.run_ref(case)
    E.assert_case_is_live(case, ref)
    _four_runs(nat, used, case, ref, case["tag"])


@pytest.mark.parametrize("index", range(len(E.TABLE)), ids=[f"N{r[0]}_A{r[1]}_D{r[2]}_{i}" for i, r in enumerate(E.TABLE)])
def test_unfused_calls_on_the_same_descriptor_tables(nat, used, index):
    case = E.table_case(E.TABLE[index], index)
    ref = E.run_ref(case)
    ratios = {}
    steps, run = X.run_unfused(nat, case)
    msgs = X.check_run(case, ref, steps, run, f"{case['tag']} unfused", ratios, unfused=True)
    _note({k + "_unfused": v for k, v in ratios.items()}, case["tag"])
    assert not msgs, "\n".join(msgs[:40])
    again, _ = X.run_unfused(used, case)
    assert not X.differing(steps, again), X.differing(steps, again)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_env_step_options(nat, used, name):
    case, records, run_kw, ref_kw = _variant(name)
    ref = E.run_ref(case, records=records, **ref_kw)
    E.assert_case_is_live(case, ref)
    tag = f"{case['tag']} {name}"
    inline, run = _four_runs(nat, used, case, ref, tag, records=records, **run_kw)
    N, K, nt = case["N"], case["K"], case["nt"]
    if name == "no_env_resets":             # log_out receives log_prev, bit for bit
        assert not ref[2]["reset"].any()
        prev, out = (run.g[k].of(inline[2]["tail"][k]) for k in ("log0", "log1"))
        assert np.array_equal(prev.view(np.uint32), out.view(np.uint32)) and np.array_equal(prev, ref[1]["log"])
    if name == "all_envs_reset":
        assert ref[2]["reset"].all() and not run.g["ep_len"].of(inline[2]["post"]["ep_len"]).any()
    if name.startswith("sim_src"):          # behind rollout_pre the state block IS the source block, bit for bit
        for t in range(E.STEPS):
            sim = run.g["sim"].of(inline[t]["pre"]["sim"]).reshape(N, case["F"])
            assert np.array_equal(sim.view(np.uint32), case["steps"][t]["block"].view(np.uint32)), t
        assert (16 * case["F"] // 4 <= 2048) == (name == "sim_src_rows_2048B")
    if name.endswith("_null"):              # what a NULL pointer switches off stays untouched
        key = {"probs_null": "probs", "dones_null": "dones", "log_out_null": "log1"}[name]
        raw = inline[2]["tail" if key == "log1" else "post"][key]
        assert (raw.view(np.uint32) == run.g[key].bits).all()
    if name == "nan_and_inf":
        c0 = case["off"][0] + 1
        rm = [run.g["rm"].of(inline[t]["tail"]["rm"]) for t in range(E.STEPS)]
        assert np.isnan(rm[1][c0]) and np.isnan(rm[2][c0]) and np.isposinf(rm[1][c0 + 1]) and not np.isnan(rm[0]).any()
    if name == "fp16_planes":
        assert inline[0]["post"]["rewards_t"].dtype == np.float16
        steps, urun = X.run_unfused(nat, case, f16=True)            # catppo_rollout_store_ex with half planes
        msgs = X.check_run(case, ref, steps, urun, f"{tag} unfused", {}, unfused=True)
        assert not msgs, "\n".join(msgs[:40])
    if name == "three_records":
        assert (ref[0]["rm"] > ref[0]["x_colmax"]).any()       # another rank's maximum wins somewhere


def test_argument_checks_return_codes_and_launch_nothing(nat):
    case = E.table_case((33, 12, 3, E.SIX_KINDS))
    run = X.Run(nat, case)
    run.begin_step(0)
    st, lib = run.st, nat.lib

    def refused(fn, match, **fields):
        old = {k: getattr(st, k) for k in fields}
        for k, v in fields.items():
            setattr(st, k, v)
        try:
            with pytest.raises(RuntimeError, match=match):
                fn(st)
        finally:
            for k, v in old.items():
                setattr(st, k, v)
    refused(nat.rollout_pre, "sizes out of range", D=513)
    refused(nat.rollout_post, "sizes out of range", D=513)
    refused(nat.rollout_pre, "sizes out of range", n_terms=17)
    refused(nat.rollout_pre, "sum of term widths", K=case["K"] + 1)
    bad_off = (C.c_int32 * (case["nt"] + 1))(*[int(v) for v in case["off"]])
    bad_off[1], bad_off[2] = bad_off[2], bad_off[1]
    refused(nat.rollout_post, "term_off not monotone", term_off=C.cast(bad_off, C.c_void_p).value)
    inside = run.g["sim"].view.data_ptr() + 64
    refused(nat.rollout_pre, "lies inside the simulator", sim_src=run.blocks[0].data_ptr(), reward=inside)
    wide = (C.c_int32 * 2)(0, 1100)
    refused(nat.rollout_post, "too wide", K=1100, n_terms=1, term_off=C.cast(wide, C.c_void_p).value)
    torch.cuda.synchronize()
    for k in ("cstr", "reward", "probs", "cstr_prob", "obs_out", "xchg", "time_outs"):
        raw = run.g[k].raw()
        assert (raw.view({1: np.uint8, 4: np.uint32}[raw.dtype.itemsize]) == run.g[k].bits).all(), k


# ====================================================================================================== the two workers
def _worker(tmp_path_factory, mode, env_extra, timeout):
    out = str(tmp_path_factory.mktemp("env_step_" + mode) / "results.json")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "constraints-as-terminations_amd"), HERE]))
    for k in ("CATPPO_ROLLOUT_TREE", "CATPPO_FUSED_FWD_MIN_ROWS", "CATPPO_FUSED_FWD_MAX_ROWS", "CATPPO_STEP16_FWD",
              "CATPPO_STEP_MERGE", "CATPPO_ROLLOUT_DEFER_TAIL", "CATPPO_ROWS_FWD_ROLLOUT", "CATPPO_FUSED_ROLLOUT"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "env_step_cases.py"), mode, out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["__process__"] = "ok" if r.returncode == 0 else (r.stdout[-2000:] + r.stderr[-4000:])
    for name, v in res.items():
        if isinstance(v, dict) and v.get("status") == "ok":
            _note({f"{mode}_{k}": x for k, x in v["ratios"].items()}, name)
    return res


@pytest.fixture(scope="module")
def tree_results(tmp_path_factory):
    return _worker(tmp_path_factory, "tree", {"CATPPO_ROLLOUT_TREE": "1"}, 300)


@pytest.fixture(scope="module")
def merge_results(tmp_path_factory, tree_results):          # (one worker after the other)
    return _worker(tmp_path_factory, "merge", {"CATPPO_FUSED_FWD_MIN_ROWS": "17", "CATPPO_FUSED_FWD_MAX_ROWS": "4096",
                                               "CATPPO_STEP16_FWD": "0"}, 300)


def _check(results, name):
    assert results["__process__"] == "ok" or name in results, results["__process__"]
    got = results.get(name, {"status": results["__process__"]})
    assert got["status"] == "ok", got["status"]


@pytest.mark.parametrize("name", [f"tree_{i}_N{row[0]}" for i, row in enumerate(E.TREE_TABLE)])
def test_in_launch_fold_tree(tree_results, name):
    """CATPPO_ROLLOUT_TREE=1: 1, 2, 31, 32, 33, 64, 65 and 1024 pre workgroups (groups of 32, two levels); the deferred tail
    gets no ride (the tree writes the record it still reads) and is flushed in front of the pre launch"""
    _check(tree_results, name)


@pytest.mark.parametrize("name", list(X.MERGE_CASES))
def test_step_fwd_kernel_carries_the_post_step(merge_results, name):
    """catppo_rollout_defer_tail(2): the post step rides in the policy forward (one, two and three hidden layers of 256;
    17, 33, 64, 95 rows; D = 1, 45, 48, 128 = 15, 3, 0, 0 pad columns; K = 64 with 16 terms); D = 129 and K = 65 fall back"""
    _check(merge_results, name)
