"""CPU checks of tests/env_step_ref.py, the reference tests/test_gpu_env_step.py compares the fused env step with:
the restatement equals the project's pinned oracle (oracle/env_oracle.CaTEnvOracle on a synthetic Solo12 stream, the term
values of tests/golden/terms.npz) bit for bit; the fp32 normaliser merge of rollout_post.h and any summation order of the
reset log sit inside a quarter of the bars they are compared at; every case of the GPU tables meets the non-vacuity
conditions; and every comparison the GPU module uses rejects a planted error and says where it is."""
import numpy as np
import pytest
import torch

import env_step_ref as E
import stat_refs as R
import streams as S
from oracle import cat_oracle as CO
from oracle import env_oracle as EO

F32 = np.float32
FEET, UPPER = [3, 6, 9, 12], [0, 2, 5, 8, 11]


# ====================================================================================================== pinned oracle
def _solo12_case(states, terms, max_p, reward, hard, ep_len0, action_in):
    """an env_step_ref case around Solo12 states (streams.sim_state dicts, one per step)"""
    N = states[0]["joint_pos"].shape[0]
    names = ("joint_pos", "default_joint_pos", "joint_vel", "joint_acc", "applied_torque", "projected_gravity_b", "root_pos_w",
             "command", "last_air_time", "first_contact")
    fields, off = {}, 0
    for nm in names:
        fields[nm] = (off, states[0][nm].shape[1])
        off += states[0][nm].shape[1]
    H, B = states[0]["net_forces_w_history"].shape[1:3]
    for nm, w in (("forces", H * B * 3), ("reward", 1), ("hard", 1)):
        fields[nm] = (off, w)
        off += w
    fields["cmd"] = fields["command"]
    steps = []
    for t, s in enumerate(states):
        blk = np.zeros((N, off), F32)
        for nm in names:
            blk[:, fields[nm][0]:fields[nm][0] + fields[nm][1]] = np.asarray(s[nm], F32)
        blk[:, fields["forces"][0]:fields["forces"][0] + H * B * 3] = s["net_forces_w_history"].reshape(N, -1)
        blk[:, fields["reward"][0]] = reward[t]
        blk[:, fields["hard"][0]] = hard[t]
        steps.append({"block": blk, "action_in": action_in[t]})
    widths = [d["width"] for d in terms]
    return dict(N=N, A=12, D=0, K=sum(widths), nt=len(terms), widths=widths, off=np.concatenate([[0], np.cumsum(widths)]).astype(int),
                terms=terms, max_p=max_p, fields=fields, F=off, H=H, B=B, stride=None, jy=None, ep_len0=ep_len0,
                action0=np.zeros((N, 12), F32), prev_action0=np.zeros((N, 12), F32), log0=np.zeros(2 * len(terms), F32),
                rms0=None, steps=steps, tag="solo12")


def _d(kind, ids, limit, aux=0.0, x=None, y=None, width=None):
    return dict(kind=kind, width=len(ids) if width is None else width, ids=list(ids), limit=limit, aux=aux, x=x, y=y)


def test_term_kinds_reproduce_the_golden_term_values(golden):
    """every descriptor kind on the Solo12 state of tests/golden/terms.npz: the reference's own outputs, bit for bit"""
    g = golden("terms")
    s = S.sim_state(int(g["seed"]), int(g["n_envs"]))
    N = int(g["n_envs"])
    all12 = list(range(12))
    table = [("joint_position", _d(E.ABS_LIMIT, [1, 4], 1.3, x="joint_pos")),
             ("joint_position_when_moving_forward", _d(E.ABS_DIFF_LIMIT_GATE_CMDY, [0, 3, 6, 9], 0.2, 0.1, "joint_pos", "default_joint_pos")),
             ("joint_torque", _d(E.ABS_LIMIT, all12, 3.0, x="applied_torque")),
             ("joint_velocity", _d(E.ABS_LIMIT, all12, 16.0, x="joint_vel")),
             ("joint_acceleration", _d(E.ABS_LIMIT, all12, 800.0, x="joint_acc")),
             ("upsidedown", _d(E.GREATER, [2], 0.0, x="projected_gravity_b", width=1)),
             ("contact", _d(E.CONTACT_ANY, UPPER, 1.0, width=1)),
             ("base_orientation", _d(E.NORM2_LIMIT, [], 0.1, x="projected_gravity_b", width=1)),
             ("air_time", _d(E.AIR_TIME, FEET, 0.25, 0.1, "last_air_time", "first_contact")),
             ("n_foot_contact", _d(E.N_FOOT_CONTACT, FEET, 2.0, 0.5, width=1)),
             ("joint_range", _d(E.ABS_DIFF_LIMIT, all12, 0.4, x="joint_pos", y="default_joint_pos")),
             ("action_rate", _d(E.ACTION_RATE, all12, 80.0, 0.02, "action", "prev_action")),
             ("foot_contact_force", _d(E.FORCE_LIMIT, FEET, 50.0)),
             ("min_base_height", _d(E.LIMIT_MINUS, [2], 0.2, x="root_pos_w", width=1)),
             ("no_move", _d(E.ABS_LIMIT_GATE_CMDNORM_LT, all12, 4.0, 0.1, x="joint_vel"))]
    case = _solo12_case([s], [d for _, d in table], [0.5] * len(table), np.zeros((1, N), F32), np.zeros((1, N), F32),
                        np.zeros(N, np.int64), [s["action"]])
    cstr = E.eval_terms(case, case["steps"][0]["block"], s["action"], s["prev_action"])
    for t, (name, d) in enumerate(table):
        want = np.asarray(g[name], F32).reshape(N, -1)
        got = cstr[:, case["off"][t]:case["off"][t + 1]]
        assert not R.bits_report(name, got, want), name


def test_restatement_equals_the_pinned_env_oracle():
    """CaTEnvOracle on a synthetic Solo12 stream - 64 envs, six terms, eight steps: everything bit for bit, the log to 1e-6"""
    N, T, max_len = 64, 8, 6
    states = [S.sim_state(500 + k, N) for k in range(T)]
    rs = np.random.RandomState(3)
    reward = rs.uniform(-0.3, 1.5, (T, N)).astype(F32)
    hard = (rs.rand(T, N) < 0.08).astype(F32)
    ep0 = rs.randint(0, max_len, N).astype(np.int64)
    action_in = rs.standard_normal((T, N, 12)).astype(F32)
    all12 = list(range(12))
    spec = [("joint_torque", "joint_torque", {"limit": 3.0}, None, None, 0.25, _d(E.ABS_LIMIT, all12, 3.0, x="applied_torque")),
            ("joint_velocity", "joint_velocity", {"limit": 16.0}, None, None, 0.25, _d(E.ABS_LIMIT, all12, 16.0, x="joint_vel")),
            ("action_rate", "action_rate", {"limit": 80.0}, None, None, 0.25, _d(E.ACTION_RATE, all12, 80.0, 0.02, "action", "prev_action")),
            ("contact", "contact", {}, None, UPPER, 1.0, _d(E.CONTACT_ANY, UPPER, 1.0, width=1)),
            ("foot_contact_force", "foot_contact_force", {"limit": 50.0}, None, FEET, 1.0, _d(E.FORCE_LIMIT, FEET, 50.0)),
            ("base_orientation", "base_orientation", {"limit": 0.1}, None, None, 0.25, _d(E.NORM2_LIMIT, [], 0.1, x="projected_gravity_b", width=1))]
    case = _solo12_case(states, [s[6] for s in spec], [s[5] for s in spec], reward, hard, ep0, action_in)
    # the oracle's stream: the same blocks (+ an observation column it hands back untouched)
    stream = np.stack([st["block"] for st in case["steps"]])
    offsets = dict(case["fields"], obs=(0, 1), hard_reset=case["fields"]["hard"])
    terms = [dict(name=s[0], func=s[1], params=s[2], joints=s[3], bodies=s[4], max_p=s[5]) for s in spec]
    orc = EO.CaTEnvOracle(stream, offsets, case["B"], case["H"], states[0]["default_joint_pos"], terms, [], ep0, max_len,
                          0.02, tau=E.TAU, min_p=E.MIN_P)
    old = E.MAX_LEN
    E.MAX_LEN = max_len
    try:
        state = E.new_state(case)
        resets = 0
        for t in range(T):
            _, r, d, to, info = orc.step(torch.from_numpy(action_in[t]))
            o = E.step_ref(case, state, t)
            tag = f"step {t}"
            msgs = E.env_report(f"{tag} reward", o["reward"], r.numpy()) + E.env_report(f"{tag} dones", o["dones"], d.numpy())
            msgs += E.env_report(f"{tag} time_outs", o["time_outs"], to.numpy()) + E.env_report(f"{tag} ep_len", o["ep_len"], orc.episode_length)
            msgs += E.env_report(f"{tag} action", o["action"], orc.action) + E.env_report(f"{tag} prev_action", o["prev_action"], orc.prev_action)
            msgs += E.col_report(case, f"{tag} rm", o["rm"], orc.mgr.cat.get_running_maxes()[0])
            msgs += E.matrix_report(case, f"{tag} probs", o["probs"], np.concatenate(list(orc.mgr.cat.probs.values()), 1))
            msgs += E.env_report(f"{tag} cstr_prob", o["cstr_prob"], orc.mgr.cat.get_probs())
            for i, nm in enumerate(orc.mgr.term_names):
                msgs += E.env_report(f"{tag} ep_viol {nm}", o["ep_viol"][i], orc.mgr.episode_sums[nm])
                msgs += E.env_report(f"{tag} ep_prob {nm}", o["ep_prob"][i], orc.mgr.cstr_mean_values[nm])
            assert not msgs, "\n".join(msgs)
            if info["log"]:
                want = np.array([info["log"][f"Episode_Constraint_{k}/{nm}"] for nm in orc.mgr.term_names
                                 for k in ("violation", "probability")])
                np.testing.assert_allclose(o["log"], want, rtol=1e-6, atol=1e-9, equal_nan=True)
            resets += int(o["reset"].sum())
        assert resets > 20 and (o["rm"] > 1e-6).any()
    finally:
        E.MAX_LEN = old


def test_env_finish_keeps_a_negative_zero_like_torch_clip():
    """cat_env.py:102-107 clips with torch.clip(min=0): a negative reward times 1 - p = 0 stays -0.0 (and the kernels'
    `r < 0 ? 0 : r` agrees); np.maximum turned it into +0.0 and the bit-for-bit comparison of the reward would have tripped"""
    raw, p = np.array([-0.5, -0.5, 0.7, np.nan], F32), np.array([1.0, 0.25, 1.0, 0.5], F32)
    r, _ = CO.env_finish(raw, p, np.zeros(4, bool))
    want = torch.clip(torch.from_numpy(raw) * (1.0 - torch.from_numpy(p)), min=0.0, max=None).numpy()
    assert not R.bits_report("reward", r, want) and np.signbit(r[0]) and not np.signbit(r[1])


# ====================================================================================================== bars
def normaliser_from32(sx, sxx, n, mean, var, cnt):
    """normaliser_from of csrc/rollout_post.h in numpy: batch mean / variance from one-pass fp64 sums, the Chan merge in
    unfused fp32 operations in the kernel's order"""
    m = sx / n
    v = np.maximum(sxx / n - m * m, 0.0)
    bm, bv = m.astype(F32), v.astype(F32)
    nf, cnt = F32(n), F32(cnt)
    tot = F32(cnt + nf)
    delta = (bm - mean).astype(F32)
    new_mean = (mean + ((delta * nf).astype(F32) / tot).astype(F32)).astype(F32)
    d2 = ((((delta * delta).astype(F32) * cnt).astype(F32) * nf).astype(F32) / tot).astype(F32)
    M2 = (((var * cnt).astype(F32) + (bv * nf).astype(F32)).astype(F32) + d2).astype(F32)
    return new_mean, (M2 / tot).astype(F32), tot


_DN = sorted({(r[2], r[0]) for r in E.TABLE if r[2]} | {(45, 300)})
_MERGE_RATIOS = {}


@pytest.mark.parametrize("family", R.RMS_FAMILIES)
@pytest.mark.parametrize("D,N", _DN)
def test_fp32_merge_sits_inside_a_quarter_of_the_normaliser_bars(D, N, family):
    state0, batches = R.rms_case(D, N, D + 3, family)
    ref = R.rms_states64(state0, batches, D)
    mean, var, cnt = state0[0].copy(), state0[1].copy(), state0[2]
    worst = 0.0
    for u, x in enumerate(batches):
        x64 = np.asarray(x[:, :D], np.float64)
        mean, var, cnt = normaliser_from32(x64.sum(0), (x64 * x64).sum(0), float(N), mean, var, cnt)
        worst = max(worst, R.bar_ratio(mean, ref[u][0], R.RMS_RTOL, R.RMS_ATOL), R.bar_ratio(var, ref[u][1], R.RMS_RTOL, R.RMS_ATOL))
        assert float(cnt) == ref[u][2]
    _MERGE_RATIOS[(D, N, family)] = worst
    print(f"fp32 merge D={D} N={N} {family}: largest error / bar {worst:.3g}")
    assert worst <= 0.25, (D, N, family, worst)


def test_any_summation_order_of_the_reset_log_sits_inside_a_quarter_of_its_bar():
    """the log is a mean of fp32 quotients; the kernels sum them in fp64 per 32-env tile and fold the tiles in a fixed order,
    the reference in one float64 sum: forwards, backwards, shuffled, tile by tile - all within a quarter of 1e-6 / 1e-9"""
    worst = 0.0
    for i, row in enumerate(E.TABLE):
        if row[0] < 32 or row[0] > 5000:
            continue
        case = E.table_case(row, i)
        state = E.new_state(case)
        rs = np.random.RandomState(i)
        for t in range(E.STEPS):
            o = E.step_ref(case, state, t)
            ids = np.nonzero(o["reset"])[0]
            if not len(ids):
                continue
            n, L = len(ids), o["ep_len_pre"][ids].astype(F32)
            tiles = [ids[ids // E.POST_ROWS == k] for k in np.unique(ids // E.POST_ROWS)]
            for k in range(case["nt"]):
                for j, (acc, scale) in enumerate(((o["acc_viol"], F32(100)), (o["acc_prob"], F32(1)))):
                    q = (acc[k][ids] / L).astype(F32).astype(np.float64)      # the reference's fp32 quotients
                    by_tile = [(acc[k][tl] / o["ep_len_pre"][tl].astype(F32)).astype(F32).astype(np.float64).sum() for tl in tiles]
                    sums = [q[::-1].sum(), q[rs.permutation(n)].sum(), sum(by_tile), sum(by_tile[::-1]), float(np.cumsum(q)[-1])]
                    means = np.array([F32(s / n) * scale for s in sums], np.float64)
                    worst = max(worst, R.bar_ratio(means, np.full(len(sums), float(o["log"][2 * k + j])), E.LOG_RTOL, E.LOG_ATOL))
    print(f"reset log, any summation order: largest error / bar {worst:.3g}")
    assert worst <= 0.25, worst         # (measured: 0 - an fp64 reordering moves the sum by ~1e-16 of itself, the fp32 mean not at all)


# ====================================================================================================== non-vacuity
@pytest.mark.parametrize("index", range(len(E.TABLE)))
def test_every_case_of_the_gpu_table_is_live(index):
    case = E.table_case(E.TABLE[index], index)
    E.assert_case_is_live(case, E.run_ref(case))


@pytest.mark.parametrize("index", range(len(E.TREE_TABLE)))
def test_every_case_of_the_tree_table_is_live(index):
    case = E.table_case(E.TREE_TABLE[index], index)
    E.assert_case_is_live(case, E.run_ref(case))


@pytest.mark.parametrize("options", [{}, {"stride": 3}, {"last_step": "none"}, {"last_step": "all"}, {"row_floats": 512},
                                     {"row_floats": 516}, {"nan_inf": True}, {"H": 1}], ids=str)
def test_every_option_variant_is_live(options):
    case = E.table_case(E.VARIANT_SHAPE, **options)
    ref = E.run_ref(case)
    E.assert_case_is_live(case, ref)
    if options.get("last_step") == "none":
        assert not ref[2]["reset"].any() and ref[1]["reset"].any()
    if options.get("last_step") == "all":
        assert ref[2]["reset"].all()
    if options.get("nan_inf"):
        assert np.isnan(ref[1]["rm"]).sum() == 1 and np.isposinf(ref[1]["rm"]).sum() == 1 and np.isnan(ref[1]["reward"]).any()


@pytest.mark.parametrize("N", [17, 33, 64, 95])
@pytest.mark.parametrize("D", [1, 45, 48, 128])
def test_every_case_of_the_merged_step_is_live(N, D):
    widths = E.widths_for(64, 16)
    case = E.env_case(N, 12, D, tuple(widths), tuple(E.kinds_for(widths, 12, 5)))
    assert case["nt"] == 16 and case["K"] == 64
    E.assert_case_is_live(case, E.run_ref(case))


# ====================================================================================================== planted errors
@pytest.fixture(scope="module")
def planted():
    case = _table_case(512)                            # all 12 kinds, 32 pre tiles, 16 post tiles
    return case, E.run_ref(case)


def _table_case(N, **options):
    index = [r[0] for r in E.TABLE].index(N)
    return E.table_case(E.TABLE[index], index, **options)


def _copy(o):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()}


def _msgs(case, got, ref, t=0):
    got = dict(got)
    if case["D"]:
        got.update(obs_raw=E.obs_of(case, t), obs_mean32=got["obs_mean"].astype(F32), obs_var32=got["obs_var"].astype(F32),
                   obs_out=R.normalize32(E.obs_of(case, t), got["obs_mean"].astype(F32), got["obs_var"].astype(F32)))
    return E.compare_step(case, got, ref, "planted")


def test_the_reference_passes_its_own_comparison(planted):
    case, ref = planted
    for t in range(E.STEPS):
        assert not _msgs(case, _copy(ref[t]), ref[t], t)


def test_planted_last_env_of_the_ragged_tile_left_out():
    case = _table_case(513)                            # one env in the last tile of either kernel
    ref = E.run_ref(case)
    got = _copy(ref[0])
    last = case["N"] - 1
    got["reward"][last] = got["raw_reward"][last] + F32(1.0)
    got["dones"][last] = F32(0.5)
    got["ep_len"][last] += 7
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "reward" in msgs and f"envs [{last}]" in msgs and "16-env pre tiles [32]" in msgs and "32-env post tiles [16]" in msgs


def test_planted_tile_missing_from_a_column_maximum(planted):
    case, ref = planted
    got = _copy(ref[0])
    c = int(np.argmax(ref[0]["x_colmax"] > 1e-6))
    e = int(np.argmax(ref[0]["cstr"][:, c]))
    keep = np.ones(case["N"], bool)
    keep[e // 16 * 16:e // 16 * 16 + 16] = False
    got["x_colmax"] = np.maximum(ref[0]["cstr"][keep].max(0), F32(1e-6))
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "x_colmax" in msgs and f"columns [{c}" in msgs and f"terms [{E.term_of(case, c)}" in msgs and "fold groups" in msgs


def test_planted_tile_missing_from_a_moment_sum_shows_in_the_record_not_in_the_state():
    """N = 16400: 1025 pre tiles on 1024 workgroups, workgroup 0 walks tile 1024 as its second one.  (a) That tile left out
    of the sums: the record's fp64 sums reject it - and so does the normaliser state, because the divisor is the caller's
    row count, not the number of rows summed (the mean moves by 16 / 16400 of itself: hundreds of bars).  (b) Tile 0 walked
    twice in its place: the state moves by the sampling noise of 16 rows, far inside its bar - the normaliser state alone
    does not see the wrong tile, the record's sums do."""
    case = _table_case(16400, family="offset")
    ref = E.run_ref(case)
    x = E.obs_of(case, 0)
    n = float(case["N"])
    left_out, twice = x[:16384], np.concatenate([x[:16384], x[:16]])
    for rows, state_sees in ((left_out, True), (twice, False)):
        got = _copy(ref[0])
        (s1, _), (s2, _) = R.moment_sums64(rows)
        got["x_sums"] = np.concatenate([s1, s2])
        got["obs_mean"], got["obs_var"], _ = normaliser_from32(s1, s2, n, case["rms0"][0], case["rms0"][1], case["rms0"][2])
        msgs = _msgs(case, got, ref[0])
        assert any("record sums" in s and "observation column 0" in s and "fold group" in s for s in msgs), msgs
        assert any("obs_mean" in s or "obs_var" in s for s in msgs) == state_sees, msgs


def test_planted_reset_count_of_one_tile_off_by_one(planted):
    case, ref = planted
    got = _copy(ref[0])
    n = int(ref[0]["reset"].sum())
    got["log"] = (ref[0]["log"].astype(np.float64) * n / (n + 1)).astype(F32)
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "log_out" in msgs and "of term" in msgs


def test_planted_division_by_the_already_zeroed_episode_length(planted):
    case, ref = planted
    state = E.new_state(case)
    o = E.step_ref(case, state, 0)
    ids = np.nonzero(o["reset"])[0]
    got = _copy(ref[0])
    # the accumulators in front of the reset: the reference's log times the lengths says they were not all zero
    viol = np.ones((case["nt"], case["N"]), F32)
    got["log"] = E.reset_log(viol, viol, o["ep_len"], ids)              # o["ep_len"]: zero for the envs that reset
    assert not np.isfinite(got["log"]).any()
    assert "log_out" in "\n".join(_msgs(case, got, ref[0]))


def test_planted_term_columns_shifted_by_one(planted):
    case, ref = planted
    got = _copy(ref[0])
    t = 6
    a, b = case["off"][t], case["off"][t + 1]
    got["cstr"][:, a:b] = np.roll(ref[0]["cstr"][:, a:b], 1, axis=1)
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "cstr" in msgs and f"terms [{t}]" in msgs


def test_planted_time_out_that_does_not_set_dones(planted):
    case, ref = planted
    got = _copy(ref[0])
    e = int(np.nonzero(ref[0]["time_outs"].astype(bool) & ~ref[0]["terminated"].astype(bool))[0][0])
    got["dones"][e] = ref[0]["cstr_prob"][e]
    assert ref[0]["cstr_prob"][e] != 1.0
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "dones" in msgs and f"envs [{e}]" in msgs


def test_planted_plane_rounded_to_fp16_by_truncation(planted):
    case, _ = planted
    ref = E.run_ref(case, f16=True)
    got = _copy(ref[0])
    r32 = ref[0]["reward"]
    trunc = (r32.view(np.uint32) & np.uint32(0xFFFFE000)).view(F32).astype(np.float16)      # drop the 13 low mantissa bits
    assert (trunc != ref[0]["rewards_t"]).any()
    got["rewards_t"] = trunc
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert "rewards_t" in msgs and "post tiles" in msgs


def test_planted_zero_action_not_applied_to_prev_action(planted):
    case, ref = planted
    got = _copy(ref[0])
    got["prev_action"] = ref[0]["prev_action_pre"].copy()
    msgs = "\n".join(_msgs(case, got, ref[0]))
    e = int(np.nonzero(ref[0]["reset"])[0][0])
    assert "prev_action" in msgs and f"envs [{e}" in msgs and ": action" not in msgs


def test_planted_tau_and_one_minus_tau_swapped(planted):
    case, ref = planted
    got = _copy(ref[1])
    tau, omt = F32(E.TAU), F32(1.0 - E.TAU)
    got["rm"] = ((ref[0]["rm"] * omt).astype(F32) + (tau * ref[1]["x_colmax"]).astype(F32)).astype(F32)
    right = ((ref[0]["rm"] * tau).astype(F32) + (omt * ref[1]["x_colmax"]).astype(F32)).astype(F32)
    assert not R.bits_report("rm restated", right, ref[1]["rm"])
    msgs = "\n".join(_msgs(case, got, ref[1], 1))
    assert ": rm" in msgs and "terms [" in msgs


def test_planted_second_rank_record_ignored():
    case = E.table_case(E.VARIANT_SHAPE)
    records = E.other_rank_records(case)
    ref = E.run_ref(case, records=records)
    short = E.run_ref(case, records=[r[:1] for r in records])
    got = _copy(short[0])
    msgs = "\n".join(_msgs(case, got, ref[0]))
    assert ": rm" in msgs and "obs_mean" in msgs and "obs_count" in msgs
