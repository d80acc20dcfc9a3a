"""CPU checks of tests/stat_refs.py, the references and comparisons behind tests/test_gpu_stat_kernels.py.

1. Bars against the references alone.  On every input family the GPU module uses, the project's fp32 reference stays within
   a QUARTER of the bar against the float64 restatement, so a kernel that is as good as the fp32 reference passes with room
   and one that is four times worse does not.  Measured (largest error / bar over all shapes and the three updates):

     normaliser state (rtol 2e-6, atol 1e-6), RMSOracle against float64, all fourteen shapes, three updates
       'spread'  randn * U(0.1, 5) + U(-2, 2)    mean 0.13   var 0.10     fp16 copy, widened: mean 0.10   var 0.11
       'offset'  0.01 randn + 100                mean 0.097  var 0.090    fp16 copy, widened: mean 0.053  var 0.018
     clip + Adam (params rtol 1e-6 atol 1e-6; grad / exp_avg / exp_avg_sq rtol 1e-5), torch Adam against float64, three
     steps (norm ~10 clipped to 1, norm ~0.01, zero gradient) at the ten sizes
       params <= 0.11, grad <= 0.0066, exp_avg <= 0.016, exp_avg_sq <= 0.014
       (with NORMAL gradient draws torch's own fp32 norm over 1048579 elements is off by 1.4e-5: grad 1.39, exp_avg 1.18,
       exp_avg_sq 0.55 of the bar, 0.18 / 0.16 / 0.16 at 262144 - the family was changed, not the bar: stat_refs.opt_case)
     advantage statistics, torch fp32 mean() / std() against float64 two-pass, in ulp of the value, n = 2 ... 524293
       'centred' 2 randn + 0.3    mean <= 0.50 ulp, std <= 0.45 ulp: every bar sits at the 2-ulp floor
       'offset'  0.01 randn + 50  mean <= 1.48 ulp, std <= 2.40 ulp (bars 2.0 - 5.9 and 2.0 - 9.6 ulp); at n = 2 the std of
                                  two samples 3.8e-6 apart in fp32 is off by 425 ulp in torch (bar 1701 ulp of 2.9e-4)
     The kernels accumulate in fp64 and round once to fp32 (once more for `+ 1e-8`): they owe at most 1 ulp.

2. Planted errors.  Each comparison rejects the error it is there for, applied to the reference's own output: the last
   row left out of the moments, columns >= 256 left stale, the idle-lane column D - 1 zeroed, count not advanced, the last
   n % 4 elements of an Adam step not updated, the clip coefficient from a norm that misses the last 1024 elements, one CaT
   column maximum taken over all rows but the last.

3. The oracle's NaN / Inf behaviour in the CaT step equals the reference implementation's (tests/golden/cat_nan_inf.npz was
   written by the reference's own `CaT` class on the inputs of stat_refs.cat_case(100, 33, 7, nan_inf=True))."""
import os

import numpy as np
import pytest

import stat_refs as R

F32 = np.float32
QUARTER = 0.25


def _f16(batches):
    return [b.astype(np.float16).astype(F32) for b in batches]


# ------------------------------------------------------------------------------------------------ 1. bars
@pytest.mark.parametrize("family", R.RMS_FAMILIES)
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_rms_oracle_stays_within_a_quarter_of_the_bar(family, half):
    worst = {"mean": 0.0, "var": 0.0}
    for D, N, ldx in R.RMS_SHAPES:
        state0, batches = R.rms_case(D, N, ldx, family)
        if half:
            batches = _f16(batches)
        s64 = R.rms_states64(state0, batches, D)
        s32 = R.rms_states_oracle32(state0, batches, D)
        for (m64, v64, c64), (m32, v32, c32) in zip(s64, s32):
            assert c32 == c64
            rm, rv = R.bar_ratio(m32, m64, R.RMS_RTOL, R.RMS_ATOL), R.bar_ratio(v32, v64, R.RMS_RTOL, R.RMS_ATOL)
            worst["mean"], worst["var"] = max(worst["mean"], rm), max(worst["var"], rv)
            assert rm <= QUARTER and rv <= QUARTER, (D, N, family, half, rm, rv)
    print(f"rms {family} {'fp16' if half else 'fp32'}: RMSOracle / bar  mean {worst['mean']:.3g}  var {worst['var']:.3g}")


@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_torch_adam_stays_within_a_quarter_of_the_bar(n):
    p0, grads = R.opt_case(n)
    t64, t32 = R.opt_trajectory64(p0, grads), R.opt_trajectory_torch(p0, grads)
    worst = {k: 0.0 for k in R.OPT_BARS}
    for a, b in zip(t32, t64):
        for k, (rtol, atol) in R.OPT_BARS.items():
            worst[k] = max(worst[k], R.bar_ratio(a[k], b[k], rtol, atol))
    print(f"adam n={n}: torch / bar " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= QUARTER, worst
    # the three steps take the branches their names say
    for g, clipped in zip(grads[:2], (True, False)):
        assert (np.sqrt(float((g.astype(np.float64) ** 2).sum())) > 1.0) == clipped
    assert not grads[2].any()


@pytest.mark.parametrize("family", R.ADV_FAMILIES)
def test_torch_advantage_statistics_error_and_bars(family):
    """torch's fp32 error in ulp, per size (the numbers of the module docstring).  The bar built from it may not be vacuous:
    at most 16 ulp of the value (a cascaded fp32 sum of n <= 2^20 values is good to a few ulp) or, for the std, 4 ulp of the
    MEAN (an fp32 algorithm subtracts an fp32-rounded mean from every sample: with 0.01 randn + 50 that alone is worth
    hundreds of ulp of a std of 3e-4 at n = 2)"""
    for n in R.ADV_SIZES:
        x = R.adv_case(n, family)
        m64, s64, bm, bs = R.adv_bars(x)
        m32, s32 = R.adv_stats_torch32(x)
        em = abs(m32 - m64) / R.ulp32(m64)
        if n == 1:
            assert np.isnan(s64) and np.isnan(s32) and np.isnan(bs)
            print(f"adv {family} n=1: mean {em:.2f} ulp, std NaN")
            continue
        es = abs(s32 - s64) / R.ulp32(s64)
        print(f"adv {family} n={n}: torch fp32 mean {em:.2f} ulp, std {es:.2f} ulp; bars {bm / R.ulp32(m64):.1f} / "
              f"{bs / R.ulp32(s64):.1f} ulp")
        assert 2 * R.ulp32(m64) <= bm <= 16 * R.ulp32(m64)
        assert 2 * R.ulp32(s64) <= bs <= max(16 * R.ulp32(s64), 4 * R.ulp32(m64))


def test_normalize_restatement_is_fp32_and_matches_the_oracle():
    """normalize32 is RMSOracle.normalize (torch fp32 on the CPU) bit for bit: same operations, same order"""
    import torch
    from oracle import ppo_oracle as PO
    for family in R.RMS_FAMILIES:
        state0, batches = R.rms_case(100, 777, 100, family)
        o = PO.RMSOracle((100,))
        o.mean, o.var = torch.from_numpy(state0[0].copy()), torch.from_numpy(state0[1].copy())
        got = R.normalize32(batches[0], state0[0], state0[1])
        assert got.dtype == F32
        assert not R.bits_report("normalize32", got, o.normalize(torch.from_numpy(batches[0])).numpy(), row_block=1)


# ------------------------------------------------------------------------------------------------ 2. planted errors
def _state_msgs(got, ref):
    msgs = R.column_report("mean", got[0], ref[0], R.RMS_RTOL, R.RMS_ATOL)
    msgs += R.column_report("var", got[1], ref[1], R.RMS_RTOL, R.RMS_ATOL)
    if got[2] != ref[2]:
        msgs.append(f"count {got[2]} != {ref[2]}")
    return msgs


@pytest.mark.parametrize("family", R.RMS_FAMILIES)
def test_planted_errors_in_the_normaliser_are_rejected(family):
    for D, N, ldx in R.RMS_SHAPES:
        state0, batches = R.rms_case(D, N, ldx, family)
        s0 = tuple(np.asarray(s, np.float64) for s in state0)
        x = np.asarray(batches[0][:, :D], np.float64)
        ref = R.rms_update64(*s0, x)
        assert not _state_msgs(ref, ref)
        # (a) the last row left out of the moments: the fp64 column sums show it at every N ...
        if N > 1:
            (s1, b1), (s2, b2) = R.moment_sums64(x)
            (t1, _), (t2, _) = R.moment_sums64(x[:-1])
            assert (np.abs(t1 - s1) > b1).all() and (np.abs(t2 - s2) > b2).all(), (D, N)
        # ... the fp32 state only while one row of N moves the mean by more than the bar: N <= 1000 of the 'spread' family
        # (one row of 0.01 randn + 100 moves a mean of 100 by 1e-5 / N, a twentieth of the bar at N = 1: the sums carry it)
        if 1 < N <= 1000 and family == "spread":
            part = R.rms_update64(*s0, x[:-1])
            bad = (part[0], part[1], part[2] + 1)
            msgs = _state_msgs(bad, ref)
            assert msgs and "column" in msgs[0], (D, N)
        # (b) columns >= 256 left stale
        if D > 256:
            stale = (np.where(np.arange(D) >= 256, s0[0], ref[0]), np.where(np.arange(D) >= 256, s0[1], ref[1]), ref[2])
            msgs = _state_msgs(stale, ref)
            assert msgs and "column blocks [1" in msgs[0] and "(block 1, lane" in msgs[1] and "(block 0," not in "\n".join(msgs), msgs
        # (c) the idle-lane column D - 1 zeroed
        z = (ref[0].copy(), ref[1].copy(), ref[2])
        z[0][D - 1] = 0.0
        z[1][D - 1] = 0.0
        msgs = _state_msgs(z, ref)
        assert msgs and f"column {D - 1} (block {(D - 1) // 256}, lane {(D - 1) % 256})" in "\n".join(msgs), msgs
        # (d) count not advanced
        assert _state_msgs((ref[0], ref[1], s0[2]), ref) == [f"count {float(s0[2])} != {ref[2]}"]
        # the normalise output: one stale row / one stale pad-adjacent column is named
        if N <= 1000:
            out = R.normalize32(batches[0][:, :D], state0[0], state0[1])
            bad = out.copy()
            bad[N - 1, D - 1] = np.nextafter(bad[N - 1, D - 1], F32(np.inf))          # one ulp, one entry
            msgs = R.bits_report("out", bad, out, row_block=1, col_block=R.COL_BLOCK)
            assert msgs and f"({N - 1}, {D - 1})" in msgs[1], msgs


@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_planted_errors_in_the_optimiser_are_rejected(n):
    p0, grads = R.opt_case(n)
    ref = R.opt_trajectory64(p0, grads)
    assert not R.opt_report("ref", ref[0], ref[0])
    z = np.zeros(n)
    # (e) the last n % 4 elements of an Adam step not updated (parameters, gradient and both moments keep their input)
    if n % 4:
        tail = slice(n - n % 4, n)
        bad = {k: v.copy() for k, v in ref[0].items()}
        bad["params"][tail], bad["grad"][tail] = p0[tail], grads[0][tail]
        bad["exp_avg"][tail] = bad["exp_avg_sq"][tail] = 0.0
        msgs = R.opt_report("step 1", bad, ref[0])
        assert len([m for m in msgs if "all in the n % 4 tail" in m]) == 4, msgs
        assert f"index % 4 = {(n - n % 4) % 4}" in "\n".join(msgs)
    # (f) the clip coefficient from a norm that misses the last 1024 elements
    p, g, m, v = R.clip_adam64(p0, grads[0], z, z, 1, norm_over=slice(0, max(n - 1024, 0)))
    msgs = R.opt_report("step 1", {"params": p, "grad": g, "exp_avg": m, "exp_avg_sq": v}, ref[0])
    assert any("grad" in s for s in msgs) and any("exp_avg_sq" in s for s in msgs), (n, msgs)
    # one element of the float4 body off by 4 bars is named with its lane of the float4
    if n >= 8:
        bad = {k: v.copy() for k, v in ref[0].items()}
        bad["grad"][6] *= 1 + 4e-5
        msgs = R.opt_report("step 1", bad, ref[0])
        assert "all in the float4 body" in msgs[0] and "element 6 (index % 4 = 2" in msgs[1], msgs


def test_planted_error_in_a_cat_column_maximum_is_rejected():
    for K, N, nt in [c for c in R.CAT_CASES if c[1] > 1 and c[1] <= 1000]:
        widths, max_p, steps = R.cat_case(K, N, nt)
        assert sum(widths) == K and len(widths) == nt and min(widths) >= 1
        ref, viol, eprob = R.cat_oracle_run(K, N, widths, max_p, steps)
        assert not R.cat_report("ref", ref, viol, eprob, ref, viol, eprob)
        # (g) the maximum of column K - 1 taken over all rows but the last (step 0 is the first call: rm = max(colmax, 1e-6))
        c = steps[0]["cstr"]
        assert c[:, K - 1].argmax() == N - 1 and c[:, 0].argmax() == 0
        bad = [dict(s) for s in ref]
        bad[0]["rm"] = ref[0]["rm"].copy()
        bad[0]["rm"][K - 1] = max(c[:-1, K - 1].max(), F32(1e-6))
        msgs = R.cat_report("cat", bad, viol, eprob, ref, viol, eprob)
        assert len(msgs) == 2 and "step 0 running maxima" in msgs[0] and f"column blocks [{(K - 1) // 256}]" in msgs[0], msgs
        # violating and never-violating columns are both present wherever there is room for them
        assert (ref[0]["probs"] > 0).any() and (K < 7 or (ref[0]["rm"] == F32(1e-6)).any())


def test_guard_report_names_an_overwritten_guard():
    buf = np.full(20, 12345.678, F32)
    bits = int(buf.view(np.uint32)[0])
    buf[4:14] = 1.0
    assert not R.guard_report("b", buf, bits, 4, 14)
    buf[14] = 1.0
    assert "flat offsets [14]" in R.guard_report("b", buf, bits, 4, 14)[0]


def test_moments_grid_restatement_reaches_what_the_table_says():
    assert R.moments_grid(1, 1) == (256, 1, 256, 1)
    assert R.moments_grid(98304, 1) == (256, 3, 768, 128)
    assert R.moments_grid(600000, 1) == (256, 16, 4096, 128) and -(-600000 // 4096) > 128
    assert R.moments_grid(40000, 45) == (5, 16, 80, 128) and -(-40000 // 80) == 500
    assert R.moments_grid(300, 128)[0] == 2 and R.moments_grid(300, 129)[0] == 1


# ------------------------------------------------------------------------------------------------ 3. NaN / Inf in the CaT oracle
def test_cat_oracle_nan_inf_follows_the_reference(golden):
    if not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cat_nan_inf.npz")):
        pytest.fail("tests/golden/cat_nan_inf.npz is missing")
    g = golden("cat_nan_inf")
    K, N, nt = int(g["K"]), int(g["N"]), int(g["n_terms"])
    widths, max_p, steps = R.cat_case(K, N, nt, nan_inf=True)
    assert widths == g["widths"].tolist() and np.array_equal(np.asarray(max_p), g["max_p"])
    for t, s in enumerate(steps):
        assert np.array_equal(s["cstr"], g["cstr"][t], equal_nan=True)          # the same inputs the reference consumed
    assert np.isnan(steps[1]["cstr"]).sum() == 1 and np.isposinf(steps[1]["cstr"]).sum() == 1
    ref, _, _ = R.cat_oracle_run(K, N, widths, max_p, steps)
    for t in range(len(steps)):
        for k, name in (("rm", "running_maxes"), ("prob", "cstr_prob"), ("probs", "probs")):
            assert not R.bits_report(f"step {t} {k}", ref[t][k], g[name][t], row_block=R.FINISH_ROWS, col_block=R.COL_BLOCK)
    # the NaN reaches the running maximum of its column and stays; the Inf column's maximum is Inf
    assert np.isnan(ref[1]["rm"][K // 3]) and np.isnan(ref[2]["rm"][K // 3]) and np.isposinf(ref[1]["rm"][2 * K // 3])
    assert np.isnan(ref[1]["prob"]).any() and not np.isnan(ref[0]["prob"]).any()
