"""The kernels between the MLP and GAE - RunningMeanStd (csrc/rms.hip), the CaT step (csrc/cat_step.hip), clip + Adam
(csrc/mlp_optim.h), the advantage statistics (csrc/env_step.hip, catppo_adv_normalize) - at the sizes where their code
branches on geometry, against the float64 restatements of tests/stat_refs.py (CaT: oracle/cat_oracle.py, bit for bit).
tests/test_stat_refs.py shows on the CPU that the bars leave the fp32 references a factor of four and that every comparison
used here rejects a planted lane-mask / block / tail error.

Every output lives inside a larger buffer filled with a sentinel: guard elements in front of and behind the result and pad
columns (ldo > D) must come back bit-identical.  Pad columns of the inputs (ldx > D) hold NaN.  Every RunningMeanStd, CaT and
optimiser case runs twice: in the module's context, and in a second context whose workspace is refilled with NaN before every
library call (the partial sums of all these kernels live there); the two runs must agree in every byte.

RunningMeanStd, three updates from a non-default state + a normalise after each, both input families, fp32 and fp16 input:
   D        N       ldx   what it reaches
   1        1       1     smallest; G = 256
   1        98304   1     per_thread = 3, 128 workgroups
   1        600000  1     16 rows per thread, grid capped at 128, grid-stride row loop
   3        1000    4     one idle lane (256 % 3)
   45       40000   48    16 rows per thread, 500 -> 128 workgroups
   100      777     100   56 idle lanes
   128/129  300     128/136   G = 2 -> G = 1
   255/256/257  64  256/256/264   second column block of one column
   512/513  40      512/520   last fused (two-launch) shape / first three-launch shape
   1000     33      1000  four column blocks, the last ragged
CaT step (fused and colmax + apply), three steps each: K x N x terms of stat_refs.CAT_CASES - G = 256 and the capped grid
(K = 1), idle lanes, G = 2 -> 1 (K = 128 / 129), the second column block (K = 255 / 256 / 257 with 64 uneven terms), 64
terms of width 1, the last shape under and the first over 64 KB of dynamic LDS (K = 480 / 512), the widest accepted
(K = 1128, 150 KB)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import parity_record
import stat_refs as R
import streams as S
from oracle import ppo_oracle as PO
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 12345.678
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def nat():
    from cat_envs import native
    return native.Native()


class Used:
    """A second context whose workspace (8 MB by default; these kernels carve their partials from its start) is refilled
    with NaN before EVERY library call: an rms_moments over 128 x 1024 NaN leaves 2 MB of fp64 NaN partials, a cat_colmax over
    1024 x 1024 NaN then 512 KB of fp32 NaN on top - more than any case of this module carves (528 KB)."""

    def __init__(self):
        from cat_envs import native
        self.nat = native.Native()
        self.xnan = torch.full((128, 1024), float("nan"), device="cuda")
        self.cnan = torch.full((1024, 1024), float("nan"), device="cuda")
        self.sums = torch.zeros(2048, dtype=torch.float64, device="cuda")
        self.colmax = torch.zeros(1024, device="cuda")

    def poison(self):
        self.nat.rms_moments(self.xnan, 128, 1024, 1024, self.sums)
        self.nat.cat_colmax(self.cnan, self.colmax)

    def __getattr__(self, name):
        f = getattr(self.nat, name)

        def call(*a, **k):
            self.poison()
            return f(*a, **k)
        return call


@pytest.fixture(scope="module")
def used():
    u = Used()
    u.poison()
    torch.cuda.synchronize()
    assert bool(torch.isnan(u.sums).all()) and bool(torch.isnan(u.colmax).all())
    return u


class Guarded:
    """n elements inside a sentinel-filled buffer: `lead` guard elements in front (4 + k floats put the result k floats
    past 16-byte alignment), 8 behind"""

    def __init__(self, n, dtype=torch.float32, lead=8, value=None):
        self.n, self.lo, self.hi = n, lead, lead + n
        self.buf = torch.full((lead + n + 8,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[self.lo:self.hi]
        np_dtype = self.buf[:1].cpu().numpy().dtype
        self.bits = int(np.array([SENTINEL], np_dtype).view(_UINT[np_dtype.itemsize])[0])
        if value is not None:
            self.set(value)

    def set(self, a):
        self.view.copy_(torch.as_tensor(np.ascontiguousarray(a)).reshape(-1).to(self.buf.dtype))

    def raw(self):
        return self.buf.cpu().numpy().copy()

    def of(self, raw):
        return raw[self.lo:self.hi]

    def guard_msgs(self, name, raw, rows=None, cols=None, ld=None):
        """the guards - and, for a (rows, ld) matrix of `cols` used columns, its pad columns - still hold the sentinel"""
        msgs = R.guard_report(name, raw, self.bits, self.lo, self.hi)
        if ld is not None and ld > cols:
            pad = self.of(raw).reshape(rows, ld)[:, cols:]
            bad = np.argwhere(np.ascontiguousarray(pad).view(_UINT[pad.dtype.itemsize]) != self.bits)
            if bad.shape[0]:
                msgs.append(f"{name}: {bad.shape[0]} pad entries overwritten, first (row {bad[0][0]}, column {cols + bad[0][1]})")
        return msgs


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_runs_identical(fresh, usedrun):
    """every buffer of a run (guards included) byte for byte, fresh context against used workspace"""
    assert fresh.keys() == usedrun.keys()
    bad = [k for k in fresh if len(fresh[k]) != len(usedrun[k]) or
           not all(_same_bytes(a, b) for a, b in zip(fresh[k], usedrun[k]))]
    assert not bad, f"differs on a used (NaN-filled) workspace: {bad}"


_RATIOS = {}


def _note_ratio(family, case, ratio):
    """largest error / bar seen per kernel family (the sanity record: the cases are not vacuous)"""
    best = _RATIOS.setdefault(family, {"ratio": -1.0, "case": None})
    if ratio > best["ratio"]:
        best["ratio"], best["case"] = float(ratio), str(case)
    parity_record.record("stat_kernels_" + family, {"largest_error_over_bar": best["ratio"]}, note=best["case"])


# ====================================================================================================== RunningMeanStd
def _ldo(D, ldx):
    return ldx if ldx > D else (D + 4 if D == 100 else D)


def _widen(x, half):
    return x.astype(np.float16).astype(F32) if half else x


def _run_rms(ctx, D, N, ldx, family, half):
    """three times: moments + merge on one state, the update entry on another, a normalise -> raw buffers per update"""
    state0, batches = R.rms_case(D, N, ldx, family)
    ldo = _ldo(D, ldx)
    fused = not half or D <= 512                     # the fp16 update entry is the fused one only (2 D <= 1024)
    one = [Guarded(D, value=state0[0]), Guarded(D, value=state0[1]), Guarded(1, value=[state0[2]])]
    two = [Guarded(D, value=state0[0]), Guarded(D, value=state0[1]), Guarded(1, value=[state0[2]])]
    sums, out = Guarded(2 * D, torch.float64), Guarded(N * ldo)
    run = {k: [] for k in ("mean", "var", "count", "mean2", "var2", "count2", "sums", "out")}
    for x in batches:
        xd = dev(x.astype(np.float16) if half else x)
        ctx.rms_moments_ex(xd, N, D, ldx, sums.view)
        ctx.rms_merge(sums.view, N, D, two[0].view, two[1].view, two[2].view)
        if fused:
            ctx.rms_update_ex(xd, N, D, ldx, one[0].view, one[1].view, one[2].view)
        st = one if fused else two
        ctx.rms_normalize_ex(xd, N, D, ldx, st[0].view, st[1].view, R.EPS, out.view, ldo)
        torch.cuda.synchronize()
        for k, g in zip(("mean", "var", "count", "mean2", "var2", "count2", "sums", "out"), one + two + [sums, out]):
            run[k].append(g.raw())
    return run, (one, two, sums, out, ldo, fused)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("family", R.RMS_FAMILIES)
@pytest.mark.parametrize("D,N,ldx", R.RMS_SHAPES)
def test_running_mean_std_at_the_geometry_edges(nat, used, D, N, ldx, family, half):
    state0, batches = R.rms_case(D, N, ldx, family)
    wide = [_widen(b, half) for b in batches]                       # fp16 input: the reference sees the exactly widened values
    ref = R.rms_states64(state0, wide, D)
    run, (one, two, sums, out, ldo, fused) = _run_rms(nat, D, N, ldx, family, half)
    msgs, worst = [], 0.0
    for u in range(R.RMS_UPDATES):
        tag = f"D={D} N={N} ldx={ldx} {family} {'fp16' if half else 'fp32'} update {u}"
        m2, v2, c2 = (g.of(run[k][u]) for g, k in zip(two, ("mean2", "var2", "count2")))
        m, v, c = (g.of(run[k][u]) for g, k in zip(one, ("mean", "var", "count"))) if fused else (m2, v2, c2)
        # the state against float64, column by column
        msgs += R.column_report(f"{tag}: mean", m, ref[u][0], R.RMS_RTOL, R.RMS_ATOL)
        msgs += R.column_report(f"{tag}: var", v, ref[u][1], R.RMS_RTOL, R.RMS_ATOL)
        if float(c[0]) != ref[u][2]:                                  # integers below 2^24: exact in fp32
            msgs.append(f"{tag}: count {float(c[0])}, expected {ref[u][2]}")
        worst = max(worst, R.bar_ratio(m, ref[u][0], R.RMS_RTOL, R.RMS_ATOL), R.bar_ratio(v, ref[u][1], R.RMS_RTOL, R.RMS_ATOL))
        # moments + merge == the update entry, bit for bit
        if fused:
            msgs += R.bits_report(f"{tag}: mean of moments + merge vs update", m2, m, col_block=R.COL_BLOCK)
            msgs += R.bits_report(f"{tag}: var of moments + merge vs update", v2, v, col_block=R.COL_BLOCK)
            msgs += R.bits_report(f"{tag}: count of moments + merge vs update", c2, c)
        # the fp64 column sums (this is where ONE missing row shows at any N)
        (s1, b1), (s2, b2) = R.moment_sums64(wide[u][:, :D])
        got = sums.of(run["sums"][u])
        for name, g_, r_, b_ in (("sum x", got[:D], s1, b1), ("sum x^2", got[D:], s2, b2)):
            bad = np.nonzero(~(np.abs(g_ - r_) <= b_))[0]
            if bad.size:
                msgs.append(f"{tag}: {name}: {bad.size} of {D} columns off, first column {bad[0]} (block {bad[0] // R.COL_BLOCK}): "
                            f"got {g_[bad[0]]!r}, reference {r_[bad[0]]!r}, bar {b_[bad[0]]:.3g}")
        # the normalised rows: IEEE sqrt and division in unfused fp32, on the device's own mean / var
        o = out.of(run["out"][u]).reshape(N, ldo)[:, :D]
        msgs += R.bits_report(f"{tag}: normalised", o, R.normalize32(wide[u][:, :D], m, v), col_block=R.COL_BLOCK)
        # guards and pad columns
        for g, k in zip(one + two + [sums], ("mean", "var", "count", "mean2", "var2", "count2", "sums")):
            msgs += g.guard_msgs(f"{tag}: {k}", run[k][u])
        msgs += out.guard_msgs(f"{tag}: out", run["out"][u], rows=N, cols=D, ld=ldo)
    print(f"rms D={D} N={N} {family} {'fp16' if half else 'fp32'}: largest state error / bar {worst:.3g}")
    _note_ratio("running_mean_std", f"D={D} N={N} {family} {'fp16' if half else 'fp32'}", worst)
    assert not msgs, "\n".join(msgs[:40])
    rerun, _ = _run_rms(used, D, N, ldx, family, half)
    _assert_runs_identical(run, rerun)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("D", [8192, 8193, 16384])
def test_normalize_wide_rows_up_to_128_kb_of_lds(nat, D, half):
    """8 D bytes of dynamic LDS: 64 KB at D = 8192, the first byte more at 8193, 128 KB at the widest accepted D"""
    N = 3
    rs = np.random.RandomState(D)
    x = _widen((rs.standard_normal((N, D)) * 3 + 1).astype(F32), half)
    mean, var = rs.uniform(-1, 1, D).astype(F32), rs.uniform(0.5, 2, D).astype(F32)
    out = Guarded(N * D)
    nat.rms_normalize_ex(dev(x.astype(np.float16) if half else x), N, D, D, dev(mean), dev(var), R.EPS, out.view, D)
    torch.cuda.synchronize()
    raw = out.raw()
    msgs = R.bits_report(f"normalise D={D}", out.of(raw).reshape(N, D), R.normalize32(x, mean, var), col_block=R.COL_BLOCK)
    msgs += out.guard_msgs("out", raw)
    assert not msgs, "\n".join(msgs)


def test_normalize_rejects_rows_wider_than_its_lds(nat):
    D = 16385
    z = torch.zeros(3 * D, device="cuda")
    with pytest.raises(RuntimeError, match="D <= 16384"):
        nat.rms_normalize(z, 3, D, D, z, z, R.EPS, torch.zeros(3 * D, device="cuda"), D)


# ====================================================================================================== CaT step
def _run_cat(ctx, K, N, nt, two_phase, nan_inf=False):
    from cat_envs import native
    widths, max_p, steps = R.cat_case(K, N, nt, nan_inf)
    off = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
    off_c = (C.c_int32 * (nt + 1))(*off.tolist())
    dp = (C.c_float * nt)(*[native.f32(p - R.CAT_MIN_P) for p in max_p])
    g = {"rm": Guarded(K, value=np.zeros(K)), "prob": Guarded(N), "probs": Guarded(N * K), "reward": Guarded(N),
         "dones": Guarded(N), "viol": Guarded(nt * N, value=np.zeros(nt * N)), "eprob": Guarded(nt * N, value=np.zeros(nt * N)),
         "colmax": Guarded(K)}
    run = {k: [] for k in g}
    for t, s in enumerate(steps):
        cstr, reset = dev(s["cstr"]), dev(s["reset"])
        g["reward"].set(s["reward"])
        kw = dict(reward=g["reward"].view, reset_mask=reset, dones=g["dones"].view, probs=g["probs"].view)
        if two_phase:
            ctx.cat_colmax(cstr, g["colmax"].view)
            ctx.cat_apply(cstr, off_c, dp, R.CAT_MIN_P, R.CAT_TAU, t == 0, g["colmax"].view, g["rm"].view, g["prob"].view,
                          g["viol"].view, g["eprob"].view, **kw)
        else:
            ctx.cat_step(cstr, off_c, dp, R.CAT_MIN_P, R.CAT_TAU, t == 0, g["rm"].view, g["prob"].view, g["viol"].view,
                         g["eprob"].view, **kw)
        torch.cuda.synchronize()
        for k in g:
            run[k].append(g[k].raw())
    return run, g


@functools.lru_cache(maxsize=2)
def _cat_ref(K, N, nt, nan_inf=False):
    widths, max_p, steps = R.cat_case(K, N, nt, nan_inf)
    return R.cat_oracle_run(K, N, widths, max_p, steps)


def _check_cat(nat, used, K, N, nt, two_phase, nan_inf=False):
    ref, viol, eprob = _cat_ref(K, N, nt, nan_inf)
    run, g = _run_cat(nat, K, N, nt, two_phase, nan_inf)
    tag = f"K={K} N={N} terms={nt} {'colmax + apply' if two_phase else 'fused'}"
    got = [{"rm": g["rm"].of(run["rm"][t]), "prob": g["prob"].of(run["prob"][t]),
            "probs": g["probs"].of(run["probs"][t]).reshape(N, K), "reward": g["reward"].of(run["reward"][t]),
            "dones": g["dones"].of(run["dones"][t])} for t in range(R.CAT_STEPS)]
    msgs = R.cat_report(tag, got, g["viol"].of(run["viol"][-1]).reshape(nt, N), g["eprob"].of(run["eprob"][-1]).reshape(nt, N),
                        ref, viol, eprob)
    if two_phase:       # the published column maxima: floored at 1e-6 = the running maxima of the first call
        msgs += R.bits_report(f"{tag}: colmax of step 0", g["colmax"].of(run["colmax"][0]), ref[0]["rm"], col_block=R.COL_BLOCK)
    for k in g:
        if k != "colmax" or two_phase:
            for t in range(R.CAT_STEPS):
                msgs += g[k].guard_msgs(f"{tag}: {k} step {t}", run[k][t])
    assert not msgs, "\n".join(msgs[:40])
    rerun, _ = _run_cat(used, K, N, nt, two_phase, nan_inf)
    _assert_runs_identical(run, rerun)
    return got


@pytest.mark.parametrize("two_phase", [False, True], ids=["fused", "colmax_apply"])
@pytest.mark.parametrize("K,N,nt", R.CAT_CASES)
def test_cat_step_at_the_geometry_edges(nat, used, K, N, nt, two_phase):
    got = _check_cat(nat, used, K, N, nt, two_phase)
    assert (got[0]["probs"] > 0).any() and (N * K < 8 or (got[0]["probs"] == 0).any())


@pytest.mark.parametrize("two_phase", [False, True], ids=["fused", "colmax_apply"])
def test_cat_step_nan_and_inf_propagate_like_torch(nat, used, two_phase):
    """one NaN and one +Inf in different columns of step 1: the NaN reaches the running maximum of its column (and stays
    there), the probabilities of its column, the env maximum, reward and dones, exactly as the reference's torch ops do
    (tests/test_stat_refs.py holds the oracle against the reference's own output on these inputs)"""
    K, N, nt = 100, 33, 7
    got = _check_cat(nat, used, K, N, nt, two_phase, nan_inf=True)
    assert np.isnan(got[1]["rm"][K // 3]) and np.isnan(got[2]["rm"][K // 3]) and np.isposinf(got[1]["rm"][2 * K // 3])
    assert np.isnan(got[1]["prob"]).any() and np.isnan(got[1]["reward"]).any() and not np.isnan(got[0]["prob"]).any()


def test_cat_step_rejects_tiles_wider_than_its_lds(nat):
    def call(K):
        N = 33
        z = torch.zeros(N * K, device="cuda")
        nat.cat_step(z.view(N, K), (C.c_int32 * 2)(0, K), (C.c_float * 1)(0.5), 0.0, 0.95, True, torch.zeros(K, device="cuda"),
                     torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"))
    with pytest.raises(RuntimeError, match="too wide"):
        call(1129)                                      # 4 (34 K + 32) bytes > 150 KB
    with pytest.raises(RuntimeError, match="K <= 4096"):
        call(4097)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [1, 1023, 1025, 5000])
def test_cat_reset_masked_means_and_zeroed_rows(nat, used, N):
    """one 1024-thread workgroup per term: one element per thread or fewer, the second pass of one element, five passes"""
    nt = 3
    rs = np.random.RandomState(N)
    viol0 = rs.randint(0, 50, (nt, N)).astype(F32)
    eprob0 = rs.uniform(0, 20, (nt, N)).astype(F32)
    L = rs.randint(1, 500, N).astype(np.int64)
    prev = rs.uniform(0, 1, 2 * nt).astype(F32)
    partial = (rs.rand(N) < 0.3) if N > 1 else np.array([True])
    for mode, mask in (("absent", None), ("all-false with prev", np.zeros(N, bool)), ("partial", partial)):
        runs = []
        for ctx in (nat, used):
            viol, eprob, out = Guarded(nt * N, value=viol0), Guarded(nt * N, value=eprob0), Guarded(2 * nt)
            ctx.cat_reset(viol.view.view(nt, N), eprob.view.view(nt, N), dev(L), None if mask is None else dev(mask), out.view,
                          prev=dev(prev))
            torch.cuda.synchronize()
            runs.append({"viol": [viol.raw()], "eprob": [eprob.raw()], "out": [out.raw()]})
        _assert_runs_identical(*runs)
        raw = runs[0]
        sel = np.ones(N, bool) if mask is None else mask
        got = out.of(raw["out"][0])
        tag = f"cat_reset N={N} mask {mode}"
        if sel.any():
            Ld = L[sel].astype(np.float64)
            want = np.stack([(viol0[:, sel] / Ld).mean(1) * 100, (eprob0[:, sel] / Ld).mean(1)], 1).ravel()
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=0, err_msg=tag)
            _note_ratio("cat_reset", tag, R.bar_ratio(got, want, 1e-5, 0.0))
        else:
            assert not R.bits_report(tag + ": log values kept", got, prev)
        msgs = R.bits_report(tag + ": violation sums", viol.of(raw["viol"][0]).reshape(nt, N), np.where(sel, F32(0), viol0),
                             col_block=1024)
        msgs += R.bits_report(tag + ": probability sums", eprob.of(raw["eprob"][0]).reshape(nt, N), np.where(sel, F32(0), eprob0),
                              col_block=1024)
        for k, g in (("viol", viol), ("eprob", eprob), ("out", out)):
            msgs += g.guard_msgs(f"{tag}: {k}", raw[k][0])
        assert not msgs, "\n".join(msgs)


# ====================================================================================================== clip + Adam
_OPT_KEYS = ("params", "grad", "exp_avg", "exp_avg_sq")


@functools.lru_cache(maxsize=2)
def _opt_ref(n):
    return R.opt_trajectory64(*R.opt_case(n))


def _run_opt(ctx, n, offs, on_device):
    """three steps (clipped, unclipped, zero gradient) of catppo_clip_adam or catppo_clip_adam_dev on slices whose bases sit
    offs[k] floats past 16-byte alignment -> raw buffers after every step"""
    from cat_envs import native
    p0, grads = R.opt_case(n)
    a = R.ADAM
    g = {k: Guarded(n, lead=4 + o) for k, o in zip(_OPT_KEYS, offs)}
    for k, o in zip(_OPT_KEYS, offs):
        assert g[k].view.data_ptr() % 16 == 4 * o
    g["params"].set(p0)
    g["exp_avg"].set(np.zeros(n))
    g["exp_avg_sq"].set(np.zeros(n))
    if on_device:
        st = ctx.iter_state_new(1, a["lr"])
        ctx.iter_begin(st, a["lr"], 10, native.LR_FIXED)
    run = {k: [] for k in _OPT_KEYS}
    for step, grad in enumerate(grads, 1):
        g["grad"].set(grad)
        v = [g[k].view for k in _OPT_KEYS]
        if on_device:
            ctx.clip_adam_dev(*v, n, a["max_norm"], a["beta1"], a["beta2"], a["eps"], st)
        else:
            ctx.clip_adam(*v, n, a["max_norm"], a["lr"], a["beta1"], a["beta2"], a["eps"], step)
        torch.cuda.synchronize()
        for k in _OPT_KEYS:
            run[k].append(g[k].raw())
    return run, g


_MIXED = (1, 0, 0, 0)            # params one float past alignment, grad aligned: float4 norm, scalar update


@pytest.mark.parametrize("offs", [(0,) * 4, (1,) * 4, (2,) * 4, (3,) * 4], ids=["off0", "off1", "off2", "off3"])
@pytest.mark.parametrize("n", R.OPT_SIZES)
def test_clip_adam_sizes_and_alignments(nat, used, n, offs):
    _check_opt(nat, used, n, offs)


@pytest.mark.parametrize("n", [1027, 263169])
def test_clip_adam_norm_and_update_on_different_paths(nat, used, n):
    _check_opt(nat, used, n, _MIXED)


def _check_opt(nat, used, n, offs):
    ref = _opt_ref(n)
    host, g = _run_opt(nat, n, offs, False)
    msgs, worst = [], 0.0
    for step in range(3):
        got = {k: g[k].of(host[k][step]) for k in _OPT_KEYS}
        msgs += R.opt_report(f"n={n} offsets {offs} step {step + 1} ({R.OPT_STEPS[step]})", got, ref[step])
        worst = max(worst, R.opt_ratio(got, ref[step]))
        for k in _OPT_KEYS:
            msgs += g[k].guard_msgs(f"n={n} offsets {offs} step {step + 1}: {k}", host[k][step])
    print(f"clip_adam n={n} offsets {offs}: largest error / bar {worst:.3g}")
    _note_ratio("clip_adam", f"n={n} offsets {offs}", worst)
    assert not msgs, "\n".join(msgs[:40])
    # the first step clipped (the gradient shrank), the second did not (bit-identical to its input), the third is zero
    _, grads = R.opt_case(n)
    assert np.abs(g["grad"].of(host["grad"][0])).max() < np.abs(grads[0]).max()
    assert np.array_equal(g["grad"].of(host["grad"][1]), grads[1]) and not g["grad"].of(host["grad"][2]).any()
    # device-resident step count / learning rate: the same bits at the same learning rate
    device, _ = _run_opt(nat, n, offs, True)
    for k in _OPT_KEYS:
        for step in range(3):
            assert not R.bits_report(f"n={n} offsets {offs} step {step + 1}: {k} of clip_adam_dev vs clip_adam",
                                     device[k][step], host[k][step]), k
    _assert_runs_identical(host, _run_opt(used, n, offs, False)[0])
    _assert_runs_identical(device, _run_opt(used, n, offs, True)[0])


# ====================================================================================================== advantages
@pytest.mark.parametrize("family", R.ADV_FAMILIES)
@pytest.mark.parametrize("n", R.ADV_SIZES)
def test_adv_normalize_sizes(nat, used, n, family):
    """4096 rows per workgroup of the moments launch: one short, exact, one over; 524293 = 128 workgroups + 5 rows"""
    x = R.adv_case(n, family)
    runs = []
    for ctx in (nat, used):
        out, stats = Guarded(n), Guarded(2)
        ctx.adv_normalize(dev(x), out.view, stats.view)
        torch.cuda.synchronize()
        runs.append({"out": [out.raw()], "stats": [stats.raw()]})
    _assert_runs_identical(*runs)
    o, st = out.of(runs[0]["out"][0]), stats.of(runs[0]["stats"][0])
    m64, s64, bm, bs = R.adv_bars(x)
    assert abs(float(st[0]) - m64) <= bm, (st[0], m64, bm)
    if n == 1:
        assert np.isnan(st[1]) and np.isnan(o).all()                 # std of one sample: NaN, like torch
    else:
        assert abs(float(st[1]) - s64) <= bs, (st[1], s64, bs)
        _note_ratio("adv_normalize", f"n={n} {family}", max(abs(float(st[0]) - m64) / bm, abs(float(st[1]) - s64) / bs))
        want = ((x - st[0]).astype(F32) / st[1]).astype(F32)         # the kernel's own fp32 statistics, IEEE division
        msgs = R.bits_report(f"adv_normalize n={n} {family}", o, want, row_block=1024)
        assert not msgs, "\n".join(msgs)
    assert not out.guard_msgs("out", runs[0]["out"][0]) + stats.guard_msgs("stats", runs[0]["stats"][0])


@pytest.mark.parametrize("ppm,M", [(1, 50), (63, 4000), (64, 4096), (65, 4100), (256, 16384)])
def test_adv_moments_parts_lane_boundaries(nat, ppm, M):
    """one wave per minibatch, lane-strided over the 64-row chunk sums: fewer chunks than lanes, one short, exact, one over,
    four per lane; the last minibatch ragged"""
    total = 2 * M + M // 3 + 1
    for family in R.ADV_FAMILIES:
        x = R.adv_case(total, family, seed=1)
        parts = R.adv_chunk_parts(x, M, ppm)
        want = R.adv_moments64(x, M)
        mom = Guarded(3 * want.shape[0], torch.float64)
        nat.adv_moments_parts(dev(parts.ravel()), ppm, total, M, mom.view)
        torch.cuda.synchronize()
        raw = mom.raw()
        got = mom.of(raw).reshape(-1, 3)
        x64 = x.astype(np.float64)
        for k in range(want.shape[0]):
            s = x64[k * M:(k + 1) * M]
            bar = s.size * 2.0 ** -52 * np.array([np.abs(s).sum(), (s * s).sum()])
            assert (np.abs(got[k, :2] - want[k, :2]) <= bar).all(), (family, k, got[k], want[k], bar)
            assert got[k, 2] == want[k, 2] == s.size
        assert want[-1, 2] == M // 3 + 1 and not mom.guard_msgs("moments", raw)


@pytest.mark.parametrize("n_mb", [1, 63, 64, 65, 200])
def test_adv_stats_thread_boundaries(nat, n_mb):
    """64 threads per workgroup, one minibatch per thread"""
    for family in R.ADV_FAMILIES:
        rs = np.random.RandomState(n_mb)
        sizes = rs.randint(2, 300, n_mb)
        xs = np.split(R.adv_case(int(sizes.sum()), family, seed=2), np.cumsum(sizes)[:-1])
        mom = np.array([[x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum(), x.size] for x in xs])
        stats = Guarded(2 * n_mb)
        nat.adv_stats(dev(mom.ravel()), n_mb, stats.view)
        torch.cuda.synchronize()
        raw = stats.raw()
        got = stats.of(raw).reshape(n_mb, 2)
        worst = 0.0
        for k, x in enumerate(xs):
            m64, s64, bm, bs = R.adv_bars(x)
            assert abs(float(got[k, 0]) - m64) <= bm and abs(float(got[k, 1]) - s64) <= bs, (family, k, got[k], m64, s64, bm, bs)
            worst = max(worst, abs(float(got[k, 0]) - m64) / bm, abs(float(got[k, 1]) - s64) / bs)
        _note_ratio("adv_stats", f"n_minibatches={n_mb} {family}", worst)
        assert not stats.guard_msgs("stats", raw)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_value_bootstrap_block_boundaries(nat, n):
    rs = np.random.RandomState(n)
    rew, val = rs.uniform(0, 1.5, n).astype(F32), rs.standard_normal(n).astype(F32)
    to = rs.rand(n) < 0.4
    r = Guarded(n, value=rew)
    nat.value_bootstrap(r.view, dev(val), dev(to.astype(np.uint8)), 0.99)
    torch.cuda.synchronize()
    raw = r.raw()
    want = PO.value_bootstrap(torch.from_numpy(rew), torch.from_numpy(val), torch.from_numpy(to), 0.99).numpy()
    msgs = R.bits_report(f"value_bootstrap n={n}", r.of(raw), want, row_block=256) + r.guard_msgs("rewards", raw)
    assert not msgs, "\n".join(msgs)


# ====================================================================================================== GAE
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["cleanrl", "rl_games", "skrl"])
@pytest.mark.parametrize("N", [513, 800, 1441])
def test_gae_workgroup_counts_that_are_no_multiple_of_eight(nat, N, kind, half):
    """the serial kernel renumbers its workgroups per XCD (eight contiguous ranges of the env axis): 9, 13 and 23
    workgroups of 64 envs leave the ranges uneven"""
    T = 5
    x = S.gae_inputs(N, T, N)
    if half:
        x = {k: v.astype(np.float16) for k, v in x.items()}
    d = {k: dev(v) for k, v in x.items()}
    f = {k: v.astype(F32) for k, v in x.items()}
    dt = torch.float16 if half else torch.float32
    adv, ret = Guarded(T * N, dt), Guarded(T * N, dt)
    a, r = adv.view.view(T, N), ret.view.view(T, N)
    if half:
        nat.gae_f16(d["rewards"], d["values"], d["dones"], d["true_dones"], d["next_value"], d["next_done"],
                    d["next_true_done"], 0.99, 0.95, a, r, kind={"cleanrl": 0, "rl_games": 1, "skrl": 2}[kind])
    elif kind == "cleanrl":
        nat.gae(d["rewards"], d["values"], d["dones"], d["true_dones"], d["next_value"], d["next_done"], d["next_true_done"],
                0.99, 0.95, a, r)
    elif kind == "rl_games":
        nat.gae_rl_games(d["next_done"], d["next_value"], d["dones"], d["values"], d["rewards"], 0.99, 0.95, a, r)
    else:
        nat.gae_skrl(d["rewards"], d["dones"], d["values"], d["next_value"], 0.99, 0.95, a, r)
    torch.cuda.synchronize()
    if kind == "skrl":
        t = {k: torch.from_numpy(v) for k, v in f.items()}
        wr, _, wa = PO.gae_skrl(t["rewards"], t["dones"], t["values"], t["next_value"], 0.99, 0.95)
        wa, wr = wa.numpy(), wr.numpy()
    else:
        z = np.zeros_like(f["dones"])
        td, ntd = (f["true_dones"], f["next_true_done"]) if kind == "cleanrl" else (z, z[0])
        wa, wr = PO.gae_numpy_exact(f["rewards"], f["values"], f["dones"], td, f["next_value"], f["next_done"], ntd, 0.99, 0.95)
    np_dt = np.float16 if half else F32
    ra, rr = adv.raw(), ret.raw()
    for name, g, raw, want in (("advantages", adv, ra, wa), ("returns", ret, rr, wr)):
        got = g.of(raw).reshape(T, N)
        bad = np.argwhere(got != want.astype(np_dt))
        assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} entries differ, envs {bad[:, 1].min()}..{bad[:, 1].max()}, "
                                   f"workgroups of 64 envs {sorted(set((bad[:, 1] // 64).tolist()))}")
        assert not g.guard_msgs(name, raw)
