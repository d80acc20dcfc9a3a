"""Shared by tests/test_stat_refs.py (CPU) and tests/test_gpu_stat_kernels.py (GPU): plain float64 restatements of the
statistics kernels (csrc/rms.hip, csrc/mlp_optim.h, the advantage statistics of csrc/env_step.hip), the input families and
shapes the GPU module drives them at, and comparisons that say WHERE an error is - column and 256-column block for the
column-wise kernels, element and element % 4 for the optimiser (float4 body / scalar tail), row and row block for the row
loops.  They live apart from the tests so that the CPU module can attack them: it measures the project's fp32 references
(RMSOracle, torch Adam, torch mean / std) against the float64 ones on every family - a bar is only worth something if the
reference it is measured from sits well inside it - and shows that every comparison rejects a planted error of the kind a
wrong lane mask or an off-by-one block would produce.

The CaT step has no restatement here: oracle/cat_oracle.py already is one, bit for bit."""
import functools
import math

import numpy as np
import torch

from oracle import cat_oracle as CO
from oracle import ppo_oracle as PO

F32 = np.float32
COL_BLOCK = 256          # kThreads of rms.hip / cat_step.hip: columns per pass of the column-block loops
FINISH_ROWS = 32         # kFinishRows of cat_finish: envs per workgroup

# the project's existing bars (tests/test_gpu_kernels.py)
RMS_RTOL, RMS_ATOL = 2e-6, 1e-6                                   # test_running_mean_std_vs_reference_golden
OPT_BARS = {"params": (1e-6, 1e-6), "grad": (1e-5, 1e-9),         # test_clip_adam_vs_torch: (rtol, atol)
            "exp_avg": (1e-5, 1e-9), "exp_avg_sq": (1e-5, 1e-12)}
EPS = 1e-8               # RunningMeanStd epsilon
ADAM = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_norm=1.0)


def ulp32(x):
    """spacing of float32 at |x| (of the smallest normal below it)"""
    return float(np.spacing(F32(max(abs(float(x)), float(np.finfo(F32).tiny)))))


# ====================================================================================================== RunningMeanStd
# (D, N, ldx): what each reaches is in the table of tests/test_gpu_stat_kernels.py
RMS_SHAPES = [(1, 1, 1), (1, 98304, 1), (1, 600000, 1), (3, 1000, 4), (45, 40000, 48), (100, 777, 100), (128, 300, 128),
              (129, 300, 136), (255, 64, 256), (256, 64, 256), (257, 64, 264), (512, 40, 512), (513, 40, 520),
              (1000, 33, 1000)]
RMS_FAMILIES = ("spread", "offset")
RMS_UPDATES = 3


def moments_grid(N, D):
    """host restatement of rms.hip's moments_grid: (G, per_thread, rows_per_block, workgroups)"""
    G = 256 // min(D, 256)
    per_thread = 16
    if -(-N // (G * 16)) < 96:
        per_thread = max(1, -(-N // (G * 128)))
    rows = G * per_thread
    return G, per_thread, rows, min(128, -(-N // rows))


@functools.lru_cache(maxsize=4)
def rms_case(D, N, ldx, family, updates=RMS_UPDATES):
    """(state0, batches): state0 = non-default (mean[D], var[D], count) in fp32; batches = `updates` fp32 arrays (N, ldx)
    whose pad columns hold NaN.  'spread': randn * U(0.1, 5) + U(-2, 2) per column (the golden test's family);
    'offset': 0.01 randn + 100 (the mean dwarfs the spread: cancellation in E[x^2] - E[x]^2 and in the merge).
    The start state is near the family's own statistics, as a running normaliser's is."""
    rs = np.random.RandomState(1000 * D + N % 997 + (7 if family == "offset" else 0))
    if family == "spread":
        scale, shift = rs.uniform(0.1, 5, D), rs.uniform(-2, 2, D)
        mean0, var0 = rs.uniform(-1, 1, D), rs.uniform(0.5, 2, D)
    else:
        scale, shift = np.full(D, 0.01), np.full(D, 100.0)
        mean0, var0 = 100 + 0.01 * rs.uniform(-1, 1, D), 1e-4 * rs.uniform(0.5, 2, D)
    batches = []
    for _ in range(updates):
        x = np.full((N, ldx), np.nan, F32)
        x[:, :D] = (rs.standard_normal((N, D)) * scale + shift).astype(F32)
        batches.append(x)
    return (mean0.astype(F32), var0.astype(F32), F32(37.0)), batches


def rms_update64(mean, var, count, x):
    """two-pass batch mean / biased variance and the Chan merge (cleanrl/ppo.py:12-62), everything in float64"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    bm = x.mean(0)
    bv = ((x - bm) ** 2).mean(0)
    delta = bm - mean
    tot = count + n
    new_mean = mean + delta * n / tot
    m2 = var * count + bv * n + delta ** 2 * count * n / tot
    return new_mean, m2 / tot, tot


def rms_states64(state0, batches, D):
    """float64 states after 1, 2, ... updates from state0: list of (mean, var, count)"""
    m, v, c = (np.asarray(s, np.float64) for s in state0)
    out = []
    for x in batches:
        m, v, c = rms_update64(m, v, c, np.asarray(x[:, :D], np.float64))
        out.append((m, v, float(c)))
    return out


def rms_states_oracle32(state0, batches, D):
    """the same updates through the project's fp32 reference (oracle.ppo_oracle.RMSOracle)"""
    o = PO.RMSOracle((D,))
    o.mean, o.var = torch.from_numpy(state0[0].copy()), torch.from_numpy(state0[1].copy())
    o.count = torch.tensor(float(state0[2]))
    out = []
    for x in batches:
        o.update(torch.from_numpy(np.ascontiguousarray(x[:, :D])))
        out.append((o.mean.numpy().copy(), o.var.numpy().copy(), float(o.count)))
    return out


def moment_sums64(x):
    """column sums of x and x^2 in float64 with the bar a fixed-order fp64 summation of n fp32 values stays inside:
    every addition rounds by at most 2^-53 of a partial sum <= sum |x| (the squares of fp32 values are exact in fp64), n - 1
    additions; doubled for the reference's own summation -> n 2^-52 sum |x|"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    s1, s2 = x.sum(0), (x * x).sum(0)
    return (s1, n * 2.0 ** -52 * np.abs(x).sum(0)), (s2, n * 2.0 ** -52 * s2)


def normalize32(x, mean, var, eps=EPS):
    """(x - mean) / sqrt(var + eps) with numpy fp32 operations in that order (IEEE sqrt and division, nothing fused)"""
    x, mean, var = np.asarray(x, F32), np.asarray(mean, F32), np.asarray(var, F32)
    den = np.sqrt((var + F32(eps)).astype(F32)).astype(F32)
    return ((x - mean).astype(F32) / den).astype(F32)


# ====================================================================================================== comparisons
def bar_ratio(got, ref, rtol, atol):
    """largest |got - ref| / (atol + rtol |ref|); inf when something is not finite"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if got.size == 0:
        return 0.0
    r = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def column_report(name, got, ref, rtol, atol, limit=4):
    """per-column values (a state vector) against a reference: [] or messages that name the columns over the bar, their
    256-column block (the pass of the column-block loop that produced them) and their position inside it"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if got.shape != ref.shape:
        return [f"{name}: {got.shape[0]} columns, expected {ref.shape[0]}"]
    bar = atol + rtol * np.abs(ref)
    bad = np.nonzero(~(np.abs(got - ref) <= bar))[0]                 # (a NaN is a miss)
    if bad.size == 0:
        return []
    msgs = [f"{name}: {bad.size} of {got.size} columns over the bar (rtol {rtol:g}, atol {atol:g}); column blocks "
            f"{sorted(set((bad // COL_BLOCK).tolist()))}"]
    for c in bad[:limit]:
        msgs.append(f"  column {c} (block {c // COL_BLOCK}, lane {c % COL_BLOCK}): got {got[c]!r}, reference {ref[c]!r}, "
                    f"error / bar {abs(got[c] - ref[c]) / bar[c]:.3g}")
    return msgs


def element_report(name, got, ref, rtol, atol, limit=4):
    """a flat optimiser array against a reference: [] or messages that name the elements over the bar, element % 4 (the
    float4 body handles whole groups of four, the scalar tail the last n % 4) and whether all of them sit in the tail"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    if got.shape != ref.shape:
        return [f"{name}: {got.shape[0]} elements, expected {ref.shape[0]}"]
    n = got.size
    bar = atol + rtol * np.abs(ref)
    bad = np.nonzero(~(np.abs(got - ref) <= bar))[0]
    if bad.size == 0:
        return []
    by_mod = np.bincount(bad % 4, minlength=4).tolist()
    tail = n - n % 4
    where = "all in the n % 4 tail" if bad.min() >= tail else ("all in the float4 body" if bad.max() < tail else "body and tail")
    msgs = [f"{name}: {bad.size} of {n} elements over the bar (rtol {rtol:g}, atol {atol:g}), {where}; "
            f"by index % 4: {by_mod}; first {bad.min()}, last {bad.max()}"]
    for e in bad[:limit]:
        msgs.append(f"  element {e} (index % 4 = {e % 4}, 1024-element block {e // 1024}): got {got[e]!r}, reference {ref[e]!r}, "
                    f"error / bar {abs(got[e] - ref[e]) / bar[e]:.3g}")
    return msgs


def _same_bits(got, ref):
    """elementwise: the same fp32 bit pattern, or both NaN (payload and sign of a NaN differ between host and device)"""
    g, r = np.ascontiguousarray(got, F32), np.ascontiguousarray(ref, F32)
    return (g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))


def bits_report(name, got, ref, row_block=None, col_block=None, limit=4):
    """bit equality (NaN == NaN) of a vector or a row-major matrix: [] or messages that name the first differing entries with
    row / row block (`row_block` rows per workgroup or pass) and column / column block"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return [f"{name}: shape {got.shape}, expected {ref.shape}"]
    bad = np.argwhere(~_same_bits(got, ref))
    if bad.shape[0] == 0:
        return []
    msgs = [f"{name}: {bad.shape[0]} of {got.size} entries not bit-equal"]
    if got.ndim == 2 or row_block:
        rows = bad[:, 0]
        msgs[0] += f"; rows {rows.min()}..{rows.max()}" + (f", row blocks {sorted(set((rows // row_block).tolist()))[:8]}"
                                                          if row_block else "")
    if got.ndim == 2 or (col_block and not row_block):
        cols = bad[:, -1]
        msgs[0] += f"; columns {cols.min()}..{cols.max()}" + (f", column blocks {sorted(set((cols // col_block).tolist()))[:8]}"
                                                             if col_block else "")
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        msgs.append(f"  {idx}: got {got[idx]!r}, reference {ref[idx]!r}")
    return msgs


def guard_report(name, buf, sentinel_bits, lo, hi):
    """everything of the flat buffer outside [lo, hi) still holds the sentinel's bit pattern"""
    b = np.ascontiguousarray(buf).ravel()
    b = b.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[b.dtype.itemsize])
    keep = np.ones(b.size, bool)
    keep[lo:hi] = False
    bad = np.nonzero(keep & (b != sentinel_bits))[0]
    if bad.size == 0:
        return []
    return [f"{name}: {bad.size} guard elements overwritten, flat offsets {bad[:6].tolist()} relative to the result "
            f"[{lo}, {hi})"]


# ====================================================================================================== clip + Adam
OPT_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 262144, 263169, 1048579)
OPT_STEPS = ("clipped", "unclipped", "zero")


@functools.lru_cache(maxsize=2)
def opt_case(n):
    """parameters ~ N(0, 1) and three gradients: norm about 10 (clipped to max_norm 1), norm about 0.01 (left alone), all
    zero.  Gradient elements are signed integers 1..4 times a power of two: their squares and every partial sum of them
    (< 2^24 units) are exact in fp32, so the squared norm is the same in ANY summation order and precision.  With normal
    draws torch's fp32 norm over 10^6 elements is itself off by 1.4e-5 (1.4 bars of the gradient: measured in
    tests/test_stat_refs.py's history, docs/HISTORY.md) and the bar could not tell a kernel from its reference."""
    rs = np.random.RandomState(50 + n % 1009)
    p0 = rs.standard_normal(n).astype(F32)
    grads = []
    for norm in (10.0, 0.01):
        k = rs.randint(1, 5, n) * rs.choice([-1, 1], n)
        grads.append((k * 2.0 ** round(math.log2(norm / math.sqrt(7.5 * n)))).astype(F32))
    grads.append(np.zeros(n, F32))
    return p0, grads


def clip_adam64(p, g, m, v, step, norm_over=None, lr=ADAM["lr"], beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"],
                max_norm=ADAM["max_norm"]):
    """clip_grad_norm_ + Adam in float64 -> (p, g, m, v): norm over the whole slice, coef = min(1, max_norm / (norm + 1e-6)),
    then torch's order as adam_elem documents it: exp_avg.lerp_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2);
    param.addcdiv_(exp_avg, sqrt(exp_avg_sq) / sqrt(bc2) + eps, -lr / bc1).  `norm_over`: elements the norm is taken over
    (None: all; the planted errors pass a short slice)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gn = g if norm_over is None else g[norm_over]
    norm = math.sqrt(float((gn * gn).sum()))
    g = g * min(1.0, max_norm / (norm + 1e-6))
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p + (-(lr / bc1) * m) / denom, g, m, v


def opt_trajectory64(p0, grads):
    """[{params, grad, exp_avg, exp_avg_sq} after step 1, 2, ...] from zero moments, float64 throughout"""
    p, m, v = np.asarray(p0, np.float64), np.zeros(p0.shape[0]), np.zeros(p0.shape[0])
    out = []
    for k, g in enumerate(grads):
        p, gc, m, v = clip_adam64(p, g, m, v, k + 1)
        out.append({"params": p, "grad": gc, "exp_avg": m, "exp_avg_sq": v})
    return out


def opt_trajectory_torch(p0, grads):
    """the same steps through torch.optim.Adam + clip_grad_norm_ on the CPU in fp32 (the project's fp32 reference)"""
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"])
    out = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        torch.nn.utils.clip_grad_norm_([p], ADAM["max_norm"])
        opt.step()
        st = opt.state[p]
        out.append({"params": p.detach().numpy().copy(), "grad": p.grad.numpy().copy(),
                    "exp_avg": st["exp_avg"].numpy().copy(), "exp_avg_sq": st["exp_avg_sq"].numpy().copy()})
    return out


def opt_report(name, got, ref):
    """{params, grad, exp_avg, exp_avg_sq} against a reference at OPT_BARS: messages of element_report"""
    msgs = []
    for k, (rtol, atol) in OPT_BARS.items():
        msgs += element_report(f"{name} {k}", got[k], ref[k], rtol, atol)
    return msgs


def opt_ratio(got, ref):
    return max(bar_ratio(got[k], ref[k], *OPT_BARS[k]) for k in OPT_BARS)


# ====================================================================================================== advantages
ADV_SIZES = (1, 2, 4095, 4096, 4097, 524293)
ADV_FAMILIES = ("centred", "offset")


@functools.lru_cache(maxsize=4)
def adv_case(n, family, seed=0):
    """'centred': 2 randn + 0.3 (what GAE hands over); 'offset': 0.01 randn + 50"""
    rs = np.random.RandomState(900 + n % 1013 + 31 * seed + (5 if family == "offset" else 0))
    z = rs.standard_normal(n)
    return ((2 * z + 0.3) if family == "centred" else (0.01 * z + 50)).astype(F32)


def adv_stats64(x):
    """two-pass mean and unbiased std + 1e-8 in float64 (NaN std for one sample, like torch)"""
    x = np.asarray(x, np.float64)
    n = x.size
    mean = float(x.mean())
    std = math.sqrt(float(((x - mean) ** 2).sum()) / (n - 1)) if n > 1 else float("nan")
    return mean, std + 1e-8


def adv_stats_torch32(x):
    """torch's fp32 mean() / std() + 1e-8 on the CPU (skrl/ppo.py:436, cleanrl/ppo.py:316-318)"""
    t = torch.from_numpy(np.ascontiguousarray(x, F32))
    return float(t.mean()), float(t.std() + 1e-8) if t.numel() > 1 else float("nan")


def adv_bars(x):
    """(mean64, std64, bar_mean, bar_std): allowed error = 4 x the error of torch's fp32 statistics on the same data, floor
    2 ulp of the value"""
    m64, s64 = adv_stats64(x)
    m32, s32 = adv_stats_torch32(x)
    bm = max(4 * abs(m32 - m64), 2 * ulp32(m64))
    bs = max(4 * abs(s32 - s64), 2 * ulp32(s64)) if np.isfinite(s64) else float("nan")
    return m64, s64, bm, bs


def adv_moments64(x, minibatch):
    """{sum, sum of squares, count} per minibatch of `minibatch` rows (the last one ragged), float64: (n_mb, 3)"""
    x = np.asarray(x, np.float64)
    n_mb = -(-x.size // minibatch)
    out = np.zeros((n_mb, 3))
    for k in range(n_mb):
        s = x[k * minibatch:(k + 1) * minibatch]
        out[k] = s.sum(), (s * s).sum(), s.size
    return out


def adv_chunk_parts(x, minibatch, parts_per_mb):
    """the 64-row chunk sums the epoch gather writes: (n_mb, parts_per_mb, 2) float64, zero where a chunk has no rows"""
    x = np.asarray(x, np.float64)
    n_mb = -(-x.size // minibatch)
    parts = np.zeros((n_mb, parts_per_mb, 2))
    for k in range(n_mb):
        s = x[k * minibatch:(k + 1) * minibatch]
        for c in range(-(-s.size // 64)):
            ch = s[64 * c:64 * c + 64]
            parts[k, c] = ch.sum(), (ch * ch).sum()
    return parts


# ====================================================================================================== CaT inputs
# (K, N, n_terms): what each reaches is in the table of tests/test_gpu_stat_kernels.py
CAT_CASES = [(1, 1, 1), (1, 300000, 1), (3, 31, 2), (3, 33, 2), (100, 1000, 7), (128, 33, 5), (129, 33, 5), (255, 33, 64),
             (256, 33, 64), (257, 33, 64), (64, 1000, 64), (480, 33, 1), (512, 33, 1), (1128, 33, 1)]
CAT_TAU, CAT_MIN_P, CAT_STEPS = 0.95, 0.02, 3


def uneven_widths(K, n_terms, rs):
    """n_terms positive widths that sum to K, uneven whenever K > n_terms"""
    cuts = np.sort(rs.choice(np.arange(1, K), n_terms - 1, replace=False)) if n_terms > 1 else np.array([], int)
    return np.diff(np.concatenate([[0], cuts, [K]])).astype(int).tolist()


@functools.lru_cache(maxsize=2)
def cat_case(K, N, n_terms, nan_inf=False):
    """widths, max_p per term and CAT_STEPS steps of {cstr (N, K) fp32, reward, reset}.  About a quarter of the entries
    violate; every 7th column never does (its maximum is floored at 1e-6); the LAST row holds the maximum of column K - 1
    and the FIRST row that of column 0 at every step, so a column maximum that skips either row is wrong.  nan_inf: one NaN
    and one +Inf in different columns of step 1 (torch.max propagates the NaN into the running maximum of its column)."""
    rs = np.random.RandomState(7000 + 13 * K + N % 1019 + n_terms)
    widths = [1, 2] if (K, n_terms) == (3, 2) else ([1] * K if n_terms == K else uneven_widths(K, n_terms, rs))
    max_p = rs.uniform(0.05, 1.0, n_terms).tolist()
    scale, shift = rs.uniform(0.2, 3.0, K), rs.uniform(-2.5, -0.2, K)
    steps = []
    for t in range(CAT_STEPS):
        c = (rs.standard_normal((N, K)) * scale + shift * scale).astype(F32)
        if K >= 7:
            c[:, 6::7] = -np.abs(c[:, 6::7]) - F32(0.5)
        top = np.abs(c).max(0) + F32(1.0)
        c[-1, K - 1] = top[K - 1]
        if N > 1:
            c[0, 0] = top[0]
        if nan_inf and t == 1:
            c[N // 2, K // 3] = np.nan
            c[N // 3, 2 * K // 3] = np.inf
        steps.append({"cstr": c, "reward": rs.uniform(-0.2, 1.5, N).astype(F32), "reset": rs.rand(N) < 0.1})
    return widths, max_p, steps


def cat_oracle_run(K, N, widths, max_p, steps):
    """ConstraintManagerOracle + env_finish over the steps -> per step {rm, prob, probs, reward, dones}, final (viol, eprob)"""
    names = [f"t{i}" for i in range(len(widths))]
    off = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    orc = CO.ConstraintManagerOracle(names, N, tau=CAT_TAU, min_p=CAT_MIN_P)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in steps:
            vals = {nm: s["cstr"][:, off[i]:off[i + 1]] for i, nm in enumerate(names)}
            prob = orc.compute(vals, dict(zip(names, max_p)))
            reward, dones = CO.env_finish(s["reward"], prob, s["reset"])
            out.append({"rm": orc.cat.get_running_maxes()[0].copy(), "prob": prob.copy(),
                        "probs": np.concatenate([orc.cat.probs[nm] for nm in names], 1), "reward": reward, "dones": dones})
    viol = np.stack([orc.episode_sums[nm] for nm in names])
    eprob = np.stack([orc.cstr_mean_values[nm] for nm in names])
    return out, viol, eprob


def cat_report(tag, got_steps, got_viol, got_eprob, ref_steps, ref_viol, ref_eprob):
    """everything a CaT step writes, bit for bit against the oracle"""
    msgs = []
    for t, (g, r) in enumerate(zip(got_steps, ref_steps)):
        msgs += bits_report(f"{tag} step {t} running maxima", g["rm"], r["rm"], col_block=COL_BLOCK)
        msgs += bits_report(f"{tag} step {t} probs", g["probs"], r["probs"], row_block=FINISH_ROWS, col_block=COL_BLOCK)
        for k in ("prob", "reward", "dones"):
            msgs += bits_report(f"{tag} step {t} {k}", g[k], r[k], row_block=FINISH_ROWS)
    msgs += bits_report(f"{tag} episode violation sums", got_viol, ref_viol, col_block=FINISH_ROWS)
    msgs += bits_report(f"{tag} episode probability sums", got_eprob, ref_eprob, col_block=FINISH_ROWS)
    return msgs
