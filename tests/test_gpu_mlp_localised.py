"""MLP kernel tests that LOCALISE an error (csrc/mlp*.h, gemm_f32.h, step16.h, fwd_rows*.h, mlp_wide.h): one row, one
64-row tile, one parameter tensor - what the whole-output bars of the other modules average away.

  bf16 forward, row by row      every row against the float64-accumulating oracle of the bf16 mode: clean (fp32 bars) or
                                flipped (one bf16 rounding fell the other way: the bf16 bar), with caps on the flipped share
                                of all rows and of every 64-row block, the ragged last one included;
  bf16 gradient, per tensor     every weight, bias and the log-std against the float64-accumulating oracle that restates
                                what the plan chose (bf16-stored or rounded at use), bars from the references alone;
  row placement                 the same rows rotated by 37 positions - interior rows land in the ragged tile and the
                                other way round: forward bit-identical, gradient equal up to the fp32 row-sum order;
  used workspace                the same call after one with twice the rows and NaN observations (rows past M of the
                                activations, dZ, the bf16 copies and the split-K partials then hold NaN): bit-identical
                                to the call in a fresh context.

Everything runs in-process at the default switches; every case first asserts from catppo_plan_log that the launch form it
names is the one that ran.  The comparisons live in tests/localised_checks.py; tests/test_oracle_bf16.py shows on the CPU
that each rejects a seeded error (mutations tried there: the last row's gradient contribution dropped, one bias gradient
zeroed, 20 rows of the ragged block off by the size of one flip, the last row's outputs zeroed)."""
import functools

import numpy as np
import pytest
import torch

import localised_checks as LC
import streams as S
from test_gpu_kernels import dev, flat_params, unflatten_grad

pytestmark = pytest.mark.gpu

REF, C256, N128_512, DEEP = (512, 256, 128), (256, 256, 256), (128, 512), (64, 128, 64, 128)
LAYERS = "layer-wise GEMM launches"
HEAD_LOSS = "layer-wise forward GEMM launches + head_loss_kernel"


@pytest.fixture(scope="module")
def nat():
    from cat_envs import native
    return native.Native()


def _tag(D, A, hidden, rows, prec=None):
    return f"{D}_{A}_{'x'.join(map(str, hidden))}_{rows}" + ("" if prec is None else f"_prec{prec}")


def _assert_plan(plan, want, absent=()):
    for s in want:
        assert s in plan, (s, plan)
    for s in absent:
        assert s not in plan, (s, plan)


@functools.lru_cache(maxsize=None)
def _net(D, A, hidden, prec, seed):
    from cat_envs import native
    shape = native.shape_of(D, A, hidden, mfma_bf16=prec)
    lay = native.layout_of(shape)
    w = S.agent_weights(seed, D, A, hidden)
    return shape, lay, w, flat_params(native, shape, lay, w)


def _padded(x, lay):
    xp = np.zeros((x.shape[0], lay.obs_pad), np.float32)
    xp[:, :x.shape[1]] = x
    return xp


# ---------------------------------------------------------------------------------------------- device calls
def _forward(nat, shape, lay, params, x, eps=None, given=None, critic_only=False):
    """one catppo_policy_step: sampled from supplied eps | given actions | critic only -> {action, logprob, value}"""
    N, A = x.shape[0], shape.act_dim
    fill = float("nan")                                  # an output row the call does not write stays NaN
    act, logp, val = (torch.full(s, fill, device="cuda") for s in ((N, A), (N,), (N,)))
    xp = dev(_padded(x, lay))
    if critic_only:
        nat.value(shape, params, xp, N, val)
    else:
        nat.policy_act(shape, params, xp, N, None if eps is None else dev(eps), act, logp, val,
                       given_action=None if given is None else dev(given))
    torch.cuda.synchronize()
    if critic_only:
        return {"value": val.cpu().numpy()}
    return {"action": act.cpu().numpy(), "logprob": logp.cpu().numpy(), "value": val.cpu().numpy()}


def _grad(nat, shape, lay, c, inds, obs=None, fill=7.0):
    """one catppo_ppo_minibatch_grad with norm_adv and clip_vloss on -> (flat grad, diag)"""
    from cat_envs import native
    params = c["params"]
    M = inds.shape[0]
    grad = torch.full((lay.n_flat,), fill, device="cuda")
    diag = torch.zeros(8, device="cuda")
    hp = native.PpoHparams(0.2, 0.001, 2.0, 1, 1, 1.0 / M, 0)
    nat.ppo_minibatch_grad(shape, hp, params, c["obs_dev"] if obs is None else obs, c["act_dev"], c["logp_dev"], c["adv_dev"],
                           c["ret_dev"], c["val_dev"], dev(inds), c["vmean_dev"], c["vvar_dev"], None, grad, diag)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), diag.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _grad_data(D, A, hidden, Bsz, M, prec, stored=False):
    """the minibatch of test_ppo_minibatch_grad_vs_autograd_oracle (old log-probs = new + 0.25 N(0,1), new ones from the
    reference the case is compared with) and its device copies; computed once per case, never written"""
    shape, lay, w, params = _net(D, A, hidden, prec, 5)
    opts = dict(bf16_hidden=True, accumulate=torch.float64, bf16_stored=stored) if prec == 1 else {}
    c = LC.minibatch_data(D, A, hidden, Bsz, M, w, **opts)
    c["params"] = params
    c["obs_dev"] = dev(_padded(c["obs"], lay))
    for k in ("act", "logp", "adv", "ret", "val"):
        c[k + "_dev"] = dev(c[k])
    c["vmean_dev"], c["vvar_dev"] = dev(np.array([c["vmean"]])), dev(np.array([c["vvar"]]))
    return c


def _named(shape, lay, w, flat):
    g = unflatten_grad(shape, lay, flat, w)
    return {k: g[k].reshape(w[k].shape) for k in w}


# ---------------------------------------------------------------------------------------------- 2. bf16 forward, row by row
@pytest.mark.parametrize("D,A,hidden,N,want,absent", [
    (48, 12, C256, 4133, ("bf16-stored activations",), ()),
    (45, 12, REF, 4133, ("bf16-stored activations",), ()),
    (235, 12, C256, 4133, ("bf16-stored activations",), ()),
    (45, 12, REF, 300, (LAYERS, "operand precision 1"), ("bf16-stored",)),      # fp32-stored, 44-row last tile
    (33, 15, DEEP, 300, (LAYERS, "operand precision 1"), ("bf16-stored",)),
    (48, 7, (64,), 100, (LAYERS, "operand precision 1"), ("bf16-stored",)),
])
def test_bf16_forward_row_by_row(nat, D, A, hidden, N, want, absent):
    """catppo_policy_step, mfma_bf16 = 1, supplied eps, against the float64-accumulating oracle of the mode.  Conditions: a
    row is clean at the fp32 bars of test_policy_act_vs_oracle_and_golden or flipped and within the bf16 bar 5e-3; at
    most 5 % of the rows and at most 25 % of the rows of any 64-row block (the ragged last one included) are flipped.
    The float32-accumulating oracle against the same reference flips 1.6-1.9 % of the rows and at most 5 of a block's 64
    (tests/test_oracle_bf16.py holds it under half the caps); a tile that took another path flips all of its rows.
    Measured on an MI355X, in case order: 1.40 / 2.03 / 1.62 / 3.00 / 0.67 / 0 % of the rows, worst block 7.8 %."""
    import parity_record
    shape, lay, w, params = _net(D, A, hidden, 1, 3)
    rs = np.random.RandomState(4)
    x = rs.standard_normal((N, D)).astype(np.float32)
    eps = rs.standard_normal((N, A)).astype(np.float32)
    nat.mlp_reserve(shape, N)
    nat.plan_log(1)
    got = _forward(nat, shape, lay, params, x, eps)
    _assert_plan(nat.plan_log(0), want, absent)
    ref = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=torch.float64)
    rep, bad = LC.row_report(got, ref)
    print(rep)
    parity_record.record("bf16_rows_" + _tag(D, A, hidden, N), rep, sizes=dict(D=D, A=A, hidden=list(hidden), N=N), seed=4)
    assert not bad, (bad, rep)


# ---------------------------------------------------------------------------------------------- 3. bf16 gradient, tensor by tensor
@pytest.mark.parametrize("D,A,hidden,Bsz,M,stored,want", [
    (48, 12, C256, 8192, 4133, True, ("bf16-stored activations", "fwd0_w16_kernel", "fwd_head_kernel<256, prec 3")),    # 37-row last tile
    (45, 12, REF, 8192, 4133, True, ("bf16-stored activations", "fwd_head_kernel<128, prec 3")),        # 128-wide head tile
    (235, 12, C256, 8192, 4133, True, ("bf16-stored activations", "fwd_head_kernel<256, prec 3")),      # fp32 observations in dW_0 (PREC 5)
    (48, 3, (256, 128), 8192, 4133, True, ("bf16-stored activations", "+ 0 layer-wise")),               # one layer below the head
    (45, 12, REF, 2048, 1000, False, (HEAD_LOSS,)),                                     # rounded at use
    (33, 15, DEEP, 1024, 300, False, (HEAD_LOSS,)),
])
def test_bf16_gradient_tensor_by_tensor(nat, D, A, hidden, Bsz, M, stored, want):
    """catppo_ppo_minibatch_grad, mfma_bf16 = 1, norm_adv and clip_vloss on.  For every parameter tensor k:
    err_k = max |device - ref64| / max |ref64| against the float64-accumulating oracle with bf16_stored as the plan chose,
    noise_k the same between the float32- and the float64-accumulating oracle, and
    bar_k = max(2e-4, 4 noise_k, largest noise among the tensors of the same network and kind) - from the references
    alone (LC.tensor_bars has the reasons).  diag[:4] at the existing rtol 2e-3 / atol 2e-4.  err, noise and bar go to the
    parity record ("bf16_per_tensor_<shape>").  Measured on an MI355X, largest err_k / bar_k in case order: 0.59, 0.50,
    0.45, 0.99 (actor_mean.0.bias at 256/128: 6.3e-4 = 4.0 noise_k, flips of mu; docs/HISTORY.md 0c), 0.25, 0.32."""
    import parity_record
    shape, lay, w, params = _net(D, A, hidden, 1, 5)
    c = _grad_data(D, A, hidden, Bsz, M, 1, stored)
    nat.mlp_reserve(shape, M)
    nat.plan_log(1)
    flat, diag = _grad(nat, shape, lay, c, c["inds"])
    plan = nat.plan_log(0)
    _assert_plan(plan, want, () if stored else ("bf16-stored",))
    assert np.isfinite(flat).all() and diag[7] == 1.0
    opts = dict(bf16_hidden=True, bf16_stored=stored)
    g64, st = LC.oracle_grad(D, A, hidden, w, c, accumulate=torch.float64, **opts)
    g32, _ = LC.oracle_grad(D, A, hidden, w, c, **opts)
    noise, bars = LC.tensor_bars(g32, g64)
    err, bad = LC.tensors_over_bar(_named(shape, lay, w, flat), g64, bars)
    worst = max(err, key=lambda k: err[k] / bars[k])
    rec = {"worst_tensor": worst, "worst_err_over_bar": err[worst] / bars[worst]}
    for k in err:
        rec[k] = [err[k], noise[k], bars[k]]
    parity_record.record("bf16_per_tensor_" + _tag(D, A, hidden, M), rec, sizes=dict(D=D, A=A, hidden=list(hidden), M=M), seed=6,
                         note="per tensor: [err_k, noise_k, bar_k]")
    print({k: rec[k] for k in ("worst_tensor", "worst_err_over_bar")})
    assert not bad, bad
    np.testing.assert_allclose(diag[:4], [float(st["pg_loss"]), float(st["v_loss"]), float(st["entropy"]), float(st["loss"])],
                               rtol=2e-3, atol=2e-4)


# ---------------------------------------------------------------------------------------------- 4 / 5. cases of both
FWD_CASES = [      # hidden, D, A, N, operand precision, plan
    pytest.param(REF, 45, 12, 300, 0, ("step16_fwd_kernel",), id="ref_300_step16_fwd"),
    pytest.param(C256, 48, 12, 2085, 0, ("rows_fwd_kernel<32>",), id="3x256_2085_rows_fwd32"),
    pytest.param(REF, 45, 12, 2085, 0, ("rows_fwd_wide_kernel<32>",), id="ref_2085_rows_fwd_wide32"),
    pytest.param(N128_512, 45, 12, 2085, 0, ("fused_fwd_kernel",), id="128x512_2085_fused_fwd"),
    pytest.param(N128_512, 45, 12, 300, 0, (LAYERS, "head_act_kernel"), id="128x512_300_layers_head_act"),
    pytest.param(REF, 45, 19, 300, 0, ("head_act_wide_kernel",), id="ref_A19_300_head_act_wide"),
    pytest.param(C256, 48, 12, 4133, 1, ("bf16-stored activations",), id="3x256_bf16_4133_stored"),
    pytest.param(REF, 45, 12, 300, 1, (LAYERS, "operand precision 1"), id="ref_bf16_300"),
]
GRAD_CASES = [     # hidden, D, A, M, operand precision, plan
    pytest.param(REF, 45, 12, 300, 0, ("step16_kernel",), id="ref_300_step16"),
    pytest.param(C256, 48, 12, 4133, 0, (LAYERS, "fwd_head_kernel<256, prec 0"), id="3x256_4133_layers_fwd_head"),
    pytest.param(C256, 48, 12, 8229, 0, ("rows_fwd_kernel<64>",), id="3x256_8229_rows_fwd64"),
    pytest.param(REF, 45, 12, 8229, 0, ("rows_fwd_wide_kernel<64>",), id="ref_8229_rows_fwd_wide64"),
    pytest.param(N128_512, 45, 12, 1000, 0, (HEAD_LOSS,), id="128x512_1000_head_loss"),
    pytest.param(REF, 45, 19, 1000, 0, ("head_loss_wide_kernel",), id="ref_A19_1000_head_loss_wide"),
    pytest.param(C256, 48, 12, 4133, 1, ("bf16-stored activations", "prec 3"), id="3x256_bf16_4133_act16"),
    pytest.param(REF, 45, 12, 1000, 1, (HEAD_LOSS,), id="ref_bf16_1000"),
    pytest.param(C256, 48, 12, 4133, 2, (LAYERS, "fwd_head_kernel<256, prec 2"), id="3x256_bf16x3_4133"),
]


def _fwd_inputs(D, A, N):
    rs = np.random.RandomState(4)
    return rs.standard_normal((N, D)).astype(np.float32), rs.standard_normal((N, A)).astype(np.float32)


def _three_forwards(nat, shape, lay, params, x, eps, before=None, given=None):
    """the sampled call, the critic-only call and the given-action call (on `given`, by default the sampled call's
    actions); `before` runs in front of each"""
    out = {}
    actions = given
    for mode in ("sample", "critic", "given"):
        if before is not None:
            before(mode)
        if mode == "sample":
            r = _forward(nat, shape, lay, params, x, eps)
            actions = r["action"] if given is None else given
        elif mode == "critic":
            r = _forward(nat, shape, lay, params, x, critic_only=True)
        else:
            r = _forward(nat, shape, lay, params, x, given=actions)
        out.update({f"{mode}_{k}": v for k, v in r.items()})
    return out


# ---------------------------------------------------------------------------------------------- 4. row placement
@pytest.mark.parametrize("hidden,D,A,N,prec,want", FWD_CASES)
def test_forward_does_not_depend_on_the_row_position(nat, hidden, D, A, N, prec, want):
    """The same rows (observations, eps, given actions) rotated by 37 positions, un-rotated afterwards: BIT-identical
    outputs - within one kernel a row's contraction order does not depend on the tile it sits in, ragged or not."""
    shape, lay, w, params = _net(D, A, hidden, prec, 3)
    x, eps = _fwd_inputs(D, A, N)
    nat.mlp_reserve(shape, N)
    nat.plan_log(1)
    out = _three_forwards(nat, shape, lay, params, x, eps)
    _assert_plan(nat.plan_log(0), want)
    assert all(np.isfinite(v).all() for v in out.values())
    np.testing.assert_array_equal(out["critic_value"], out["sample_value"])
    # (the given-action call of the rotated batch gets the rotated actions of the PLAIN call: the same rows)
    out_r = _three_forwards(nat, shape, lay, params, LC.rot(x), LC.rot(eps), given=LC.rot(out["sample_action"]))
    assert LC.forward_rotation_mismatch(out, out_r) == []


@pytest.mark.parametrize("hidden,D,A,M,prec,want", GRAD_CASES)
def test_gradient_does_not_depend_on_the_row_position(nat, hidden, D, A, M, prec, want):
    """mb_inds rotated by 37 positions: per-row values are identical (bf16 modes too), only the fp32 summation order over the
    rows changes - every tensor within 2e-4 of its maximum, diag[:7] within rtol 2e-4."""
    shape, lay, w, params = _net(D, A, hidden, prec, 5)
    c = _grad_data(D, A, hidden, 2 * M, M, prec, False)
    nat.mlp_reserve(shape, M)
    nat.plan_log(1)
    flat, diag = _grad(nat, shape, lay, c, c["inds"])
    _assert_plan(nat.plan_log(0), want)
    flat_r, diag_r = _grad(nat, shape, lay, c, LC.rot(c["inds"]))
    assert np.isfinite(flat).all() and np.isfinite(flat_r).all() and np.abs(flat).max() > 0
    bad = LC.grad_rotation_mismatch(_named(shape, lay, w, flat), _named(shape, lay, w, flat_r), diag, diag_r)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- 5. used workspace
@pytest.mark.parametrize("hidden,D,A,N,prec,want", FWD_CASES)
def test_forward_on_a_used_workspace(hidden, D, A, N, prec, want):
    """Each of the three calls in a fresh context against the same call in a second context right after a 2 N-row call of the
    same kind whose observations are all NaN (eps / given actions finite): the workspace rows past N hold NaN
    activations.  Only arithmetic sees the NaN; row counts and pointers are valid.  Bit-identical outputs.
    The 2 N-row call may take another launch form than the N-row one (its plan is printed next to the real call's): what the
    case covers is what THAT form leaves in the workspace - every activation for the layer-wise forms, nothing for the
    one-launch forms (step16_fwd / rows_fwd / fused_fwd keep activations on chip), which are then held only to "not
    disturbed by a previous call of another size"."""
    from cat_envs import native
    shape, lay, w, params = _net(D, A, hidden, prec, 3)
    x, eps = _fwd_inputs(D, A, N)
    fresh = native.Native()
    fresh.mlp_reserve(shape, 2 * N)
    fresh.plan_log(1)
    out = _three_forwards(fresh, shape, lay, params, x, eps)
    plan = fresh.plan_log(0)
    _assert_plan(plan, want)
    del fresh
    used = native.Native()
    used.mlp_reserve(shape, 2 * N)
    x_nan = np.full((2 * N, D), np.nan, np.float32)
    rs = np.random.RandomState(9)
    eps2, given2 = rs.standard_normal((2 * N, A)).astype(np.float32), rs.standard_normal((2 * N, A)).astype(np.float32)

    def pollute(mode):
        r = _forward(used, shape, lay, params, x_nan, eps2 if mode == "sample" else None,
                     given2 if mode == "given" else None, critic_only=mode == "critic")
        assert np.isnan(r["value"]).all()                  # the NaN went through the network

    used.plan_log(1)
    out_u = _three_forwards(used, shape, lay, params, x, eps, before=pollute)
    plan_u = used.plan_log(0)
    print("real calls:\n" + plan + "\nNaN calls interleaved:\n" + plan_u)
    assert f"{2 * N} rows" in plan_u and f" {N} rows" in plan_u
    for k in out:
        np.testing.assert_array_equal(out_u[k], out[k], err_msg=k)
    assert all(np.isfinite(v).all() for v in out.values())


@pytest.mark.parametrize("hidden,D,A,M,prec,want", GRAD_CASES)
def test_gradient_on_a_used_workspace(hidden, D, A, M, prec, want):
    """The minibatch gradient in a fresh context against the same call in a second context right after a 2 M-row minibatch
    whose observations are all NaN (actions, log-probs, advantages, returns, values and indices finite and valid): rows past
    M of the activations, dZ, their bf16 copies and the split-K / head partials hold NaN.  grad (pre-filled alike) and
    diag bit-identical.  The 2 M-row step may take another launch form than the M-row one (both plans are printed): the
    case covers what THAT form leaves behind - step16_kernel keeps the last hidden activations on chip, 4133 rows run
    layer-wise while 8266 take rows_fwd_kernel<64>; gathered inputs, stored activations, dZ and partials hold NaN in all."""
    from cat_envs import native
    shape, lay, w, params = _net(D, A, hidden, prec, 5)
    c = _grad_data(D, A, hidden, 2 * M, M, prec, False)
    fresh = native.Native()
    fresh.mlp_reserve(shape, 2 * M)
    fresh.plan_log(1)
    flat, diag = _grad(fresh, shape, lay, c, c["inds"])
    plan = fresh.plan_log(0)
    _assert_plan(plan, want)
    del fresh
    used = native.Native()
    used.mlp_reserve(shape, 2 * M)
    obs_nan = torch.full((2 * M, lay.obs_pad), float("nan"), device="cuda")
    used.plan_log(1)
    flat_p, diag_p = _grad(used, shape, lay, c, np.random.RandomState(9).permutation(2 * M).astype(np.int64), obs=obs_nan)
    plan_p = used.plan_log(0)
    print("real call:\n" + plan + "\nNaN call:\n" + plan_p)
    assert f"{2 * M} rows" in plan_p
    assert np.isnan(flat_p[lay.off_w[0][0]]) and np.isnan(diag_p[3])          # the NaN went through the step
    flat_u, diag_u = _grad(used, shape, lay, c, c["inds"])
    assert np.isfinite(diag).all() and np.abs(flat).max() > 0
    np.testing.assert_array_equal(flat_u, flat)
    np.testing.assert_array_equal(diag_u, diag)
