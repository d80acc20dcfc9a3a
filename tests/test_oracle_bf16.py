"""CPU tests of the oracle's restatements of the bf16-operand mode (oracle/ppo_oracle.py: ``accumulate`` and
``bf16_stored`` of _BF16OperandLinear / mlp_forward / AgentOracle) and of the localising comparisons meant for the
kernels' outputs (tests/localised_checks.py): the references have to justify the caps and bars of those comparisons,
and every comparison has to reject a seeded error.  No GPU, no kernel."""
import numpy as np
import pytest
import torch

import localised_checks as LC
import streams as S
from oracle import ppo_oracle as PO

REF, C256 = (512, 256, 128), (256, 256, 256)
# the forward shapes (D, A, hidden, N) at which the flip statistics are quoted
FWD_SHAPES = [(48, 12, C256, 4133), (45, 12, REF, 4133), (235, 12, C256, 4133), (33, 15, (64, 128, 64, 128), 300)]


def _inputs(D, A, N, seed=4):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((N, D)).astype(np.float32), rs.standard_normal((N, A)).astype(np.float32)


@pytest.mark.parametrize("opts", [dict(accumulate=torch.float64), dict(bf16_stored=True),
                                  dict(accumulate=torch.float64, bf16_stored=True)])
def test_new_options_change_nothing_without_bf16_hidden(opts):
    D, A, hidden = 45, 7, (64, 128)
    w = S.agent_weights(3, D, A, hidden)
    x, eps = _inputs(D, A, 70)
    f0, f1 = LC.oracle_forward(D, A, hidden, w, x, eps), LC.oracle_forward(D, A, hidden, w, x, eps, **opts)
    for k in f0:
        np.testing.assert_array_equal(f0[k], f1[k], err_msg=k)
    c = LC.minibatch_data(D, A, hidden, 128, 70, w)
    g0, st0 = LC.oracle_grad(D, A, hidden, w, c)
    g1, st1 = LC.oracle_grad(D, A, hidden, w, c, **opts)
    for k in g0:
        np.testing.assert_array_equal(g0[k], g1[k], err_msg=k)
    assert float(st0["loss"]) == float(st1["loss"])


@pytest.mark.parametrize("D,A,hidden,N", FWD_SHAPES)
def test_float64_and_float32_accumulation_agree_within_the_flip_statistics(D, A, hidden, N):
    """The two accumulations are two summation orders of the same bf16 products: all but a few rows agree to fp32
    rounding, the others by a bf16 step of one activation.  Measured here (seeds 3 / 4): 0.3-0.6 % of the rows flipped on
    the value, 1.1-1.3 % on the mean action, at most 4.7 % of a 64-row block, none in the ragged block, median error 6e-8.
    A row counts as flipped when ANY of value, action, log-prob misses its fp32 bar: at the three 4133-row shapes 1.6-1.9 %
    of the rows, at most 5 of the 64 rows of a block (7.8 %); at the 300-row shape one row (0.33 %).  The device against the float64 oracle is the same comparison with another fp32
    order, so the caps (5 % / 25 %) must hold here with room to spare: half of each cap."""
    w = S.agent_weights(3, D, A, hidden)
    x, eps = _inputs(D, A, N)
    f32 = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True)
    f64 = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=torch.float64)
    rep, bad = LC.row_report(f32, f64)
    print(rep)
    assert not bad, bad
    assert rep["flipped_share"] <= LC.ROW_CAP / 2 and rep["worst_block_share"] <= LC.BLOCK_CAP / 2, rep
    assert rep["median_abs_error_value"] < 1e-6, rep
    # the mode rounds: the fp32 network is a bf16-sized distance away on most rows, not on a few
    rep32, _ = LC.row_report(LC.oracle_forward(D, A, hidden, w, x, eps), f64)
    assert rep32["flipped_share"] > 0.5, rep32


@pytest.mark.parametrize("D,A,hidden,N,k_step", [(*FWD_SHAPES[0], 4), (*FWD_SHAPES[0], 16), (*FWD_SHAPES[1], 4)])
def test_device_like_arithmetic_stays_under_the_flip_caps(D, A, hidden, N, k_step):
    """LC.device_like_forward (fp32 accumulator fed 4 or 16 k at a time, the kernels' exp2-based ELU) against the float64
    oracle: 1.5-2.2 % of the 4133 rows flipped, at most 5 of a block's 64 (7.8 %), largest error 2.6e-3.  The conditions are
    the caps themselves (5 % / 25 % / 5e-3): arithmetic cruder than the kernels' must still meet what the kernels are held to."""
    w = S.agent_weights(3, D, A, hidden)
    x, eps = _inputs(D, A, N)
    f64 = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=torch.float64)
    rep, bad = LC.row_report(LC.device_like_forward(D, A, hidden, w, x, eps, k_step), f64)
    print(rep)
    assert not bad, bad


def test_per_tensor_bars_tell_the_two_restatements_apart():
    """At a shape of the GPU module's act16 cases (one layer below the head, 4133 rows): the float64 oracle that rounds at use,
    held against the bf16-stored one with the bars of the stored pair, is rejected - the hidden layers' bias gradients
    (column sums of the rounded against the unrounded dZ) among the tensors over their bars.  So a device that stores bf16
    and an oracle that does not (or the reverse) cannot pass the per-tensor check."""
    D, A, hidden, Bsz, M = 48, 3, (256, 128), 8192, 4133
    w = S.agent_weights(5, D, A, hidden)
    c = LC.minibatch_data(D, A, hidden, Bsz, M, w, bf16_hidden=True, accumulate=torch.float64, bf16_stored=True)
    opts = dict(bf16_hidden=True, bf16_stored=True)
    g64, _ = LC.oracle_grad(D, A, hidden, w, c, accumulate=torch.float64, **opts)
    g32, _ = LC.oracle_grad(D, A, hidden, w, c, **opts)
    _, bars = LC.tensor_bars(g32, g64)
    g_use, _ = LC.oracle_grad(D, A, hidden, w, c, bf16_hidden=True, accumulate=torch.float64)
    err, bad = LC.tensors_over_bar(g_use, g64, bars)
    print(bad)
    assert len(bad) >= 3 and any(".bias" in b for b in bad), (err, bars)


@pytest.mark.parametrize("acc", [torch.float32, torch.float64], ids=["acc32", "acc64"])
def test_bf16_stored_differs_from_rounded_at_use_only_in_the_backward(acc):
    """Rounding is idempotent: storing an activation as bf16 gives the GEMM that consumes it the operand it would have
    rounded itself, and the last hidden layer stays fp32 for the head.  The backward sees the rounded values outside
    the GEMMs: elu'(H) = H + 1 of a rounded activation and the bias gradients' column sums of the rounded dZ."""
    D, A, hidden = 48, 3, (256, 128, 64)
    w = S.agent_weights(5, D, A, hidden)
    x, eps = _inputs(D, A, 150)
    use = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=acc)
    sto = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=acc, bf16_stored=True)
    for k in use:
        np.testing.assert_array_equal(use[k], sto[k], err_msg=k)
    c = LC.minibatch_data(D, A, hidden, 256, 150, w, bf16_hidden=True)
    g_use, st_use = LC.oracle_grad(D, A, hidden, w, c, bf16_hidden=True, accumulate=acc)
    g_sto, st_sto = LC.oracle_grad(D, A, hidden, w, c, bf16_hidden=True, accumulate=acc, bf16_stored=True)
    assert float(st_use["loss"]) == float(st_sto["loss"])
    err = LC.tensor_errors(g_sto, g_use)
    # heads and log-std take no rounded value: identical.  The last hidden layer's weight gradient has the same bf16 operands
    # either way (its dZ comes from the fp32 activation); its bias gradient sums the rounded dZ, and every tensor below it
    # moves by a bf16-sized amount (2^-9 per element)
    for k in ("actor_logstd", "critic.6.weight", "critic.6.bias", "actor_mean.6.weight", "actor_mean.6.bias"):
        assert err[k] == 0.0, (k, err[k])
    for k, e in err.items():
        if "." in k and k.split(".")[1] in ("0", "2", "4"):
            assert e < 2e-2 and (e > 0.0 or k.endswith("4.weight")), (k, e)


def _grad_case():
    D, A, hidden, Bsz, M = 33, 15, (64, 128, 64, 128), 1024, 300        # deepest network, widest action, ragged 300-row minibatch
    w = S.agent_weights(5, D, A, hidden)
    c = LC.minibatch_data(D, A, hidden, Bsz, M, w, bf16_hidden=True, accumulate=torch.float64)
    return D, A, hidden, w, c


def test_per_row_check_rejects_a_wrong_tile_and_a_dropped_row():
    """Seeded errors tried (oracle level, tests/localised_checks.py): (1) the 20 last rows of the 37-row ragged block off
    by a quarter of their distance to the fp32 network - every error below the bulk bars of tests/test_gpu_bf16.py, which therefore accept it; the
    per-block cap rejects it.  (2) the last row's outputs dropped (zero): the 5e-3 bar on flipped rows rejects it."""
    D, A, hidden, N = 48, 12, C256, 4133
    w = S.agent_weights(3, D, A, hidden)
    x, eps = _inputs(D, A, N)
    f64 = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True, accumulate=torch.float64)
    f32 = LC.oracle_forward(D, A, hidden, w, x, eps, bf16_hidden=True)
    assert not LC.row_report(f32, f64)[1]
    mutant = LC.forward_with_wrong_tile(f32, LC.oracle_forward(D, A, hidden, w, x, eps), N - 20)
    dv, da = np.abs(mutant["value"] - f64["value"]), np.abs(mutant["action"] - f64["action"])
    assert dv.max() < 5e-3 and dv.mean() < 2e-5 and da.max() < 5e-3 and da.mean() < 2e-5       # the bulk bars pass it
    rep, bad = LC.row_report(mutant, f64)
    assert len(bad) == 1 and "rows 4096..4132" in bad[0], (rep, bad)
    dropped = {k: v.copy() for k, v in f32.items()}
    for k in dropped:
        dropped[k][-1] = 0.0
    rep, bad = LC.row_report(dropped, f64)
    assert bad and "bf16 bar" in bad[0], (rep, bad)


def test_per_tensor_check_rejects_a_dropped_row_and_a_zeroed_bias_gradient():
    """Seeded errors tried: (1) LC.DropsLastRow - the last minibatch row's contribution to every weight and bias gradient
    dropped; (2) one bias gradient zeroed.  The per-tensor bars, computed from the two references alone, reject both (at
    this 300-row minibatch a row is a 5e-2 share of the gradient; at 4133 rows it is 3e-3 to 1e-1 of most tensors and
    below the whole-gradient bars of tests/test_gpu_bf16.py), and accept the float32-accumulating oracle (which is how
    noise_k is defined, so that is no more than a consistency check)."""
    D, A, hidden, w, c = _grad_case()
    g64, _ = LC.oracle_grad(D, A, hidden, w, c, bf16_hidden=True, accumulate=torch.float64)
    g32, _ = LC.oracle_grad(D, A, hidden, w, c, bf16_hidden=True)
    noise, bars = LC.tensor_bars(g32, g64)
    print({k: (noise[k], bars[k]) for k in bars})
    assert max(bars.values()) < 5e-3, bars                      # (issue: noise <= 9.4e-4 for weights, 2.1e-4 for biases)
    assert not LC.tensors_over_bar(g32, g64, bars)[1]
    g_drop, st = LC.oracle_grad(D, A, hidden, w, c, agent_cls=LC.DropsLastRow, bf16_hidden=True)
    for name, mutant in (("dropped row", g_drop), ("zeroed bias gradient", LC.zero_one_bias_gradient(g32, "critic.2.bias"))):
        err, bad = LC.tensors_over_bar(mutant, g64, bars)
        print(name, bad)
        assert bad, (name, err)
    # one dropped row of 300 moves most tensors, not one
    assert len(LC.tensors_over_bar(g_drop, g64, bars)[1]) > len(g64) // 2


def test_rotation_checks_accept_the_oracle_and_reject_a_dropped_row():
    """The row-placement comparisons need no reference: the same rows rotated by 37 positions.  On the float64-accumulating
    oracle (whose result does not depend on a summation order) the un-rotated outputs are bit-identical and the
    gradients agree; seeded error tried: LC.DropsLastRow, which drops ANOTHER original row after the rotation - the forward
    comparison sees nothing (its outputs are right), the gradient comparison rejects it; and a forward whose last row is
    wrong (zeroed) is rejected by the bit comparison."""
    D, A, hidden, w, c = _grad_case()
    opts = dict(bf16_hidden=True, accumulate=torch.float64)
    M = c["inds"].shape[0]
    x, eps = c["obs"][c["inds"]], _inputs(D, A, M)[1]
    out = LC.oracle_forward(D, A, hidden, w, x, eps, **opts)
    out_r = LC.oracle_forward(D, A, hidden, w, LC.rot(x), LC.rot(eps), **opts)
    assert not LC.forward_rotation_mismatch(out, out_r)
    wrong = {k: v.copy() for k, v in out_r.items()}
    wrong["value"][-1] = 0.0
    assert LC.forward_rotation_mismatch(out, wrong) == ["value"]
    g, st = LC.oracle_grad(D, A, hidden, w, c, **opts)
    g_r, st_r = LC.oracle_grad(D, A, hidden, w, c, inds=LC.rot(c["inds"]), **opts)
    assert not LC.grad_rotation_mismatch(g, g_r)
    gm, _ = LC.oracle_grad(D, A, hidden, w, c, agent_cls=LC.DropsLastRow, **opts)
    gm_r, _ = LC.oracle_grad(D, A, hidden, w, c, inds=LC.rot(c["inds"]), agent_cls=LC.DropsLastRow, **opts)
    bad = LC.grad_rotation_mismatch(gm, gm_r)
    assert len(bad) > len(g) // 2, bad
