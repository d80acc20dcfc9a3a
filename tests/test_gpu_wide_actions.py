"""Wide action heads (16 <= act_dim <= 63): head_act_wide_kernel (rollout forward) and head_loss_wide_kernel (heads + PPO
loss + head backward) against the oracle (oracle/ppo_oracle.py is generic in the action width), through the C ABI, the
Agent / PPOTrainer layer and the export path."""
import math

import numpy as np
import pytest
import torch

import streams as S
from oracle import ppo_oracle as PO
from oracle import rng_oracle as RO

pytestmark = pytest.mark.gpu
ARCHS = {"ref": (45, (512, 256, 128)), "3x256": (48, (256, 256, 256))}


@pytest.fixture(scope="module")
def nat():
    from cat_envs import native
    return native.get(torch.device("cuda", 0))


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _setup(D, A, hidden, seed=3, prec=0):
    from cat_envs import native
    from test_gpu_kernels import flat_params
    shape = native.shape_of(D, A, hidden, mfma_bf16=prec)
    lay = native.layout_of(shape)
    w = S.agent_weights(seed, D, A, hidden)
    ag = PO.AgentOracle(D, A, hidden)
    ag.load(w)
    return shape, lay, w, ag, flat_params(native, shape, lay, w)


def _padded(x, lay):
    xp = np.zeros((x.shape[0], lay.obs_pad), np.float32)
    xp[:, :x.shape[1]] = x
    return xp


# ------------------------------------------------------------------------------------------ rollout forward
@pytest.mark.parametrize("N", [7, 1000, 2048, 3000, 4096, 16384])
@pytest.mark.parametrize("arch", list(ARCHS))
@pytest.mark.parametrize("A", [16, 19, 37, 63])
def test_policy_step_wide_vs_oracle(nat, A, arch, N):
    """supplied eps, given action and deterministic forms; bars of test_policy_act_vs_oracle_and_golden (fp32)"""
    _rollout_case(nat, *ARCHS[arch], A, N)


@pytest.mark.parametrize("N", [7, 3000, 4096])
@pytest.mark.parametrize("A", [19, 63])
@pytest.mark.parametrize("hidden", [(256, 64), (128, 512)], ids=["HL64", "HL512"])
def test_policy_step_wide_narrowest_and_widest_last_layer(nat, hidden, A, N):
    """the HL = 64 instance (weights staged in LDS) and the HL = 512 one (weights read through the caches)"""
    _rollout_case(nat, 33, hidden, A, N)


def _rollout_case(nat, D, hidden, A, N):
    shape, lay, w, ag, params = _setup(D, A, hidden)
    rs = np.random.RandomState(4)
    x = rs.standard_normal((N, D)).astype(np.float32)
    eps = rs.standard_normal((N, A)).astype(np.float32)
    given = (rs.standard_normal((N, A)) * 0.7).astype(np.float32)
    xp = dev(_padded(x, lay))
    nat.mlp_reserve(shape, N)
    act, logp, val = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    tol = dict(rtol=1e-5, atol=2e-5)
    xt = torch.from_numpy(x)
    nat.policy_act(shape, params, xp, N, dev(eps), act, logp, val)
    torch.cuda.synchronize()
    with torch.no_grad():
        a, lp, _, v = ag.get_action_and_value(xt, eps=torch.from_numpy(eps))
    np.testing.assert_allclose(act.cpu().numpy(), a.numpy(), **tol)
    np.testing.assert_allclose(val.cpu().numpy(), v.numpy()[:, 0], **tol)
    np.testing.assert_allclose(logp.cpu().numpy(), lp.numpy(), rtol=1e-5, atol=1e-4)
    # critic only (the bootstrap value): the same values bit for bit
    val2 = torch.empty(N, device="cuda")
    nat.value(shape, params, xp, N, val2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(val2.cpu().numpy(), val.cpu().numpy())
    # given actions: log-prob / value of stored actions
    nat.policy_act(shape, params, xp, N, None, act, logp, val, given_action=dev(given))
    torch.cuda.synchronize()
    with torch.no_grad():
        _, lp, _, v = ag.get_action_and_value(xt, torch.from_numpy(given))
    np.testing.assert_array_equal(act.cpu().numpy(), given)
    np.testing.assert_allclose(logp.cpu().numpy(), lp.numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), v.numpy()[:, 0], **tol)
    # deterministic: action = mean
    nat.policy_act(shape, params, xp, N, None, act, logp, val)
    torch.cuda.synchronize()
    with torch.no_grad():
        am, lp, _, _ = ag.get_action_and_value(xt, deterministic=True)
    np.testing.assert_allclose(act.cpu().numpy(), am.numpy(), **tol)
    np.testing.assert_allclose(logp.cpu().numpy(), lp.numpy(), rtol=1e-5, atol=1e-4)


def test_plan_names_the_wide_kernels(nat):
    D, hidden = ARCHS["ref"]
    shape, lay, w, ag, params = _setup(D, 19, hidden)
    N = 4096
    nat.mlp_reserve(shape, N)
    x = dev(_padded(np.random.RandomState(1).standard_normal((N, D)).astype(np.float32), lay))
    act, logp, val = torch.empty(N, 19, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    nat.plan_log(1)
    nat.policy_act(shape, params, x, N, None, act, logp, val)
    torch.cuda.synchronize()
    log = nat.plan_log(0)
    assert "head_act_wide_kernel" in log and "rows_fwd" not in log and "step16" not in log, log


# ------------------------------------------------------------------------------------------ Philox noise
@pytest.mark.parametrize("arch", list(ARCHS))
@pytest.mark.parametrize("N,A", [(4096, 19), (1000, 37), (300, 63)])
def test_philox_noise_wide(nat, N, A, arch):
    """eps_out = the catppo.h convention (rng_oracle restatement); replayed through the oracle it gives the device's actions
    and log-probs; dimension k < 12 of an A = 19 run draws what dimension k of an A = 12 run draws"""
    from cat_envs import native
    D, hidden = ARCHS[arch]
    shape, lay, w, ag, params = _setup(D, A, hidden)
    rs = np.random.RandomState(5)
    x = rs.standard_normal((N, D)).astype(np.float32)
    xp = dev(_padded(x, lay))
    seed = 0x1234567890ABCDEF
    st = nat.iter_state_new(seed, 3e-4)
    nat.iter_begin(st, 3e-4, 10, native.LR_FIXED)
    nat.iter_begin(st, 3e-4, 10, native.LR_FIXED)          # iteration 2
    nat.mlp_reserve(shape, N)
    act, logp, val = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    eps = torch.zeros(N, A, device="cuda")
    for step in (0, 5):
        nat.policy_act_rng(shape, params, xp, N, st, step, act, logp, val, eps_out=eps)
        torch.cuda.synchronize()
        e = eps.cpu().numpy()
        np.testing.assert_allclose(e, RO.action_noise(seed, 2, step, N, A), rtol=2e-5, atol=2e-6)
        with torch.no_grad():
            a, lp, _, v = ag.get_action_and_value(torch.from_numpy(x), eps=torch.from_numpy(e))
        np.testing.assert_allclose(act.cpu().numpy(), a.numpy(), rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(logp.cpu().numpy(), lp.numpy(), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(val.cpu().numpy(), v.numpy()[:, 0], rtol=1e-5, atol=2e-5)
        if A == 19:
            shape12, _, _, _, params12 = _setup(D, 12, hidden)
            nat.mlp_reserve(shape12, N)
            e12 = torch.zeros(N, 12, device="cuda")
            nat.policy_act_rng(shape12, params12, xp, N, st, step, torch.empty(N, 12, device="cuda"),
                               torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), eps_out=e12)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(e[:, :12], e12.cpu().numpy())


# ------------------------------------------------------------------------------------------ minibatch gradient
def _grad_case(nat, D, A, hidden, Bsz, M, norm_adv, clip_vloss, prec=0, ext_stats=False):
    from cat_envs import native
    from test_gpu_kernels import _minibatch_case, unflatten_grad
    shape, lay, w, ag, params = _setup(D, A, hidden, seed=5, prec=prec)
    c = _minibatch_case(D, A, hidden, Bsz, M, 6)
    ag.value_rms.mean, ag.value_rms.var = torch.tensor(float(c["vmean"])), torch.tensor(float(c["vvar"]))
    with torch.no_grad():
        _, lp0, _, _ = ag.get_action_and_value(torch.from_numpy(c["obs"]), torch.from_numpy(c["act"]))
    rs = np.random.RandomState(7)
    c["logp"] = (lp0.numpy() + rs.standard_normal(Bsz).astype(np.float32) * 0.25).astype(np.float32)
    mb = torch.from_numpy(c["inds"])
    adv_stats = None
    adv_mb = torch.from_numpy(c["adv"])[mb]
    if ext_stats:        # advantage statistics supplied by the caller (the multi-rank form): the oracle normalises with them
        st = np.array([float(adv_mb.double().mean()) + 0.1, float(adv_mb.double().std()) * 1.3 + 1e-8], np.float32)
        adv_stats = dev(st)
        adv_mb = (adv_mb - float(st[0])) / float(st[1])
    cfg = dict(clip_coef=0.2, ent_coef=0.001, vf_coef=2.0, norm_adv=norm_adv and not ext_stats, clip_vloss=clip_vloss)
    for p in ag.parameters():
        p.requires_grad_(True)
    loss, stats = PO.ppo_minibatch_loss(ag, torch.from_numpy(c["obs"])[mb], torch.from_numpy(c["act"])[mb],
                                        torch.from_numpy(c["logp"])[mb], adv_mb, torch.from_numpy(c["ret"])[mb],
                                        torch.from_numpy(c["val"])[mb], cfg)
    loss.backward()
    ref = {k: v.grad.numpy() for k, v in ag.p.items()}
    obs_p = _padded(c["obs"], lay)
    hp = native.PpoHparams(0.2, 0.001, 2.0, int(norm_adv), int(clip_vloss), 1.0 / M, int(ext_stats))
    nat.mlp_reserve(shape, M)
    grad, diag = torch.zeros(lay.n_flat, device="cuda"), torch.zeros(8, device="cuda")
    vm, vv = dev(np.array([c["vmean"]])), dev(np.array([c["vvar"]]))
    inputs = [dev(obs_p), dev(c["act"]), dev(c["logp"]), dev(c["adv"]), dev(c["ret"]), dev(c["val"])]
    nat.ppo_minibatch_grad(shape, hp, params, *inputs, dev(c["inds"]), vm, vv, adv_stats, grad, diag)
    torch.cuda.synchronize()
    exp = [float(stats["pg_loss"]), float(stats["v_loss"]), float(stats["entropy"]), float(stats["loss"]),
           float(stats["approx_kl"]), float(stats["old_approx_kl"]), float(stats["clipfrac"])]
    return dict(shape=shape, lay=lay, w=w, params=params, ref=ref, grad=grad, diag=diag, exp=exp, c=c, hp=hp, vm=vm, vv=vv,
                inputs=inputs, adv_stats=adv_stats, unflatten=unflatten_grad, ag=ag, adv_mb=adv_mb)


def _check_grad(r, grad, diag, rel=2e-4):
    d = diag.cpu().numpy()
    np.testing.assert_allclose(d[:7], r["exp"], rtol=2e-4, atol=2e-6)
    assert d[7] == 1.0
    got = r["unflatten"](r["shape"], r["lay"], grad.cpu().numpy(), r["w"])
    for k, v in r["ref"].items():
        err = np.abs(got[k].reshape(v.shape) - v).max() / max(np.abs(v).max(), 1e-8)
        assert err < rel, (k, err)
    gn = math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in r["ref"].values()))
    gn_got = math.sqrt(sum(float((got[k].astype(np.float64) ** 2).sum()) for k in r["ref"]))
    assert abs(gn_got - gn) < 1e-4 * gn


@pytest.mark.parametrize("flags", [(True, True), (False, False), (True, False)], ids=["norm_vclip", "plain", "norm"])
@pytest.mark.parametrize("M", [512, 4096, 16384])
@pytest.mark.parametrize("A", [19, 37, 63])
@pytest.mark.parametrize("arch", list(ARCHS))
def test_minibatch_grad_wide_vs_autograd(nat, arch, A, M, flags):
    """catppo_ppo_minibatch_grad (gather + layer-wise forward + head_loss_wide_kernel + backward + fold) against autograd
    through the oracle's loss; bars of test_ppo_minibatch_grad_vs_autograd_oracle.  Then the packed one-call step on the
    same gathered minibatch folds the same gradient bit for bit."""
    D, hidden = ARCHS[arch]
    r = _grad_case(nat, D, A, hidden, max(M + 500, 2 * M), M, *flags)
    _check_grad(r, r["grad"], r["diag"])
    # the same minibatch through the packed entries: gather, then grad_packed and the one-call optimiser step
    lay, shape = r["lay"], r["shape"]
    obs, act, logp, adv, ret, val = r["inputs"]
    x_g, act_g = torch.empty(M, lay.obs_pad, device="cuda"), torch.empty(M, A, device="cuda")
    scal_g = torch.empty(4 * M, device="cuda")
    adv_part = torch.empty(2 * ((M + nat.GATHER_ROWS - 1) // nat.GATHER_ROWS), dtype=torch.float64, device="cuda")
    nat.ppo_gather(shape, obs, act, logp, adv, ret, val, dev(r["c"]["inds"]), M, x_g, act_g, scal_g, adv_part)
    g2, d2 = torch.zeros_like(r["grad"]), torch.zeros(8, device="cuda")
    nat.ppo_minibatch_grad_packed(shape, r["hp"], r["params"], x_g, act_g, scal_g, adv_part, M, r["vm"], r["vv"], None,
                                  g2, d2)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(g2.cpu().numpy(), r["grad"].cpu().numpy())
    np.testing.assert_array_equal(d2.cpu().numpy(), r["diag"].cpu().numpy())
    from cat_envs import native
    st = nat.iter_state_new(7, 3e-4)
    nat.iter_begin(st, 3e-4, 10, native.LR_FIXED)
    p3 = r["params"].clone()
    g3, d3 = torch.zeros_like(r["grad"]), torch.zeros(8, device="cuda")
    m1, m2 = torch.zeros_like(p3), torch.zeros_like(p3)
    nat.ppo_minibatch_step_packed(shape, r["hp"], p3, x_g, act_g, scal_g, adv_part, M, r["vm"], r["vv"], None, g3, d3,
                                  m1, m2, 1.0, 0.9, 0.999, 1e-5, st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d3.cpu().numpy(), r["diag"].cpu().numpy())
    # = the gradient of the grad entry through the separate clip + Adam launch (the norm is summed in another order)
    st4 = nat.iter_state_new(7, 3e-4)
    nat.iter_begin(st4, 3e-4, 10, native.LR_FIXED)
    p4 = r["params"].clone()
    nat.clip_adam_dev(p4, r["grad"].clone(), torch.zeros_like(p4), torch.zeros_like(p4), lay.n_flat, 1.0, 0.9, 0.999, 1e-5,
                      st4)
    torch.cuda.synchronize()
    assert float((p3 - r["params"]).abs().max()) > 0.0       # the Adam step moved the parameters
    np.testing.assert_allclose(p3.cpu().numpy(), p4.cpu().numpy(), rtol=0, atol=1e-7)


@pytest.mark.parametrize("M", [1000, 2048, 4097])
@pytest.mark.parametrize("A", [19, 63])
@pytest.mark.parametrize("arch", list(ARCHS))
def test_minibatch_grad_wide_ragged_last_tile(nat, arch, A, M):
    """minibatch sizes that leave head_loss_wide_kernel a partial last 16-row tile (1000: 8 rows, 4097: 1 row) and the
    2048 rows of an env-sharded rank"""
    D, hidden = ARCHS[arch]
    r = _grad_case(nat, D, A, hidden, M + 700, M, True, True)
    _check_grad(r, r["grad"], r["diag"])


@pytest.mark.parametrize("A", [19, 63])
def test_minibatch_grad_wide_external_adv_stats_and_branch_codes(nat, A):
    D, hidden = ARCHS["ref"]
    M = 4096
    r = _grad_case(nat, D, A, hidden, 6000, M, True, True, ext_stats=True)
    _check_grad(r, r["grad"], r["diag"])
    # clip-branch codes (catppo_debug_clip_branches) in the encoding of head_loss_kernel
    buf = torch.full((2 * M,), -1, dtype=torch.int32, device="cuda")
    nat.debug_clip_branches(buf)
    try:
        g, d = torch.zeros_like(r["grad"]), torch.zeros(8, device="cuda")
        nat.ppo_minibatch_grad(r["shape"], r["hp"], r["params"], *r["inputs"], dev(r["c"]["inds"]), r["vm"], r["vv"],
                               r["adv_stats"], g, d)
        torch.cuda.synchronize()
    finally:
        nat.debug_clip_branches(None)
    codes = buf.cpu().numpy()
    assert codes.min() >= 0
    # against the oracle's branches of the same samples (cleanrl/ppo.py:320-341); a sample within 1e-5 of a boundary may
    # fall either way (device and oracle agree on ratio / value to ~1e-6)
    c, ag, mb, clip = r["c"], r["ag"], r["c"]["inds"], 0.2
    with torch.no_grad():
        _, lp, _, v = ag.get_action_and_value(torch.from_numpy(c["obs"][mb]), torch.from_numpy(c["act"][mb]))
    ratio = np.exp(lp.numpy().astype(np.float64) - c["logp"][mb])
    nv = (v.numpy()[:, 0].astype(np.float64) - float(c["vmean"])) / np.sqrt(float(c["vvar"]) + 1e-8)
    dl = nv - c["val"][mb]
    code = lambda x, centre: (x < centre - clip).astype(int) + 2 * (x > centre + clip).astype(int)  # noqa: E731
    e1, e2 = nv - c["ret"][mb], c["val"][mb] + np.clip(dl, -clip, clip) - c["ret"][mb]
    vmax = (e1 * e1 > e2 * e2).astype(int) + 2 * (e1 * e1 < e2 * e2).astype(int)
    far_pg = np.abs(np.abs(ratio - 1.0) - clip) > 1e-5
    far_v = np.abs(np.abs(dl) - clip) > 1e-5
    far_max = far_v & (np.abs(np.abs(e1) - np.abs(e2)) > 1e-5)
    np.testing.assert_array_equal(codes[:M][far_pg], code(ratio, 1.0)[far_pg])
    np.testing.assert_array_equal((codes[M:] & 3)[far_v], code(dl, 0.0)[far_v])
    np.testing.assert_array_equal((codes[M:] >> 2)[far_max], vmax[far_max])
    assert far_pg.mean() > 0.99 and far_v.mean() > 0.99 and far_max.sum() > M // 4
    for k in (1, 2):                                       # every branch is exercised
        assert (codes[:M] == k).any() and ((codes[M:] & 3) == k).any() and ((codes[M:] >> 2) == k).any()


@pytest.mark.parametrize("HL_hidden", [(256, 64), (256, 512)], ids=["HL64", "HL512"])
def test_minibatch_grad_wide_narrow_and_widest_last_layer(nat, HL_hidden):
    r = _grad_case(nat, 33, 37, HL_hidden, 3000, 2048, True, True)
    _check_grad(r, r["grad"], r["diag"])


# ------------------------------------------------------------------------------------------ precision modes
def test_bf16x3_mode_wide(nat):
    """split-bf16 operands at A = 19: the fp32 bars (the heads are fp32 in every mode), as the bf16x3 rows of
    test_ppo_minibatch_grad_vs_autograd_oracle"""
    D, hidden = ARCHS["3x256"]
    A, N = 19, 4096
    shape, lay, w, ag, params = _setup(D, A, hidden, prec=2)
    rs = np.random.RandomState(4)
    x = rs.standard_normal((N, D)).astype(np.float32)
    eps = rs.standard_normal((N, A)).astype(np.float32)
    nat.mlp_reserve(shape, N)
    act, logp, val = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    nat.policy_act(shape, params, dev(_padded(x, lay)), N, dev(eps), act, logp, val)
    torch.cuda.synchronize()
    with torch.no_grad():
        a, lp, _, v = ag.get_action_and_value(torch.from_numpy(x), eps=torch.from_numpy(eps))
    np.testing.assert_allclose(act.cpu().numpy(), a.numpy(), rtol=2e-5, atol=5e-5)
    np.testing.assert_allclose(val.cpu().numpy(), v.numpy()[:, 0], rtol=2e-5, atol=5e-5)
    r = _grad_case(nat, D, A, hidden, 6000, 4096, True, True, prec=2)
    _check_grad(r, r["grad"], r["diag"])


@pytest.mark.parametrize("arch,B", [("3x256", 4096), ("ref", 1000)])
def test_bf16_mode_wide_rollout_vs_bf16_operand_oracle(nat, arch, B):
    """mfma_bf16 = 1 at A = 19 (layer-wise bf16 forward, bf16-stored activations from 4096 rows, head_act_wide_kernel):
    the bars of test_gpu_bf16.py::test_bf16_policy_act_vs_bf16_operand_oracle"""
    D, hidden = ARCHS[arch]
    A = 19
    shape, lay, w, ag32, params = _setup(D, A, hidden, prec=1)
    ag = PO.AgentOracle(D, A, hidden, bf16_hidden=True)
    ag.load(w)
    rs = np.random.RandomState(4)
    x = rs.standard_normal((B, D)).astype(np.float32)
    eps = rs.standard_normal((B, A)).astype(np.float32)
    nat.mlp_reserve(shape, B)
    act, logp, val = torch.empty(B, A, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    nat.policy_act(shape, params, dev(_padded(x, lay)), B, dev(eps), act, logp, val)
    torch.cuda.synchronize()
    with torch.no_grad():
        a, lp, _, v = ag.get_action_and_value(torch.from_numpy(x), eps=torch.from_numpy(eps))
        _, _, _, v32 = ag32.get_action_and_value(torch.from_numpy(x), eps=torch.from_numpy(eps))
    dv = np.abs(val.cpu().numpy() - v.numpy()[:, 0])
    da = np.abs(act.cpu().numpy() - a.numpy())
    assert dv.max() < 5e-3 and dv.mean() < 2e-5, (dv.max(), dv.mean())
    assert da.max() < 5e-3 and da.mean() < 2e-5, (da.max(), da.mean())
    d32 = np.abs(val.cpu().numpy() - v32.numpy()[:, 0])
    assert 1e-4 < d32.mean() < 3e-2, d32.mean()


@pytest.mark.parametrize("arch,Bsz,M", [("3x256", 8192, 4096), ("ref", 32768, 16384), ("ref", 4000, 2048)])
def test_bf16_mode_wide_grad_vs_bf16_operand_autograd(nat, arch, Bsz, M):
    """mfma_bf16 = 1 at A = 19 (layer-wise bf16 forward, head_loss_wide_kernel, layer-wise bf16 backward): the bars of
    test_gpu_bf16.py::test_bf16_minibatch_grad_vs_bf16_operand_autograd against the bf16-operand and the fp32 oracle"""
    from cat_envs import native
    from test_gpu_kernels import _minibatch_case, flat_params, unflatten_grad
    D, hidden = ARCHS[arch]
    A = 19
    shape = native.shape_of(D, A, hidden, mfma_bf16=1)
    lay = native.layout_of(shape)
    w = S.agent_weights(5, D, A, hidden)
    c = _minibatch_case(D, A, hidden, Bsz, M, 6)
    grads = {}
    for name, bf in (("bf16", True), ("fp32", False)):
        ag = PO.AgentOracle(D, A, hidden, bf16_hidden=bf)
        ag.load(w)
        ag.value_rms.mean, ag.value_rms.var = torch.tensor(float(c["vmean"])), torch.tensor(float(c["vvar"]))
        if name == "bf16":
            with torch.no_grad():
                _, lp0, _, _ = ag.get_action_and_value(torch.from_numpy(c["obs"]), torch.from_numpy(c["act"]))
            rs = np.random.RandomState(7)
            c["logp"] = (lp0.numpy() + rs.standard_normal(Bsz).astype(np.float32) * 0.25).astype(np.float32)
        cfg = dict(clip_coef=0.2, ent_coef=0.001, vf_coef=2.0, norm_adv=True, clip_vloss=True)
        for p in ag.parameters():
            p.requires_grad_(True)
        mb = torch.from_numpy(c["inds"])
        loss, st = PO.ppo_minibatch_loss(ag, torch.from_numpy(c["obs"])[mb], torch.from_numpy(c["act"])[mb],
                                         torch.from_numpy(c["logp"])[mb], torch.from_numpy(c["adv"])[mb],
                                         torch.from_numpy(c["ret"])[mb], torch.from_numpy(c["val"])[mb], cfg)
        loss.backward()
        grads[name] = ({k: v.grad.numpy() for k, v in ag.p.items()}, st)
    params = flat_params(native, shape, lay, w)
    grad, diag = torch.zeros(lay.n_flat, device="cuda"), torch.zeros(8, device="cuda")
    hp = native.PpoHparams(0.2, 0.001, 2.0, 1, 1, 1.0 / M, 0)
    nat.mlp_reserve(shape, M)
    nat.ppo_minibatch_grad(shape, hp, params, dev(_padded(c["obs"], lay)), dev(c["act"]), dev(c["logp"]), dev(c["adv"]),
                           dev(c["ret"]), dev(c["val"]), dev(c["inds"]), dev(np.array([c["vmean"]])),
                           dev(np.array([c["vvar"]])), None, grad, diag)
    torch.cuda.synchronize()
    assert np.isfinite(grad.cpu().numpy()).all()
    got = unflatten_grad(shape, lay, grad.cpu().numpy(), w)

    def flat(gd):
        return np.concatenate([np.asarray(gd[k], np.float64).reshape(-1) for k in sorted(grads["bf16"][0])])

    g_dev = flat({k: got[k].reshape(v.shape) for k, v in grads["bf16"][0].items()})
    g_bf, g_32 = flat(grads["bf16"][0]), flat(grads["fp32"][0])
    cos = lambda a, b: float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))  # noqa: E731
    assert cos(g_dev, g_bf) > 0.9999, cos(g_dev, g_bf)
    assert cos(g_dev, g_32) > 0.995, cos(g_dev, g_32)
    assert cos(g_dev, g_bf) > cos(g_dev, g_32)
    rel = np.linalg.norm(g_dev - g_bf) / np.linalg.norm(g_bf)
    assert rel < 1e-2, rel
    st = grads["bf16"][1]
    np.testing.assert_allclose(diag.cpu().numpy()[:4], [float(st["pg_loss"]), float(st["v_loss"]), float(st["entropy"]),
                                                       float(st["loss"])], rtol=2e-3, atol=2e-4)
    # the head segments on their own: a wrong head gradient would hide in the whole-vector cosine
    for k in ("actor_logstd", f"actor_mean.{2 * len(hidden)}.weight", f"actor_mean.{2 * len(hidden)}.bias",
              f"critic.{2 * len(hidden)}.weight"):
        a_, b_ = got[k].reshape(-1).astype(np.float64), grads["bf16"][0][k].reshape(-1).astype(np.float64)
        assert cos(a_, b_) > 0.9999, (k, cos(a_, b_))


# ------------------------------------------------------------------------------------------ whole iteration
class _Space:
    def __init__(self, shape):
        self.shape = shape


class _StreamEnv:
    """A plain vectorised env (``envs.step()``, no fused step) that replays recorded observations / rewards / dones: device
    trainer and CPU oracle see identical inputs, the comparison is about the policy, GAE and the update."""

    def __init__(self, N, D, A, steps, device, seed=11):
        rs = np.random.RandomState(seed)
        self.num_envs, self.device, self.t = N, device, 0
        self.single_observation_space = {"policy": _Space((D,))}
        self.single_action_space = _Space((A,))
        self.obs = torch.from_numpy(rs.standard_normal((steps + 1, N, D)).astype(np.float32) * 1.5 + 0.2).to(device)
        self.rew = torch.from_numpy(rs.standard_normal((steps, N)).astype(np.float32)).to(device)
        self.done = torch.from_numpy((rs.uniform(size=(steps, N)) < 0.02).astype(np.float32)).to(device)

    @property
    def unwrapped(self):
        return self

    def reset(self):
        self.t = 0
        return {"policy": self.obs[0]}, {}

    def step(self, action):
        assert action.shape[-1] == self.single_action_space.shape[0]
        t = self.t
        self.t += 1
        return ({"policy": self.obs[t + 1]}, self.rew[t], self.done[t], torch.zeros_like(self.done[t], dtype=torch.bool), {})


TIGHT = dict(values=8e-6, logprobs=1.6e-5 * 19 / 12, advantages=1e-5, returns=1e-5, params=1.2e-5, actions=1e-5)


def _flip_proof(trainer, orc, tight_bar):
    """test_gpu_parity_sizes.py's precondition for the looser parameter bar, on this iteration's trace: the tight bar held up
    to the step the trajectories part at, a clip-branch flip happened in that step's minibatch, and every flipped sample is
    closer to the boundary than device and oracle disagree about it, that disagreement itself at rounding level"""
    import smoke_impl
    from test_gpu_parity_sizes import PER_SAMPLE_DISAGREEMENT_CAP
    flip = smoke_impl.branch_flip_report(trainer, orc, tight_bar)
    rec = {k: v for k, v in flip.items() if k != "errs"}
    print("branch flip:", rec)
    assert flip["first_step"] is not None, ("the per-step traces do not show the divergence", rec)
    assert flip["err_before"] < tight_bar, rec                                                              # (1)
    assert flip["flipped_surrogate"] + flip["flipped_value"] >= 1, ("no clip-branch disagreement", rec)      # (2)
    disagreement = max(flip["max_device_oracle_ratio_diff"] if flip["flipped_surrogate"] else 0.0,
                       flip["max_device_oracle_value_diff"] if flip["flipped_value"] else 0.0)
    assert flip["max_margin_of_flipped"] <= disagreement < PER_SAMPLE_DISAGREEMENT_CAP, rec                 # (3)
    return rec


def _resync_oracle_params(trainer, orc):
    """after a proven flip: the oracle network continues from the device's parameters (its Adam moments stay its own), so
    the next rollout is compared under equal parameters again"""
    import smoke_impl
    flat = smoke_impl.logical_params(trainer.agent, trainer.agent.flat)
    off = 0
    with torch.no_grad():
        for p in orc.agent.parameters():          # the registration order of logical_params (smoke_impl.compare relies on it)
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
    assert off == flat.numel()


@pytest.mark.parametrize("minibatch", [16384, 2048])
def test_ppo_trainer_wide_plain_env_vs_oracle(minibatch):
    """PPOTrainer on a plain env with 69-d observations and 19 actions (4096 envs x 24 steps, reference MLP), two iterations
    of two epochs, device noise and permutations recorded and replayed by PPOOracle, parameters traced after every optimiser
    step on both sides.  Bars of test_gpu_parity_sizes.py (log-probs: its bar times 19 / 12, a log-prob sums the action
    dimensions); the parameters get its post-flip bar (4e-4) only through its branch-flip proof, iteration by iteration.
    Once an iteration has parted at a proven flip (2048 rows: one surrogate sample at step 75 of 96 of the first iteration,
    2.3e-6 from the clip boundary), the oracle network continues from the device's parameters, so the next iteration is
    again held to every tight bar but the parameters' (post-flip bar: the Adam moments of the two sides differ)."""
    from cat_envs.tasks.locomotion.velocity.config.solo12.agents.clean_rl_ppo_cfg import Solo12FlatPPORunnerCfg as Cfg
    from cat_envs.tasks.utils.cleanrl.ppo import PPOTrainer
    from test_gpu_parity_sizes import PARAMS_BAR_AFTER_A_BRANCH_FLIP
    import smoke_impl
    N, T, D, A, hidden, epochs, iters = 4096, 24, 69, 19, (512, 256, 128), 2, 2
    cfg = Cfg()
    cfg.num_steps, cfg.minibatch_size, cfg.updates_epochs, cfg.num_iterations = T, minibatch, epochs, iters
    cfg.hidden, cfg.save_interval = hidden, 10 ** 9
    env = _StreamEnv(N, D, A, T * iters, "cuda")
    torch.manual_seed(42)
    trainer = PPOTrainer(env, cfg)
    assert trainer.sink is None and trainer.A == A
    sd = {k: v.detach().cpu().clone() for k, v in trainer.agent.state_dict().items()}
    ag = PO.AgentOracle(D, A, hidden)
    ag.load({k: v for k, v in sd.items() if not k.startswith(("obs_rms", "value_rms"))})
    ocfg = {k: getattr(cfg, k) for k in PO.PPOOracle.DEFAULT_CFG}
    orc = PO.PPOOracle(_StreamEnv(N, D, A, T * iters, "cpu"), N, D, A, cfg=ocfg, hidden=hidden, agent=ag)
    trainer.trace_params, orc.trace = True, True
    flipped = False
    for it in range(iters):
        trainer.record_noise = True
        trainer.run_iteration(log=False)
        torch.cuda.synchronize()
        eps, perms = trainer.noise_rec.cpu().numpy().copy(), trainer.perm_rec.cpu().numpy().copy()
        acts = trainer.actions.cpu()
        out = orc.run_iteration(eps_fn=lambda s: torch.from_numpy(eps[s]), perm_fn=lambda e: torch.from_numpy(perms[e]),
                                actions_fn=lambda s: acts[s])
        rep = smoke_impl.compare(trainer, orc, out, check=False)
        print(f"iteration {it + 1}:", rep)
        assert rep["rewards"] == 0.0 and rep["dones"] == 0.0, rep
        for k in ("values", "logprobs", "actions", "advantages", "returns"):
            assert rep[k] < TIGHT[k], (it, k, rep[k], TIGHT[k], rep)
        if flipped:
            assert rep["params"] < PARAMS_BAR_AFTER_A_BRANCH_FLIP, (it, rep)
        elif rep["params"] >= TIGHT["params"]:
            _flip_proof(trainer, orc, TIGHT["params"])
            assert rep["params"] < PARAMS_BAR_AFTER_A_BRANCH_FLIP, (it, rep)
            flipped = True
        if flipped and it + 1 < iters:
            _resync_oracle_params(trainer, orc)


# ------------------------------------------------------------------------------------------ export
def test_export_wide_checkpoint_matches_agent_forward(tmp_path):
    from cat_envs.tasks.utils.cleanrl import export as EX
    from cat_envs.tasks.utils.cleanrl.ppo import Agent
    from test_export import _run_onnx
    D, A, hidden = 69, 19, (512, 256, 128)
    env = _StreamEnv(96, D, A, 1, "cpu")
    torch.manual_seed(3)
    agent = Agent(env, hidden=hidden).cuda()
    rs = np.random.RandomState(2)
    with torch.no_grad():
        agent.obs_rms(torch.from_numpy(rs.standard_normal((256, D)).astype(np.float32) * 2 + 1).cuda())
        agent.actor_mean[-1].weight.add_(torch.from_numpy(rs.standard_normal((A, hidden[-1])).astype(np.float32) * 0.05).cuda())
    x = rs.standard_normal((96, D)).astype(np.float32)
    with torch.no_grad():
        want = agent(torch.from_numpy(x).cuda()).cpu().numpy()
    assert want.shape == (96, A)
    sd = {k: v.detach().cpu() for k, v in agent.state_dict().items()}
    jit = torch.jit.load(EX.export_policy_as_jit(sd, str(tmp_path / "policy.pt")))
    with torch.no_grad():
        np.testing.assert_allclose(jit(torch.from_numpy(x)).numpy(), want, rtol=1e-5, atol=1e-6)
    got, ops, shp = _run_onnx(open(EX.export_policy_as_onnx(sd, str(tmp_path / "policy.onnx")), "rb").read(), x)
    assert shp == [[[1], [D]], [[1], [A]]]
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
