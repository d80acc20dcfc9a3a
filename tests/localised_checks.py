"""Shared by tests/test_oracle_bf16.py (CPU) and tests/test_gpu_mlp_localised.py (GPU): the comparisons that localise an
error of the MLP kernels to one row, one 64-row tile or one parameter tensor, and the oracle calls they compare against.
Keeping them here lets the CPU module show, on oracle-level mutations, that exactly the checks the GPU module applies to
the kernels reject a dropped row or a zeroed bias gradient (which the bulk bars of tests/test_gpu_bf16.py accept).

Numbers behind the caps (bf16-operand mode): an fp32 activation that differs in its last bit between two summation orders can
round to the other bf16 neighbour, which moves the outputs of that ROW by up to ~1e-3; every other row agrees to fp32
rounding.  Between the float32- and the float64-accumulating oracle, 0.3-0.6 % of the rows flip on the value, 1.1-1.3 %
on the mean action, 4.7 % in the worst 64-row block (tests/test_oracle_bf16.py re-measures this and holds it under the
caps), so 5 % of all rows and 25 % of a 64-row block leave room for the device's third summation order and still
reject a wrong tile: a 64-row tile computed wrongly is 100 % of its block."""
import numpy as np
import torch

from oracle import ppo_oracle as PO

ROW_CAP, BLOCK_CAP, BLOCK = 0.05, 0.25, 64
FLIP_BAR = 5e-3                    # the existing bf16 bar of tests/test_gpu_bf16.py (absolute, value and action)
CFG = dict(clip_coef=0.2, ent_coef=0.001, vf_coef=2.0, norm_adv=True, clip_vloss=True)


# ------------------------------------------------------------------------------------------------ forward, row by row
def oracle_forward(D, A, hidden, w, x, eps, agent_cls=PO.AgentOracle, **opts):
    """{action, logprob, value} of the oracle on supplied noise; opts: bf16_hidden / accumulate / bf16_stored"""
    ag = agent_cls(D, A, hidden, **opts)
    ag.load(w)
    with torch.no_grad():
        a, lp, _, v = ag.get_action_and_value(torch.from_numpy(x), eps=torch.from_numpy(eps))
    return {"action": a.numpy(), "logprob": lp.numpy(), "value": v.numpy()[:, 0]}


def flipped_rows(got, ref):
    """bool per row: NOT clean, i.e. value, action or log-prob miss the fp32 bars of test_policy_act_vs_oracle_and_golden
    (rtol 1e-5 / atol 2e-5; log-prob atol 1e-4)"""
    def miss(g, r, rtol, atol):
        bad = ~(np.abs(g - r) <= atol + rtol * np.abs(r))          # (a NaN is a miss)
        return bad.reshape(bad.shape[0], -1).any(1)
    return (miss(got["value"], ref["value"], 1e-5, 2e-5) | miss(got["action"], ref["action"], 1e-5, 2e-5) |
            miss(got["logprob"], ref["logprob"], 1e-5, 1e-4))


def row_report(got, ref):
    """flip statistics + the list of violated conditions (empty: the forward passes, row by row)"""
    flipped = flipped_rows(got, ref)
    n = flipped.shape[0]
    worst = max(float(np.abs(got[k] - ref[k]).max()) if np.isfinite(got[k]).all() else float("inf")
                for k in ("value", "action", "logprob"))
    blocks = [(b, flipped[b:b + BLOCK]) for b in range(0, n, BLOCK)]
    shares = [float(f.mean()) for _, f in blocks]
    rep = {"rows": n, "flipped_share": float(flipped.mean()), "worst_block_share": max(shares),
           "last_block_share": shares[-1], "last_block_rows": int(blocks[-1][1].shape[0]), "max_abs_error": worst,
           "median_abs_error_value": float(np.median(np.abs(got["value"] - ref["value"])))}
    bad = []
    if not worst < FLIP_BAR:
        bad.append(f"a flipped row misses the bf16 bar: max |error| {worst:.3g} >= {FLIP_BAR}")
    if rep["flipped_share"] > ROW_CAP:
        bad.append(f"{100 * rep['flipped_share']:.2f} % of the rows flipped > {100 * ROW_CAP:.0f} %")
    for (b, f), s in zip(blocks, shares):
        if s > BLOCK_CAP:
            bad.append(f"rows {b}..{b + f.shape[0] - 1}: {int(f.sum())} of {f.shape[0]} flipped > {100 * BLOCK_CAP:.0f} %")
    return rep, bad


def device_like_forward(D, A, hidden, w, x, eps, k_step):
    """The bf16 mode's forward with the DEVICE's kind of fp32 arithmetic instead of the CPU BLAS's: bf16 operands, an fp32
    accumulator that takes the contraction `k_step` k at a time (each step's partial sum exact, as inside one matrix
    instruction; the smaller the step, the longer the rounding chain), ELU as gemm::elu_f computes it
    (exp2(z log2 e) - 1, absolute error of an ulp of 1 on every negative activation), fp32 head.  Not the kernels' order -
    a third, cruder realisation of the same flips, to show how much room the caps leave."""
    f = np.float32

    def q(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()

    def net(pre):
        h = x
        for i in range(len(hidden) + 1):
            wt, b = w[f"{pre}.{2 * i}.weight"], w[f"{pre}.{2 * i}.bias"]
            if i == len(hidden):
                return (h.astype(np.float64) @ wt.T.astype(np.float64) + b).astype(f)
            hq, wq = q(h).astype(np.float64), q(wt).astype(np.float64)
            acc = np.zeros((x.shape[0], wt.shape[0]), f)
            for k in range(0, hq.shape[1], k_step):
                acc = (acc + hq[:, k:k + k_step] @ wq[:, k:k + k_step].T).astype(f)
            z = (acc + b).astype(f)
            e = (np.exp2((z * f(1.44269504088896340736)).astype(f)).astype(f) - f(1)).astype(f)
            h = np.where(z > 0, z, e)

    mu, v = net("actor_mean"), net("critic")[:, 0]
    logstd = w["actor_logstd"].astype(f)
    sd = np.exp(logstd).astype(f)
    act = (mu + sd * eps).astype(f)
    lp = (-((act - mu) ** 2) / (2 * sd * sd) - logstd - f(PO.HALF_LOG_2PI)).astype(f).sum(1)
    return {"action": act, "logprob": lp, "value": v}


# ------------------------------------------------------------------------------------------------ gradient, tensor by tensor
def minibatch_data(D, A, hidden, Bsz, M, w, seed=6, **logp_opts):
    """the data of test_gpu_kernels.test_ppo_minibatch_grad_vs_autograd_oracle (same draws in the same order); old log-probs =
    the oracle's new ones (options logp_opts) + 0.25 N(0,1)"""
    rs = np.random.RandomState(seed)
    c = dict(obs=rs.standard_normal((Bsz, D)).astype(np.float32),
             act=rs.standard_normal((Bsz, A)).astype(np.float32) * 0.7,
             logp=(rs.standard_normal(Bsz) * 0.5 - 12.0).astype(np.float32),
             adv=rs.standard_normal(Bsz).astype(np.float32) * 2 + 0.3,
             ret=rs.standard_normal(Bsz).astype(np.float32),
             val=rs.standard_normal(Bsz).astype(np.float32),
             inds=rs.permutation(Bsz)[:M].astype(np.int64),
             vmean=np.float32(0.37), vvar=np.float32(2.3))
    ag = PO.AgentOracle(D, A, hidden, **logp_opts)
    ag.load(w)
    with torch.no_grad():
        _, lp0, _, _ = ag.get_action_and_value(torch.from_numpy(c["obs"]), torch.from_numpy(c["act"]))
    rs = np.random.RandomState(7)
    c["logp"] = (lp0.numpy() + rs.standard_normal(Bsz).astype(np.float32) * 0.25).astype(np.float32)
    return c


def oracle_grad(D, A, hidden, w, c, inds=None, agent_cls=PO.AgentOracle, **opts):
    """autograd gradient of the PPO minibatch loss, {state_dict key: array}, and the loss statistics"""
    ag = agent_cls(D, A, hidden, **opts)
    ag.load(w)
    ag.value_rms.mean, ag.value_rms.var = torch.tensor(float(c["vmean"])), torch.tensor(float(c["vvar"]))
    for p in ag.parameters():
        p.requires_grad_(True)
    mb = torch.from_numpy(c["inds"] if inds is None else inds)
    t = lambda k: torch.from_numpy(c[k])[mb]  # noqa: E731
    loss, st = PO.ppo_minibatch_loss(ag, t("obs"), t("act"), t("logp"), t("adv"), t("ret"), t("val"), CFG)
    loss.backward()
    return {k: v.grad.numpy().copy() for k, v in ag.p.items()}, st


def tensor_errors(got, ref):
    """err_k = max |got - ref| / max |ref| per parameter tensor"""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(v.shape) - v).max() / max(float(np.abs(v).max()), 1e-30))
            for k, v in ref.items()}


def _kind(key):
    return key if key == "actor_logstd" else key.split(".")[0] + "." + key.split(".")[2]      # network + weight | bias


def tensor_bars(g32, g64):
    """(noise_k, bar_k) from the two references alone: noise_k = err_k of the float32- against the float64-accumulating
    oracle, bar_k = max(2e-4 [the project's fp32 reassociation bar], 4 noise_k [the device's summation order is a third,
    independent realisation of the same flips], the largest noise among the tensors of the same network and kind [a
    tensor whose own noise sample happens to be tiny])"""
    noise = tensor_errors(g32, g64)
    bars = {k: max(2e-4, 4 * n, max(m for j, m in noise.items() if _kind(j) == _kind(k))) for k, n in noise.items()}
    return noise, bars


def tensors_over_bar(got, g64, bars):
    err = tensor_errors(got, g64)
    return err, [f"{k}: err {err[k]:.3g} > bar {bars[k]:.3g}" for k in g64 if not err[k] <= bars[k]]


# ------------------------------------------------------------------------------------------------ row placement
ROT = 37


def rot(a, r=ROT):
    return np.roll(a, r, axis=0)


def forward_rotation_mismatch(out, out_rot, r=ROT):
    """outputs of the call on rows rotated by r, un-rotated, against the plain call's: names that are not bit-identical"""
    return [k for k in out if not np.array_equal(np.roll(out_rot[k], -r, axis=0), out[k], equal_nan=False)]


def grad_rotation_mismatch(g, g_rot, diag=None, diag_rot=None):
    """every tensor within 2e-4 of its maximum (only the fp32 summation order over the rows changed), diag[:7] rtol 2e-4"""
    err = tensor_errors(g_rot, {k: np.asarray(v, np.float64) for k, v in g.items()})
    bad = [f"{k}: {e:.3g}" for k, e in err.items() if not e <= 2e-4]
    if diag is not None and not np.allclose(diag_rot[:7], diag[:7], rtol=2e-4, atol=0):
        bad.append(f"diag {diag[:7]} vs {diag_rot[:7]}")
    return bad


# ------------------------------------------------------------------------------------------------ seeded errors (oracle level)
class DropsLastRow(PO.AgentOracle):
    """MUTANT: the last row of a batch reaches the outputs but not the parameters - what a backward that masks the ragged
    tile one row short computes (its weight / bias gradient contribution is dropped; the loss values stay right)"""

    def get_action_and_value(self, x, action=None, eps=None):
        assert action is not None or eps is not None      # given actions or supplied noise: the two forms the checks use
        keep = torch.ones(x.shape[0], 1)
        keep[-1] = 0.0
        mean = PO.mlp_forward(x, self.layers("actor_mean"), self.bf16_hidden, self.accumulate, self.bf16_stored)
        mean = mean * keep + mean.detach() * (1 - keep)
        if action is None:
            action = mean + torch.exp(self.p["actor_logstd"].expand_as(mean)) * eps
        logp, ent = PO.gaussian_logp_entropy(mean, self.p["actor_logstd"], action)
        v = self.get_value(x)
        return action, logp, ent, v * keep + v.detach() * (1 - keep)


def zero_one_bias_gradient(g, key="critic.2.bias"):
    """MUTANT: one bias gradient never written (a fold segment left out)"""
    out = dict(g)
    out[key] = np.zeros_like(g[key])
    return out


def forward_with_wrong_tile(ref_bf16, ref_fp32, first_row, share=0.25):
    """MUTANT: rows from first_row on are off by a quarter of the distance to the fp32 network (~1e-3: the size of one
    flip, on every row of a tile) - below the bulk bars of tests/test_gpu_bf16.py (max < 5e-3, mean < 2e-5 over thousands
    of rows)"""
    out = {k: v.copy() for k, v in ref_bf16.items()}
    for k in out:
        out[k][first_row:] += np.float32(share) * (ref_fp32[k][first_row:] - out[k][first_row:])
    return out
