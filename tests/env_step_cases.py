"""Device side of tests/test_gpu_env_step.py: drives the cases of tests/env_step_ref.py through catppo_rollout_pre /
catppo_rollout_post (native.RolloutStep and native.TermDesc filled by hand) and through the unfused calls, every output in a
guarded buffer, and compares with the reference.

Run as a program it is the worker for the two switches a process reads once:

    CATPPO_ROLLOUT_TREE=1 python env_step_cases.py tree OUT.json
    CATPPO_FUSED_FWD_MIN_ROWS=17 CATPPO_FUSED_FWD_MAX_ROWS=4096 CATPPO_STEP16_FWD=0 python env_step_cases.py merge OUT.json

It writes one JSON of results (case -> "ok" or the failure) after every case and stops at the first error that is not an
assertion: nothing more is started on the device after a device error."""
import ctypes as C
import json
import sys
import time
import traceback

import numpy as np
import torch

import env_step_ref as E
import stat_refs as R
from test_gpu_stat_kernels import Guarded, Used

F32 = np.float32
TAIL_KEYS = ("rm", "obs_mean", "obs_var", "obs_count", "log0", "log1")
POISON_BYTES = 128 * 2048 * 8            # what Used.poison leaves behind: rms_moments' fp64 partial rows, 2 MiB from offset 0
FALLBACK = "rollout_post_kernel as a launch of its own"
MERGED = "step_fwd_kernel"


class ByteGuard:
    """n bytes inside a buffer filled with 0xA5 (Guarded's sentinel does not fit a byte): masks and the exchange record"""

    def __init__(self, n, lead=16):
        self.n, self.lo, self.hi = n, lead, lead + n
        self.buf = torch.full((lead + n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.lo:self.hi]
        self.bits = 0xA5

    def raw(self):
        return self.buf.cpu().numpy().copy()

    def of(self, raw):
        return raw[self.lo:self.hi]

    def guard_msgs(self, name, raw, **_):
        return R.guard_report(name, raw, self.bits, self.lo, self.hi)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class Run:
    """the device buffers of one run of a case, and the argument block of the fused step"""

    def __init__(self, ctx, case, f16=False, null=(), zero_action=True, records=None, sim_src=False, obs_out_ld=None,
                 zero_pads=False):
        from cat_envs import native
        self.native, self.ctx, self.case = native, ctx, case
        self.f16, self.null, self.records, self.sim_src = f16, set(null), records, sim_src
        N, A, D, K, nt, Fl = (case[k] for k in ("N", "A", "D", "K", "nt", "F"))
        g = self.g = {}
        g["action"], g["prev_action"] = Guarded(N * A, value=case["action0"]), Guarded(N * A, value=case["prev_action0"])
        g["ep_len"] = Guarded(N, torch.int64, value=case["ep_len0"])
        for k in ("time_outs", "terminated", "reset"):
            g[k] = ByteGuard(N)
        for k in ("reward", "cstr_prob", "dones"):
            g[k] = Guarded(N)
        g["cstr"], g["probs"], g["rm"] = Guarded(N * K), Guarded(N * K), Guarded(K)
        g["ep_viol"], g["ep_prob"] = Guarded(nt * N, value=np.zeros(nt * N)), Guarded(nt * N, value=np.zeros(nt * N))
        g["log0"], g["log1"] = Guarded(2 * nt, value=case["log0"]), Guarded(2 * nt)
        pdt = torch.float16 if f16 else torch.float32
        for k in ("rewards_t", "dones_t1", "true_dones_t1"):
            g[k] = Guarded(N, pdt)
        self.ldo = obs_out_ld or D + 3
        if D:
            g["obs_mean"], g["obs_var"] = Guarded(D, value=case["rms0"][0]), Guarded(D, value=case["rms0"][1])
            g["obs_count"] = Guarded(1, value=[case["rms0"][2]])
            g["obs_out"] = Guarded(N * self.ldo, value=np.zeros(N * self.ldo) if zero_pads else None)
        self.x_bytes, self.x_off = ctx._xchg_layout(K, D)
        g["xchg"] = ByteGuard(self.x_bytes)
        g["sim"] = Guarded(N * Fl)
        # inputs
        self.jy = dev(case["jy"])
        self.blocks = [dev(s["block"]) for s in case["steps"]]
        self.ain = [dev(s["action_in"]) for s in case["steps"]]
        self.rw = [dev(s["reward_arr"]) for s in case["steps"]] if case["stride"] else None
        self.hr = [dev(s["hard_arr"]) for s in case["steps"]] if case["stride"] else None
        self.keep = []
        self._describe()
        self._fill(zero_action)

    def _ptr(self, name, col=0):
        c = self.case
        if name == "jy":
            return self.jy.data_ptr(), E.JY_LD
        if name in ("action", "prev_action"):
            return self.g[name].view.data_ptr(), c["A"]
        return self.g["sim"].view.data_ptr() + 4 * (c["fields"][name][0] + col), c["F"]

    def _describe(self):
        native, c = self.native, self.case
        rows = []
        for d in c["terms"]:
            td = native.TermDesc()
            td.kind, td.width, td.n_ids = d["kind"], d["width"], len(d["ids"])
            for i, v in enumerate(d["ids"]):
                td.ids[i] = int(v)
            td.limit, td.aux = float(d["limit"]), float(d["aux"])
            if d["x"]:
                td.x, td.x_ld = self._ptr(d["x"])
            if d["y"]:
                td.y, td.y_ld = self._ptr(d["y"])
            rows.append(td)
        self.descs = (native.TermDesc * len(rows))(*rows)
        self.off_c = (C.c_int32 * (c["nt"] + 1))(*[int(v) for v in c["off"]])
        self.dp_c = (C.c_float * c["nt"])(*[native.f32(p - E.MIN_P) for p in c["max_p"]])

    def _fill(self, zero_action):
        native, c, g = self.native, self.case, self.g
        N, A, D, K, nt, Fl = (c[k] for k in ("N", "A", "D", "K", "nt", "F"))
        st = self.st = native.RolloutStep()
        p = lambda k: None if k in self.null else g[k].view.data_ptr()        # noqa: E731
        st.N, st.A, st.D, st.K, st.n_terms = N, A, D, K, nt
        st.action, st.prev_action, st.episode_length = p("action"), p("prev_action"), p("ep_len")
        st.max_episode_length = E.MAX_LEN
        st.time_outs, st.terminated, st.reset, st.reward = p("time_outs"), p("terminated"), p("reset"), p("reward")
        st.desc = C.cast(self.descs, C.c_void_p)
        st.forces, st.forces_env_stride = self._ptr("forces")
        st.H, st.B = c["H"], c["B"]
        st.command, st.command_ld = self._ptr("cmd")
        st.cstr = p("cstr")
        st.term_off, st.term_dp = C.cast(self.off_c, C.c_void_p), C.cast(self.dp_c, C.c_void_p)
        st.min_p, st.tau, st.one_minus_tau = native.f32(E.MIN_P), native.f32(E.TAU), native.f32(1.0 - E.TAU)
        st.rm, st.cstr_prob, st.dones = p("rm"), p("cstr_prob"), p("dones")
        st.ep_viol, st.ep_prob, st.probs = p("ep_viol"), p("ep_prob"), p("probs")
        st.zero_action_on_reset = 1 if zero_action else 0
        st.rewards_t, st.dones_t1, st.true_dones_t1 = p("rewards_t"), p("dones_t1"), p("true_dones_t1")
        st.plane_dtype = native.F16 if self.f16 else native.F32
        if D:
            st.obs_raw, st.obs_ld = self._ptr("obs")
            st.obs_mean, st.obs_var, st.obs_count = p("obs_mean"), p("obs_var"), p("obs_count")
            st.obs_eps, st.obs_rows_total = native.f32(R.EPS), float(N)
            st.obs_out, st.obs_out_ld = p("obs_out"), self.ldo
        st.xchg = p("xchg")
        st.sim_state, st.sim_row_bytes = g["sim"].view.data_ptr(), 4 * Fl

    def begin_step(self, t):
        c, st, g = self.case, self.st, self.g
        if self.sim_src:
            st.sim_src = self.blocks[t].data_ptr()
        else:
            st.sim_src = None
            g["sim"].view.copy_(self.blocks[t].reshape(-1))
        st.action_in = self.ain[t].data_ptr()
        st.first_call = 1 if t == 0 else 0
        if c["stride"]:
            st.hard_reset, st.hard_reset_stride = self.hr[t].data_ptr(), c["stride"]
            st.reward_src, st.reward_stride = self.rw[t].data_ptr(), c["stride"]
        else:
            st.hard_reset, st.hard_reset_stride = self._ptr("hard")
            st.reward_src, st.reward_stride = self._ptr("reward")
        prev, out = ("log0", "log1") if t % 2 == 0 else ("log1", "log0")
        st.log_prev = g[prev].view.data_ptr()
        st.log_out = None if "log_out" in self.null else g[out].view.data_ptr()
        return out

    def gather_records(self, t):
        """the local record (as rollout_pre left it) + the other ranks' records of the reference, rank order"""
        c, st = self.case, self.st
        K, D = c["K"], c["D"]
        local = self.g["xchg"].view.cpu().numpy()
        recs = [local]
        for cm, rows in self.records[t]:
            b = np.zeros(self.x_bytes, np.uint8)
            b[:4 * K] = np.asarray(cm, F32).view(np.uint8)
            (s1, _), (s2, _) = R.moment_sums64(rows)
            b[self.x_off:self.x_off + 16 * D] = np.concatenate([s1, s2]).view(np.uint8)
            recs.append(b)
        self.gathered = dev(np.concatenate(recs))
        st.xchg_gathered, st.xchg_records = self.gathered.data_ptr(), len(recs)
        st.obs_rows_total = float(c["N"] + sum(r[1].shape[0] for r in self.records[t]))

    def snap(self, keys):
        return {k: self.g[k].raw() for k in keys if k in self.g}


def run_fused(ctx, case, defer=False, forward=None, **kw):
    """STEPS fused steps -> per step {'pre': raw buffers behind rollout_pre, 'post': behind rollout_post (and the forward),
    'tail': what the tail publishes}, the Run.  defer: False (inline tail) | 1 | 2.  forward: callable(run, t) started behind
    every post call (the policy step of the merged launch); its return value lands in post['fwd']."""
    run = Run(ctx, case, **kw)
    pre_keys = ("action", "prev_action", "ep_len", "time_outs", "terminated", "reset", "reward", "cstr", "xchg")
    post_keys = [k for k in run.g if k not in TAIL_KEYS and k != "sim"]
    steps = []
    ctx.rollout_defer_tail(bool(defer), merge=defer == 2)
    try:
        for t in range(E.STEPS):
            run.begin_step(t)
            ctx.rollout_pre(run.st)
            torch.cuda.synchronize()
            if defer and t > 0:
                steps[-1]["tail"] = run.snap(TAIL_KEYS)
            rec = {"pre": run.snap(pre_keys + (("sim",) if run.sim_src else ()))}
            if run.records:
                run.gather_records(t)
            ctx.rollout_post(run.st)
            if forward is not None:
                rec["fwd"] = forward(run, t)
            torch.cuda.synchronize()
            rec["post"] = run.snap(post_keys)
            if not defer:
                rec["tail"] = run.snap(TAIL_KEYS)
            steps.append(rec)
        if defer:
            ctx.rollout_flush()
            torch.cuda.synchronize()
            steps[-1]["tail"] = run.snap(TAIL_KEYS)
    finally:
        ctx.rollout_defer_tail(False)
    return steps, run


def run_unfused(ctx, case, f16=False):
    """the same steps through env_pre_step + cat_terms + cat_terms_step + cat_reset + rollout_store_ex (and the torch fills of
    the unfused env for the episode length and the action history)"""
    run = Run(ctx, case, f16=f16)
    c, g = case, run.g
    N, A, K, nt, Fl, H, B = (c[k] for k in ("N", "A", "K", "nt", "F", "H", "B"))
    sim = g["sim"].view
    fo = c["fields"]

    def col(name):
        return sim.view(N, Fl)[:, fo[name][0]]
    forces = sim.view(N, Fl)[:, fo["forces"][0]:fo["forces"][0] + H * B * 3].unflatten(1, (H, B, 3))    # env stride = row floats
    command = sim.view(N, Fl)[:, fo["cmd"][0]:fo["cmd"][0] + 3]
    g["cstr2"] = Guarded(N * K)
    keys = [k for k in g if k not in ("sim", "xchg", "obs_mean", "obs_var", "obs_count", "obs_out")]
    steps = []
    for t in range(E.STEPS):
        out = run.begin_step(t)
        prev = "log0" if out == "log1" else "log1"
        hard = run.hr[t][::c["stride"]] if c["stride"] else col("hard")
        rsrc = run.rw[t][::c["stride"]] if c["stride"] else col("reward")
        ctx.env_pre_step(run.ain[t], g["action"].view.view(N, A), g["prev_action"].view.view(N, A), g["ep_len"].view, E.MAX_LEN,
                         hard, rsrc, g["time_outs"].view, g["terminated"].view, g["reset"].view, g["reward"].view)
        torch.cuda.synchronize()
        rec = {"pre": run.snap(("action", "prev_action", "ep_len", "time_outs", "terminated", "reset", "reward"))}
        ctx.cat_terms(run.descs, N, forces, H, B, command, g["cstr2"].view.view(N, K))
        ctx.cat_terms_step(run.descs, forces, H, B, command, g["cstr"].view.view(N, K), run.off_c, run.dp_c, E.MIN_P, E.TAU,
                           t == 0, g["rm"].view, g["cstr_prob"].view, g["ep_viol"].view, g["ep_prob"].view,
                           reward=g["reward"].view, reset_mask=g["reset"].view, dones=g["dones"].view, probs=g["probs"].view)
        ctx.cat_reset(g["ep_viol"].view.view(nt, N), g["ep_prob"].view.view(nt, N), g["ep_len"].view, g["reset"].view,
                      g[out].view, prev=g[prev].view)
        mask = g["reset"].view.bool()
        g["ep_len"].view.masked_fill_(mask, 0)
        g["action"].view.view(N, A)[mask] = 0
        g["prev_action"].view.view(N, A)[mask] = 0
        ctx.rollout_store_ex(g["reward"].view, g["dones"].view, g["time_outs"].view, g["rewards_t"].view, g["dones_t1"].view,
                             g["true_dones_t1"].view)
        torch.cuda.synchronize()
        rec["post"] = run.snap(keys)
        rec["tail"] = rec["post"]
        steps.append(rec)
    return steps, run


# ====================================================================================================== got / checks
def got_of(run, rec, t, unfused=False):
    """plain result arrays (keys of env_step_ref.step_ref) out of the raw buffers of one step"""
    c, g = run.case, run.g
    N, A, D, K, nt = (c[k] for k in ("N", "A", "D", "K", "nt"))
    pre, post, tail = rec["pre"], rec["post"], rec["tail"]
    o = lambda d, k: g[k].of(d[k])          # noqa: E731
    got = {"time_outs": o(pre, "time_outs"), "terminated": o(pre, "terminated"), "reset": o(pre, "reset"),
           "raw_reward": o(pre, "reward"), "ep_len_pre": o(pre, "ep_len"), "action_pre": o(pre, "action").reshape(N, A),
           "prev_action_pre": o(pre, "prev_action").reshape(N, A)}
    if unfused:
        got["cstr"] = o(post, "cstr").reshape(N, K)
        got["cstr_terms_only"] = o(post, "cstr2").reshape(N, K)
    else:
        got["cstr"] = o(pre, "cstr").reshape(N, K)
        xb = o(pre, "xchg")
        got["x_colmax"] = xb[:4 * K].view(F32)
        if D:
            got["x_sums"] = xb[run.x_off:run.x_off + 16 * D].view(np.float64)
    for k in ("ep_len", "reward", "cstr_prob", "rewards_t", "dones_t1", "true_dones_t1"):
        got[k] = o(post, k)
    for k in ("action", "prev_action"):
        got[k] = o(post, k).reshape(N, A)
    for k in ("ep_viol", "ep_prob"):
        got[k] = o(post, k).reshape(nt, N)
    if "dones" not in run.null:
        got["dones"] = o(post, "dones")
    if "probs" not in run.null:
        got["probs"] = o(post, "probs").reshape(N, K)
    got["rm"] = o(tail, "rm")
    if "log_out" not in run.null:
        got["log"] = o(tail, "log1" if t % 2 == 0 else "log0")
    if D and not unfused:
        got.update(obs_mean=o(tail, "obs_mean"), obs_var=o(tail, "obs_var"), obs_count=o(tail, "obs_count")[0],
                   obs_out=o(post, "obs_out").reshape(N, run.ldo)[:, :D], obs_raw=E.obs_of(c, t))
        got["obs_mean32"], got["obs_var32"] = got["obs_mean"], got["obs_var"]
    return got


def guard_msgs(run, steps, tag, pad_bits=None):
    """every guard element of every buffer at every snapshot, and the pad columns of obs_out"""
    c, msgs = run.case, []
    for t, rec in enumerate(steps):
        for part in ("pre", "post", "tail"):
            for k, raw in rec[part].items():
                if k not in run.g:
                    continue
                kw = {}
                if k == "obs_out" and pad_bits is None:
                    kw = dict(rows=c["N"], cols=c["D"], ld=run.ldo)
                msgs += run.g[k].guard_msgs(f"{tag} step {t} behind {part}: {k}", raw, **kw)
                if k == "obs_out" and pad_bits is not None:
                    pad = run.g[k].of(raw).reshape(c["N"], run.ldo)[:, c["D"]:]
                    if (np.ascontiguousarray(pad).view(np.uint32) != pad_bits).any():
                        msgs.append(f"{tag} step {t}: pad columns of obs_out changed")
    return msgs


def check_run(case, ref, steps, run, tag, ratios, unfused=False):
    msgs = []
    for t, rec in enumerate(steps):
        got = got_of(run, rec, t, unfused)
        msgs += E.compare_step(case, got, ref[t], f"{tag} step {t}", ratios)
        if unfused:
            msgs += E.matrix_report(case, f"{tag} step {t}: cstr of cat_terms", got["cstr_terms_only"], ref[t]["cstr"])
    msgs += guard_msgs(run, steps, tag)
    return msgs


def flat_bytes(steps):
    """{step/part/key: bytes} of a run, for the byte-for-byte comparison of two runs"""
    return {f"{t}/{part}/{k}": v.tobytes() for t, rec in enumerate(steps) for part in ("pre", "post", "tail")
            for k, v in rec[part].items()}


def differing(a, b):
    fa, fb = flat_bytes(a), flat_bytes(b)
    return sorted(k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k))


# ====================================================================================================== worker: tree
def tree_case(nat, used, row, index):
    case = E.table_case(row, index)
    ref = E.run_ref(case)
    E.assert_case_is_live(case, ref)
    ratios = {}
    inline, run = run_fused(nat, case)
    msgs = check_run(case, ref, inline, run, f"{case['tag']} tree, inline tail", ratios)
    deferred, run_d = run_fused(nat, case, defer=1)
    msgs += check_run(case, ref, deferred, run_d, f"{case['tag']} tree, deferred tail", ratios)
    assert not msgs, "\n".join(msgs[:30])
    # the in-launch tree writes the record the pending tail still reads: the tail gets no ride, it is flushed in front of
    # the pre launch - the state it publishes is there behind that pre call (check_run took it from exactly there)
    assert not differing(inline, deferred), differing(inline, deferred)
    again, _ = run_fused(used, case, defer=1)
    assert not differing(inline, again), differing(inline, again)
    return ratios


# ====================================================================================================== worker: merge
def merge_case(nat, N, D, hidden, K=64, expect_merged=True):
    from cat_envs import native
    import streams as S
    from oracle import ppo_oracle as PO
    from test_gpu_kernels import flat_params
    A = 12
    widths = E.widths_for(K, 16)
    case = E.env_case(N, A, D, tuple(widths), tuple(E.kinds_for(widths, A, 5)))
    ref = E.run_ref(case)
    shape = native.shape_of(D, A, hidden)
    lay = native.layout_of(shape)
    w = S.agent_weights(3, D, A, hidden)
    ag = PO.AgentOracle(D, A, hidden)
    ag.load(w)
    params = flat_params(native, shape, lay, w)
    nat.mlp_reserve(shape, N)
    rs = np.random.RandomState(N + D)
    eps = rs.standard_normal((E.STEPS, N, A)).astype(F32)
    eps_d = dev(eps)
    tag = f"{case['tag']} hidden={hidden}"

    def forward(run, t):
        out = [Guarded(N * A), Guarded(N), Guarded(N)]
        nat.policy_act(shape, params, run.g["obs_out"].view, N, eps_d[t], out[0].view, out[1].view, out[2].view)
        run.keep.append(out)
        return out

    def arm(defer):
        nat.plan_log(1)
        steps, run = run_fused(nat, case, defer=defer, forward=forward, obs_out_ld=lay.obs_pad, zero_pads=True)
        plan = nat.plan_log(0)
        for rec in steps:
            rec["post"].update({f"fwd{i}": gd.raw() for i, gd in enumerate(rec.pop("fwd"))})
        return steps, run, plan
    merged, run, plan = arm(2)
    if expect_merged:
        assert plan.count(MERGED) == E.STEPS and FALLBACK not in plan, plan
    else:
        assert MERGED not in plan and plan.count(FALLBACK) == E.STEPS, plan
    ratios, msgs = {}, []
    for t, rec in enumerate(merged):
        fw = {k: rec["post"].pop(k) for k in ("fwd0", "fwd1", "fwd2")}
        got = got_of(run, rec, t)
        msgs += E.compare_step(case, got, ref[t], f"{tag} step {t}", ratios)
        gd = run.keep[t]
        for i, (g, name) in enumerate(zip(gd, ("action", "logprob", "value"))):
            msgs += g.guard_msgs(f"{tag} step {t}: forward {name}", fw[f"fwd{i}"])
        with torch.no_grad():
            a, lp, _, v = ag.get_action_and_value(torch.from_numpy(np.ascontiguousarray(got["obs_out"])),
                                                  eps=torch.from_numpy(eps[t]))
        act, logp, val = (g.of(fw[f"fwd{i}"]) for i, g in enumerate(gd))
        for name, x, y, rtol, atol in (("action", act.reshape(N, A), a.numpy(), 1e-5, 2e-5), ("value", val, v.numpy()[:, 0], 1e-5, 2e-5),
                                       ("logprob", logp, lp.numpy(), 1e-5, 1e-4)):
            r = R.bar_ratio(x, y, rtol, atol)
            ratios["forward"] = max(ratios.get("forward", 0.0), r)
            if not r <= 1.0:
                bad = np.argwhere(~(np.abs(x - y) <= atol + rtol * np.abs(y)))
                msgs.append(f"{tag} step {t}: forward {name} over its bar ({r:.3g}), rows {sorted(set(bad[:, 0].tolist()))[:8]}, "
                            f"32-row tiles {sorted(set((bad[:, 0] // 32).tolist()))[:8]}")
        rec["post"].update(fw)
    pad_bits = 0
    msgs += guard_msgs(run, merged, tag, pad_bits=pad_bits)
    assert not msgs, "\n".join(msgs[:30])
    separate, _, plan_s = arm(1)
    assert MERGED not in plan_s, plan_s
    assert not differing(merged, separate), differing(merged, separate)
    return ratios


MERGE_CASES = {f"merge_N{N}_D{D}_L{len(h)}": (lambda nat, N=N, D=D, h=h: merge_case(nat, N, D, h))
               for h in ((256,), (256, 256), (256, 256, 256)) for N in (17, 33, 64, 95) for D in (1, 45, 48, 128)}
MERGE_CASES["fallback_D129"] = lambda nat: merge_case(nat, 33, 129, (256, 256, 256), expect_merged=False)
MERGE_CASES["fallback_K65"] = lambda nat: merge_case(nat, 33, 48, (256, 256, 256), K=65, expect_merged=False)


def main(mode, out):
    from cat_envs import native
    nat = native.Native()
    results = {}
    if mode == "tree":
        used = Used()
        cases = {f"tree_{i}_N{row[0]}": (lambda row=row, i=i: tree_case(nat, used, row, i)) for i, row in enumerate(E.TREE_TABLE)}
    else:
        cases = {k: (lambda f=f: f(nat)) for k, f in MERGE_CASES.items()}
    for name, fn in cases.items():
        t0 = time.time()
        try:
            results[name] = {"status": "ok", "ratios": fn(), "seconds": round(time.time() - t0, 3)}
        except BaseException:                              # noqa: BLE001 - the parent reports it
            results[name] = {"status": traceback.format_exc()[-3000:]}
            if "AssertionError" not in results[name]["status"]:   # a device or library error: nothing more runs
                with open(out, "w") as f:
                    json.dump(results, f)
                sys.exit(1)
        with open(out, "w") as f:
            json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
