"""Shared by tests/test_env_step_ref.py (CPU), tests/test_gpu_env_step.py and tests/env_step_cases.py (GPU): ONE env step
of the fused rollout family (csrc/rollout.hip, rollout_post.h, step_merge.h) and of its unfused counterparts restated on plain
arrays - no simulator stream, no cat_envs objects - with the statements of the reference's cat/cat_env.py:92-121 and
cat/constraint_manager.py:39-82,190-229:

    env_case(N, A, D, widths, kinds, **options)   host arrays of a three-step sequence (first_call = 1, two EMA steps)
    eval_terms(case, x)                           one value per descriptor kind, through oracle/cat_oracle.py's own functions
    step_ref(case, state, t)                      counters, terminations, raw reward, action shift, CaT step, episode
                                                  statistics, manager reset + log, zeroing, planes, normaliser, record
    compare_step(...)                             what tests compare, with messages that say WHERE: env, 16-env tile of the
                                                  pre kernel and 32-env tile of the post kernel; column, term, 16-column group
                                                  of the fold kernel
    assert_case_is_live(case, ref)                the non-vacuity conditions, on the reference alone

Bit for bit: counters, masks, rewards, actions, cstr, column maxima, running maxima, probabilities, dones, planes, episode
sums, the normaliser count.  Inside a bar: the record's fp64 sums (stat_refs.moment_sums64's own bound), the normaliser state
(RMS_RTOL / RMS_ATOL of the float64 two-pass state), the reset log (1e-6 / 1e-9: its mean is a sum in an unspecified
order)."""
import functools

import numpy as np

import stat_refs as R
from oracle import cat_oracle as CO

F32 = np.float32

# catppo_term_kind (include/catppo.h)
ABS_LIMIT, ABS_DIFF_LIMIT, ABS_DIFF_LIMIT_GATE_CMDY, GREATER, CONTACT_ANY, NORM2_LIMIT, AIR_TIME, N_FOOT_CONTACT, \
    ACTION_RATE, FORCE_LIMIT, LIMIT_MINUS, ABS_LIMIT_GATE_CMDNORM_LT = range(12)
PER_ID = (ABS_LIMIT, ABS_DIFF_LIMIT, ABS_DIFF_LIMIT_GATE_CMDY, AIR_TIME, ACTION_RATE, FORCE_LIMIT, ABS_LIMIT_GATE_CMDNORM_LT)
TERM_MAX_IDS, MAX_TERMS = 32, 16
PRE_ROWS, POST_ROWS, FOLD_COLS = 16, 32, 16       # envs per tile of rollout_pre / rollout_post, columns per fold workgroup
TAU, MIN_P, MAX_LEN, STEPS = 0.95, 0.02, 20, 3
LOG_RTOL, LOG_ATOL = 1e-6, 1e-9
J, JY_LD = 32, 35                                 # columns of the joint-like tensors; leading dimension of the secondary one
STEP_DT = 0.02

ALL_KINDS = [(ABS_LIMIT, 12), (ABS_DIFF_LIMIT, 12), (ABS_DIFF_LIMIT_GATE_CMDY, 7), (GREATER, 1), (CONTACT_ANY, 1),
             (NORM2_LIMIT, 1), (AIR_TIME, 9), (N_FOOT_CONTACT, 1), (ACTION_RATE, 12), (FORCE_LIMIT, 4), (LIMIT_MINUS, 1),
             (ABS_LIMIT_GATE_CMDNORM_LT, 9)]                                                     # K = 70
SIX_KINDS = [(ABS_LIMIT, 12), (ACTION_RATE, 12), (CONTACT_ANY, 1), (FORCE_LIMIT, 4), (NORM2_LIMIT, 1), (AIR_TIME, 4)]   # K = 34
SIXTEEN = ALL_KINDS + [(ABS_LIMIT, 5), (ABS_DIFF_LIMIT, 3), (AIR_TIME, 2), (ABS_LIMIT_GATE_CMDNORM_LT, 1)]  # K = 81


def widths_for(K, n):
    """n widths in [1, 32] that sum to K, as uneven as that allows: 32, 1, 31, 2, ... pulled towards K one column at a time"""
    w = [(32 - i // 2) if i % 2 == 0 else (1 + i // 2) for i in range(n)]
    assert n <= K <= 32 * n
    while sum(w) > K:
        w[int(np.argmax(w))] -= 1
    while sum(w) < K:
        w[int(np.argmin(w))] += 1
    return w


def kinds_for(widths, A, B):
    """a kind per width: width 1 cycles through the five single-column kinds, wider terms through the per-id kinds (the
    force limit only where the width fits the body count, the action rate only where it fits the action width)"""
    single = [GREATER, CONTACT_ANY, NORM2_LIMIT, N_FOOT_CONTACT, LIMIT_MINUS]
    wide = [ABS_LIMIT, ABS_DIFF_LIMIT, ABS_DIFF_LIMIT_GATE_CMDY, AIR_TIME, ACTION_RATE, FORCE_LIMIT, ABS_LIMIT_GATE_CMDNORM_LT]
    out, si, wi = [], 0, 0
    for i, w in enumerate(widths):
        if w == 1 and i > 0:
            out.append(single[si % 5])
            si += 1
            continue
        while True:
            k = wide[wi % 7]
            wi += 1
            if (k == FORCE_LIMIT and w > B) or (k == ACTION_RATE and w > A):
                continue
            out.append(k)
            break
    return out


# ====================================================================================================== the case builder
def _layout(D, H, B, row_floats):
    fields, off = {}, 0
    for name, w in (("jx", J), ("jv", J), ("jz", J), ("grav", 3), ("root", 3), ("cmd", 3), ("air", J), ("fc", J),
                    ("forces", H * B * 3), ("reward", 1), ("hard", 1), ("obs", D + 3 if D else 0)):
        fields[name] = (off, w)
        off += w
    F = (off + 3) // 4 * 4
    if row_floats:
        assert row_floats >= F and row_floats % 4 == 0
        F = row_floats
    return fields, F


def _tile_plan(N):
    """(first-tile env, interior env or None, last env, quiet 32-env tile or None): where resets are planted"""
    n_tiles = -(-N // POST_ROWS)
    quiet = 1 if N >= 96 else None
    interior = None
    if n_tiles >= 4:
        interior = 2 * POST_ROWS + 5
    elif n_tiles == 3 and quiet is None:
        interior = POST_ROWS + 5
    return interior, quiet


@functools.lru_cache(maxsize=3)
def env_case(N, A, D, widths, kinds, family="spread", H=3, B=5, stride=None, row_floats=0, nan_inf=False, last_step=None,
             seed=0):
    """Host arrays of STEPS env steps.  widths / kinds: tuples.  stride: None - raw reward and hard-reset flag live in the
    state block (stride = row floats, as the product's simulator views); 1 / 3 - arrays of their own.  last_step: None |
    'none' (no env resets in the last step) | 'all' (every env does).  The state block of step t is steps[t]['block']
    (N, F) fp32; every term input is a column range of it except the secondary joint tensor `jy` (N, JY_LD; pad NaN) and the
    action history."""
    widths, kinds = list(widths), list(kinds)
    nt, K = len(widths), int(sum(widths))
    rs = np.random.RandomState(31 * N + 7 * K + D + 1000 * seed)
    fields, F = _layout(D, H, B, row_floats)
    # ---- descriptor table: non-contiguous, unsorted id lists
    terms = []
    joint_x = ("jx", "jv", "jz")
    for t, (w, k) in enumerate(zip(widths, kinds)):
        per_id = k in PER_ID
        assert (per_id or w == 1) and 1 <= w <= TERM_MAX_IDS
        d = dict(kind=k, width=w, limit=0.0, aux=0.0, x=None, y=None, ids=[])
        if k in (ABS_LIMIT, ABS_DIFF_LIMIT, ABS_DIFF_LIMIT_GATE_CMDY, ABS_LIMIT_GATE_CMDNORM_LT):
            d["x"], d["ids"] = joint_x[t % 3], rs.permutation(J)[:w].tolist()
            d["limit"] = float(rs.uniform(0.9, 1.4))
            if k in (ABS_DIFF_LIMIT, ABS_DIFF_LIMIT_GATE_CMDY):
                d["y"] = "jy"
            if k == ABS_DIFF_LIMIT_GATE_CMDY:
                d["aux"] = 0.3
            if k == ABS_LIMIT_GATE_CMDNORM_LT:
                d["aux"] = 0.8
        elif k == GREATER:
            d["x"], d["ids"], d["limit"] = "grav", [2], 0.4
        elif k == LIMIT_MINUS:
            d["x"], d["ids"], d["limit"] = "root", [1], 0.2
        elif k == NORM2_LIMIT:
            d["x"], d["limit"] = "grav", 0.9
        elif k == CONTACT_ANY:
            d["ids"], d["limit"] = rs.permutation(B)[:min(3, B)].tolist(), 1.0
        elif k == N_FOOT_CONTACT:
            d["ids"], d["limit"], d["aux"] = rs.permutation(B)[:min(4, B)].tolist(), 2.0, 0.5
        elif k == FORCE_LIMIT:
            assert w <= B
            d["ids"], d["limit"] = rs.permutation(B)[:w].tolist(), 25.0
        elif k == AIR_TIME:
            d["x"], d["y"], d["ids"], d["limit"], d["aux"] = "air", "fc", rs.permutation(J)[:w].tolist(), 0.25, 0.4
        elif k == ACTION_RATE:
            assert w <= A
            d["x"], d["y"], d["ids"], d["limit"], d["aux"] = "action", "prev_action", rs.permutation(A)[:w].tolist(), 60.0, STEP_DT
        terms.append(d)
    max_p = [1.0 if t == 1 else float(rs.uniform(0.05, 0.9)) for t in range(nt)]
    off = np.concatenate([[0], np.cumsum(widths)]).astype(int)
    # ---- resets: chosen envs, a quiet 32-env tile
    interior, quiet = _tile_plan(N)
    in_quiet = np.zeros(N, bool)
    if quiet is not None:
        in_quiet[quiet * POST_ROWS:(quiet + 1) * POST_ROWS] = True
    ep_len0 = rs.randint(0, MAX_LEN - STEPS - 1, N).astype(np.int64)           # no time-out by chance
    hard = (rs.rand(STEPS, N) < 0.04) & ~in_quiet
    chosen = [e for e in (0, interior, N - 1) if e is not None]
    for t in range(STEPS):
        for e in chosen:
            hard[t, min(N - 1, e + t) if e != N - 1 else max(0, N - 1 - t)] = True
    # time-outs at step t on envs next to the chosen ones (some coincide with a hard reset when N is tiny)
    for t in range(STEPS):
        for e in chosen:
            i = (e + 3 + t) if e != N - 1 else (N - 4 - t)
            if 0 <= i < N and not in_quiet[i]:
                ep_len0[i] = MAX_LEN - 1 - t
                hard[:, i] = False                                               # a time-out that is no hard reset
    if last_step == "none":
        hard[STEPS - 1] = False
        ep_len0[ep_len0 == MAX_LEN - STEPS] = 0
    elif last_step == "all":
        hard[STEPS - 1] = True
    # ---- normaliser inputs: the two families of stat_refs.rms_case, from its non-default state
    rms0, batches = (R.rms_case(D, N, D + 3, family) if D else (None, None))
    # ---- static tensors and the per-step state blocks
    jy = np.full((N, JY_LD), np.nan, F32)
    jy[:, :J] = (rs.standard_normal((N, J)) * 0.05).astype(F32)
    never = None                                      # (tensor, column) whose constraint never turns positive
    if K >= 2 and terms[0]["kind"] in (ABS_LIMIT, ABS_DIFF_LIMIT):
        never = (terms[0]["x"], terms[0]["ids"][0])
    steps = []
    for t in range(STEPS):
        blk = np.zeros((N, F), F32)

        def put(name, a):
            o, w = fields[name]
            blk[:, o:o + w] = a
        scale = F32(1.0 + 0.4 * np.sin(1.3 * t))      # the running maxima grow and decay
        for name in joint_x:
            put(name, (rs.standard_normal((N, J)) * scale).astype(F32))
        g = rs.standard_normal((N, 3))
        put("grav", (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32))
        put("root", (rs.standard_normal((N, 3)) * 0.1 + 0.25).astype(F32))
        cmd = np.stack([rs.uniform(-0.3, 1.0, N), rs.uniform(-0.7, 0.7, N), rs.uniform(-0.78, 0.78, N)], 1)
        cmd[rs.rand(N) < 0.3] *= 0.05
        put("cmd", cmd.astype(F32))
        put("air", rs.uniform(0, 0.5, (N, J)).astype(F32))
        put("fc", (rs.rand(N, J) < 0.3).astype(F32))
        f = np.abs(rs.standard_normal((N, H, B, 3))) * 20.0
        f[rs.rand(N, H, B) > 0.35] = 0.0
        put("forces", f.reshape(N, -1).astype(F32))
        # several constraint values exactly 0: |x| == limit / x - y == limit on planted (env, id) pairs
        for d in terms:
            if d["kind"] in (ABS_LIMIT, ABS_DIFF_LIMIT) and N >= 4:
                o, _ = fields[d["x"]]
                envs = rs.choice(N, max(1, N // 16), replace=False)
                lim = F32(d["limit"])
                if d["kind"] == ABS_LIMIT:
                    blk[envs, o + d["ids"][-1]] = lim * F32(rs.choice([-1.0, 1.0]))
                else:
                    jy[envs, d["ids"][-1]] = F32(0.0)                           # (jy is static: the same pairs every step)
                    blk[envs, o + d["ids"][-1]] = lim
        if never is not None:
            o, _ = fields[never[0]]
            blk[:, o + never[1]] = (rs.uniform(-0.05, 0.05, N)).astype(F32)
        if nan_inf and t == 1:
            o, _ = fields[terms[0]["x"]]
            blk[N // 2, o + terms[0]["ids"][1]] = np.nan
            blk[N // 3, o + terms[0]["ids"][2]] = np.inf
        raw = rs.uniform(-0.4, 1.5, N).astype(F32)                               # raw rewards include negative ones
        st = {"action_in": rs.standard_normal((N, A)).astype(F32)}
        if stride is None:
            put("reward", raw[:, None])
            put("hard", hard[t].astype(F32)[:, None])
        else:
            for name, v in (("reward_arr", raw), ("hard_arr", hard[t].astype(F32))):
                a = np.full(N * stride, np.nan, F32)
                a[::stride] = v
                st[name] = a
        if D:
            put("obs", batches[t])
        st["block"] = blk
        steps.append(st)
    log0 = rs.uniform(0.1, 1.0, 2 * nt).astype(F32)
    return dict(N=N, A=A, D=D, K=K, nt=nt, widths=widths, kinds=kinds, off=off, terms=terms, max_p=max_p, fields=fields, F=F,
                H=H, B=B, stride=stride, jy=jy, ep_len0=ep_len0, action0=rs.standard_normal((N, A)).astype(F32),
                prev_action0=rs.standard_normal((N, A)).astype(F32), log0=log0, rms0=rms0, steps=steps, family=family,
                never=never, tag=f"N={N} A={A} D={D} K={K} terms={nt}")


def field(case, blk, name):
    o, w = case["fields"][name]
    return blk[:, o:o + w]


def obs_of(case, t):
    return field(case, case["steps"][t]["block"], "obs")[:, :case["D"]]


def raw_reward_of(case, t):
    st = case["steps"][t]
    return field(case, st["block"], "reward")[:, 0] if case["stride"] is None else st["reward_arr"][::case["stride"]]


def hard_of(case, t):
    st = case["steps"][t]
    return field(case, st["block"], "hard")[:, 0] if case["stride"] is None else st["hard_arr"][::case["stride"]]


# ====================================================================================================== term evaluation
def eval_terms(case, blk, action, prev_action):
    """cstr (N, K): every descriptor through the function of oracle/cat_oracle.py that states its kind"""
    N, H, B = case["N"], case["H"], case["B"]
    s = {"command": field(case, blk, "cmd"), "net_forces_w_history": field(case, blk, "forces").reshape(N, H, B, 3)}

    def tensor(name):
        if name == "jy":
            return case["jy"]
        if name == "action":
            return action
        if name == "prev_action":
            return prev_action
        return field(case, blk, name)
    cols = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for d in case["terms"]:
            k, ids, lim, aux = d["kind"], d["ids"], d["limit"], d["aux"]
            x = tensor(d["x"]) if d["x"] else None
            y = tensor(d["y"]) if d["y"] else None
            if k == ABS_LIMIT:
                c = CO.joint_position({"joint_pos": x}, lim, ids)
            elif k == ABS_DIFF_LIMIT:
                c = CO.joint_range({"joint_pos": x, "default_joint_pos": y}, lim, ids)
            elif k == ABS_DIFF_LIMIT_GATE_CMDY:
                c = CO.joint_position_when_moving_forward({**s, "joint_pos": x, "default_joint_pos": y}, lim, aux, ids)
            elif k == GREATER:                      # (the named term reads column 2: hand it the descriptor's column there)
                c = CO.upsidedown({"projected_gravity_b": x[:, [ids[0]] * 3]}, lim)
            elif k == CONTACT_ANY:
                assert lim == 1.0                   # the named term's threshold
                c = CO.contact(s, ids)
            elif k == NORM2_LIMIT:
                c = CO.base_orientation({"projected_gravity_b": x}, lim)
            elif k == AIR_TIME:
                c = CO.air_time({**s, "first_contact": y, "last_air_time": x}, lim, aux, ids)
            elif k == N_FOOT_CONTACT:
                c = CO.n_foot_contact(s, int(lim), aux, ids)
            elif k == ACTION_RATE:
                c = CO.action_rate({"action": x, "prev_action": y, "step_dt": aux}, lim, ids)
            elif k == FORCE_LIMIT:
                c = CO.foot_contact_force(s, lim, ids)
            elif k == LIMIT_MINUS:
                c = CO.min_base_height({"root_pos_w": x[:, [ids[0]] * 3]}, lim)
            elif k == ABS_LIMIT_GATE_CMDNORM_LT:
                c = CO.no_move({**s, "joint_vel": x}, aux, lim, ids)
            else:
                raise ValueError(k)
            c = CO._as_2d_f32(c)
            assert c.shape == (N, d["width"]), (k, c.shape)
            cols.append(c)
    return np.ascontiguousarray(np.concatenate(cols, 1), F32)


# ====================================================================================================== one env step
def new_state(case, extra_rows=0):
    """what an env carries from step to step.  extra_rows: pseudo-envs behind the real ones that carry the column maxima of
    other ranks' exchange records into the CaT oracle's column maximum (MAX is exact and order independent)"""
    names = [f"t{i}" for i in range(case["nt"])]
    st = dict(ep_len=case["ep_len0"].copy(), action=case["action0"].copy(), prev_action=case["prev_action0"].copy(),
              mgr=CO.ConstraintManagerOracle(names, case["N"] + extra_rows, tau=TAU, min_p=MIN_P), names=names,
              log=case["log0"].copy(), rms=None)
    if case["D"]:
        st["rms"] = tuple(np.asarray(v, np.float64) for v in case["rms0"])
    return st


def reset_log(viol, prob, L, ids):
    """ConstraintManager.reset's log (constraint_manager.py:190-211): per term the fp32 quotients sum / length of the envs
    that reset, averaged (in float64 here: the order of the mean is the implementation's), violation x 100"""
    out = np.zeros(2 * viol.shape[0], F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        Lf = np.asarray(L)[ids].astype(F32)
        for t in range(viol.shape[0]):
            out[2 * t] = CO._torch_like_mean((viol[t][ids] / Lf).astype(F32)) * F32(100)
            out[2 * t + 1] = CO._torch_like_mean((prob[t][ids] / Lf).astype(F32))
    return out


def round_plane(x, f16):
    return np.asarray(x, F32).astype(np.float16) if f16 else np.asarray(x, F32)


def step_ref(case, state, t, zero_action=True, f16=False, records=()):
    """env step t on `state` (updated in place) -> every output of the step.  records: [(colmax [K], obs rows (n, D))] of
    OTHER ranks, folded behind the local record in rank order (xchg_records = 1 + len(records))."""
    N, K, D, nt = case["N"], case["K"], case["D"], case["nt"]
    inp = case["steps"][t]
    blk = inp["block"]
    out = {}
    # -- process_action, counters, terminations, raw reward (cat_env.py:62,92-97)
    state["prev_action"], state["action"] = state["action"], inp["action_in"].copy()
    state["ep_len"] = state["ep_len"] + 1
    time_outs = state["ep_len"] >= MAX_LEN
    terminated = hard_of(case, t) > F32(0.5)
    reset = time_outs | terminated
    raw = np.asarray(raw_reward_of(case, t), F32).copy()
    out.update(time_outs=time_outs.astype(np.uint8), terminated=terminated.astype(np.uint8), reset=reset.astype(np.uint8),
               raw_reward=raw, ep_len_pre=state["ep_len"].copy(), action_pre=state["action"].copy(),
               prev_action_pre=state["prev_action"].copy())
    # -- constraint terms, this rank's exchange record
    cstr = eval_terms(case, blk, state["action"], state["prev_action"])
    out["cstr"] = cstr
    with np.errstate(invalid="ignore"):
        out["x_colmax"] = np.maximum(cstr.max(axis=0), F32(1e-6)).astype(F32)
        # -- CaT step (constraint_manager.py:39-82,213-229) through the oracle; other ranks' maxima ride as pseudo-envs
        mgr, names, off = state["mgr"], state["names"], case["off"]
        full = cstr if not records else np.concatenate([cstr] + [np.asarray(r[0], F32)[None] for r in records], 0)
        vals = {nm: full[:, off[i]:off[i + 1]] for i, nm in enumerate(names)}
        prob = mgr.compute(vals, dict(zip(names, case["max_p"])))[:N]
        reward, dones = CO.env_finish(raw, prob, reset)
    out.update(rm=mgr.cat.get_running_maxes()[0].copy(), probs=np.concatenate([mgr.cat.probs[nm] for nm in names], 1)[:N],
               cstr_prob=prob.copy(), reward=reward, dones=dones)
    # -- manager reset of the envs that reset: log, accumulators, episode length, action history
    ids = np.nonzero(reset)[0]
    if len(ids):
        viol = np.stack([mgr.episode_sums[nm][:N] for nm in names])
        eprob = np.stack([mgr.cstr_mean_values[nm][:N] for nm in names])
        L = np.concatenate([state["ep_len"], np.ones(len(records), np.int64)])
        log = mgr.reset(ids, L)
        state["log"] = np.array([log[f"Episode_Constraint_{k}/{nm}"] for nm in names for k in ("violation", "probability")], F32)
        assert np.array_equal(state["log"], reset_log(viol, eprob, state["ep_len"], ids), equal_nan=True)
        out.update(acc_viol=viol, acc_prob=eprob)           # the accumulators in front of the reset
        state["ep_len"] = state["ep_len"].copy()
        state["ep_len"][ids] = 0
        if zero_action:
            state["action"], state["prev_action"] = state["action"].copy(), state["prev_action"].copy()
            state["action"][ids] = 0
            state["prev_action"][ids] = 0
    out.update(log=state["log"].copy(), ep_len=state["ep_len"].copy(), action=state["action"].copy(),
               prev_action=state["prev_action"].copy(),
               ep_viol=np.stack([mgr.episode_sums[nm][:N] for nm in names]),
               ep_prob=np.stack([mgr.cstr_mean_values[nm][:N] for nm in names]))
    # -- rollout-buffer planes (cleanrl/ppo.py:215-216,226)
    out.update(rewards_t=round_plane(reward, f16), dones_t1=round_plane(dones, f16),
               true_dones_t1=round_plane(time_outs.astype(F32), f16))
    # -- observation moments of the record and the normaliser (cleanrl/ppo.py:12-62), float64 two-pass
    if D:
        x = obs_of(case, t)
        (s1, b1), (s2, b2) = R.moment_sums64(x)
        out.update(x_sums=np.concatenate([s1, s2]), x_sums_bar=np.concatenate([b1, b2]))
        rows = [x] + [np.asarray(r[1], F32) for r in records]
        tot1, tot2, bar1, bar2 = s1.copy(), s2.copy(), b1.copy(), b2.copy()
        for r in rows[1:]:                                                     # rank order
            (a1, c1), (a2, c2) = R.moment_sums64(r)
            tot1, tot2, bar1, bar2 = tot1 + a1, tot2 + a2, bar1 + c1, bar2 + c2
        out.update(sums_total=np.concatenate([tot1, tot2]), obs_rows_total=float(sum(r.shape[0] for r in rows)))
        m, v, c = R.rms_update64(*state["rms"], np.concatenate(rows, 0).astype(np.float64))
        state["rms"] = (m, v, float(c))
        out.update(obs_mean=m, obs_var=v, obs_count=float(c))
    return out


def run_ref(case, zero_action=True, f16=False, records=None):
    """the three steps -> list of step_ref outputs.  records: per step, the other ranks' [(colmax, obs rows)]"""
    state = new_state(case, extra_rows=len(records[0]) if records else 0)
    return [step_ref(case, state, t, zero_action, f16, records[t] if records else ()) for t in range(STEPS)]


def other_rank_records(case, seeds=(1, 2), n_rows=(40, 77)):
    """exchange records of two other ranks, built by the reference for other envs: per step [(colmax [K], obs (n, D))]"""
    out = [[] for _ in range(STEPS)]
    for seed, n in zip(seeds, n_rows):
        other = env_case(n, case["A"], case["D"], tuple(case["widths"]), tuple(case["kinds"]), family=case["family"],
                         seed=seed)
        # (the other rank's descriptor limits are its own draw: only its record's shape matters here)
        for t, o in enumerate(run_ref(other)):
            out[t].append((o["x_colmax"] * F32(1.5), obs_of(other, t).copy()))
    return out


# ====================================================================================================== comparisons
def term_of(case, c):
    return int(np.searchsorted(case["off"], c, side="right") - 1)


def env_report(name, got, ref, limit=4):
    """env-indexed output, bit for bit: [] or messages that name the envs, their 16-env tiles of the pre kernel and their
    32-env tiles of the post kernel"""
    msgs = R.bits_report(name, got, ref, row_block=PRE_ROWS, limit=limit)
    if msgs and np.asarray(got).shape == np.asarray(ref).shape:
        bad = np.argwhere(~R._same_bits(got, ref))[:, 0]
        msgs[0] += (f"; envs {sorted(set(bad.tolist()))[:8]}, 16-env pre tiles {sorted(set((bad // PRE_ROWS).tolist()))[:8]}, "
                    f"32-env post tiles {sorted(set((bad // POST_ROWS).tolist()))[:8]}")
    return msgs


def _where_cols(case, bad):
    return (f"columns {bad[:8].tolist()}, terms {sorted(set(term_of(case, c) for c in bad))[:8]}, 16-column fold groups "
            f"{sorted(set((bad // FOLD_COLS).tolist()))[:8]}")


def col_report(case, name, got, ref):
    """column-indexed output (K entries), bit for bit: names the column, its term and its 16-column fold group"""
    msgs = R.bits_report(name, got, ref, col_block=FOLD_COLS)
    if msgs and np.asarray(got).shape == np.asarray(ref).shape:
        msgs[0] += "; " + _where_cols(case, np.nonzero(~R._same_bits(got, ref))[0])
    return msgs


def matrix_report(case, name, got, ref):
    """(N, K) output: env, tiles, column, term"""
    msgs = R.bits_report(name, got, ref, row_block=PRE_ROWS, col_block=FOLD_COLS)
    if msgs and np.asarray(got).shape == np.asarray(ref).shape:
        bad = np.argwhere(~R._same_bits(got, ref))
        msgs[0] += (f"; 32-env post tiles {sorted(set((bad[:, 0] // POST_ROWS).tolist()))[:8]}, "
                    + _where_cols(case, np.unique(bad[:, 1])))
    return msgs


def sums_report(name, got, ref, bar, D):
    """the record's fp64 sums inside moment_sums64's bar: names the observation column and its 16-column fold group"""
    got, ref, bar = (np.asarray(a, np.float64) for a in (got, ref, bar))
    if got.shape != ref.shape:
        return [f"{name}: shape {got.shape}, expected {ref.shape}"], float("inf")
    bad = np.nonzero(~(np.abs(got - ref) <= bar))[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(bar > 0, np.abs(got - ref) / bar, np.where(got == ref, 0.0, np.inf)))) if got.size else 0.0
    if bad.size == 0:
        return [], ratio
    c = bad[0]
    return [f"{name}: {bad.size} of {got.size} sums off; first: {'sum x' if c < D else 'sum x^2'} of observation column {c % D} "
            f"(fold group {c // FOLD_COLS} of the sums): got {got[c]!r}, reference {ref[c]!r}, bar {bar[c]:.3g}"], ratio


def log_report(case, name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    both_nan = np.isnan(got) & np.isnan(ref)
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(~(both_nan | same_inf | (np.abs(got - ref) <= LOG_ATOL + LOG_RTOL * np.abs(ref))))[0]
    if bad.size == 0:
        return []
    return [f"{name}: {bad.size} of {got.size} log values off (rtol {LOG_RTOL:g}, atol {LOG_ATOL:g}); first: "
            f"{'probability' if bad[0] % 2 else 'violation'} of term {bad[0] // 2}: got {got[bad[0]]!r}, reference {ref[bad[0]]!r}"]


PRE_KEYS = ("time_outs", "terminated", "reset", "raw_reward", "ep_len_pre", "action_pre", "prev_action_pre")
POST_ENV_KEYS = ("ep_len", "reward", "action", "prev_action", "cstr_prob", "dones", "rewards_t", "dones_t1", "true_dones_t1")


def compare_step(case, got, ref, tag, ratios=None, skip=()):
    """everything one step wrote (got: plain arrays of the result regions, keys of step_ref) against the reference.
    ratios: dict that receives the largest error / bar per family.  skip: keys this run does not produce."""
    msgs = []
    ratios = {} if ratios is None else ratios

    def note(k, v):
        ratios[k] = max(ratios.get(k, 0.0), float(v))
    for k in PRE_KEYS + POST_ENV_KEYS:
        if k in got and k not in skip:
            msgs += env_report(f"{tag}: {k}", got[k], ref[k])
    for k in ("cstr", "probs"):
        if k in got and k not in skip:
            msgs += matrix_report(case, f"{tag}: {k}", got[k], ref[k])
    for k in ("x_colmax", "rm"):
        if k in got and k not in skip:
            msgs += col_report(case, f"{tag}: {k}", got[k], ref[k])
    for k in ("ep_viol", "ep_prob"):
        if k in got and k not in skip:
            g, r = np.asarray(got[k]), np.asarray(ref[k])
            for t in range(min(g.shape[0], r.shape[0])):
                msgs += env_report(f"{tag}: {k} of term {t}", g[t], r[t], limit=2)
    if "log" in got and "log" not in skip:
        msgs += log_report(case, f"{tag}: log_out", got["log"], ref["log"])
        fin = np.isfinite(ref["log"])
        note("log", R.bar_ratio(np.asarray(got["log"])[fin], ref["log"][fin], LOG_RTOL, LOG_ATOL))
    if case["D"]:
        if "x_sums" in got and "x_sums" not in skip:
            m, ratio = sums_report(f"{tag}: record sums", got["x_sums"], ref["x_sums"], ref["x_sums_bar"], case["D"])
            msgs += m
            note("record_sums", ratio)
        for k in ("obs_mean", "obs_var"):
            if k in got and k not in skip:
                msgs += R.column_report(f"{tag}: {k}", got[k], ref[k], R.RMS_RTOL, R.RMS_ATOL)
                note("normaliser", R.bar_ratio(got[k], ref[k], R.RMS_RTOL, R.RMS_ATOL))
        if "obs_count" in got and "obs_count" not in skip and float(got["obs_count"]) != ref["obs_count"]:
            msgs.append(f"{tag}: obs_count {float(got['obs_count'])}, expected {ref['obs_count']}")
        if "obs_out" in got and "obs_out" not in skip:          # on the PUBLISHED (device) mean / var: unfused fp32 ops
            want = R.normalize32(got["obs_raw"], got["obs_mean32"], got["obs_var32"])
            msgs += R.bits_report(f"{tag}: obs_out", got["obs_out"], want, row_block=POST_ROWS, col_block=R.COL_BLOCK)
    return msgs


# ====================================================================================================== non-vacuity
def live_report(case, ref):
    """[] or the conditions of the issue that this case's reference does not meet (each must hold in at least one step)"""
    N, K = case["N"], case["K"]
    n_tiles = -(-N // POST_ROWS)
    multi = N > PRE_ROWS
    if not multi:
        return []
    seen = {}

    def hit(name, cond):
        seen[name] = seen.get(name, False) or bool(cond)
    for o in ref:
        rs, to, hr = o["reset"].astype(bool), o["time_outs"].astype(bool), o["terminated"].astype(bool)
        tile = np.arange(N) // POST_ROWS
        hit("a reset in the first tile", rs[tile == 0].any())
        hit("a reset in the last (ragged) tile", rs[tile == n_tiles - 1].any())
        if n_tiles >= 4 or (n_tiles == 3 and N < 96):
            hit("a reset in an interior tile", rs[(tile > 0) & (tile < n_tiles - 1)].any())
        if N >= 96:
            hit("a 32-env tile without a reset", any(not rs[tile == k].any() for k in range(n_tiles)))
        hit("a time-out that is no hard reset", (to & ~hr).any())
        hit("a hard reset that is no time-out", (hr & ~to).any())
        if K >= 2:
            with np.errstate(invalid="ignore"):
                raw_max = o["cstr"].max(axis=0)
            hit("a column maximum clamped at 1e-6", (raw_max < 1e-6).any() and (o["x_colmax"] == F32(1e-6)).any())
            hit("a column maximum not clamped", (o["x_colmax"] > F32(1e-6)).any())
        term = np.array([term_of(case, c) for c in range(K)])
        hi = (F32(MIN_P) + np.array([F32(p - MIN_P) for p in case["max_p"]], F32)[term]).astype(F32)
        with np.errstate(invalid="ignore"):
            hit("a probability strictly between min_p and max_p", ((o["probs"] > F32(MIN_P)) & (o["probs"] < hi[None])).any())
            hit("a final reward clipped to 0", ((o["raw_reward"] < 0) & (o["reward"] == 0)).any())
            hit("a positive final reward", (o["reward"] > 0).any())
            hit("several constraint values exactly 0", (o["cstr"] == 0).sum() >= 2 or K < 2)
    return [name for name, ok in seen.items() if not ok]


def assert_case_is_live(case, ref):
    missing = live_report(case, ref)
    assert not missing, f"{case['tag']}: the case is vacuous in: {missing}"


# ====================================================================================================== the GPU table
# (N, A, D, terms): terms = ('w', K, n) widths_for(K, n) with kinds_for | a list of (kind, width)
TABLE = [
    (1, 1, 1, [(ABS_LIMIT, 1)]),
    *[(N, 12, 3, ("w", K, 3)) for N in (15, 16, 17) for K in (32, 33)],
    *[(N, 12, D, ("w", D, 5)) for N in (31, 32, 33) for D in (64, 65)],
    (95, 17, 128, ("w", 96, 5)), (95, 17, 129, ("w", 96, 5)),
    (100, 12, 255, ("w", 255, 16)), (100, 12, 256, ("w", 256, 16)), (100, 12, 257, ("w", 257, 16)),
    (40, 12, 512, ("w", 512, 16)),
    (512, 12, 48, ALL_KINDS), (513, 12, 48, ALL_KINDS),
    (4096, 12, 48, SIXTEEN), (4097, 12, 48, SIXTEEN), (4112, 12, 48, SIXTEEN),
    (16384, 12, 48, SIX_KINDS), (16400, 12, 48, SIX_KINDS), (32784, 12, 48, SIX_KINDS),
    (300, 12, 0, SIX_KINDS),
]
# rows the CATPPO_ROLLOUT_TREE=1 worker runs: 1, 2, 31, 32, 33, 64, 65 and 1024 pre workgroups
TREE_TABLE = [(1, 1, 1, [(ABS_LIMIT, 1)]), (17, 12, 3, ("w", 33, 3)), (16 * 31, 12, 48, SIX_KINDS), (512, 12, 48, ALL_KINDS),
              (513, 12, 48, ALL_KINDS), (1024, 12, 48, SIX_KINDS), (1040, 12, 48, SIX_KINDS), (16400, 12, 48, SIX_KINDS)]
VARIANT_SHAPE = (300, 12, 45, SIX_KINDS)


def table_case(row, index=0, **options):
    N, A, D, terms = row
    if isinstance(terms, tuple):
        widths = widths_for(terms[1], terms[2])
        kinds = kinds_for(widths, A, 5)
    else:
        kinds, widths = [k for k, _ in terms], [w for _, w in terms]
    options.setdefault("family", R.RMS_FAMILIES[index % 2])
    return env_case(N, A, D, tuple(widths), tuple(kinds), **options)


def row_dims(row):
    """{N, K, D, nt} of a table row without building its arrays"""
    N, A, D, terms = row
    widths = widths_for(terms[1], terms[2]) if isinstance(terms, tuple) else [w for _, w in terms]
    return dict(N=N, K=sum(widths), D=D, nt=len(widths))


def carve_bytes(case):
    """workspace bytes rollout_pre / rollout_post carve for this case (256 B of slack per piece for its alignment)"""
    N, K, D, nt = case["N"], case["K"], max(case["D"], 1), case["nt"]
    nblk = min(1024, -(-N // PRE_ROWS))
    ngrp = -(-nblk // 32)
    pre = nblk * K * 4 + nblk * 2 * D * 8 + ngrp * K * 4 + ngrp * 2 * D * 8 + 4 * 256
    post = -(-N // POST_ROWS) * (2 * nt + 1) * 8 + 256
    return max(pre, post)
