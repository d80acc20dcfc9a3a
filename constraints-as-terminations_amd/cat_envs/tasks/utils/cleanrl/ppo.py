"""CleanRL-style PPO for CaT (float dones) on MI355X.

Same entry points as the reference (cleanrl/ppo.py): ``RunningMeanStd``, ``layer_init``,
``Agent(envs)`` with ``get_value / get_action_and_value / forward`` and the 23-key
``state_dict``, and ``PPO(envs, ppo_cfg, run_path)``.  The algorithm is the reference's, step
for step (rollout bookkeeping :201-230, GAE with float dones and a separate time-out mask
:251-277, value normaliser updated twice :287-288, epochs x minibatches with clipped policy /
value losses, global-norm clip, Adam, linear lr anneal :294-354); every tensor operation of it
runs in libcatppo.so (hand-written HIP, see include/catppo.h):

    iteration      catppo_iter_begin                          (iteration counter, lr schedule: device state)
    rollout step   catppo_policy_step                         (ONE launch at 2049-4096 rows - all hidden layers + heads
                                                               per 32-row workgroup - else 3 GEMM launches + head:
                                                               actions/logprobs/values[step]; Philox action noise inside)
                   env.step_into -> catppo_rollout_pre/_post  (simulator state advance, terms, CaT, resets, buffer rows,
                                                               obs normaliser: 3 launches; a foreign env takes the
                                                               unfused calls)
    after rollout  catppo_value, catppo_gae, 2x (catppo_rms_update + catppo_rms_normalize)
    epoch          catppo_ppo_gather_ex                       (keyed on-device permutation, no index array)
    minibatch      catppo_ppo_minibatch_grad_packed  [catppo_allreduce: RCCL SUM of the flat gradient]
                   catppo_clip_adam_dev                       (lr / step count from the device state)
                   single process: both in one call, catppo_ppo_minibatch_step_packed (one launch fewer)
    [KL-adaptive]  catppo_kl_mean [catppo_allreduce] catppo_kl_adaptive_lr   after every epoch, no host sync
The update phase is replayed from a hipGraph (``graph_update``; collectives of an env-sharded run included, with a
reported eager fallback when the capture fails).

There is no host synchronisation inside an iteration (the reference syncs once per
constraint term per env step and once per minibatch); diagnostics accumulate on the device
and are read once per iteration.  Parameters, gradients and Adam moments live in ONE flat
fp32 buffer each, so the gradient exchange of an env-sharded run is a single all-reduce.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn

from cat_envs import native, parallel

DEFAULT_HIDDEN = (512, 256, 128)     # reference Agent (ppo.py:78-95)
#: arithmetic of the hidden-layer GEMMs -> catppo_mlp_shape.mfma_bf16
MLP_PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2}


# ------------------------------------------------------------------------------------------------
class RunningMeanStd(nn.Module):
    """Running mean / variance with Chan's merge (reference ppo.py:12-62); count starts at 1."""

    def __init__(self, shape=(), epsilon=1e-08, device=None):
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(shape, device=device))
        self.register_buffer("running_var", torch.ones(shape, device=device))
        self.register_buffer("count", torch.ones((), device=device))
        self.epsilon = epsilon
        #: torch.distributed group over which batch moments are summed (env-sharded runs)
        self.dist_group = None

    @property
    def dim(self) -> int:
        return max(1, self.running_mean.numel())

    def forward(self, obs: torch.Tensor, update: bool = True) -> torch.Tensor:
        x = obs if obs.dtype in (torch.float32, torch.float16) else obs.float()
        rows = x.reshape(-1, self.dim)
        if rows.stride(-1) != 1:
            rows = rows.contiguous()
        out = torch.empty(rows.shape, device=rows.device)
        self.normalize_into(rows, out, update=update)
        return out.reshape(obs.shape)

    def update(self, x: torch.Tensor):
        rows = x.float().reshape(-1, self.dim)
        self._update_rows(rows if rows.stride(-1) == 1 else rows.contiguous())

    def _update_rows(self, rows: torch.Tensor):
        nat = native.get(rows.device)
        n, d = rows.shape
        group = self.dist_group
        if group is not None and parallel.active(group):
            if not hasattr(self, "_sums"):
                self._sums = torch.zeros(2 * d, dtype=torch.float64, device=rows.device)
                self._n_global = {}
            nat.rms_moments_ex(rows, n, d, rows.stride(0), self._sums)
            parallel.global_moment_sums(self._sums, group)
            # true global row count (shards may differ by one env): exchanged once per batch size, not assumed
            if n not in self._n_global:
                cnt = torch.tensor([float(n)], dtype=torch.float64, device=rows.device)
                parallel.allreduce_sum_(cnt, group)
                self._n_global[n] = float(cnt.item())
            nat.rms_merge(self._sums, self._n_global[n], d, self.running_mean, self.running_var, self.count)
        else:
            nat.rms_update_ex(rows, n, d, rows.stride(0), self.running_mean, self.running_var, self.count)

    def update_normalize_pair(self, rows_a, out_a, rows_b, out_b):
        """``normalize_into(rows_a, out_a)`` followed by ``normalize_into(rows_b, out_b)`` (the value normaliser's two
        updates per iteration, reference ppo.py:287-288) with ONE exchange between ranks: the batch moments of the two
        batches do not depend on each other - only the two Chan merges are sequential - so an env-sharded run sums
        both moment pairs in a single all-reduce (round 5; one collective per iteration instead of two).  Same
        arithmetic, same order, as the two separate calls."""
        group = self.dist_group
        if group is None or not parallel.active(group) or os.environ.get("CATPPO_VRMS_PAIR", "1") == "0":   # (A/B switch)
            self.normalize_into(rows_a, out_a)
            self.normalize_into(rows_b, out_b)
            return
        nat = native.get(rows_a.device)
        (na, d), (nb, db) = rows_a.shape, rows_b.shape
        assert d == db == self.dim
        if not hasattr(self, "_sums_pair"):
            self._sums_pair = torch.zeros(4 * d, dtype=torch.float64, device=rows_a.device)
            self._n_global = getattr(self, "_n_global", {})
        sa, sb = self._sums_pair[:2 * d], self._sums_pair[2 * d:]
        nat.rms_moments_ex(rows_a, na, d, rows_a.stride(0), sa)
        nat.rms_moments_ex(rows_b, nb, d, rows_b.stride(0), sb)
        parallel.global_moment_sums(self._sums_pair, group)
        for n in (na, nb):
            if n not in self._n_global:
                cnt = torch.tensor([float(n)], dtype=torch.float64, device=rows_a.device)
                parallel.allreduce_sum_(cnt, group)
                self._n_global[n] = float(cnt.item())
        nat.rms_merge(sa, self._n_global[na], d, self.running_mean, self.running_var, self.count)
        self.normalize_into(rows_a, out_a, update=False)
        nat.rms_merge(sb, self._n_global[nb], d, self.running_mean, self.running_var, self.count)
        self.normalize_into(rows_b, out_b, update=False)

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        """Chan merge of externally computed batch moments (reference ppo.py:33-45).  Not on the training path -
        ``update()`` fuses the moment pass and this merge on the device - so plain tensor ops, in place."""
        m, v, c = update_mean_var_count_from_moments(self.running_mean, self.running_var, self.count,
                                                     torch.as_tensor(batch_mean, device=self.running_mean.device),
                                                     torch.as_tensor(batch_var, device=self.running_mean.device),
                                                     batch_count)
        self.running_mean.copy_(m)
        self.running_var.copy_(v)
        self.count.copy_(c)

    def normalize_into(self, rows: torch.Tensor, out: torch.Tensor, update: bool = True):
        """rows (n,d) with unit inner stride -> out (n,d') written in place (d' >= d, padding untouched)"""
        if update:
            self._update_rows(rows)
        n, d = rows.shape
        native.get(rows.device).rms_normalize_ex(rows, n, d, rows.stride(0), self.running_mean, self.running_var,
                                                 self.epsilon, out, out.stride(0))


def update_mean_var_count_from_moments(mean, var, count, batch_mean, batch_var, batch_count):
    """(new_mean, new_var, new_count) of Chan's parallel merge, in the reference's operation order
    (ppo.py:48-62): ``M2 = var*count + batch_var*batch_count + delta^2 * count * batch_count / tot``."""
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m2 = var * count + batch_var * batch_count + torch.square(delta) * count * batch_count / tot_count
    return new_mean, m2 / tot_count, tot_count


def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class Agent(nn.Module):
    """Actor / critic MLPs + observation / value normalisers (reference ppo.py:71-123).

    ``critic`` and ``actor_mean`` are ordinary ``nn.Sequential`` stacks, so ``state_dict()``
    has the reference's 23 keys and shapes and loads into / from the reference ``Agent``.  Their
    parameters are *views into one flat fp32 buffer* (``self.flat``) laid out by
    ``catppo_mlp_layout_of`` (first-layer rows padded from D to a multiple of 16); the HIP
    kernels read and update that buffer directly.
    """

    def __init__(self, envs, hidden=DEFAULT_HIDDEN, device=None, mlp_precision: str = "fp32"):
        super().__init__()
        if mlp_precision not in MLP_PRECISIONS:
            raise ValueError(f"mlp_precision must be one of {sorted(MLP_PRECISIONS)}, got {mlp_precision!r}")
        self.mlp_precision = mlp_precision
        obs_shape = envs.unwrapped.single_observation_space["policy"].shape
        act_shape = envs.unwrapped.single_action_space.shape
        self.obs_dim, self.act_dim = int(np.array(obs_shape).prod()), int(np.prod(act_shape))
        self.hidden = tuple(int(h) for h in hidden)
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        device = torch.device(device)
        self.shape = native.shape_of(self.obs_dim, self.act_dim, self.hidden, mfma_bf16=MLP_PRECISIONS[mlp_precision])
        self.layout = native.layout_of(self.shape)

        def mlp(out_dim, out_std):
            dims = [self.obs_dim, *self.hidden]
            layers = []
            for i, o in zip(dims[:-1], dims[1:]):
                layers += [layer_init(nn.Linear(i, o)), nn.ELU()]
            layers.append(layer_init(nn.Linear(dims[-1], out_dim), std=out_std))
            return nn.Sequential(*layers)

        self.critic = mlp(1, 1.0)
        self.actor_mean = mlp(self.act_dim, 0.01)
        self.actor_logstd = nn.Parameter(torch.zeros(1, self.act_dim))
        self.obs_rms = RunningMeanStd(shape=obs_shape)
        self.value_rms = RunningMeanStd(shape=())
        self.flat = None
        self._tie(device)

    # -- flat buffer <-> module parameters ---------------------------------------------------
    def _tie(self, device):
        """move everything to ``device`` and re-point every parameter at its slice of ``flat``"""
        lay, L = self.layout, self.shape.n_hidden
        flat = torch.zeros(lay.n_flat, device=device)
        with torch.no_grad():
            v = flat[lay.off_logstd:lay.off_logstd + self.act_dim].view(1, self.act_dim)
            v.copy_(self.actor_logstd.detach())
            self.actor_logstd = nn.Parameter(v)
            for net, seq in ((0, self.critic), (1, self.actor_mean)):
                for l in range(L + 1):
                    lin = seq[2 * l]
                    out_f, in_f = lin.weight.shape
                    ld = lay.in_dim[l]
                    w = flat[lay.off_w[net][l]:lay.off_w[net][l] + out_f * ld].view(out_f, ld)[:, :in_f]
                    b = flat[lay.off_b[net][l]:lay.off_b[net][l] + out_f]
                    w.copy_(lin.weight.detach())
                    b.copy_(lin.bias.detach())
                    lin.weight, lin.bias = nn.Parameter(w), nn.Parameter(b)
        self.flat = flat
        for rms in (self.obs_rms, self.value_rms):
            for name in ("running_mean", "running_var", "count"):
                setattr(rms, name, getattr(rms, name).to(device))

    def _apply(self, fn, recurse=True):
        probe = fn(torch.zeros(1, device=self.flat.device))
        if probe.device != self.flat.device or probe.dtype != torch.float32:
            if probe.dtype != torch.float32:
                raise TypeError("Agent parameters are fp32 (the HIP kernels compute in fp32)")
            self._tie(probe.device)
        return self

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # copies into the views, i.e. into the flat buffer (never re-assigns parameter storage)
        return super().load_state_dict(state_dict, strict=strict, assign=False)

    @property
    def n_params(self) -> int:
        return int(self.layout.n_params)

    # -- reference API --------------------------------------------------------------------------
    def _padded(self, x: torch.Tensor) -> torch.Tensor:
        x = x.reshape(-1, self.obs_dim)
        if self.layout.obs_pad == self.obs_dim and x.is_contiguous() and x.dtype == torch.float32:
            return x
        xp = torch.zeros(x.shape[0], self.layout.obs_pad, device=x.device)
        xp[:, :self.obs_dim] = x
        return xp

    def get_value(self, x):
        xp = self._padded(x)
        nat = native.get(xp.device)
        nat.mlp_reserve(self.shape, xp.shape[0])
        v = torch.empty(xp.shape[0], device=xp.device)
        nat.value(self.shape, self.flat, xp, xp.shape[0], v)
        return v.unsqueeze(1)

    def get_action_and_value(self, x, action=None, deterministic=False, eps=None):
        """(action, log_prob.sum(1), entropy.sum(1), value (B,1)); ``eps`` optionally supplies the
        N(0,1) noise of ``Normal.sample()`` (otherwise drawn from torch's generator)."""
        xp = self._padded(x)
        n = xp.shape[0]
        nat = native.get(xp.device)
        nat.mlp_reserve(self.shape, n)
        act = torch.empty(n, self.act_dim, device=xp.device)
        logp, val = torch.empty(n, device=xp.device), torch.empty(n, device=xp.device)
        given = None
        if action is not None:
            given = action.reshape(n, self.act_dim).float().contiguous()
        elif not deterministic and eps is None:
            eps = torch.randn(n, self.act_dim, device=xp.device)
        nat.policy_act(self.shape, self.flat, xp, n, None if (given is not None or deterministic) else eps,
                       act, logp, val, given_action=given)
        entropy = (0.5 + 0.5 * math.log(2 * math.pi) + self.actor_logstd.detach()).sum().expand(n)
        return (action if action is not None else act), logp, entropy, val.unsqueeze(1)

    def forward(self, x, deterministic=True):
        action, _, _, _ = self.get_action_and_value(self.obs_rms(x, update=False), deterministic=deterministic)
        return action


# ------------------------------------------------------------------------------------------------
class _JsonlWriter:
    """scalar writer used when tensorboard is not installed (same add_scalar surface)"""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self._f = open(os.path.join(log_dir, "scalars.jsonl"), "a")

    def add_scalar(self, key, value, step):
        import json
        self._f.write(json.dumps({"key": key, "value": float(value), "step": int(step)}) + "\n")
        self._f.flush()


def _make_writer(ppo_cfg, run_path):
    if ppo_cfg.logger == "wandb":
        from rsl_rl.utils.wandb_utils import WandbSummaryWriter
        return WandbSummaryWriter(log_dir=run_path, flush_secs=10, cfg=ppo_cfg.to_dict())
    if ppo_cfg.logger == "tensorboard":
        try:
            from torch.utils.tensorboard import SummaryWriter as TensorboardSummaryWriter
            return TensorboardSummaryWriter(log_dir=run_path)
        except ImportError:
            return _JsonlWriter(run_path)
    raise AssertionError("logger type not found")


class RolloutSink:
    """Where an env's fused step (``step_into``) delivers this rollout step: the rollout-buffer rows
    rewards[step] / dones[step+1] / true_dones[step+1], and the observation normaliser whose statistics are
    updated with the raw next observation and whose output lands in obs[step+1].  Addresses are computed from base
    pointers (no tensor slicing on the per-step host path)."""

    def __init__(self, trainer: "PPOTrainer"):
        t = self.t = trainer
        self.step = 0
        rms = t.agent.obs_rms
        self._rms = (rms.running_mean.data_ptr(), rms.running_var.data_ptr(), rms.count.data_ptr(),
                     native.f32(rms.epsilon))
        isz = t.rewards.element_size()
        self._row = t.N * isz
        self._p_rew, self._p_done, self._p_td = t.rewards.data_ptr(), t.dones.data_ptr(), t.true_dones.data_ptr()
        self._p_obs, self._obs_row = t.obs.data_ptr(), t.N * t.Dp * 4
        self._dtype = native.F16 if t.plane_dtype == torch.float16 else native.F32
        self._struct = None
        #: process group over which the env all-reduces the observation moment sums of the fused step (None: this
        #: rank's rows are the whole batch).  Independent of ``dist_exact``: like the unfused path, whose
        #: ``obs_rms.dist_group`` is always the world, the normaliser sees the GLOBAL batch in every sharded run.
        self.obs_group = rms.dist_group if (rms.dist_group is not None and parallel.active(rms.dist_group)) else None

    def fill(self, st):
        k = self.step
        if st is not self._struct:               # constants of the run: once per argument block
            self._struct = st
            st.plane_dtype = self._dtype
            st.obs_mean, st.obs_var, st.obs_count, st.obs_eps = self._rms
            # the divisor of the moment sums must match what was summed: all ranks' rows only if they are exchanged
            st.obs_rows_total = self.t.n_envs_global if self.obs_group is not None else float(self.t.N)
            st.obs_out_ld = self.t.Dp
        row = self._row
        st.rewards_t = self._p_rew + k * row
        st.dones_t1 = self._p_done + (k + 1) * row
        st.true_dones_t1 = self._p_td + (k + 1) * row
        st.obs_out = self._p_obs + (k + 1) * self._obs_row


class PPOTrainer:
    """State of one ``PPO()`` run; ``run_iteration`` is one pass of the hot path."""

    def __init__(self, envs, ppo_cfg, run_path=None, writer=None, agent: Agent | None = None, eval_env=None):
        from . import periodic_eval
        c = ppo_cfg
        self.cfg, self.envs, self.run_path, self.writer = c, envs, run_path, writer
        # periodic evaluation (cfg eval_interval > 0): refused here, before anything is built
        eval_settings = periodic_eval.EvalSettings.from_cfg(c)
        evaluating = periodic_eval.check_setup(eval_settings, eval_env, envs, parallel.world_size())
        if not torch.cuda.is_available():
            raise RuntimeError("PPO needs a HIP device (MI355X): every step of the update runs in libcatppo.so; "
                               "there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.nat = native.get(self.device)
        self.T, self.N = int(c.num_steps), int(envs.unwrapped.num_envs)
        self.batch = self.T * self.N
        self.mb = int(c.minibatch_size)
        self.world, self.rank = parallel.world_size(), parallel.rank()
        #: (run directory of the run states, cfg save_state, cfg keep_states); env-sharded runs take rank 0's (below)
        self._state_plan = (None if run_path is None else os.path.abspath(run_path), bool(getattr(c, "save_state", True)),
                            int(getattr(c, "keep_states", 2)))
        hidden = tuple(getattr(c, "hidden", None) or DEFAULT_HIDDEN)
        self.agent = agent if agent is not None else Agent(
            envs, hidden=hidden, mlp_precision=str(getattr(c, "mlp_precision", "fp32"))).to(self.device)
        a = self.agent
        self.D, self.A, self.Dp = a.obs_dim, a.act_dim, a.layout.obs_pad
        self.rng = str(getattr(c, "rng", "device"))
        if self.rng not in ("device", "torch"):
            raise ValueError(f"rng must be 'device' or 'torch', got {self.rng!r}")
        rd = str(getattr(c, "rollout_dtype", "fp32"))
        if rd not in ("fp32", "fp16"):
            raise ValueError(f"rollout_dtype must be 'fp32' or 'fp16', got {rd!r}")
        self.plane_dtype = torch.float16 if rd == "fp16" else torch.float32
        self.gae_mode = str(getattr(c, "gae_mode", "serial"))
        sched = getattr(c, "lr_schedule", None)
        if sched is None:
            sched = "linear" if c.anneal_lr else "fixed"
        if sched not in ("linear", "fixed", "adaptive"):
            raise ValueError(f"lr_schedule must be None, 'linear', 'fixed' or 'adaptive', got {sched!r}")
        self.lr_schedule = sched
        self.n_envs_global = float(self.N)
        rows_per_rank, me = [self.batch], 0
        if parallel.active():
            parallel.init_native_comm(self.nat)                 # RCCL under the C ABI (catppo_comm_init)
            parallel.broadcast_(a.flat, src=0)                  # replicas start identical (cf. skrl ppo.py:126-131)
            if self.world > 1:
                # run states (section 10): the files of ALL ranks go into rank 0's run directory, and whether and how many
                # are kept is rank 0's cfg - so that no rank enters a save vote its peers do not (once, at construction)
                plan = [self._state_plan]
                torch.distributed.broadcast_object_list(plan, src=0)
                self._state_plan = plan[0]
            a.obs_rms.dist_group = a.value_rms.dist_group = torch.distributed.group.WORLD
            cm = getattr(envs.unwrapped, "constraint_manager", None)
            if cm is not None and getattr(c, "dist_exact", True):
                cm.dist_group = torch.distributed.group.WORLD
            counts = parallel.gather_counts(self.N, self.device)      # shards may differ by one env
            self.n_envs_global = float(sum(counts))
            rows_per_rank, me = [self.T * n for n in counts], (self.rank if len(counts) > 1 else 0)
            mbs = parallel.gather_counts(self.mb, self.device)
            if len(set(mbs)) != 1:
                raise ValueError(f"minibatch_size differs between ranks: {mbs}")
        # ONE minibatch schedule for all ranks (ragged shards would otherwise disagree on the number of gradient
        # all-reduces), with the true global row count of every minibatch for the 1/M_global loss scaling
        self.n_mb, m_r, per_rank, self._mb_rows_global = parallel.minibatch_plan(rows_per_rank, self.mb)
        self.M, self._mb_rows = m_r[me], per_rank[me]
        cm = getattr(envs.unwrapped, "constraint_manager", None)
        if cm is not None and hasattr(cm, "ensure_log_ring"):
            cm.ensure_log_ring(self.T + 2)      # the per-step episode logs are read after the rollout
        n_flat = a.layout.n_flat
        dev, T, N = self.device, self.T, self.N
        z = lambda *s, **k: torch.zeros(*s, device=dev, **k)
        pz = lambda *s: torch.zeros(*s, device=dev, dtype=self.plane_dtype)
        self.grad, self.exp_avg, self.exp_avg_sq = z(n_flat), z(n_flat), z(n_flat)
        self.adam_step = 0
        # device-resident iteration state: lr, Adam step count, RNG counters (catppo_iter_state)
        self.state = self.nat.iter_state_new(int(getattr(c, "seed", 0)) * 1000003 + 977 * self.rank + 1,
                                             float(c.learning_rate))
        self.kl_buf = z(1)
        # time-major rollout buffers; slot T holds the bootstrap observation / dones (reference keeps them in
        # next_obs / next_done / next_true_done).  The six (T,N) planes GAE touches are fp32 or fp16.
        self.obs = z(T + 1, N, self.Dp)
        self.actions = z(T, N, self.A)
        self.logprobs = z(T, N)
        self.rewards, self.values = pz(T, N), pz(T, N)
        self.dones, self.true_dones = pz(T + 1, N), pz(T + 1, N)
        self.advantages, self.returns = pz(T, N), pz(T, N)
        self.values_n, self.returns_n = z(T, N), z(T, N)
        self.next_value = pz(N)
        self._act_rows = list(self.actions.unbind(0))
        self.noise = z(T, N, self.A) if self.rng == "torch" else None
        self.record_noise = False        # device rng: keep the noise / permutations used (parity tests replay them)
        self.noise_rec = None
        self.perm_rec = None
        self.diag = z(8)
        self.adv_stats = z(2)
        self.hp = native.PpoHparams(float(c.clip_coef), float(c.ent_coef), float(c.vf_coef), int(bool(c.norm_adv)),
                                    int(bool(c.clip_vloss)), 1.0 / self._mb_rows_global[0], 0)
        # (an evaluation forwards its eval env's rows: reserved NOW - a workspace that grows later drops the captured graph)
        self.nat.mlp_reserve(a.shape, max(self.M, N, int(eval_env.unwrapped.num_envs) if evaluating else 0))
        self.iteration = 0
        self.global_step = 0
        # fused env step (two launches) when the env offers it
        env_u = envs.unwrapped
        self.sink = None
        if bool(getattr(c, "fused_rollout", True)) and hasattr(env_u, "step_into") and \
                getattr(env_u, "can_step_into", lambda: False)() and os.environ.get("CATPPO_FUSED_ROLLOUT", "1") != "0":
            self.sink = RolloutSink(self)
        dt = getattr(c, "defer_rollout_tail", None)
        if os.environ.get("CATPPO_ROLLOUT_DEFER_TAIL") is not None:
            dt = os.environ["CATPPO_ROLLOUT_DEFER_TAIL"] != "0"
        #: catppo_rollout_defer_tail around the env steps of a rollout (fused path only)
        self.defer_tail = True if dt is None else bool(dt)
        #: the env step's post launch rides in the next policy forward (catppo_rollout_defer_tail mode 2; needs defer_tail;
        #: cfg ``merge_rollout_step`` / CATPPO_STEP_MERGE=0: the separate launches, for A/B)
        sm = getattr(c, "merge_rollout_step", None)
        if os.environ.get("CATPPO_STEP_MERGE") is not None:
            sm = os.environ["CATPPO_STEP_MERGE"] != "0"
        self.step_merge = True if sm is None else bool(sm)
        # hipGraph replay of the update phase
        g = getattr(c, "graph_update", None)
        env_g = os.environ.get("CATPPO_GRAPH_UPDATE")
        if env_g is not None:
            g = env_g == "1"
        if g is None:
            # replay pays at every minibatch size: -5 % of an iteration at 2048 rows (launch bound), -1.3 % at 16384
            # (9.57 -> 9.41 ms of update phase at cfg2, round 3: ~330 launches whose host-side enqueue and inter-launch
            # gaps the graph removes); round 2 only enabled it up to 4096 rows
            g = True
        dist_on_torch = parallel.active() and not parallel.native_comm_active()
        # RCCL collectives inside the captured graph (they are stream operations under the C ABI): exercised on a world of
        # one (tests) - but no run with real peers has been possible on the one-GPU development boxes, a hang or an
        # asynchronous fault inside a REPLAYED graph cannot be caught and turned into the eager fallback, and the update
        # phase of an env-sharded run is GPU bound (graph replay buys ~1 % at 16384-row minibatches).  So with real peers
        # it is OPT-IN again (round 5): CATPPO_GRAPH_COMM=1 / cfg ``graph_comm=True`` once a node has shown it
        # works.  When on: the ranks agree (a vote over the rendezvous group) on whether EVERY rank captured and replayed;
        # otherwise all of them drop to eager launches together on a fresh communicator (``graph_fallback``).
        gc = getattr(c, "graph_comm", None)
        if os.environ.get("CATPPO_GRAPH_COMM") is not None:
            gc = os.environ["CATPPO_GRAPH_COMM"] != "0"
        dist_in_graph_ok = self.world == 1 or bool(gc)
        self.graph_update = bool(g) and self.rng == "device" and not dist_on_torch and dist_in_graph_ok
        #: why the update phase left the graph path (None: it did not)
        self.graph_fallback = None
        # gradient all-reduce in per-layer buckets on the library's side stream, under the backward launches of the
        # layers below (catppo_set_grad_overlap; cf. skrl/ppo.py:534-537, which reduces after the whole backward).
        # Needs libcatppo's own communicator.  OPT-IN (cfg ``grad_overlap`` / CATPPO_GRAD_OVERLAP=1): measured on a world of
        # one with every exchange point forced on (profiles/r4_grad_overlap_world1.txt) the two fork / join pairs and the
        # per-bucket fold launches cost +29 us per optimiser step (9.50 -> 10.38 ms of update phase at cfg2) - more than a
        # 1.5 MB ring all-reduce over xGMI is expected to take serialised, so it only pays on a fabric
        # where that all-reduce is slower than ~30 us.
        go = getattr(c, "grad_overlap", None)
        env_go = os.environ.get("CATPPO_GRAD_OVERLAP")
        if env_go is not None:
            go = {"1": True, "2": "tail", "tail": "tail"}.get(env_go, False)
        if go is None:
            go = False
        # (round 5: "tail" / CATPPO_GRAD_OVERLAP=2 = the no-extra-launch form, catppo_set_grad_overlap(ctx, 2): measured
        # in profiles/r5_grad_overlap_tail_world1.txt)
        self.grad_overlap = False
        if parallel.active() and parallel.native_comm_active():
            self.grad_overlap = self.nat.set_grad_overlap(go)
        self._grad_overlap_mode = go
        # single process: an optimiser step is ONE library call (catppo_ppo_minibatch_step_packed) whose fold launches
        # emit the squared gradient norm of the clip - the launch that re-read the gradient for it is gone.  Not with
        # exchange points on (the gradient all-reduce sits between fold and clip).
        ocs = getattr(c, "one_call_step", None)
        if os.environ.get("CATPPO_ONE_CALL_STEP") is not None:
            ocs = os.environ["CATPPO_ONE_CALL_STEP"] == "1"
        self.one_call_step = (True if ocs is None else bool(ocs)) and not parallel.active()
        self._graph_id = None
        self._eager_updates_left = 1 if parallel.active() else 0
        self.graph_nodes = 0
        self.stream = torch.cuda.Stream(device=dev) if self.graph_update else None
        # first observation (ppo.py:186-189)
        first = envs.reset()[0]["policy"]
        a.obs_rms.normalize_into(self._rows(first), self.obs[0])
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream(dev))
        self.time_phases = False
        self._phase_events = []
        #: None unless cfg eval_interval > 0: then the iterations it names gain one evaluation each, the others nothing
        self.evaluator = periodic_eval.PeriodicEvaluator(self, eval_env, eval_settings, run_path, writer) if evaluating else None

    def phase_summary(self, reset: bool = True):
        """mean device milliseconds per iteration of the three phases (needs ``time_phases = True``); synchronises"""
        torch.cuda.synchronize()
        n = max(len(self._phase_events), 1)
        out = {"rollout_ms": 0.0, "gae_and_normalisers_ms": 0.0, "update_ms": 0.0, "iterations": len(self._phase_events)}
        for e in self._phase_events:
            out["rollout_ms"] += e[0].elapsed_time(e[1]) / n
            out["gae_and_normalisers_ms"] += e[1].elapsed_time(e[2]) / n
            out["update_ms"] += e[2].elapsed_time(e[3]) / n
        if reset:
            self._phase_events = []
        return out

    @staticmethod
    def _rows(x):
        x = x if x.dtype == torch.float32 else x.float()
        x = x.reshape(x.shape[0], -1)
        return x if x.stride(1) == 1 else x.contiguous()

    # ------------------------------------------------------------------ rollout (ppo.py:201-230)
    def rollout(self, eps_fn=None):
        c, a, nat, T, N = self.cfg, self.agent, self.nat, self.T, self.N
        ep_infos = []
        if eps_fn is None and self.rng == "torch":
            self.noise.normal_()                                 # all N(0,1) draws of the iteration at once
        if self.record_noise and self.noise_rec is None:
            self.noise_rec = torch.zeros(T, N, self.A, device=self.device)
        env_u = self.envs.unwrapped
        # per-step host path: raw addresses instead of tensor slices, the library called directly
        lib, h, shp = nat.lib, nat.h, C.byref(a.shape)
        p_flat, p_state = a.flat.data_ptr(), self.state.data_ptr()
        p_obs, p_act, p_lp, p_val = self.obs.data_ptr(), self.actions.data_ptr(), self.logprobs.data_ptr(), \
            self.values.data_ptr()
        s_obs, s_act, s_lp, s_val = N * self.Dp * 4, N * self.A * 4, N * 4, N * self.values.element_size()
        vdt = native.F16 if self.plane_dtype == torch.float16 else native.F32
        act_rows = self._act_rows
        use_rng = eps_fn is None and self.rng != "torch"
        # the one-workgroup tail of the fused env step (running maxima / normaliser state / episode log: read by the NEXT
        # env step and by the logging below, not by the policy forward) rides in the next step's first launch instead of
        # standing between catppo_rollout_post and the forward (catppo_rollout_defer_tail; CATPPO_ROLLOUT_DEFER_TAIL=0: A/B)
        defer = self.sink is not None and self.defer_tail
        # ... and the post launch itself rides in the next step's policy forward: catppo_rollout_post records the step,
        # the catppo_policy_step below carries it (nothing of this loop reads a step's outputs in between); the last
        # step of the rollout has no forward behind it and runs as its own launch from the flush in `finally`
        if defer:
            nat.rollout_defer_tail(True, merge=self.step_merge)
        try:
            for step in range(T):
                self.global_step += N * self.world
                if use_rng:                                          # Philox noise inside the head kernel
                    rc = lib.catppo_policy_step(
                        h, shp, p_flat, p_obs + step * s_obs, N, None, None, p_state, step,
                        self.noise_rec[step].data_ptr() if self.record_noise else None, p_act + step * s_act,
                        p_lp + step * s_lp, p_val + step * s_val, vdt, nat._stream())
                else:
                    eps = self.noise[step] if eps_fn is None else eps_fn(step)
                    rc = lib.catppo_policy_step(h, shp, p_flat, p_obs + step * s_obs, N, eps.data_ptr(), None, None, 0, None,
                                                p_act + step * s_act, p_lp + step * s_lp, p_val + step * s_val, vdt,
                                                nat._stream())
                if rc:
                    nat._ok(rc)
                if self.sink is not None:
                    self.sink.step = step
                    next_obs, reward, next_done, timeouts, info = env_u.step_into(act_rows[step], self.sink)
                else:
                    next_obs, reward, next_done, timeouts, info = self.envs.step(self.actions[step])
                    if (reward.dtype == torch.float32 and next_done.dtype == torch.float32 and timeouts.dtype == torch.bool
                            and reward.is_contiguous() and next_done.is_contiguous() and timeouts.is_contiguous()):
                        nat.rollout_store_ex(reward, next_done, timeouts, self.rewards[step], self.dones[step + 1],
                                             self.true_dones[step + 1])
                    else:                                            # foreign env: dtype conversions in the copies
                        self.rewards[step].copy_(reward)
                        self.dones[step + 1].copy_(next_done)
                        self.true_dones[step + 1].copy_(timeouts)
                    a.obs_rms.normalize_into(self._rows(next_obs["policy"]), self.obs[step + 1])
                if "episode" in info:
                    ep_infos.append(info["episode"])
                elif "log" in info:
                    packed = info.get("log_packed")
                    if packed is None:
                        ep_infos.append(info["log"])
                    else:                                 # (keys, device tensor) + the host-side scalars of the log
                        host = info.get("log_host")
                        extra = dict(host) if host is not None else \
                            {k: v for k, v in info["log"].items() if not isinstance(v, torch.Tensor)}
                        ep_infos.append((packed[0], packed[1], extra))
                info["true_dones"] = timeouts
                if "time_outs" in info:
                    if info["time_outs"].any():
                        print("time outs", info["time_outs"].sum())
                        exit(0)
        finally:
            if defer:
                nat.rollout_defer_tail(False)          # = flush: everything the steps wrote is current from here on
        return ep_infos

    # ------------------------------------------------------------------ GAE + normalisers (:251-288)
    def compute_returns(self):
        c, a, nat, T, N = self.cfg, self.agent, self.nat, self.T, self.N
        nat.value_ex(a.shape, a.flat, self.obs[T], N, self.next_value)
        args = (self.rewards, self.values, self.dones[:T], self.true_dones[:T], self.next_value, self.dones[T],
                self.true_dones[T], c.gamma, c.gae_lambda, self.advantages, self.returns)
        if self.plane_dtype == torch.float16:
            nat.gae_f16(*args)
        elif self.gae_mode == "scan":
            nat.gae_mode(native.GAE_SCAN, *args)
        else:
            nat.gae(*args)
        # value_rms is updated with the values and then, a second time, with the returns (:287-288); env-sharded runs
        # exchange both batches' moments in one all-reduce
        a.value_rms.update_normalize_pair(self.values.view(-1, 1), self.values_n.view(-1, 1),
                                          self.returns.view(-1, 1), self.returns_n.view(-1, 1))

    # ------------------------------------------------------------------ update (:294-354)
    def _update_buffers(self):
        if not hasattr(self, "_x_g"):
            # packed epoch buffers: one gather launch per epoch, minibatch k = contiguous slice k
            B, M, n_mb = self.batch, self.M, self.n_mb
            self._parts = (M + self.nat.GATHER_ROWS - 1) // self.nat.GATHER_ROWS
            self._x_g = torch.empty(B, self.Dp, device=self.device)
            self._act_g = torch.empty(B, self.A, device=self.device)
            self._scal_g = torch.empty(4 * B, device=self.device)
            self._advp_g = torch.empty(n_mb * self._parts * 2, dtype=torch.float64, device=self.device)
            E = int(self.cfg.updates_epochs)
            self._advp_all = torch.empty(E * n_mb * self._parts * 2, dtype=torch.float64, device=self.device)
            self._adv_mom = torch.zeros(E * n_mb, 3, dtype=torch.float64, device=self.device)
            self._adv_stats_all = torch.zeros(E * n_mb, 2, device=self.device)

    def _update_body(self, perms):
        """the launches of one update phase (E epochs x minibatches).  ``perms``: list of index tensors (injected /
        torch.randperm) or None = keyed on-device permutation.  Contains no host synchronisation, no allocation and
        only library calls (+ RCCL through the C ABI), so it can be captured into a hipGraph."""
        c, a, nat = self.cfg, self.agent, self.nat
        B, M, n_mb = self.batch, self.M, self.n_mb
        b_obs = self.obs[:self.T].view(B, self.Dp)
        b_act = self.actions.view(B, self.A)
        b_logp, b_adv = self.logprobs.view(-1), self.advantages.view(-1)
        b_ret, b_val = self.returns_n.view(-1), self.values_n.view(-1)
        vmean, vvar = a.value_rms.running_mean, a.value_rms.running_var
        E = int(c.updates_epochs)
        exact_adv = parallel.active() and bool(c.norm_adv) and getattr(c, "dist_exact", True)
        self.hp.adv_stats_external = int(exact_adv)
        # keyed on-device permutations: the minibatch advantage moments of ALL epochs are a function of (seed, iteration,
        # epoch) and the advantages alone, so they are formed before the first gather and exchanged in ONE all-reduce per
        # iteration (round 5; one per epoch before).  Injected / torch permutations keep the per-epoch route.
        adv_upfront = exact_adv and perms is None and os.environ.get("CATPPO_ADV_UPFRONT", "1") != "0"
        if adv_upfront:
            nat.adv_moments_keyed(b_adv, self.state, E, B, M, self._advp_all, self._adv_mom)
            parallel.allreduce_sum_(self._adv_mom)
            nat.adv_stats(self._adv_mom, E * n_mb, self._adv_stats_all)
        # trace_params (tests: the branch-flip analysis of tests/test_gpu_parity_sizes.py): the flat parameters after every
        # optimiser step of this update phase, [E * n_mb, n_flat] (device-to-device copies in stream order)
        trace = None
        if getattr(self, "trace_params", False):
            if getattr(self, "param_trace", None) is None or self.param_trace.shape[0] != E * n_mb:
                self.param_trace = torch.empty(E * n_mb, a.layout.n_flat, device=self.device)
            trace = self.param_trace
            self.param_trace_start = a.flat.clone()
            # (and what this update phase reads: the next rollout's first rows overwrite the buffers' step 0 before a test looks)
            self.trace_batch = dict(obs=b_obs.clone(), actions=b_act.clone(), logprobs=b_logp.clone(), values_n=b_val.clone(),
                                    advantages=b_adv.clone(), returns_n=b_ret.clone())
        for epoch in range(E):
            rec = self.perm_rec[epoch] if self.perm_rec is not None else None
            nat.ppo_gather_ex(a.shape, b_obs, b_act, b_logp, b_adv, b_ret, b_val, B, M, self._x_g, self._act_g,
                              self._scal_g, self._advp_g, inds=None if perms is None else perms[epoch],
                              st=self.state, epoch=epoch, inds_out=rec if perms is None else None)
            if exact_adv and not adv_upfront:
                # minibatch advantage mean / unbiased std over ALL ranks (ppo.py:316-318): the moments of every
                # minibatch of the epoch from the chunk sums the gather just wrote (any plane precision, no index
                # array), ONE all-reduce, one finishing launch
                mom = self._adv_mom[epoch * n_mb:(epoch + 1) * n_mb]
                nat.adv_moments_parts(self._advp_g, self._parts, B, M, mom)
                parallel.allreduce_sum_(mom)
                nat.adv_stats(mom, n_mb, self._adv_stats_all[epoch * n_mb:(epoch + 1) * n_mb])
            for k in range(n_mb):
                start, m = k * M, self._mb_rows[k]
                self.hp.inv_global_batch = 1.0 / self._mb_rows_global[k]     # mean over the GLOBAL minibatch
                adv_stats = self._adv_stats_all[epoch * n_mb + k] if exact_adv else None
                if self.one_call_step:
                    # single process: gradient, clip and Adam in one call (the fold launches emit the squared norm)
                    nat.ppo_minibatch_step_packed(a.shape, self.hp, a.flat, self._x_g[start:], self._act_g[start:],
                                                  self._scal_g[4 * start:], self._advp_g[2 * k * self._parts:], m,
                                                  vmean, vvar, adv_stats, self.grad, self.diag, self.exp_avg,
                                                  self.exp_avg_sq, c.max_grad_norm, 0.9, 0.999, 1e-5, self.state)
                    if trace is not None:
                        trace[epoch * n_mb + k].copy_(a.flat)
                    continue
                nat.ppo_minibatch_grad_packed(a.shape, self.hp, a.flat, self._x_g[start:], self._act_g[start:],
                                              self._scal_g[4 * start:], self._advp_g[2 * k * self._parts:], m,
                                              vmean, vvar, adv_stats, self.grad, self.diag)
                if not self.grad_overlap:                       # (else: reduced bucket by bucket inside the call above)
                    parallel.allreduce_sum_(self.grad)          # RCCL SUM of the flat gradient over xGMI
                nat.clip_adam_dev(a.flat, self.grad, self.exp_avg, self.exp_avg_sq, a.layout.n_flat,
                                  c.max_grad_norm, 0.9, 0.999, 1e-5, self.state)
                if trace is not None:
                    trace[epoch * n_mb + k].copy_(a.flat)
            if self.lr_schedule == "adaptive":
                # KL-adaptive learning rate after every epoch (skrl/ppo.py:558-567), entirely on the device
                nat.kl_mean(self.state, self.diag, self.kl_buf)
                parallel.allreduce_sum_(self.kl_buf)            # per-rank values SUM to the global mean KL
                nat.kl_adaptive_lr(self.state, self.kl_buf, float(getattr(c, "kl_threshold", 0.01)))
        return E * n_mb

    def update(self, perm_fn=None):
        c = self.cfg
        B = self.batch
        E = int(c.updates_epochs)
        self._update_buffers()
        self.diag.zero_()
        if self.record_noise and self.perm_rec is None:
            self.perm_rec = torch.zeros(E, B, dtype=torch.int64, device=self.device)
        perms = None
        if perm_fn is not None:
            perms = [perm_fn(e) for e in range(E)]
        elif self.rng == "torch":
            perms = [torch.randperm(B, device=self.device) for e in range(E)]
        tracing = bool(getattr(self, "trace_params", False))      # (a traced update phase runs eagerly)
        if self.graph_update and perms is None and not self.record_noise and not tracing and self._eager_updates_left > 0:
            # env-sharded runs: the FIRST update phase runs eagerly, so that RCCL's first collectives of every size
            # (channel set-up, lazily loaded kernels, possibly allocations) happen outside a stream capture
            self._eager_updates_left -= 1
        elif self.graph_update and perms is None and not self.record_noise and not tracing:
            if self._graph_id is not None:
                try:
                    self.nat.graph_launch(self._graph_id)
                    self.adam_step += self._graph_steps
                    return
                except RuntimeError as e:                        # workspace grew: the graph was dropped
                    self._graph_id = None
                    if parallel.active() and self.world > 1:
                        #  the re-capture below ends in a vote (all_gather_object) that only re-capturing ranks
                        # enter: peers whose replay succeeded are already in the next rollout's collectives, so a rank
                        # that loses its graph alone must not walk into that vote - it fails loudly instead of hanging
                        raise RuntimeError(f"rank {self.rank}: replay of the captured update phase failed ({e}) in an "
                                           f"env-sharded run of {self.world} ranks; re-capturing on one rank would wait in a "
                                           "vote its peers never join") from e
            try:
                self.nat.graph_begin()
                try:
                    self._graph_steps = self._update_body(None)
                except BaseException:
                    # a failure between begin and end leaves a PARTIAL capture: never instantiate or replay it (ending
                    # the capture may itself fail once the capture is invalidated)
                    self.nat.graph_abort()
                    raise
                gid, self.graph_nodes = self.nat.graph_end()
            except RuntimeError as e:
                gid, err = None, e
            else:
                err = None
            if parallel.active() and self.world > 1:
                # every rank learns whether EVERY rank holds a graph before anybody replays: a rank whose capture failed
                # after enqueueing collectives may have left its communicator ahead of its peers'  - then
                # nobody replays, and all ranks continue eagerly on a FRESH communicator
                votes = [None] * self.world
                torch.distributed.all_gather_object(votes, None if err is None else f"{type(err).__name__}: {err}")
                bad = [(i, v) for i, v in enumerate(votes) if v is not None]
                if bad:
                    if gid is not None:
                        self.nat.graph_destroy(gid)
                    gid = None
                    err = err or RuntimeError("capture failed on " + "; ".join(f"rank {i}: {v}" for i, v in bad))
                    parallel.reinit_native_comm()
            if err is None:
                # nothing has executed so far (a capture records, it does not run)
                steps_before = int(self.nat.iter_state_read(self.state).adam_step) if parallel.active() else None
                try:
                    self.nat.graph_launch(gid)
                except RuntimeError as e:
                    err = e
                    # a failing launch normally leaves the phase undone - but a deferred asynchronous error, or a
                    # partially enqueued graph, would make the eager re-run below apply optimiser steps twice on this
                    # rank only.  The device-side Adam step count says which: re-run only if it has not moved.
                    if parallel.active():
                        torch.cuda.synchronize()
                        moved = int(self.nat.iter_state_read(self.state).adam_step) - steps_before
                        self.nat.graph_destroy(gid)
                        if moved != 0:
                            raise RuntimeError(f"hipGraph replay of the update phase failed after {moved} optimiser steps "
                                               f"had executed ({e}); refusing to re-run the phase eagerly") from e
            if err is not None:
                self._graph_id = None
                if not parallel.active():
                    raise err                                    # single process: the error surfaces as before
                # env-sharded run: collectives inside a graph are the one thing a one-GPU box cannot prove.  Fall back
                # to eager launches (same launches, same order, same collectives)
                self.graph_update = False
                self.graph_fallback = f"{type(err).__name__}: {err}"
                import sys
                print(f"[catppo] rank {self.rank}: hipGraph capture / first replay of the update phase failed, "
                      f"falling back to eager launches: {self.graph_fallback}", file=sys.stderr)
            else:
                self._graph_id = gid
                self.adam_step += self._graph_steps
                return
        self.adam_step += self._update_body(perms)

    # ------------------------------------------------------------------ run state
    def state_fingerprint(self) -> dict:
        """everything that must be equal for a saved state to continue THIS run (checkpoint.check_fingerprint); an
        env-sharded run adds its rank (env count, env seed and env offset already differ between the ranks)"""
        from . import checkpoint
        env_u = self.envs.unwrapped
        if not hasattr(env_u, "state_fingerprint"):
            raise NotImplementedError(f"run state: {type(env_u).__name__} has no state_fingerprint() / state_dict()")
        c, a = self.cfg, self.agent
        fp = dict(env_u.state_fingerprint())
        fp.update({"hidden": [int(h) for h in a.hidden], "num_steps": self.T, "minibatch_size": self.mb,
                   "updates_epochs": int(c.updates_epochs), "mlp_precision": a.mlp_precision,
                   "rollout_dtype": "fp16" if self.plane_dtype == torch.float16 else "fp32", "rng": self.rng,
                   "lr_schedule": self.lr_schedule, "world": int(self.world),
                   "sizeof_iter_state": int(C.sizeof(native.IterState)),
                   "catppo_version": int(self.nat.lib.catppo_version())})
        return checkpoint.rank_fingerprint(fp, self.world, self.rank)

    def _schedule_fields(self) -> dict:
        """recorded, not compared: a user may extend a run or change a coefficient"""
        c = self.cfg
        out = {k: float(getattr(c, k)) for k in ("learning_rate", "gamma", "gae_lambda", "clip_coef", "ent_coef", "vf_coef",
                                                  "max_grad_norm", "kl_threshold") if hasattr(c, k)}
        out.update(num_iterations=int(c.num_iterations), anneal_lr=bool(c.anneal_lr), norm_adv=bool(c.norm_adv),
                   clip_vloss=bool(c.clip_vloss), seed=int(getattr(c, "seed", 0)))
        return out

    def _state_payload(self) -> dict:
        """this process's run state as ``checkpoint.write_state`` takes it (the tensors are the live ones: it copies them).
        One device synchronisation; the copies to the host that follow find the device idle."""
        from . import checkpoint
        fp = self.state_fingerprint()
        env_sd = self.envs.unwrapped.state_dict()             # raises while an evaluation is attached
        torch.cuda.synchronize()
        st = self.nat.iter_state_read(self.state)
        if int(st.iteration) != self.iteration or int(st.adam_step) != self.adam_step:
            raise RuntimeError(f"run state: the device iteration state (iteration {int(st.iteration)}, {int(st.adam_step)} "
                               f"optimiser steps) and the trainer ({self.iteration}, {self.adam_step}) disagree: not at an "
                               "iteration boundary")
        tr = {"agent": dict(self.agent.state_dict()), "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
              "iter_state": self.state, "sizeof_iter_state": int(self.state.numel()),
              "iter_state_fields": {"iteration": int(st.iteration), "adam_step": int(st.adam_step), "lr": float(st.lr),
                                    "seed": int(st.seed)},
              "adam_step": int(self.adam_step), "iteration": int(self.iteration), "global_step": int(self.global_step),
              "obs0": self.obs[0], "dones0": self.dones[0], "true_dones0": self.true_dones[0], "kl_buf": self.kl_buf,
              "eager_updates_left": int(self._eager_updates_left), "schedule": self._schedule_fields()}
        if self.rng == "torch":
            tr["torch_rng"] = {"cpu": torch.get_rng_state(), "device": torch.cuda.get_rng_state(self.device)}
        return {"format": checkpoint.FORMAT, "fingerprint": fp, "trainer": tr, "env": env_sd}

    def save_state(self, path: str) -> str:
        """Write the whole run state to ``path`` (atomically).  Only legal at an iteration boundary - after
        ``run_iteration`` has returned, or straight after construction.

        Env-sharded run (``world > 1``): COLLECTIVE - every rank calls it with the same ``path``, rank 0's
        ``state_<it>.pt``.  Rank r >= 1 writes ``state_<it>.rank<r>.pt`` beside it, the ranks vote, and only when every
        rank wrote its file does rank 0 write ``path``, which commits the set; otherwise this iteration's files are removed
        and every rank raises ``RuntimeError`` naming the failing ranks.  Returns the path of this rank's file."""
        from . import checkpoint
        if self.world > 1:
            return self._save_state_set(path)
        return checkpoint.write_state(path, self._state_payload())

    def _save_state_set(self, path: str) -> str:
        import uuid
        from . import checkpoint
        dist = torch.distributed
        mine, payload, err = None, None, None
        try:
            mine = checkpoint.sibling_path(path, self.rank)
            payload = self._state_payload()
        except Exception as e:                                   # said in the vote: the peers must not wait for this rank
            err = f"{type(e).__name__}: {e}"
        # one token per save (never from a torch generator: rng="torch" runs stay bit-identical): files of two saves of one
        # iteration are told apart when they are loaded
        token = [uuid.uuid4().hex if self.rank == 0 else None]
        dist.broadcast_object_list(token, src=0)
        if payload is not None:
            payload["trainer"]["set"] = {"world": int(self.world), "rank": int(self.rank), "token": str(token[0])}
        wrote = False
        if err is None and self.rank > 0:
            try:
                checkpoint.write_state(mine, payload)
                wrote = True
            except Exception as e:
                err = f"{type(e).__name__}: {e}"
        votes = [None] * self.world
        dist.all_gather_object(votes, err)
        bad = [(r, v) for r, v in enumerate(votes) if v is not None]
        it = checkpoint.state_iteration(path)
        if bad:
            if wrote:
                try:
                    os.remove(mine)
                except FileNotFoundError:
                    pass
            if self.rank == 0 and it is not None:
                checkpoint.remove_siblings(os.path.dirname(path) or ".", it)
            raise RuntimeError(f"{path}: the run state of {self.world} ranks was not written ({len(bad)} rank(s) failed; this "
                               "iteration's files are removed): " + "; ".join(f"rank {r}: {v}" for r, v in bad))
        if self.rank == 0:
            try:
                checkpoint.write_state(mine, payload)            # the commit: from here on the set exists
            except BaseException:
                if it is not None:
                    checkpoint.remove_siblings(os.path.dirname(path) or ".", it)
                raise
        return mine

    _STATE_KEYS = ("agent", "exp_avg", "exp_avg_sq", "iter_state", "sizeof_iter_state", "iter_state_fields", "adam_step",
                   "iteration", "global_step", "obs0", "dones0", "true_dones0", "kl_buf", "eager_updates_left", "schedule")

    def _read_checked(self, path: str):
        """everything a load does BEFORE it writes: read ``path``, fingerprint, required keys, every tensor's shape and
        dtype in trainer, env, manager and simulator.  Returns (payload, [(name, own tensor, saved tensor)])."""
        from . import checkpoint
        payload = checkpoint.read_state(path)
        checkpoint.check_fingerprint(payload["fingerprint"], self.state_fingerprint(), path)
        tr, env_u = payload["trainer"], self.envs.unwrapped
        checkpoint.require(tr, self._STATE_KEYS + (("torch_rng",) if self.rng == "torch" else ())
                           + (("set",) if self.world > 1 else ()), path, "trainer")
        own = self.agent.state_dict()
        pairs = [(f"agent.{k}", own[k], tr["agent"].get(k)) for k in own]
        pairs += [("exp_avg", self.exp_avg, tr["exp_avg"]), ("exp_avg_sq", self.exp_avg_sq, tr["exp_avg_sq"]),
                  ("iter_state", self.state, tr["iter_state"]), ("obs0", self.obs[0], tr["obs0"]),
                  ("dones0", self.dones[0], tr["dones0"]), ("true_dones0", self.true_dones[0], tr["true_dones0"]),
                  ("kl_buf", self.kl_buf, tr["kl_buf"])]
        extra = [k for k in tr["agent"] if k not in own]
        bad = [f"{n}: saved {None if s is None else (tuple(s.shape), s.dtype)}, this run {(tuple(t.shape), t.dtype)}"
               for n, t, s in pairs if s is None or tuple(s.shape) != tuple(t.shape) or s.dtype != t.dtype]
        if bad or extra:
            raise ValueError(f"{path}: trainer tensors do not fit: {'; '.join(bad + ['unexpected agent.' + k for k in extra])}")
        try:
            env_u.check_state_dict(payload["env"])
        except (ValueError, KeyError) as e:
            raise ValueError(f"{path}: {e}") from e
        return payload, pairs

    def _read_checked_set(self, path: str):
        """``_read_checked`` of this rank's file of the set that ``path`` (rank 0's file) names, then ONE vote: the load
        goes on only if every rank's file passed and the files are one save of this world - same token, iteration and
        optimiser step count, written by ``world`` ranks, each by the rank that reads it.  Otherwise every rank raises
        ``ValueError`` naming each offending rank, and no rank has written a byte."""
        from . import checkpoint
        payload = pairs = err = None
        rec = (None,) * 5
        try:
            mine = checkpoint.sibling_path(path, self.rank)
            if not os.path.isfile(mine):
                raise FileNotFoundError(f"{mine} does not exist: rank {self.rank}'s file of the set is missing")
            payload, pairs = self._read_checked(mine)
            tr = payload["trainer"]
            checkpoint.require(tr["set"], ("world", "rank", "token"), mine, "trainer.set")
            rec = (int(tr["set"]["world"]), int(tr["set"]["rank"]), str(tr["set"]["token"]), int(tr["iteration"]),
                   int(tr["adam_step"]))
        except Exception as e:                                   # said in the vote: the peers must not wait for this rank
            err = f"{type(e).__name__}: {e}"
        votes = [None] * self.world
        torch.distributed.all_gather_object(votes, (err,) + rec)
        bad = checkpoint.check_set_votes(votes)
        if bad:
            short = lambda r, m: m if r == self.rank or len(m) <= 600 else m[:600] + " ..."
            raise ValueError(f"{path}: the run state of {self.world} ranks was refused by {len(bad)} rank(s) and nothing was "
                             "loaded on any rank: " + "; ".join(f"rank {r}: {short(r, m)}" for r, m in bad))
        return payload, pairs

    def load_state(self, path: str) -> dict:
        """Continue from the run state in ``path``: afterwards the next ``run_iteration`` is iteration ``saved + 1`` of the
        run that wrote it, bit for bit.  The fingerprint and every shape are checked BEFORE anything is written - a refused
        load leaves trainer and env as they were.  Loads in place (``copy_``); a captured update graph is dropped and
        captured again; the launch-time switches (graph_update, one_call_step, defer_tail, ...) stay as this process chose
        them.  Returns the file's ``trainer`` section.

        Env-sharded run (``world > 1``): COLLECTIVE - every rank calls it with the same ``path``, rank 0's
        ``state_<it>.pt``, and reads its own file of the set; all ranks load or none does (``_read_checked_set``)."""
        payload, pairs = self._read_checked_set(path) if self.world > 1 else self._read_checked(path)
        tr, env_u = payload["trainer"], self.envs.unwrapped
        # -- nothing was written up to here ---------------------------------------------------------------------------
        torch.cuda.synchronize()
        if self._graph_id is not None:                           # captured again by the next update phase
            self.nat.graph_destroy(self._graph_id)
            self._graph_id = None
        with torch.no_grad():
            for _, t, s in pairs:
                t.copy_(s)
        env_u.load_state_dict(payload["env"])
        self.adam_step, self.iteration = int(tr["adam_step"]), int(tr["iteration"])
        self.global_step = int(tr["global_step"])
        left = int(tr["eager_updates_left"])
        if self.world > 1:
            # the eager first update phase of an env-sharded run warms up the PROCESS's communicator outside a stream
            # capture (see update()): a process that has not run one yet still owes it, whatever the saving process had done
            left = max(left, self._eager_updates_left)
        self._eager_updates_left = left
        if self.rng == "torch":
            torch.set_rng_state(tr["torch_rng"]["cpu"])
            torch.cuda.set_rng_state(tr["torch_rng"]["device"], self.device)
        torch.cuda.synchronize()
        sched = tr["schedule"]
        if self.lr_schedule == "linear" and int(sched.get("num_iterations", self.cfg.num_iterations)) != int(self.cfg.num_iterations):
            print(f"[catppo] resumed at iteration {self.iteration}: the linear learning-rate anneal now follows "
                  f"num_iterations={int(self.cfg.num_iterations)} (the saved run had {int(sched['num_iterations'])})")
        return tr

    def _save_run_state(self, it: int):
        """``state_<it>.pt`` beside ``model_<it>.pt`` (rank 0, cfg ``save_state``), older ones pruned (``keep_states``).
        Env-sharded run: called on EVERY rank (``save_state`` is collective there); directory and switches are rank 0's."""
        from . import checkpoint
        if self.world > 1:
            run_dir, on, keep = self._state_plan
            if run_dir is None or not on:
                return
            self.save_state(os.path.join(run_dir, f"state_{it}.pt"))
            if self.rank == 0:
                checkpoint.prune_states(run_dir, keep, siblings=True)
            return
        if not bool(getattr(self.cfg, "save_state", True)):
            return
        self.save_state(f"{self.run_path}/state_{it}.pt")
        checkpoint.prune_states(self.run_path, int(getattr(self.cfg, "keep_states", 2)))

    # ------------------------------------------------------------------ one iteration
    def run_iteration(self, eps_fn=None, perm_fn=None, log: bool = True):
        if self.stream is None:
            return self._run_iteration(eps_fn, perm_fn, log)
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):                     # graph capture needs a non-default stream
            out = self._run_iteration(eps_fn, perm_fn, log)
        cur.wait_stream(self.stream)
        return out

    def _run_iteration(self, eps_fn=None, perm_fn=None, log: bool = True):
        c = self.cfg
        ev_run = self.evaluator
        if ev_run is not None and self.iteration == 0:            # a fresh run: the untrained policy, recorded as iteration 0
            ev_run.evaluate(0)
        self.iteration += 1
        it = self.iteration
        self.lr = float(c.learning_rate)
        sched = {"fixed": native.LR_FIXED, "linear": native.LR_LINEAR, "adaptive": native.LR_KEEP}[self.lr_schedule]
        if self.lr_schedule == "linear":
            frac = 1.0 - (it - 1.0) / c.num_iterations
            self.lr = frac * c.learning_rate                     # host mirror of the device-side schedule (logging)
        self.nat.iter_begin(self.state, float(c.learning_rate), int(c.num_iterations), sched)
        ev = None
        if self.time_phases:                                     # HIP events on the stream the launches go to
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        ep_infos = self.rollout(eps_fn)
        if ev:
            ev[1].record()
        self.compute_returns()
        if ev:
            ev[2].record()
        self.update(perm_fn)
        if ev:
            ev[3].record()
            self._phase_events.append(ev)
        # slot T becomes slot 0 of the next rollout (next_obs / next_done / next_true_done carry over)
        self.obs[0].copy_(self.obs[self.T])
        self.dones[0].copy_(self.dones[self.T])
        self.true_dones[0].copy_(self.true_dones[self.T])
        if ev_run is not None and it % ev_run.interval == 0:      # absolute iterations: a resumed run keeps the grid
            ev_run.evaluate(it)
        if not log:
            return None
        if self.world > 1:
            parallel.allreduce_sum_(self.diag)
            self.diag[7] /= self.world
        d = self.diag.cpu().numpy()                              # the one host sync of the iteration
        # per-term episode sums of a configured reward block: read where the host has just waited anyway (env-sharded
        # runs log rank 0's shard; every rank pops, so that every shard's ended sums cover the same iterations)
        rm = getattr(self.envs.unwrapped, "reward_manager", None)
        reward_log = rm.pop_log() if rm is not None else None
        # ... and how the ended episodes of a configured termination block ended, likewise
        tm = getattr(self.envs.unwrapped, "termination_manager", None)
        termination_log = tm.pop_log() if tm is not None else None
        if self.lr_schedule == "adaptive":
            self.lr = float(self.nat.iter_state_read(self.state).lr)
        n_upd = max(d[7], 1.0)
        stats = {"mean_pg_loss": d[0] / n_upd, "mean_v_loss": d[1] / n_upd, "mean_entropy_loss": d[2] / n_upd,
                 "mean_surrogate_loss": d[3] / n_upd, "approx_kl": d[4] / n_upd, "old_approx_kl": d[5] / n_upd,
                 "clipfrac": d[6] / n_upd, "learning_rate": self.lr}
        if self.writer is not None and self.rank == 0:
            self._log_episode_infos(ep_infos, it)
            w = self.writer
            w.add_scalar("Loss/mean_pg_loss", stats["mean_pg_loss"], it)
            w.add_scalar("Loss/mean_entropy_loss", stats["mean_entropy_loss"], it)
            w.add_scalar("Loss/mean_v_loss", stats["mean_v_loss"], it)
            w.add_scalar("Loss/mean_surrogate_loss", stats["mean_surrogate_loss"], it)
            w.add_scalar("Loss/learning_rate", self.lr, it)
            for key, value in (reward_log or {}).items():        # "Episode_Reward/<term>"
                w.add_scalar(key, value, it)
            for key, value in (termination_log or {}).items():   # "Episode_Termination/<term>"
                w.add_scalar(key, value, it)
        if self.run_path is not None and self.rank == 0 and (it + 1) % c.save_interval == 0:
            torch.save(self.agent.state_dict(), f"{self.run_path}/model_{it}.pt")     # same off-by-one naming
            print("Saved model")
            if self.world == 1:
                self._save_run_state(it)                         # (only where a model is written: no further sync elsewhere)
        if self.world > 1 and (it + 1) % c.save_interval == 0:
            self._save_run_state(it)                             # every rank: its own file, and the vote that commits the set
        return stats

    def _log_episode_infos(self, ep_infos, it):
        """mean of every logged key over the steps of the rollout (ppo.py:233-248)"""
        if not ep_infos:
            return
        first = ep_infos[0]
        if isinstance(first, tuple):                             # packed (keys, tensor, host scalars) from CaTEnv
            keys = first[0]
            vals = torch.stack([e[1] for e in ep_infos]).mean(0).cpu().numpy()
            items = list(zip(keys, vals))
            for key in first[2]:                                 # e.g. "Curriculum/<term>" (reference logs them too)
                vs = [float(e[2][key]) for e in ep_infos if key in e[2]]
                items.append((key, sum(vs) / len(vs)))
        else:
            items = []
            for key in first:
                vs = []
                for ep in ep_infos:
                    if key not in ep:
                        continue
                    v = ep[key]
                    v = v if isinstance(v, torch.Tensor) else torch.tensor([float(v)])
                    vs.append(v.reshape(-1).to(self.device).float())
                items.append((key, float(torch.cat(vs).mean())))
        for key, value in items:
            self.writer.add_scalar(key if "/" in key else "Episode/" + key, value, it)


def PPO(envs, ppo_cfg, run_path, resume_state=None, stop_after=None, eval_env=None):
    """Train with CleanRL-style PPO on CaT float dones (reference ppo.py:126-372).

    ``resume_state``: path of a run state (``state_<it>.pt``, written beside every ``model_<it>.pt``): the run continues
    with iteration ``it + 1`` exactly as the run that wrote it would have (env-sharded runs: rank 0's ``state_<it>.pt`` and
    the same ``run_path`` on every rank; every rank loads its own file of the set).  ``stop_after``: leave after that iteration
    (what a killed run looks like; the schedules still follow ``num_iterations``).  ``eval_env``: the dedicated env of the
    periodic evaluation (cfg ``eval_interval > 0``; ``periodic_eval.make_eval_env``); a resumed run starts from the
    ``model_best.pt`` / ``eval/best.json`` of the run it continues."""
    # env-sharded runs: the ranks share rank 0's run directory (train.py), where rank 0 alone logs
    writer = _make_writer(ppo_cfg, run_path) if parallel.rank() == 0 else None
    os.makedirs(run_path, exist_ok=True)
    trainer = PPOTrainer(envs, ppo_cfg, run_path, writer, eval_env=eval_env)
    total = int(ppo_cfg.num_iterations)
    first = 1
    if resume_state is not None:
        trainer.load_state(resume_state)
        if trainer.iteration >= total:
            raise ValueError(f"{resume_state} was saved after iteration {trainer.iteration}: nothing is left of a run of "
                             f"num_iterations={total} (raise --num_iterations to extend the run)")
        first = trainer.iteration + 1
        print(f"Resuming from {resume_state} at iteration {first}")
        if trainer.evaluator is not None:
            best = trainer.evaluator.carry_over_from(os.path.dirname(os.path.abspath(resume_state)))
            if best is not None:
                print(f"[INFO] Carried over the best evaluation so far: {best['metric']} {best['value']:.6g} at iteration {best['iteration']}")
    last = total if stop_after is None else min(total, int(stop_after))
    print(f"Starting training for {ppo_cfg.num_iterations} steps")
    t0, steps0 = time.time(), trainer.global_step
    for _ in range(first, last + 1):
        trainer.run_iteration()
    torch.cuda.synchronize()
    dt = time.time() - t0
    steps = trainer.global_step - steps0
    print(f"[PPO] {steps} env steps in {dt:.2f} s ({steps / max(dt, 1e-9):,.0f} env-steps/s)")
    if trainer.evaluator is not None and trainer.evaluator.tracker.summary() is not None:
        print(trainer.evaluator.tracker.summary())
    return trainer
