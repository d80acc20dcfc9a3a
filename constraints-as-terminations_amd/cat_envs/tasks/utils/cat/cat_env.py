"""CaT environment: manager-based RL env whose ``step`` returns the constraint termination
probability as float ``dones`` and scales the reward by ``(1 - p)``.

Reference: cat/cat_env.py.  Only lines 92-121 and 147 of the reference ``step`` are on the hot
path (counters, terminations, ``constraint_manager.compute()``, reward scaling, float dones,
hard resets, manager resets, return tuple); the physics loop (:61-88) is Isaac Sim / PhysX,
which cannot run on AMD GPUs and is out of scope.  This class therefore drives the same
managers from a *synthetic simulator*: seeded, device-resident, pre-generated streams of Solo12
sim state (joint state, gravity, commands, contact forces, air times), rewards, hard resets
and observations.  Every step the current slab of the stream is moved into persistent state
buffers (what a simulator's ``scene.update`` does) - by one ``copy_`` in ``step``, inside the
first launch of the fused ``step_into`` (``catppo_rollout_step.sim_src``) - and every manager
reads views of those buffers, exactly like IsaacLab's ``scene[...]`` data objects.
``SyntheticCfg.kind = "servo"`` selects ``Solo12ServoSim`` instead: a closed-loop surrogate whose next state is computed
from the state buffers and the action by one kernel launch per step.

No host synchronisation happens inside ``step``: resets are handled with masks
(``exact_reset_sync=True`` restores the reference's ``nonzero()``-based control flow).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import types
from collections.abc import Sequence

import torch

from cat_envs import native
from cat_envs.shim import SceneEntityCfg  # noqa: F401  (re-export for term configs)

from .constraint_manager import ConstraintManager

SOLO12_JOINTS = ["FL_HAA", "FL_HFE", "FL_KFE", "FR_HAA", "FR_HFE", "FR_KFE",
                 "HL_HAA", "HL_HFE", "HL_KFE", "HR_HAA", "HR_HFE", "HR_KFE"]
SOLO12_BODIES = ["base_link"] + [f"{leg}_{part}" for leg in ("FL", "FR", "HL", "HR")
                                 for part in ("SHOULDER", "UPPER_LEG", "LOWER_LEG", "FOOT")]
DEFAULT_JOINT_POS = [0.05, 0.4, -0.8, -0.05, 0.4, -0.8, 0.05, 0.4, -0.8, -0.05, 0.4, -0.8]


class _Space:
    def __init__(self, shape):
        self.shape = tuple(shape)


#: the fused env step advances the simulator state inside catppo_rollout_pre (A/B switch, read once)
_FUSED_SIM_COPY = os.environ.get("CATPPO_FUSED_SIM_COPY", "1") != "0"


class SyntheticSolo12Sim:
    """Pre-generated sim-state streams (SURVEY 8d distributions), resident in HBM.

    Packed layout per env and step (floats): joint_pos 12 | joint_vel 12 | joint_acc 12 |
    applied_torque 12 | projected_gravity_b 3 | root_pos_w 3 | command 3 | last_air_time B |
    first_contact B | net_forces_w_history H*B*3 | reward 1 | hard_reset 1 | obs D.
    """

    H = 3

    def __init__(self, num_envs: int, obs_dim: int, device, seed: int, stream_steps: int):
        self.N, self.D, self.device, self.S = num_envs, obs_dim, torch.device(device), stream_steps
        J, B, H = len(SOLO12_JOINTS), len(SOLO12_BODIES), self.H
        self.J, self.B = J, B
        fields = [("joint_pos", J), ("joint_vel", J), ("joint_acc", J), ("applied_torque", J),
                  ("projected_gravity_b", 3), ("root_pos_w", 3), ("command", 3), ("last_air_time", B),
                  ("first_contact", B), ("forces", H * B * 3), ("reward", 1), ("hard_reset", 1), ("obs", obs_dim)]
        self.off, o = {}, 0
        for name, w in fields:
            self.off[name] = (o, w)
            o += w
        self.F = (o + 3) // 4 * 4
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        N, S, F = num_envs, stream_steps, self.F
        st = torch.zeros(S, N, F, device=self.device)

        def put(name, value):
            a, w = self.off[name]
            st[:, :, a:a + w] = value.reshape(S, N, w)

        def randn(*shape):
            return torch.randn(*shape, device=self.device, generator=g)

        def rand(*shape):
            return torch.rand(*shape, device=self.device, generator=g)

        dq = torch.tensor(DEFAULT_JOINT_POS, device=self.device)
        put("joint_pos", dq + randn(S, N, J) * 0.5)
        put("joint_vel", randn(S, N, J) * 8.0)
        put("joint_acc", randn(S, N, J) * 400.0)
        put("applied_torque", randn(S, N, J) * 2.0)
        grav = torch.cat([randn(S, N, 2) * 0.12, -torch.ones(S, N, 1, device=self.device)], -1)
        grav[..., 2] = torch.where(rand(S, N) < 0.003, 1.0, -1.0)      # rare roll-over
        put("projected_gravity_b", grav / grav.norm(dim=-1, keepdim=True))
        put("root_pos_w", torch.cat([randn(S, N, 2), 0.25 + randn(S, N, 1) * 0.03], -1))
        lo = torch.tensor([-0.3, -0.7, -0.78], device=self.device)
        hi = torch.tensor([1.0, 0.7, 0.78], device=self.device)
        cmd = lo + rand(S, N, 3) * (hi - lo)
        cmd = cmd * (cmd.norm(dim=-1, keepdim=True) > 0.1)              # dead-zone like the reference commands
        cmd = cmd * (rand(S, N, 1) > 0.02)                              # rel_standing_envs = 0.02
        put("command", cmd)
        put("last_air_time", rand(S, N, B) * 0.5)
        put("first_contact", (rand(S, N, B) < 0.1).float())
        is_foot = torch.tensor([n.endswith("_FOOT") for n in SOLO12_BODIES], device=self.device)
        p_contact = torch.where(is_foot, 0.5, 0.002)
        forces = randn(S, N, H, B, 3).abs() * 20.0 * (rand(S, N, H, B, 1) < p_contact.view(1, 1, 1, B, 1))
        put("forces", forces)
        put("reward", rand(S, N, 1) * 1.5)
        put("hard_reset", (rand(S, N, 1) < 0.01).float())
        put("obs", randn(S, N, obs_dim))
        self.stream = st
        self._slabs = list(st.unbind(0))
        self.cur = torch.zeros(N, F, device=self.device)       # persistent "simulator state" buffers
        self.cursor = -1
        self.default_joint_pos = dq.repeat(N, 1).contiguous()
        self._build_scene()

    def view(self, name):
        a, w = self.off[name]
        return self.cur[:, a:a + w]

    def _build_scene(self):
        N, H, B = self.N, self.H, self.B
        a, w = self.off["forces"]
        forces = self.cur.as_strided((N, H, B, 3), (self.F, B * 3, 3, 1), self.cur.storage_offset() + a)
        robot = types.SimpleNamespace(
            joint_names=list(SOLO12_JOINTS), body_names=list(SOLO12_BODIES),
            data=types.SimpleNamespace(
                joint_pos=self.view("joint_pos"), default_joint_pos=self.default_joint_pos,
                joint_vel=self.view("joint_vel"), joint_acc=self.view("joint_acc"),
                applied_torque=self.view("applied_torque"), projected_gravity_b=self.view("projected_gravity_b"),
                root_pos_w=self.view("root_pos_w")))
        fc = self.view("first_contact")
        sensor = types.SimpleNamespace(
            joint_names=[], body_names=list(SOLO12_BODIES),
            data=types.SimpleNamespace(net_forces_w_history=forces, last_air_time=self.view("last_air_time")),
            first_contact_f32=fc, compute_first_contact=lambda dt: fc > 0.5)
        self.scene = {"robot": robot, "contact_forces": sensor}

    def advance(self, action=None) -> torch.Tensor:
        """(``action`` is ignored: the stream is open loop)  move to the next step of the stream WITHOUT touching the state buffer: returns the slab that holds the new
        state (the fused env step hands it to catppo_rollout_pre, which copies it into ``cur`` inside its own launch)"""
        self.cursor = (self.cursor + 1) % self.S
        return self._slabs[self.cursor]

    def step(self, action=None):
        self.cur.copy_(self.advance())                         # "scene.update": one contiguous slab

    # run state: the state buffer and the position in the stream; the stream itself is a pure
    # function of (seed, N, obs_dim, stream_steps) - those are part of the fingerprint and construction regenerates it
    def fingerprint(self) -> dict:
        return {"stream_steps": int(self.S)}

    def state_dict(self) -> dict:
        return {"cur": self.cur, "cursor": int(self.cursor)}

    def check_state_dict(self, sd: dict):
        s = sd["cur"]
        if tuple(s.shape) != tuple(self.cur.shape) or s.dtype != self.cur.dtype:
            raise ValueError(f"run state: simulator state is {tuple(s.shape)} {s.dtype}, this simulator's is "
                             f"{tuple(self.cur.shape)} {self.cur.dtype}")
        if not -1 <= int(sd["cursor"]) < len(self._slabs):
            raise ValueError(f"run state: simulator cursor {sd['cursor']} outside this simulator's {len(self._slabs)} slabs")

    def load_state_dict(self, sd: dict):
        """in place: term descriptors, the fused step and the servo kernel's argument block hold the address of ``cur``"""
        self.check_state_dict(sd)
        self.cur.copy_(sd["cur"])
        self.cursor = int(sd["cursor"])


class Solo12ServoSim(SyntheticSolo12Sim):
    """Closed-loop stand-in simulator: the Solo12 servo surrogate (csrc/servo_sim.hip).

    Same surface and packed layout as ``SyntheticSolo12Sim`` (plus 14 floats of private state per env, field ``servo``),
    but nothing is pre-generated: ``advance(action)`` launches one kernel that maps (state buffer, action) to the next
    state in one of two slabs and returns that slab; ``step(action)`` also copies it into the state buffer ``cur``.
    ``episode_length`` / ``reset`` are the env's own buffers (the kernel reads which envs ended their episode in the
    previous step and how far the others are); ``env_offset`` is the global id of env 0 of an env-sharded run."""

    NX = 14

    def __init__(self, num_envs: int, obs_dim: int, device, seed: int, syn, dt: float, decimation: int,
                 max_episode_length: int, episode_length: torch.Tensor, reset: torch.Tensor, env_offset: int = 0,
                 policy_obs_dim: int = 0, events: bool = False, commands: bool = False, terminations: bool = False,
                 actions: bool = False, actuators: bool = False, randomize: bool = False, history_floats: int = 0,
                 disturbances: bool = False, event_timer: bool | None = None):
        """``policy_obs_dim`` = P > 0: the row gets a second observation field ``policy_obs`` of P floats (padded to a
        multiple of 4) that ``set_observation_table`` configures; the raw field ``obs`` stays what it is.
        ``events``: the descriptor carries the event descriptor, too, and ``set_event_block`` configures it.
        ``commands``: the row gets one more 16-byte field ``cmd_state`` behind everything else (float 0: the time left until
        the timed resample), the descriptor carries the command descriptor and ``set_command_block`` configures it.
        ``terminations``: the row gets one more 16-byte field ``term_state`` behind everything else (float 0: the terms that
        fired in the step, bit k = term k), the descriptor carries the termination descriptor and
        ``set_termination_table`` configures it.
        ``actions``: the descriptor carries the action descriptor and ``set_action_table`` configures it (which action
        column drives which joint, through which scale, offset and clip, as what kind of target); the row stays what it is.
        ``actuators``: the row gets one more field ``act_hist`` of 48 floats behind everything else (three slots of processed
        actions), the descriptor carries the action and the actuator descriptors and ``set_actuator_table`` configures the
        latter (per-joint gains, inertia, effort limits, DC-motor clamps and the actuator delay).
        ``randomize``: the descriptor carries the actuator and the randomisation descriptors and ``set_randomize_block``
        configures the latter (per-env gains, joint friction, armature and base mass); the row is that of ``actuators``.
        ``history_floats`` = T > 0 (needs ``policy_obs_dim``): the row gets a second policy field ``policy_obs_hist`` of T
        floats (padded to a multiple of 4) behind ``row_floats``, the part of the row the kernel stages in LDS, so ``F``, the
        stride of the state buffers, exceeds ``row_floats``; the descriptor carries all eight descriptors and
        ``set_history_table`` configures the last (which float of the field shows which float of the current frame, and how
        far the next slot is).  The row is that of ``randomize``.
        ``disturbances`` (implies ``events``): the event block is the extended one of ``native.SERVO_EVENT_FLOATS_EXT`` words
        (a timed push, an external wrench); ``event_timer`` (default: as ``disturbances``) gives the row one more 16-byte field
        ``ev_state`` (float 0: the time left until the env's next timed push), which the timed push needs"""
        self._disturbances = bool(disturbances)
        self._event_timer = self._disturbances if event_timer is None else bool(event_timer)
        if self._event_timer and not self._disturbances:
            raise ValueError("the ev_state field goes with the extended event block (disturbances = True)")
        events = bool(events or self._disturbances)
        self.T = int(history_floats)
        if self.T and not (int(policy_obs_dim) and 1 <= self.T <= native.SERVO_OBS_HISTORY_MAX_FLOATS):
            raise ValueError(f"an observation history needs a policy observation and 1 <= floats <= "
                             f"{native.SERVO_OBS_HISTORY_MAX_FLOATS} (got policy_obs_dim {policy_obs_dim}, floats {self.T})")
        randomize = bool(randomize or self.T)
        actuators = bool(actuators or randomize)
        actions = bool(actions or actuators)
        self.N, self.D, self.device = num_envs, obs_dim, torch.device(device)
        self.P = int(policy_obs_dim)
        if self.P and not (1 <= self.P <= native.SERVO_OBS_MAX_WIDTH and obs_dim == native.SERVO_OBS_RAW):
            raise ValueError(f"a policy observation needs 1 <= width <= {native.SERVO_OBS_MAX_WIDTH} and the raw observation "
                             f"of {native.SERVO_OBS_RAW} floats (got width {self.P}, obs_dim {obs_dim})")
        J, B, H = len(SOLO12_JOINTS), len(SOLO12_BODIES), self.H
        self.J, self.B = J, B
        fields = [("joint_pos", J), ("joint_vel", J), ("joint_acc", J), ("applied_torque", J),
                  ("projected_gravity_b", 3), ("root_pos_w", 3), ("command", 3), ("last_air_time", B),
                  ("first_contact", B), ("forces", H * B * 3), ("reward", 1), ("hard_reset", 1), ("obs", obs_dim),
                  ("servo", self.NX)]
        self.off, o = {}, 0
        for name, w in fields:
            self.off[name] = (o, w)
            o += w
        self.F = (o + 3) // 4 * 4
        if self.P:                                                      # behind everything else, on a 16-byte boundary
            self.off["policy_obs"] = (self.F, self.P)
            self.F += (self.P + 3) // 4 * 4
        if commands:
            self.off["cmd_state"] = (self.F, 4)
            self.F += 4
        if terminations:
            self.off["term_state"] = (self.F, 4)
            self.F += 4
        if actuators:
            self.off["act_hist"] = (self.F, native.SERVO_ACT_HIST_FLOATS)
            self.F += native.SERVO_ACT_HIST_FLOATS
        if self._event_timer:
            self.off["ev_state"] = (self.F, 4)
            self.F += 4
        self.row_floats = self.F                                        # what the kernel assembles in LDS
        if self.T:                                                      # behind it, written straight to memory
            self.off["policy_obs_hist"] = (self.F, self.T)
            self.F += (self.T + 3) // 4 * 4
        self.cur = torch.zeros(num_envs, self.F, device=self.device)
        self._slabs = [torch.zeros(num_envs, self.F, device=self.device) for _ in range(2)]
        self.cursor = -1
        self.default_joint_pos = torch.tensor(DEFAULT_JOINT_POS, device=self.device).repeat(num_envs, 1).contiguous()
        self._episode_length, self._reset = episode_length, reset       # referenced by the descriptor: keep alive
        self._nat = native.get(self.device)
        # the descriptor carries the descriptors of every level of native.SERVO_EXTS up to the highest that is switched on
        switched = (self.P, events, commands, terminations, actions, actuators, randomize, self.T)
        top = max((level for level, on in enumerate(switched) if on), default=None)
        d = self._desc = (native.ServoSimRewards if top is None else native.SERVO_EXTS[top][2])()
        d.N, d.env_offset, d.row_stride, d.row_floats = num_envs, int(env_offset), self.F, self.row_floats
        d.obs_dim, d.H, d.B = obs_dim, H, B
        names = {"projected_gravity": "projected_gravity_b", "root_pos": "root_pos_w"}
        for n in native.SERVO_OFFSETS:
            setattr(d, "off_" + n, self.off[names.get(n, n)][0])
        d.state_in, d.reset, d.episode_length = self.cur.data_ptr(), reset.data_ptr(), episode_length.data_ptr()
        d.max_episode_length, d.decimation = int(max_episode_length), int(decimation)
        d.resample_steps, d.seed = int(syn.servo_resample_steps), int(seed) & (2 ** 64 - 1)
        for j, v in enumerate(DEFAULT_JOINT_POS):
            d.default_joint_pos[j] = v
        d.dt = dt
        for n in native.SERVO_CONSTANTS[1:]:
            setattr(d, n, float(getattr(syn, "servo_" + n)))
        self._fixed_command = self._eval_record = self._trace = None    # referenced by the descriptor: keep alive
        self._reward_record = self._reward_table = None                 # likewise; allocated by the first set_reward_table
        self._reward_entries = []
        self._obs_table = None                                          # device table of the observation descriptor
        self._obs_entries = []
        self._events = bool(events)
        self._event_block, self._event_words = None, None               # device block of the event descriptor, its host copy
        self._commands = bool(commands)
        self._command_block, self._command_words = None, None           # likewise, of the command descriptor
        self._terminations = bool(terminations)
        self._term_table = self._term_record = None                     # device table and record of the termination descriptor
        self._term_entries = []
        self._actions = bool(actions)
        self._action_table, self._action_entries, self.action_width = None, [], J   # device table of the action descriptor
        self._actuators = bool(actuators)
        self._actuator_table, self._actuator_entries = None, []         # device table of the actuator descriptor
        self._randomize = bool(randomize)
        self._randomize_block, self._randomize_words = None, None       # device block of the randomisation descriptor, its host copy
        self._history_map, self._history_words = None, None             # device map of the history descriptor, its host copy
        self._plant_table, self._plant_undo = None, None                # device table of the plant descriptor; how to detach it
        self._build_scene()

    def _table(self, t, width, what, lead=()):
        if t is None:
            return None
        shape = (*lead, self.N, width)
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.device == self.cur.device
                and tuple(t.shape) == shape):
            raise ValueError(f"{what} must be a contiguous fp32 tensor of shape {shape} on {self.cur.device}")
        return t

    def set_fixed_command(self, t: torch.Tensor | None, segment_steps: int | None = None):
        """``t`` [N, 3]: env i's command is row i in every step and every episode, as it stands (no dead zone, no standing
        fraction); None: the simulator draws the commands itself again.  The kernel reads the tensor at every launch.

        ``t`` [S, N, 3] with ``segment_steps`` = L >= 1 is a schedule: a step that starts at episode length ``k`` uses row
        ``min(k // L, S - 1)`` of env i.  It is keyed on the episode length like command resampling, so an episode that
        ends restarts its schedule at segment 0."""
        if t is not None and isinstance(t, torch.Tensor) and t.dim() == 3:
            if segment_steps is None or int(segment_steps) < 1:
                raise ValueError("a command schedule [S, N, 3] needs segment_steps >= 1")
            if t.shape[0] < 1:
                raise ValueError("a command schedule needs at least one segment")
            table, segments = self._table(t, 3, "a command schedule", lead=(int(t.shape[0]),)), int(t.shape[0])
        else:
            if segment_steps is not None:
                raise ValueError("segment_steps goes with a command schedule [S, N, 3]")
            table, segments = self._table(t, 3, "fixed commands"), 0
        self._fixed_command = table
        d = self._desc
        d.fixed_command = None if table is None else table.data_ptr()
        d.fixed_segments, d.fixed_segment_steps = segments, int(segment_steps) if segments else 0

    def set_eval_record(self, t: torch.Tensor | None):
        """``t`` [N, 12] (``native.SERVO_EVAL_FIELDS``): every following step adds its terms to row i of the record inside
        the simulator's own launch, ``reset()`` zeroes it; None: detach."""
        self._eval_record = self._table(t, len(native.SERVO_EVAL_FIELDS), "the evaluation record")
        self._desc.eval = None if t is None else t.data_ptr()

    def set_trace(self, t: torch.Tensor | None):
        """``t`` [T, K, 72] (``native.SERVO_TRACE_FIELDS``), zeroed by the caller: every following step writes one row per
        env 0 .. K - 1 inside the simulator's own launch, at the slot the env's evaluation record has counted so far (so
        an evaluation record must be attached while it steps); slots >= T are dropped.  None: detach."""
        if t is not None:
            ok = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and t.device == self.cur.device
            if not (ok and t.dim() == 3 and t.shape[0] >= 1 and 1 <= t.shape[1] <= self.N
                    and t.shape[2] == native.SERVO_TRACE_FLOATS):
                raise ValueError(f"the trace must be a contiguous fp32 tensor of shape (T >= 1, 1 <= K <= {self.N}, "
                                 f"{native.SERVO_TRACE_FLOATS}) on {self.cur.device}")
        self._trace = t
        d = self._desc
        d.trace = None if t is None else t.data_ptr()
        d.trace_capacity, d.trace_envs = (0, 0) if t is None else (int(t.shape[0]), int(t.shape[1]))

    def set_reward_table(self, entries):
        """``entries``: up to 15 ``(kind, joint_mask, weight, param)`` (``native.SERVO_REWARD_KINDS``; what the terms of
        ``mdp.rewards`` describe).  Every following step writes their sum into the row's ``reward`` field instead of the
        built-in expression and keeps the per-term episode sums in ``reward_record`` [N, 32], inside the simulator's own
        launch.  The table lives on the device and is rewritten here, in stream order: a new weight is in the next launch.
        Empty or None: back to the built-in reward.  The entries are checked here - the library cannot read them."""
        entries = [(int(k), int(m), float(w), float(p)) for k, m, w, p in (entries or [])]
        if len(entries) > native.SERVO_REWARD_MAX_TERMS:
            raise ValueError(f"{len(entries)} reward terms: the simulator evaluates at most {native.SERVO_REWARD_MAX_TERMS}")
        for k, m, w, p in entries:
            if not 1 <= k <= 16:
                raise ValueError(f"unknown reward kind {k}")
            if k <= 4 and not p > 0.0:
                raise ValueError(f"reward kind {k} needs param > 0, got {p}")
            if 7 <= k <= 10 and not (m != 0 and (m & ~0xFFF) == 0):
                raise ValueError(f"reward kind {k} needs a joint mask in 1 .. 0xFFF, got {m:#x}")
            if k == 11 and self.D < 45:
                raise ValueError(f"action_rate_l2 reads the last-action block of the observation: obs_dim {self.D} < 45")
        d = self._desc
        self._reward_entries = entries
        if not entries:
            d.reward_terms, d.reward_rec, d.reward_table = 0, None, None
            return
        if self._reward_record is None:
            self._reward_record = torch.zeros(self.N, native.SERVO_REWARD_FLOATS, device=self.device)
            self._reward_table = torch.zeros(native.SERVO_REWARD_MAX_TERMS * C.sizeof(native.ServoRewardTerm),
                                             dtype=torch.uint8, device=self.device)
        host = (native.ServoRewardTerm * native.SERVO_REWARD_MAX_TERMS)()
        for i, (k, m, w, p) in enumerate(entries):
            host[i].kind, host[i].joint_mask, host[i].weight, host[i].param = k, m, w, p
        self._reward_table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        d.reward_terms, d.reward_rec, d.reward_table = len(entries), self._reward_record.data_ptr(), self._reward_table.data_ptr()

    @property
    def reward_record(self):
        """[N, 32] fp32 or None: 0..14 running sums per term | 15 zero | 16..30 sums of the ended episodes | 31 their count"""
        return self._reward_record if self._reward_entries else None

    def set_observation_table(self, entries):
        """``entries``: exactly ``policy_obs_dim`` rows ``(src, flags, bias, noise_lo, noise_width, clip_lo, clip_hi, scale)``
        (``native.ServoObsEntry``; what ``mdp.observation_manager.build_table`` returns).  Every following launch, init
        launches included, fills the row's ``policy_obs`` field from the finished raw observation.  The table lives on the
        device and is rewritten here, in stream order: new noise bits are in the next launch.  The entries are checked
        here - the library cannot read them (the kernel clamps ``src`` anyway)."""
        entries = [tuple(e) for e in entries]
        if not self.P:
            raise ValueError("this simulator was built without a policy observation field (policy_obs_dim = 0)")
        if len(entries) != self.P:
            raise ValueError(f"{len(entries)} observation entries, the row's policy observation has {self.P} floats")
        host = (native.ServoObsEntry * native.SERVO_OBS_MAX_WIDTH)()
        for i, e in enumerate(entries):
            src, flags = int(e[0]), int(e[1])
            vals = [float(v) for v in e[2:]]
            if len(vals) != 6 or not 0 <= src < native.SERVO_OBS_RAW or flags & ~7:
                raise ValueError(f"observation entry {i}: src must be in 0 .. {native.SERVO_OBS_RAW - 1}, flags in 0 .. 7 and "
                                 f"six floats must follow, got {e!r}")
            if not all(math.isfinite(v) for v in vals) or vals[2] < 0.0 or vals[3] > vals[4]:
                raise ValueError(f"observation entry {i}: floats must be finite, noise_width >= 0 and clip_lo <= clip_hi, got {e!r}")
            h = host[i]
            h.src, h.flags = src, flags
            h.bias, h.noise_lo, h.noise_width, h.clip_lo, h.clip_hi, h.scale = vals
        if self._obs_table is None:
            self._obs_table = torch.zeros(C.sizeof(host), dtype=torch.uint8, device=self.device)
            d = self._desc
            d.obs.width, d.obs.off_policy_obs, d.obs.table = self.P, self.off["policy_obs"][0], self._obs_table.data_ptr()
            self._announce()                                            # from now on every launch fills the field
        self._obs_table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        self._obs_entries = entries

    def set_event_block(self, words):
        """``words``: the ``native.SERVO_EVENT_FLOATS`` fp32 words of the event block (``mdp.event_manager.pack``; words 0
        and 2 hold the flags and the bucket count as integers).  Every following launch, init launches included, applies
        the events the flags name.  The block lives on the device and is rewritten here and nowhere else, in stream order:
        a new flag word is in the next launch (when nothing but word 0 changed, that word alone is copied).  The values are
        checked here - the library cannot read them."""
        import numpy as np
        if not self._events:
            raise ValueError("this simulator was built without an event descriptor (events = False)")
        words = np.ascontiguousarray(words, np.float32)
        floats = native.SERVO_EVENT_FLOATS_EXT if self._disturbances else native.SERVO_EVENT_FLOATS
        if words.shape != (floats,):
            raise ValueError(f"the event block has {floats} words, got shape {words.shape}")
        W, WX = native.SERVO_EVENT_WORDS, native.SERVO_EVENT_WORDS_EXT
        ints = words.view(np.int32)
        flags, buckets = int(ints[W["flags"]]), int(ints[W["num_buckets"]])
        both = native.SERVO_EVENT_JOINT_SCALE | native.SERVO_EVENT_JOINT_OFFSET
        if flags & ~31 or flags & both == both:
            timed, wrench, per_ep = native.SERVO_EVENT_PUSH_TIMED, native.SERVO_EVENT_WRENCH, native.SERVO_EVENT_WRENCH_RESET
            if not self._disturbances or flags & ~(31 | timed | wrench | per_ep) or flags & both == both:
                raise ValueError(f"event block: flags {flags:#x} (known bits 1 .. 16; at most one joint-reset mode)")
            if flags & timed and flags & native.SERVO_EVENT_PUSH:
                raise ValueError(f"event block: flags {flags:#x} name both pushes; at most one is evaluated")
            if flags & timed and not self._event_timer:
                raise ValueError("event block: the timed push needs the row's ev_state field (event_timer = True)")
            if flags & per_ep and not flags & wrench:
                raise ValueError(f"event block: flags {flags:#x}: the per-episode bit goes with the wrench bit")
        if self._disturbances:
            if (words[[WX["T_width"], WX["force"] + 1, WX["torque"] + 1]] < 0).any() or words[WX["torque"] + 2:].any():
                raise ValueError("event block: every width of the extended words must be >= 0 and the spare words zero")
            # the timer's range is read whenever the timed bit is set, by a later copy of the flag word, too
            t_set = flags & native.SERVO_EVENT_PUSH_TIMED or words[[WX["T_lo"], WX["T_width"]]].any()
            if t_set and not float(words[WX["T_lo"]]) > 0.0:
                raise ValueError(f"event block: the timed push needs T_lo > 0, got {float(words[WX['T_lo']])}")
        if buckets < 1:
            raise ValueError(f"event block: num_buckets must be >= 1, got {buckets}")
        vals = np.delete(words, [W["flags"], W["num_buckets"]])
        if not np.isfinite(vals).all():
            raise ValueError("event block: every range and the probability must be finite")
        if not 0.0 <= float(words[W["p"]]) <= 1.0:
            raise ValueError(f"event block: the push probability must be in [0, 1], got {float(words[W['p']])}")
        if (words[5:30:2] < 0).any() or words[[3, 30, 31]].any():
            raise ValueError("event block: every width must be >= 0 and the spare words zero")
        if flags & native.SERVO_EVENT_FRICTION and float(words[W["friction"]]) < 0.0:
            raise ValueError("event block: the friction range must be >= 0")
        if int(self._desc.max_episode_length) >= 2 ** 27:
            raise ValueError("events need max_episode_length < 2^27: the step index is part of a Philox counter word")
        if self._event_block is None:
            self._event_block = torch.zeros(floats, dtype=torch.float32, device=self.device)
            d = self._desc
            d.ev.block, d.ev.floats = self._event_block.data_ptr(), floats
            d.ev.reserved = self.off["ev_state"][0] if self._event_timer else 0      # off_ev_state
            self._announce()                                            # from now on every launch reads the block
        old = self._event_words
        if old is not None and (old.view(np.int32)[1:] == ints[1:]).all():
            self._event_block[:1].copy_(torch.from_numpy(words[:1].copy()))
        else:
            self._event_block.copy_(torch.from_numpy(words.copy()))
        self._event_words = words.copy()

    def _announce(self):
        """``reserved`` names the descriptors behind the 368 bytes that are configured by now"""
        self._desc.reserved = next((magic for _, magic, _, attr in reversed(native.SERVO_EXTS) if getattr(self, attr) is not None), 0)

    def set_command_block(self, words):
        """``words``: the ``native.SERVO_COMMAND_FLOATS`` fp32 words of the command block (``mdp.command_manager.pack``; word 0
        holds the flags as an integer).  Every following launch, init launches included, runs the configured command process
        instead of the built-in generator.  The block lives on the device and is rewritten here and nowhere else, in stream
        order: new ranges are in the next launch (when only the ranges changed, those six words alone are copied).  The
        values are checked here - the library cannot read them."""
        import numpy as np
        if not self._commands:
            raise ValueError("this simulator was built without a command descriptor (commands = False)")
        words = np.ascontiguousarray(words, np.float32)
        if words.shape != (native.SERVO_COMMAND_FLOATS,):
            raise ValueError(f"the command block has {native.SERVO_COMMAND_FLOATS} words, got shape {words.shape}")
        W = native.SERVO_COMMAND_WORDS
        flags = int(words.view(np.int32)[W["flags"]])
        if flags & ~15:
            raise ValueError(f"command block: flags {flags:#x} (known bits 1 .. 8)")
        if not np.isfinite(words[1:]).all():
            raise ValueError("command block: every range, probability and time must be finite")
        if float(words[W["dz"]]) < 0.0 or any(not 0.0 <= float(words[W[k]]) <= 1.0 for k in ("p_still", "p_move", "rel_standing")):
            raise ValueError("command block: the dead zone must be >= 0 and p_still, p_move, rel_standing in [0, 1]")
        if (words[W["ranges"] + 1:W["ranges"] + 6:2] < 0).any() or float(words[W["T_width"]]) < 0.0 or words[13:].any():
            raise ValueError("command block: every width must be >= 0 and the spare words zero")
        if not float(words[W["T_lo"]]) > 0.0:
            raise ValueError("command block: the resampling time must be > 0")
        if int(self._desc.max_episode_length) >= 2 ** 27:
            raise ValueError("commands need max_episode_length < 2^27: the step index is part of a Philox counter word")
        if self._command_block is None:
            self._command_block = torch.zeros(native.SERVO_COMMAND_FLOATS, dtype=torch.float32, device=self.device)
            c = self._desc.cmd
            c.block, c.floats, c.off_cmd_state = self._command_block.data_ptr(), native.SERVO_COMMAND_FLOATS, self.off["cmd_state"][0]
            self._announce()                                            # from now on every launch reads the block
        old, a = self._command_words, W["ranges"]
        if old is not None and (np.delete(old, range(a, a + 6)).view(np.int32) == np.delete(words, range(a, a + 6)).view(np.int32)).all():
            self._command_block[a:a + 6].copy_(torch.from_numpy(words[a:a + 6].copy()))
        else:
            self._command_block.copy_(torch.from_numpy(words.copy()))
        self._command_words = words.copy()

    def set_termination_table(self, entries):
        """``entries``: 1 to 15 ``(kind, mask, p0, p1)`` (``native.SERVO_TERM_KINDS``; what the terms of ``mdp.terminations``
        describe).  Every following step decides with them when an episode is over, writes the fired terms into the row's
        ``term_state`` and counts them at episode ends in ``termination_record`` [N, 16], inside the simulator's own launch.
        The table lives on the device and is rewritten here and nowhere else, in stream order: new params are in the next
        launch.  Kinds, masks and the number of entries are fixed by the first call.  The entries are checked here - the
        library cannot read them."""
        if not self._terminations:
            raise ValueError("this simulator was built without a termination descriptor (terminations = False)")
        entries = [(int(k), int(m), float(p0), float(p1)) for k, m, p0, p1 in (entries or [])]
        if not 1 <= len(entries) <= native.SERVO_TERM_MAX_TERMS:
            raise ValueError(f"{len(entries)} termination terms: the simulator evaluates 1 .. {native.SERVO_TERM_MAX_TERMS}")
        for k, m, p0, p1 in entries:
            if not 1 <= k <= 8:
                raise ValueError(f"unknown termination kind {k}")
            if not (math.isfinite(p0) and math.isfinite(p1)):
                raise ValueError(f"termination kind {k}: params must be finite, got {p0}, {p1}")
            if k == 2 and not (m != 0 and (m & ~0x1FFFF) == 0):
                raise ValueError(f"termination kind {k} needs a body mask in 1 .. 0x1FFFF, got {m:#x}")
            if k in (6, 7) and not (m != 0 and (m & ~0xFFF) == 0):
                raise ValueError(f"termination kind {k} needs a joint mask in 1 .. 0xFFF, got {m:#x}")
            if k == 6 and p1 < p0:
                raise ValueError(f"termination kind 6 needs p0 <= p1, got {p0} > {p1}")
        if self._term_entries and [e[:2] for e in entries] != [e[:2] for e in self._term_entries]:
            raise ValueError("the termination table's kinds and masks are fixed by the first call; only params may change")
        host = (native.ServoTermEntry * native.SERVO_TERM_MAX_TERMS)()
        for i, (k, m, p0, p1) in enumerate(entries):
            host[i].kind, host[i].mask, host[i].p0, host[i].p1 = k, m, p0, p1
        if self._term_table is None:
            self._term_table = torch.zeros(C.sizeof(host), dtype=torch.uint8, device=self.device)
            self._term_record = torch.zeros(self.N, native.SERVO_TERM_FLOATS, device=self.device)
            t = self._desc.term
            t.table, t.rec = self._term_table.data_ptr(), self._term_record.data_ptr()
            t.terms, t.off_term_state = len(entries), self.off["term_state"][0]
            self._announce()                                            # from now on every launch evaluates the table
        self._term_table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        self._term_entries = entries

    def set_action_table(self, entries, width: int):
        """``entries``: 12 ``(col, kind, scale, offset, clip)``, one per simulator joint (``native.SERVO_ACTION_KINDS``; ``col``
        -1 and kind 0 for a joint no term drives; ``clip`` None or ``(lo, hi)``; what ``mdp.actions.build_table`` describes),
        ``width`` = A the width of the action.  Every following step reads an action [N, A] and turns it into servo targets
        with the table, inside the simulator's own launch.  The table lives on the device and is rewritten here and nowhere
        else, in stream order: new scales, offsets and clips are in the next launch.  Columns, kinds, the clip bits and the
        width are fixed by the first call.  The entries are checked here - the library cannot read them."""
        if not self._actions:
            raise ValueError("this simulator was built without an action descriptor (actions = False)")
        width = int(width)
        if not 1 <= width <= self.J:
            raise ValueError(f"an action of width {width}: the simulator reads 1 .. {self.J} columns")
        entries = [(int(c), int(k), float(sc), float(of), None if cl is None else (float(cl[0]), float(cl[1])))
                   for c, k, sc, of, cl in (entries or [])]
        if len(entries) != self.J:
            raise ValueError(f"the action table has one entry per joint ({self.J}), got {len(entries)}")
        cols = [c for c, k, *_ in entries if k != 0]
        for j, (c, k, sc, of, cl) in enumerate(entries):
            if not 0 <= k <= 4:
                raise ValueError(f"joint {j}: unknown action kind {k}")
            if (k == 0) != (c == -1) or not -1 <= c < width:
                raise ValueError(f"joint {j}: column {c} with kind {k} (a driven joint has a column in 0 .. {width - 1}, any other -1)")
            if not (math.isfinite(sc) and math.isfinite(of)):
                raise ValueError(f"joint {j}: scale and offset must be finite, got {sc}, {of}")
            if cl is not None and not (math.isfinite(cl[0]) and math.isfinite(cl[1]) and cl[0] <= cl[1]):
                raise ValueError(f"joint {j}: a clip needs finite lo <= hi, got {cl}")
        if sorted(cols) != list(range(width)):
            raise ValueError(f"the action's {width} columns must drive one joint each, got columns {sorted(cols)}")
        fixed = [(c, k, cl is not None) for c, k, _, _, cl in entries]
        if self._action_entries and (fixed != [(c, k, cl is not None) for c, k, _, _, cl in self._action_entries]
                                     or width != self.action_width):
            raise ValueError("the action table's columns, kinds, clip bits and width are fixed by the first call; only scale, "
                             "offset and clip bounds may change")
        host = (native.ServoActionEntry * self.J)()
        for j, (c, k, sc, of, cl) in enumerate(entries):
            h = host[j]
            h.col, h.flags, h.scale, h.offset = c, k | (native.SERVO_ACTION_CLIP if cl is not None else 0), sc, of
            h.clip_lo, h.clip_hi = cl if cl is not None else (0.0, 0.0)
        if self._action_table is None:
            self._action_table = torch.zeros(C.sizeof(host), dtype=torch.uint8, device=self.device)
            a = self._desc.act
            a.table, a.width, a.reserved = self._action_table.data_ptr(), width, 0
            self.action_width = width
            self._announce()                                            # from now on every launch reads the table
        self._action_table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        self._action_entries = entries

    def identity_actuator_entries(self):
        """the table that must change nothing: the descriptor's own scalars on every joint, ideal PD, no delay"""
        d = self._desc
        return [dict(kp=float(d.kp), kd=float(d.kd), inertia=float(d.inertia), effort_limit=float(d.tau_max))] * self.J

    def set_actuator_table(self, entries):
        """``entries``: 12 dicts, one per simulator joint, with ``kp``, ``kd``, ``inertia`` (link inertia + armature),
        ``effort_limit`` and optionally ``saturation_effort``, ``velocity_limit``, ``dc_motor``, ``min_delay``, ``max_delay``
        (physics steps) and ``group`` (what ``mdp.actuators.build_table`` returns).  Every following step takes joint j's gains,
        inertia and clamp from entry j and lets its processed action act ``min_delay .. max_delay`` physics steps late, inside
        the simulator's own launch.  The table lives on the device and is rewritten here and nowhere else, in stream order:
        new gains and limits are in the next launch.  Kinds, groups and delay ranges are fixed by the first call.  A
        simulator without an action table gets the identity one here, so ``set_action_table`` comes first where it is
        wanted.  The entries are checked here - the library cannot read them."""
        if not self._actuators:
            raise ValueError("this simulator was built without an actuator descriptor (actuators = False)")
        entries = [dict(e) for e in (entries or [])]
        if len(entries) != self.J:
            raise ValueError(f"the actuator table has one entry per joint ({self.J}), got {len(entries)}")
        max_lag = native.SERVO_ACTUATOR_MAX_LAG_STEPS * int(self._desc.decimation)
        rows, ranges = [], {}
        for j, e in enumerate(entries):
            unknown = set(e) - {"kp", "kd", "inertia", "effort_limit", "saturation_effort", "velocity_limit", "dc_motor",
                                "min_delay", "max_delay", "group"}
            if unknown:
                raise ValueError(f"joint {j}: unknown actuator fields {sorted(unknown)}")
            vals = [float(e[k]) for k in ("kp", "kd", "inertia", "effort_limit")]
            vals += [float(e.get("saturation_effort") or 0.0), float(e.get("velocity_limit") or 0.0)]
            dc = bool(e.get("dc_motor", False))
            mn, mx, g = int(e.get("min_delay", 0)), int(e.get("max_delay", 0)), int(e.get("group", 0))
            if not all(math.isfinite(v) and v >= 0.0 for v in vals):
                raise ValueError(f"joint {j}: gains, inertia and limits must be finite and >= 0, got {e!r}")
            if not vals[2] > 0.0:
                raise ValueError(f"joint {j}: inertia must be > 0, got {vals[2]}")
            if dc and not (vals[4] > 0.0 and vals[5] > 0.0):
                raise ValueError(f"joint {j}: a DC motor needs saturation_effort > 0 and velocity_limit > 0, got {e!r}")
            if not (0 <= mn <= mx <= max_lag and mx <= 255):
                raise ValueError(f"joint {j}: the delay needs 0 <= min_delay <= max_delay <= {min(max_lag, 255)} physics steps "
                                 f"(three control steps), got {mn} .. {mx}")
            if not 0 <= g <= 255:
                raise ValueError(f"joint {j}: the group index must be in 0 .. 255, got {g}")
            if ranges.setdefault(g, (mn, mx)) != (mn, mx):
                raise ValueError(f"joint {j}: the joints of group {g} share one lag, so one delay range; got {ranges[g]} and {(mn, mx)}")
            rows.append((*vals, dc, mn, mx, g))
        fixed = [r[6:] for r in rows]
        if self._actuator_entries and fixed != [r[6:] for r in self._actuator_entries]:
            raise ValueError("the actuator table's kinds, groups and delay ranges are fixed by the first call; only gains, inertia "
                             "and limits may change")
        host = (native.ServoActuatorEntry * self.J)()
        for h, (kp, kd, inertia, eff, sat, vlim, dc, mn, mx, g) in zip(host, rows):
            h.kp, h.kd, h.inertia, h.effort_limit, h.saturation_effort, h.velocity_limit = kp, kd, inertia, eff, sat, vlim
            h.flags, h.delay = (native.SERVO_ACTUATOR_DC_MOTOR if dc else 0), mn | mx << 8 | g << 16
        if self._actuator_table is None:
            if self._action_table is None:                              # the identity action table (byte-identical to none)
                self.set_action_table([(j, native.SERVO_ACTION_KINDS["joint_position"], float(self._desc.action_scale),
                                        float(self._desc.default_joint_pos[j]), None) for j in range(self.J)], self.J)
            self._actuator_table = torch.zeros(C.sizeof(host), dtype=torch.uint8, device=self.device)
            a = self._desc.actu
            a.table, a.off_act_hist, a.reserved = self._actuator_table.data_ptr(), self.off["act_hist"][0], 0
            self._announce()                                            # from now on every launch reads the table
        self._actuator_table.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8))
        self._actuator_entries = rows

    def set_randomize_block(self, words):
        """``words``: the ``native.SERVO_RANDOMIZE_FLOATS`` fp32 words of the randomisation block (``mdp.randomization.pack``;
        words 0 .. 4 hold the flags, the operations and the masks as integers).  Every following step draws the env's gains,
        joint friction, armature and base mass inside the simulator's own launch.  The block lives on the device and is
        rewritten here and nowhere else, in stream order: a new flag word is in the next launch (when nothing but word 0
        changed, that word alone is copied).  A simulator without an actuator table gets the identity one here, so
        ``set_actuator_table`` comes first where it is wanted.  The values are checked here - the library cannot read them."""
        import numpy as np
        if not self._randomize:
            raise ValueError("this simulator was built without a randomisation descriptor (randomize = False)")
        words = np.ascontiguousarray(words, np.float32)
        if words.shape != (native.SERVO_RANDOMIZE_FLOATS,):
            raise ValueError(f"the randomisation block has {native.SERVO_RANDOMIZE_FLOATS} words, got shape {words.shape}")
        W, FL = native.SERVO_RANDOMIZE_WORDS, native.SERVO_RANDOMIZE_FLAGS
        ints = words.view(np.int32)
        flags, ops = int(ints[W["flags"]]), int(ints[W["ops"]])
        if flags & ~sum(FL.values()):
            raise ValueError(f"randomisation block: flags {flags:#x} has unknown bits")
        if ops & ~0xFFFFFF or any(((ops >> s) & 0xFF) not in native.SERVO_RANDOMIZE_OPS.values() for s in (0, 8, 16)):
            raise ValueError(f"randomisation block: operations {ops:#x} (one of 0 scale, 1 add, 2 abs per byte)")
        if any(int(ints[W[k]]) & ~0xFFF for k in ("gains_mask", "joint_mask")) or int(ints[W["body_mask"]]) & ~1:
            raise ValueError("randomisation block: the joint masks have 12 bits, the body mask one")
        if not np.isfinite(words[5:]).all() or words[5] != 0 or words[19] != 0:
            raise ValueError("randomisation block: every value must be finite and the spare words zero")
        if (words[7:16:2] < 0).any() or (words[W["armatures"]:] < 0).any():
            raise ValueError("randomisation block: every width and every armature must be >= 0")
        if not (words[W["m0"]] > 0 and words[W["g"]] > 0 and words[W["servo_inertia"]] > 0):
            raise ValueError("randomisation block: m0, g and servo_inertia must be > 0")
        if flags & FL["friction"] and ((ops >> 8) & 0xFF) == native.SERVO_RANDOMIZE_OPS["scale"]:
            raise ValueError("randomisation block: friction cannot be scaled, its nominal value is 0")
        if self._randomize_block is None:
            if self._actuator_table is None:                            # the identity actuator table (byte-identical to none)
                self.set_actuator_table(self.identity_actuator_entries())
            self._randomize_block = torch.zeros(native.SERVO_RANDOMIZE_FLOATS, dtype=torch.float32, device=self.device)
            r = self._desc.rnd
            r.block, r.reserved[0], r.reserved[1] = self._randomize_block.data_ptr(), 0, 0
            self._announce()                                            # from now on every launch reads the block
        old = self._randomize_words
        if old is not None and (old.view(np.int32)[1:] == ints[1:]).all():
            self._randomize_block[:1].copy_(torch.from_numpy(words[:1].copy()))
        else:
            self._randomize_block.copy_(torch.from_numpy(words.copy()))
        self._randomize_words = words.copy()

    def neutral_randomize_words(self):
        """the block that must change nothing: the switch off, no quantity, the simulator's own mass and servo inertia"""
        import numpy as np
        W = native.SERVO_RANDOMIZE_WORDS
        words = np.zeros(native.SERVO_RANDOMIZE_FLOATS, np.float32)
        words[W["m0"]] = np.float32(float(self._desc.weight) / 9.81)
        words[W["g"]], words[W["servo_inertia"]] = np.float32(9.81), np.float32(self._desc.inertia)
        # the nominal armatures: what the joints' inertia has above the servo's own (never read while the switch is off)
        for j, row in enumerate(self._actuator_entries):
            words[W["armatures"] + j] = max(np.float32(row[2]) - words[W["servo_inertia"]], np.float32(0))
        return words

    def set_fixed_plant(self, table: torch.Tensor | None):
        """``table`` [N, 8] (``native.SERVO_PLANT_WORDS``; what ``cleanrl.evaluate.plant_grid`` packs): row i pins the plant of
        env i - gains, joint friction, armature, base mass and actuator lag, each where its bit of word 0 is set - in every
        step and every episode, inside the simulator's own launch, after the lag draw and the randomisation block's draws.
        The kernel reads the tensor at every launch.  While a table is attached the descriptor is a ``native.ServoSimPlant``
        and the launch an evaluation launch, so a fixed-command table, an evaluation record or a trace must be attached when
        the simulator steps; a simulator without a robot gets the identity action and actuator tables and a switched-off
        randomisation block for the time.  None: back to exactly the descriptor class and ``reserved`` the simulator had.
        Every row is checked here (``mdp.randomization.check_plant_table``) - the library cannot read them."""
        if table is None:
            if self._plant_table is None:
                return
            cls, installed = self._plant_undo
            self._plant_table = self._plant_undo = None
            for attrs, field in installed:                              # what was installed for the table's time goes with it
                for name, empty in attrs:
                    setattr(self, name, empty)
                C.memset(C.addressof(getattr(self._desc, field)), 0, C.sizeof(getattr(self._desc, field)))
            old = cls()
            C.memmove(C.addressof(old), C.addressof(self._desc), C.sizeof(old))
            self._desc = old
            self._announce()
            return
        from cat_envs.tasks.utils.mdp import randomization as RZ
        if not self._actuators:
            raise ValueError("a plant table needs the row's act_hist field: this simulator was built without an actuator "
                             "descriptor (actuators = False)")
        t = self._table(table, native.SERVO_PLANT_FLOATS, "the plant table")
        entries = self._actuator_entries or [(float(self._desc.kp), float(self._desc.kd), float(self._desc.inertia))] * self.J
        si = float(self._desc.inertia) if self._randomize_words is None else float(self._randomize_words[native.SERVO_RANDOMIZE_WORDS["servo_inertia"]])
        RZ.check_plant_table(t.cpu().numpy(), int(self._desc.decimation), float(self._desc.dt),
                             [dict(kp=e[0], kd=e[1], inertia=e[2]) for e in entries], si)
        if self._plant_table is None:
            cls, new = type(self._desc), native.ServoSimPlant()
            C.memmove(C.addressof(new), C.addressof(self._desc), C.sizeof(self._desc))
            self._desc, installed = new, []
            had = self._action_table is None, self._actuator_table is None, self._randomize_block is None
            self._randomize, was = True, self._randomize
            try:
                if had[2]:                                              # installs the identity tables where they are missing, too
                    self.set_randomize_block(self.neutral_randomize_words())
            finally:
                self._randomize = was
            if had[0]:
                installed.append(((("_action_table", None), ("_action_entries", []), ("action_width", self.J)), "act"))
            if had[1]:
                installed.append(((("_actuator_table", None), ("_actuator_entries", [])), "actu"))
            if had[2]:
                installed.append(((("_randomize_block", None), ("_randomize_words", None)), "rnd"))
            self._plant_undo = (cls, installed)
        self._plant_table = t
        p = self._desc.plant
        p.table, p.reserved[0], p.reserved[1] = t.data_ptr(), 0, 0
        self._announce()

    def set_history_table(self, words):
        """``words``: the T words ``cur | w << 8 | newest << 16`` of the history map, one per float of the row's
        ``policy_obs_hist`` field (``mdp.observation_manager.history_map``): ``cur`` the float of the current frame that the
        float shows when it is new, ``w`` the frame width of its term (the float one slot later is ``w`` floats on), ``newest``
        set in a term's last slot.  Every following launch, init launches included, writes the field: the first frame of an
        episode fills every slot, any other step moves the input row's slots one back and puts the current frame last.  The
        map lives on the device and is rewritten here and nowhere else, in stream order.  ``set_observation_table`` comes
        first; a simulator without a robot gets the identity action and actuator tables and a switched-off randomisation
        block here.  Every word is checked here - the library cannot read them (the kernel clamps ``cur`` and ``i + w``
        anyway)."""
        import numpy as np
        if not self.T:
            raise ValueError("this simulator was built without a history field (history_floats = 0)")
        if self._obs_table is None:
            raise ValueError("the history shows the policy observation's frames: set_observation_table comes first")
        words = np.ascontiguousarray(words, np.uint32)
        if words.shape != (self.T,):
            raise ValueError(f"the history map has one word per float of the field ({self.T}), got shape {words.shape}")
        cur, w, newest = words & 0xFF, (words >> 8) & 0xFF, (words >> 16) & 1
        if (words >> 17).any():
            raise ValueError("history map: the bits above 16 must be zero")
        i = 0
        while i < self.T:
            # one term: H slots of w floats each, slot s float k shows cur0 + k; only the last slot is the newest
            wi, c0 = int(w[i]), int(cur[i])
            if not 1 <= wi <= self.P:
                raise ValueError(f"history map: word {i} has frame width {wi}, the current frame has {self.P} floats")
            j, slots = i, 0
            while j < self.T and int(w[j]) == wi and int(cur[j]) == c0 and (slots == 0 or not newest[j - 1]):
                blk = slice(j, j + wi)
                ok = (j + wi <= self.T and (w[blk] == wi).all() and (cur[blk] == c0 + np.arange(wi)).all()
                      and c0 + wi <= self.P and (newest[blk] == newest[j]).all())
                if not ok:
                    raise ValueError(f"history map: the {wi} words from {j} on are not one slot of a term "
                                     f"(cur {c0} .. {c0 + wi - 1}, one width, one newest bit)")
                j, slots = j + wi, slots + 1
            if not newest[j - 1] or slots > native.SERVO_OBS_HISTORY_MAX_DEPTH:
                raise ValueError(f"history map: the term from word {i} on has {slots} slots and "
                                 f"{'no' if not newest[j - 1] else 'a'} newest one (at most "
                                 f"{native.SERVO_OBS_HISTORY_MAX_DEPTH} slots, the last one the newest)")
            i = j
        if self._history_map is None:
            if self._randomize_block is None:                           # the neutral block (byte-identical to none)
                self.set_randomize_block(self.neutral_randomize_words())
            self._history_map = torch.zeros((self.T + 3) // 4 * 4, dtype=torch.int32, device=self.device)
            h = self._desc.hist
            h.map, h.off_hist, h.floats = self._history_map.data_ptr(), self.off["policy_obs_hist"][0], self.T
            self._announce()                                            # from now on every launch writes the field
        self._history_map[:self.T].copy_(torch.from_numpy(words.view(np.int32).copy()))
        self._history_words = words.copy()

    @property
    def history_words(self):
        """the history map as last written (a host copy), or None"""
        return None if self._history_words is None else self._history_words.copy()

    @property
    def randomize_words(self):
        """the randomisation block as last written (a host copy), or None"""
        return None if self._randomize_words is None else self._randomize_words.copy()

    @property
    def termination_record(self):
        """[N, 16] fp32 or None: 0..14 how many ended episodes had term k set in their last step | 15 the ended episodes"""
        return self._term_record

    @property
    def command_words(self):
        """the host copy of the command block as last written (fp32 [16]) or None"""
        return None if self._command_words is None else self._command_words.copy()

    @property
    def event_words(self):
        """the host copy of the event block as last written (fp32 [32], or [64] of an extended block) or None"""
        return None if self._event_words is None else self._event_words.copy()

    def reset(self):
        """the first state of episode 0 in the state buffer"""
        d = self._desc
        d.init, d.state_out, d.action = 1, self.cur.data_ptr(), None
        self._nat.servo_sim_step(d)
        d.init = 0

    def advance(self, action: torch.Tensor) -> torch.Tensor:
        if action is None:
            raise ValueError("Solo12ServoSim.advance needs the action: the simulator is closed loop")
        if action.dtype != torch.float32 or not action.is_contiguous():
            action = action.float().contiguous()
        if self._action_table is not None and tuple(action.shape) != (self.N, self.action_width):
            raise ValueError(f"Solo12ServoSim.advance: the action is {tuple(action.shape)}, the simulator reads "
                             f"[{self.N}, {self.action_width}]")
        self.cursor = (self.cursor + 1) % 2
        slab = self._slabs[self.cursor]
        d = self._desc
        d.state_out, d.action = slab.data_ptr(), action.data_ptr()
        self._nat.servo_sim_step(d)
        return slab

    def step(self, action=None):
        if action is None:
            self.reset()
        else:
            self.cur.copy_(self.advance(action))

    # run state: the state buffer (the 14 private floats per env included) and which slab is written next; the slabs are
    # scratch - the kernel reads ``cur`` and writes the other slab
    def fingerprint(self) -> dict:
        d = self._desc
        fp = {n: float(getattr(d, n)) for n in native.SERVO_CONSTANTS}
        fp["resample_steps"], fp["decimation"] = int(d.resample_steps), int(d.decimation)
        return {"servo": fp}

    def state_dict(self) -> dict:
        if self._plant_table is not None:
            raise RuntimeError("run state: a plant table is attached to the simulator; an evaluation is not a resumable state "
                               "(detach it before saving)")
        if self._fixed_command is not None or self._eval_record is not None or self._trace is not None:
            raise RuntimeError("run state: a fixed-command table, an evaluation record or a trace is attached to the simulator; "
                               "an evaluation is not a resumable state (detach them before saving)")
        return super().state_dict()


class _ActionManager:
    def __init__(self, n, a, device):
        self._action = torch.zeros(n, a, device=device)
        self._prev_action = torch.zeros(n, a, device=device)
        self.total_action_dim = a

    def process_action(self, action):
        self._prev_action.copy_(self._action)
        self._action.copy_(action)

    def reset(self, env_ids=None):
        """IsaacLab's ActionManager.reset: the action history of the envs that reset starts from zero, so the
        action-rate constraint of their first step sees ``|a - 0| / dt`` (mask, index list or None = all)."""
        if env_ids is None or isinstance(env_ids, slice):
            self._action.zero_()
            self._prev_action.zero_()
        elif isinstance(env_ids, torch.Tensor) and env_ids.dtype == torch.bool:
            keep = (~env_ids).unsqueeze(1)
            self._action.mul_(keep)
            self._prev_action.mul_(keep)
        else:
            self._action[env_ids] = 0.0
            self._prev_action[env_ids] = 0.0
        return {}


class _CurriculumManager:
    def __init__(self, cfg, env):
        self._env = env
        items = cfg.items() if isinstance(cfg, dict) else (cfg.__dict__.items() if cfg is not None else [])
        self._terms = [(n, t) for n, t in items if t is not None]
        self._keyed = [(f"Curriculum/{n}", t) for n, t in self._terms]
        self._state = {}

    def compute(self, env_ids=None):
        env, state = self._env, self._state
        for key, term in self._keyed:
            state[key] = term.func(env, env_ids, **term.params)

    def reset(self, env_ids=None):
        return {k: v for k, v in self._state.items() if isinstance(v, (int, float))}

    @contextlib.contextmanager
    def frozen(self):
        """no term runs inside the block: ``max_p`` of every constraint term stays what it is"""
        keyed, self._keyed = self._keyed, []
        try:
            yield
        finally:
            self._keyed = keyed

    # run state: the logged scalars and, for every constraint term, the ``max_p`` the curriculum has reached (a Python
    # double on the term cfg; it reaches the device as a launch argument of the next step)
    def state_dict(self) -> dict:
        cm = getattr(self._env, "constraint_manager", None)
        max_p = {n: float(cm.get_term_cfg(n).max_p) for n in cm.active_terms} if cm is not None else {}
        return {"state": {k: float(v) for k, v in self._state.items() if isinstance(v, (int, float))}, "max_p": max_p}

    def load_state_dict(self, sd: dict):
        cm = getattr(self._env, "constraint_manager", None)
        for name, p in sd["max_p"].items():
            cfg = cm.get_term_cfg(name)
            cfg.max_p = float(p)
            cm.set_term_cfg(name, cfg)
        self._state.clear()
        self._state.update(sd["state"])


class CaTEnv:
    """Drop-in for the reference ``CaTEnv`` on the path PPO consumes (``unwrapped.num_envs``,
    ``single_observation_space["policy"]``, ``single_action_space``, ``reset()``, ``step()``)."""

    persistent_state_buffers = True      # term descriptors may cache raw pointers

    def __init__(self, cfg, render_mode: str | None = None, **kwargs):
        self.cfg = cfg
        self.render_mode = render_mode
        self.num_envs = int(cfg.scene.num_envs)
        dev = getattr(cfg.sim, "device", "cuda:0")
        if not torch.cuda.is_available() or torch.device(dev).type != "cuda":
            raise RuntimeError("CaTEnv needs a HIP device (MI355X): the constraint manager and the synthetic "
                               "simulator are device resident; there is no CPU fallback")
        self.device = torch.device(dev)
        self.physics_dt = cfg.sim.dt
        self.step_dt = cfg.sim.dt * cfg.decimation
        self.max_episode_length_s = cfg.episode_length_s
        self.max_episode_length = math.ceil(cfg.episode_length_s / self.step_dt)
        syn = cfg.synthetic
        self.obs_dim, self.act_dim = int(syn.obs_dim), len(SOLO12_JOINTS)
        seed = int(getattr(cfg, "seed", 0) or 0)
        kind = str(getattr(syn, "kind", "stream"))
        if kind not in ("stream", "servo"):
            raise ValueError(f"SyntheticCfg.kind must be 'stream' or 'servo', got {kind!r}")
        # cfg.actions: which action column drives which joint, through which scale, offset and clip, as what kind of target,
        # is IsaacLab's action block, evaluated inside the simulator's launch ("Actions"); without it column
        # j is joint j's position target default + servo_action_scale * a.  Built first: its width A is the policy's output
        # width and the width of a last_action observation term
        self._action_table = None
        if getattr(cfg, "actions", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.actions needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the action terms "
                                "are evaluated inside its launch; the stream simulator is open loop and reads no action")
            from cat_envs.tasks.utils.mdp import actions as AM
            self._action_table = AM.build_table(cfg.actions, SOLO12_JOINTS, DEFAULT_JOINT_POS)
            self.act_dim = max(t["slice"][1] for t in self._action_table[1].values())
        # cfg.observations: the policy's input is a second field of the simulator's row, filled inside its launch (DESIGN
        # section 9, "Observations"); the table is built first because its width is part of the row's layout
        self._obs_field, self._obs_table = "obs", None
        if getattr(cfg, "observations", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.observations needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the "
                                "observation terms are evaluated inside its launch; the stream simulator's observation is a "
                                "pre-generated stream")
            if int(syn.obs_dim) != native.SERVO_OBS_RAW:
                raise ValueError(f"cfg.observations reads the simulator's raw observation of {native.SERVO_OBS_RAW} floats: "
                                 f"synthetic.obs_dim is {syn.obs_dim}")
            from cat_envs.tasks.utils.mdp import observation_manager as OM
            self._obs_table = OM.build_table(OM.policy_group(cfg.observations), SOLO12_JOINTS, DEFAULT_JOINT_POS,
                                             action_terms=None if self._action_table is None else
                                             {n: t["slice"] for n, t in self._action_table[1].items()})
            self._obs_field, self.obs_dim = "policy_obs", len(self._obs_table[0])
            self._frame_dim = self.obs_dim
            # history_length on a term or the group: the policy reads a second field of the row that the same launch shifts and
            # fills ("History"); with every depth 1 nothing changes
            if self._obs_table.has_history:
                self._obs_field, self.obs_dim = "policy_obs_hist", self._obs_table.history_floats
        # cfg.events: pushes, reset ranges and traction are evaluated inside the simulator's launch, too (DESIGN section 9,
        # "Events"); the block is built before the simulator because an error in the cfg should cost no device memory
        self._event_block = None
        if getattr(cfg, "events", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.events needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the events are "
                                "evaluated inside its launch; the stream simulator is a pre-generated stream")
            from cat_envs.tasks.utils.mdp import event_manager as EM
            self._event_block = EM.build_block(cfg.events, cfg.sim.dt, cfg.episode_length_s)
        # cfg.commands: the velocity command is IsaacLab's command term, evaluated inside the simulator's launch as a stateful
        # process on the row ("Commands"); the servo_resample_steps / servo_standing_fraction /
        # servo_command_deadzone fields of SyntheticCfg are then unused
        self._command_block = None
        if getattr(cfg, "commands", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.commands needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the command term "
                                "is evaluated inside its launch; the stream simulator's command is a pre-generated stream")
            from cat_envs.tasks.utils.mdp import command_manager as KM
            self._command_block = KM.build_block(cfg.commands, cfg.sim.dt, cfg.episode_length_s)
            self._check_command_names(self._command_block["name"])
        # cfg.terminations: when an episode is over is IsaacLab's termination block, evaluated inside the simulator's launch
        # ("Terminations"); without it the surrogate's own roll-over flag and the time-out end episodes
        self._term_table = None
        if getattr(cfg, "terminations", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.terminations needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the termination "
                                "terms are evaluated inside its launch; the stream simulator's resets are a pre-generated stream")
            from cat_envs.tasks.utils.mdp import terminations as TM
            self._term_table = TM.build_table(cfg.terminations, SOLO12_JOINTS, SOLO12_BODIES)
        # cfg.scene.robot: the robot's actuators - per-joint gains, armature, effort limits, a DC motor's curve, the actuator
        # delay - are IsaacLab's ArticulationCfg, evaluated inside the simulator's launch ("Actuators");
        # without it all twelve joints share the servo_kp / servo_kd / servo_inertia / servo_tau_max scalars
        self._actuator_table = None
        if getattr(cfg.scene, "robot", None) is not None:
            if kind != "servo":
                raise TypeError("cfg.scene.robot needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the actuators "
                                "are evaluated inside its launch; the stream simulator has no joints to drive")
            from cat_envs.tasks.utils.mdp import actuators as UM
            self._actuator_table = UM.build_table(cfg.scene.robot, SOLO12_JOINTS, syn, cfg.decimation, DEFAULT_JOINT_POS)
        # randomize_actuator_gains / randomize_joint_parameters / randomize_rigid_body_mass among cfg.events: per-env gains,
        # joint friction, armature and base mass are drawn inside the simulator's launch ("Randomisation");
        # an EventCfg of such terms alone launches no event pack
        self._randomization, self._event_pack = None, False
        if self._event_block is not None:
            from cat_envs.tasks.utils.mdp import randomization as RZ
            robot = getattr(cfg.scene, "robot", None)
            self._randomization = RZ.build_randomization(
                cfg.events, None if self._actuator_table is None else self._actuator_table[0], SOLO12_JOINTS, syn, cfg.sim.dt,
                cfg.decimation, armatures=None if robot is None else UM.armatures(robot, SOLO12_JOINTS))[0]
            self._event_pack = any(k not in EM.RANDOMIZE_KINDS for k in self._event_block["kinds"].values())
        if kind == "stream":
            self.sim = SyntheticSolo12Sim(self.num_envs, self.obs_dim, self.device, seed + int(syn.seed_offset),
                                          int(syn.stream_steps))
            self.scene = self.sim.scene
        self.exact_reset_sync = bool(getattr(syn, "exact_reset_sync", False))
        g = torch.Generator(device=self.device)
        g.manual_seed(seed + 17)
        self.episode_length_buf = torch.randint(0, self.max_episode_length, (self.num_envs,), device=self.device,
                                                generator=g, dtype=torch.long)
        self.common_step_counter = 0
        self._sim_step_counter = 0
        self.extras: dict = {}
        self.single_observation_space = {"policy": _Space((self.obs_dim,))}
        self.single_action_space = _Space((self.act_dim,))
        self.reward_buf = torch.zeros(self.num_envs, device=self.device)
        self._dones = torch.zeros(self.num_envs, device=self.device)
        self.reset_buf = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        self.reset_terminated = torch.zeros_like(self.reset_buf)
        self.reset_time_outs = torch.zeros_like(self.reset_buf)
        if kind == "servo":
            # the closed-loop simulator reads the env's own episode counters and reset mask; an env-sharded run names the
            # global id of its first env (cfg.scene.env_offset), so that the shards reproduce the single-process envs
            self.sim = Solo12ServoSim(self.num_envs, int(syn.obs_dim), self.device, seed + int(syn.seed_offset), syn,
                                      cfg.sim.dt, cfg.decimation, self.max_episode_length, self.episode_length_buf,
                                      self.reset_buf, env_offset=int(getattr(cfg.scene, "env_offset", 0) or 0),
                                      policy_obs_dim=self._frame_dim if self._obs_table is not None else 0,
                                      history_floats=self.obs_dim if self._obs_field == "policy_obs_hist" else 0,
                                      events=self._event_pack, commands=self._command_block is not None,
                                      terminations=self._term_table is not None, actions=self._action_table is not None,
                                      actuators=self._actuator_table is not None, randomize=self._randomization is not None,
                                      # the extended block and the timer field only when the cfg needs them
                                      disturbances=self._event_block is not None and bool(self._event_block.get("flags_ext", 0)),
                                      event_timer=self._event_block is not None and "interval_range" in self._event_block)
            self.scene = self.sim.scene
        self.obs_buf = {"policy": self.sim.view(self._obs_field)}
        self._rstep = None
        self._nat = None
        self.load_managers()

    # gym-style plumbing ---------------------------------------------------------------------
    @property
    def unwrapped(self):
        return self

    def close(self):
        pass

    def seed(self, seed: int = -1) -> int:
        return seed

    def _check_command_names(self, known: str):
        """every ``command_name`` of a reward or observation term names the command term"""
        groups = []
        if getattr(self.cfg, "rewards", None) is not None:
            groups.append(("reward", self.cfg.rewards))
        obs = getattr(self.cfg, "observations", None)
        if obs is not None and getattr(obs, "policy", None) is not None:
            groups.append(("observation", obs.policy))
        for what, group in groups:
            items = group.items() if isinstance(group, dict) else group.__dict__.items()
            for name, term in items:
                wanted = (getattr(term, "params", None) or {}).get("command_name")
                if wanted is not None and wanted != known:
                    raise ValueError(f"{what} term '{name}': command_name '{wanted}' names no command term of cfg.commands "
                                     f"(the command term is '{known}')")

    # managers --------------------------------------------------------------------------------
    def load_managers(self):
        """reference: cat_env.py:18-40 (constraint manager created after the base managers)"""
        if self._action_table is not None:
            from cat_envs.tasks.utils.mdp.action_manager import ActionManager
            self.action_manager = ActionManager(self.cfg.actions, self, self._action_table)
            print("[INFO] Action Manager: ", self.action_manager)
        else:
            self.action_manager = _ActionManager(self.num_envs, self.act_dim, self.device)
        if self._actuator_table is not None:                           # behind the action manager: its table comes first
            from cat_envs.tasks.utils.mdp.actuator_model import ActuatorModel
            self.actuators = ActuatorModel(self.cfg.scene.robot, self, self._actuator_table, randomization=self._randomization)
            print("[INFO] Actuator Model: ", self.actuators)
        cmd = self.sim.view("command")
        self.command_manager = types.SimpleNamespace(get_command=lambda name: cmd, reset=lambda ids=None: {},
                                                     compute=lambda dt: None)
        if self._command_block is not None:
            from cat_envs.tasks.utils.mdp.command_manager import CommandManager
            self.command_manager = CommandManager(self.cfg.commands, self, self._command_block)
            print("[INFO] Command Manager: ", self.command_manager)
        self.curriculum_manager = _CurriculumManager(getattr(self.cfg, "curriculum", None), self)
        if hasattr(self.cfg, "constraints"):
            self.constraint_manager = ConstraintManager(self.cfg.constraints, self)
            print("[INFO] Constraint Manager: ", self.constraint_manager)
        if getattr(self.cfg, "rewards", None) is not None:
            if not isinstance(self.sim, Solo12ServoSim):
                raise TypeError("cfg.rewards needs the closed-loop simulator (SyntheticCfg.kind = 'servo'): the reward terms "
                                "are evaluated inside its launch; the stream simulator's reward is a pre-generated stream")
            from cat_envs.tasks.utils.mdp.reward_manager import RewardManager
            self.reward_manager = RewardManager(self.cfg.rewards, self)
            print("[INFO] Reward Manager: ", self.reward_manager)
        if self._obs_table is not None:
            from cat_envs.tasks.utils.mdp.observation_manager import ObservationManager
            self.observation_manager = ObservationManager(self.cfg.observations, self, *self._obs_table,
                                                          depths=self._obs_table.depths)
            print("[INFO] Observation Manager: ", self.observation_manager)
        if self._event_block is not None:
            from cat_envs.tasks.utils.mdp.event_manager import EventManager
            # cfg.pushes = False (the play cfgs): reset and startup terms as configured, interval events off
            self.event_manager = EventManager(self.cfg.events, self, self._event_block,
                                              interval_enabled=bool(getattr(self.cfg, "pushes", True)),
                                              randomization=self._randomization)
            print("[INFO] Event Manager: ", self.event_manager)
        if self._term_table is not None:
            from cat_envs.tasks.utils.mdp.termination_manager import TerminationManager
            self.termination_manager = TerminationManager(self.cfg.terminations, self, self._term_table)
            print("[INFO] Termination Manager: ", self.termination_manager)

    # evaluation ------------------------------------------------------------------------------
    def _servo_sim(self) -> Solo12ServoSim:
        if not isinstance(self.sim, Solo12ServoSim):
            raise TypeError("fixed commands and the evaluation record need the closed-loop simulator "
                            "(SyntheticCfg.kind = 'servo'); the stream simulator is open loop")
        return self.sim

    def set_fixed_commands(self, commands: torch.Tensor | None, segment_steps: int | None = None):
        """per-env commands [N, 3], or a schedule [S, N, 3] of ``segment_steps`` control steps per segment, that replace
        the simulator's own draws (None: back to the draws)"""
        self._servo_sim().set_fixed_command(commands, segment_steps)

    def set_fixed_plant(self, table: torch.Tensor | None):
        """per-env pinned plants [N, 8] (``cleanrl.evaluate.plant_grid``): gains, joint friction, armature, base mass and
        actuator lag of env i are what row i pins, whatever the randomisation draws (None: back to the draws)"""
        self._servo_sim().set_fixed_plant(table)

    def set_trace(self, trace: torch.Tensor | None):
        """attach (or, with None, detach) the simulator's step trace [T, K, 72]"""
        self._servo_sim().set_trace(trace)

    def set_observation_corruption(self, on: bool):
        """observation noise on or off from the next step on (needs cfg.observations)"""
        if not hasattr(self, "observation_manager"):
            raise TypeError("observation corruption needs cfg.observations")
        self.observation_manager.set_corruption(on)

    def set_pushes(self, on: bool):
        """interval events (the pushes) on or off from the next step on (needs cfg.events)"""
        if not hasattr(self, "event_manager"):
            raise TypeError("pushes need cfg.events")
        self.event_manager.set_interval_enabled(on)

    def set_wrench(self, on: bool):
        """the external wrench on or off from the next step on (needs apply_external_force_torque in cfg.events)"""
        if not hasattr(self, "event_manager"):
            raise TypeError("the wrench needs cfg.events with apply_external_force_torque")
        self.event_manager.set_wrench_enabled(on)

    def set_randomization(self, on: bool):
        """the randomised robot on or off (off: the nominal robot) from the next step on (needs such terms in cfg.events)"""
        if not hasattr(self, "event_manager"):
            raise TypeError("randomization needs cfg.events with randomize_actuator_gains, randomize_joint_parameters or "
                            "randomize_rigid_body_mass")
        self.event_manager.set_randomization_enabled(on)

    def set_eval_record(self, record: torch.Tensor | None):
        """attach (or, with None, detach) the simulator's per-env evaluation record [N, 12]"""
        self._servo_sim().set_eval_record(record)

    def fresh_cat_state(self):
        """the constraint manager's state as at construction, in place (``ConstraintManager.fresh_state``); ``max_p`` of the
        terms is left alone: it belongs to whoever drives the curriculum"""
        if hasattr(self, "constraint_manager"):
            self.constraint_manager.fresh_state()

    @contextlib.contextmanager
    def curriculum_frozen(self):
        """inside the block the curriculum does not run and afterwards its step counter stands where it stood: stepping
        the env in here moves no ``max_p``, now or later"""
        counter = self.common_step_counter
        try:
            with self.curriculum_manager.frozen():
                yield
        finally:
            self.common_step_counter = counter

    # run state ----------------------------------------------------------------
    def _state_tensors(self) -> dict:
        am = self.action_manager
        return {"episode_length_buf": self.episode_length_buf, "reset_buf": self.reset_buf,
                "reset_terminated": self.reset_terminated, "reset_time_outs": self.reset_time_outs,
                "reward_buf": self.reward_buf, "dones": self._dones, "action": am._action, "prev_action": am._prev_action}

    def state_fingerprint(self) -> dict:
        """what has to be equal between the env that saved a state and the env that loads it"""
        syn, cm = self.cfg.synthetic, getattr(self, "constraint_manager", None)
        if cm is not None and cm._term_names and not cm._bound:
            cm._bind(native.get(self.device))
        fp = {"task_kind": "servo" if isinstance(self.sim, Solo12ServoSim) else "stream",
              "num_envs": self.num_envs, "obs_dim": self.obs_dim, "act_dim": self.act_dim,
              "env_seed": int(getattr(self.cfg, "seed", 0) or 0), "seed_offset": int(syn.seed_offset),
              "env_offset": int(getattr(self.cfg.scene, "env_offset", 0) or 0),
              "max_episode_length": int(self.max_episode_length), "decimation": int(self.cfg.decimation),
              "exact_reset_sync": bool(self.exact_reset_sync),
              "constraint_terms": [[n, int(w)] for n, w in zip(cm._term_names, cm._widths)] if cm is not None else []}
        fp.update(self.sim.fingerprint())
        if hasattr(self, "reward_manager"):          # only then: fingerprints of runs without rewards keep their fields
            fp["reward_terms"] = self.reward_manager.fingerprint()
        if hasattr(self, "observation_manager"):     # likewise
            fp["observation_terms"] = self.observation_manager.fingerprint()
        if hasattr(self, "event_manager"):           # likewise
            fp["event_terms"] = self.event_manager.fingerprint()
        if getattr(self, "_command_block", None) is not None:          # likewise
            fp["command_terms"] = self.command_manager.fingerprint()
        if getattr(self, "_term_table", None) is not None:             # likewise
            fp["termination_terms"] = self.termination_manager.fingerprint()
        if getattr(self, "_action_table", None) is not None:           # likewise
            fp["action_terms"] = self.action_manager.fingerprint()
        if getattr(self, "_actuator_table", None) is not None:         # likewise
            fp["actuators"] = self.actuators.fingerprint()
        return fp

    def state_dict(self) -> dict:
        """the env's part of a run state: counters, reset masks, action history, the curriculum's scalars and the
        ``max_p`` values it has reached, the constraint manager's and the simulator's own parts.  Legal between two steps.
        The tensors are the live ones: the caller copies them (``checkpoint.to_plain``)."""
        sd = {"common_step_counter": int(self.common_step_counter), "sim_step_counter": int(self._sim_step_counter),
              "curriculum": self.curriculum_manager.state_dict(), "sim": self.sim.state_dict()}
        sd.update(self._state_tensors())
        if hasattr(self, "constraint_manager"):
            sd["constraints"] = self.constraint_manager.state_dict()
        if hasattr(self, "reward_manager"):
            sd["rewards"] = self.reward_manager.state_dict()
        if hasattr(self, "observation_manager"):     # the policy field is part of the simulator's ``cur``; the switch is not
            sd["observations"] = self.observation_manager.state_dict()
        if hasattr(self, "event_manager"):           # the draws are stateless; the interval switch is the state
            sd["events"] = self.event_manager.state_dict()
        if getattr(self, "_command_block", None) is not None:          # command and time left are part of the simulator's ``cur``; the ranges are not
            sd["commands"] = self.command_manager.state_dict()
        if getattr(self, "_term_table", None) is not None:             # the record of the ended episodes and the current params
            sd["terminations"] = self.termination_manager.state_dict()
        if getattr(self, "_action_table", None) is not None:           # the table's current scales, offsets and clip bounds
            sd["actions"] = self.action_manager.state_dict()
        if getattr(self, "_actuator_table", None) is not None:         # the history is part of the simulator's ``cur``; the gains are not
            sd["actuators"] = self.actuators.state_dict()
        return sd

    def check_state_dict(self, sd: dict):
        """``ValueError`` unless every part of ``sd`` fits this env; loads nothing"""
        keys = ["common_step_counter", "sim_step_counter", "curriculum", "sim", *self._state_tensors()]
        if hasattr(self, "constraint_manager"):
            keys.append("constraints")
        if hasattr(self, "reward_manager"):
            keys.append("rewards")
        elif "rewards" in sd:
            raise ValueError("run state: it carries reward terms, this env has no cfg.rewards")
        if hasattr(self, "observation_manager"):
            keys.append("observations")
        elif "observations" in sd:
            raise ValueError("run state: it carries observation terms, this env has no cfg.observations")
        if hasattr(self, "event_manager"):
            keys.append("events")
        elif "events" in sd:
            raise ValueError("run state: it carries events, this env has no cfg.events")
        if getattr(self, "_command_block", None) is not None:
            keys.append("commands")
        elif "commands" in sd:
            raise ValueError("run state: it carries commands, this env has no cfg.commands")
        if getattr(self, "_term_table", None) is not None:
            keys.append("terminations")
        elif "terminations" in sd:
            raise ValueError("run state: it carries terminations, this env has no cfg.terminations")
        if getattr(self, "_action_table", None) is not None:
            keys.append("actions")
        elif "actions" in sd:
            raise ValueError("run state: it carries actions, this env has no cfg.actions")
        if getattr(self, "_actuator_table", None) is not None:
            keys.append("actuators")
        elif "actuators" in sd:
            raise ValueError("run state: it carries actuators, this env has no cfg.scene.robot")
        missing = [k for k in keys if k not in sd]
        if missing:
            raise ValueError(f"run state: the env's part lacks {missing}")
        for k, t in self._state_tensors().items():
            s = sd[k]
            if tuple(s.shape) != tuple(t.shape) or s.dtype != t.dtype:
                raise ValueError(f"run state: env tensor '{k}' is {tuple(s.shape)} {s.dtype}, this env's is "
                                 f"{tuple(t.shape)} {t.dtype}")
        self.sim.check_state_dict(sd["sim"])
        if hasattr(self, "constraint_manager"):
            cm = self.constraint_manager
            cm.check_state_dict(sd["constraints"])
            unknown = [n for n in sd["curriculum"]["max_p"] if n not in cm.active_terms]
            if unknown:
                raise ValueError(f"run state: max_p of constraint terms {unknown} that this env does not have")
        if hasattr(self, "reward_manager"):
            self.reward_manager.check_state_dict(sd["rewards"])
        if hasattr(self, "observation_manager"):
            self.observation_manager.check_state_dict(sd["observations"])
        if hasattr(self, "event_manager"):
            self.event_manager.check_state_dict(sd["events"])
        if getattr(self, "_command_block", None) is not None:
            self.command_manager.check_state_dict(sd["commands"])
        if getattr(self, "_term_table", None) is not None:
            self.termination_manager.check_state_dict(sd["terminations"])
        if getattr(self, "_action_table", None) is not None:
            self.action_manager.check_state_dict(sd["actions"])
        if getattr(self, "_actuator_table", None) is not None:
            self.actuators.check_state_dict(sd["actuators"])

    def load_state_dict(self, sd: dict):
        """IN PLACE (``copy_`` into the existing tensors, never a rebound attribute): the fused step's argument block, the
        servo simulator's, the constraint manager's descriptor table and a trainer's ``RolloutSink`` hold raw device
        addresses of these tensors, and captured graphs bake them in.  Everything is checked before anything is written."""
        self.check_state_dict(sd)
        for k, t in self._state_tensors().items():
            t.copy_(sd[k])
        self.common_step_counter = int(sd["common_step_counter"])
        self._sim_step_counter = int(sd["sim_step_counter"])
        self.sim.load_state_dict(sd["sim"])
        if hasattr(self, "constraint_manager"):
            self.constraint_manager.load_state_dict(sd["constraints"])
        if hasattr(self, "reward_manager"):
            self.reward_manager.load_state_dict(sd["rewards"])
        if hasattr(self, "observation_manager"):
            self.observation_manager.load_state_dict(sd["observations"])
        if hasattr(self, "event_manager"):
            self.event_manager.load_state_dict(sd["events"])
        if getattr(self, "_command_block", None) is not None:
            self.command_manager.load_state_dict(sd["commands"])
        if getattr(self, "_term_table", None) is not None:
            self.termination_manager.load_state_dict(sd["terminations"])
        if getattr(self, "_action_table", None) is not None:
            self.action_manager.load_state_dict(sd["actions"])
        if getattr(self, "_actuator_table", None) is not None:
            self.actuators.load_state_dict(sd["actuators"])
        self.curriculum_manager.load_state_dict(sd["curriculum"])      # through set_term_cfg: the next launch carries it

    # episode control -------------------------------------------------------------------------
    def reset(self, seed: int | None = None, options=None):
        self.sim.step()
        self.extras = {}
        return self.obs_buf, self.extras

    def step(self, action: torch.Tensor):
        """reference: cat_env.py:42-147 with the physics loop replaced by the synthetic stream."""
        self._sim_step_counter += self.cfg.decimation
        self.sim.step(action)
        self.common_step_counter += 1
        # -- one launch: process_action, episode_length_buf += 1 (:92), terminations (:95-97: hard resets
        #    from the stream, time-outs from the counter), reward_manager output -> reward_buf
        am = self.action_manager
        action = action if (action.dtype == torch.float32 and action.is_contiguous()) else action.float().contiguous()
        native.get(self.device).env_pre_step(action, am._action, am._prev_action, self.episode_length_buf,
                                             self.max_episode_length, self.sim.view("hard_reset"),
                                             self.sim.view("reward"), self.reset_time_outs, self.reset_terminated,
                                             self.reset_buf, self.reward_buf)
        # -- CaT (:99-107,118-121): probability, reward *= (1-p) clipped at 0, dones = p, dones[reset] = 1
        if hasattr(self.cfg, "constraints"):
            self.constraint_manager.compute(reward=self.reward_buf, reset_mask=self.reset_buf, dones=self._dones)
            dones = self._dones
        else:
            dones = self.reset_buf.float()
        # -- resets (:118-125)
        if self.exact_reset_sync:
            ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1)   # host sync, reference control flow
            if len(ids) > 0:
                self._reset_idx(ids)
        else:
            self._reset_idx(self.reset_buf)
        # -- observations (:144)
        return self.obs_buf, self.reward_buf, dones, self.reset_time_outs, self.extras

    # fused path ------------------------------------------------------------------------------------
    def can_step_into(self, obs_dim_ok: bool = True) -> bool:
        """``step_into`` is available: constraints configured with describable terms, mask-based resets"""
        cm = getattr(self, "constraint_manager", None)
        return (cm is not None and not self.exact_reset_sync and obs_dim_ok and self.obs_dim <= 512
                and cm.can_fuse_rollout(native.get(self.device)))

    def step_into(self, action: torch.Tensor, sink):
        """``step`` with everything after the simulator update fused into two calls (catppo_rollout_pre /
        catppo_rollout_post: three launches), including the consumer's part: ``sink`` (see ``cleanrl.ppo.RolloutSink``) names the
        rollout-buffer rows of this step and the observation normaliser, so rewards / dones / time-outs and the
        normalised next observation are written where PPO wants them.  Same return tuple as ``step``; ``extras["log"]``
        is the manager's view dict of the ring slot written by this step, the curriculum scalars ride in
        ``extras["log_host"]``."""
        nat = self._nat
        cm = self.constraint_manager
        self._sim_step_counter += self.cfg.decimation
        # "scene.update": the new simulator state.  Fused: catppo_rollout_pre copies the stream's next slab into the state
        # buffer inside its own launch and reads its inputs straight from the slab (catppo_rollout_step.sim_src) - one
        # 5 us copy kernel and a launch boundary less per env step; CATPPO_FUSED_SIM_COPY=0 keeps the separate copy.
        slab = None
        if _FUSED_SIM_COPY:
            slab = self.sim.advance(action)
        else:
            self.sim.step(action)
        self.common_step_counter += 1
        st = self._rstep
        if st is None:
            from cat_envs import parallel
            self._parallel = parallel
            nat = self._nat = native.get(self.device)
            st = self._rstep = native.RolloutStep()
            am = self.action_manager
            st.N, st.A, st.D = self.num_envs, self.act_dim, self.obs_dim
            st.action, st.prev_action = am._action.data_ptr(), am._prev_action.data_ptr()
            st.episode_length, st.max_episode_length = self.episode_length_buf.data_ptr(), self.max_episode_length
            hr, rw = self.sim.view("hard_reset"), self.sim.view("reward")
            st.hard_reset, st.hard_reset_stride = hr.data_ptr(), hr.stride(0)
            st.reward_src, st.reward_stride = rw.data_ptr(), rw.stride(0)
            st.time_outs, st.terminated = self.reset_time_outs.data_ptr(), self.reset_terminated.data_ptr()
            st.reset, st.reward, st.dones = self.reset_buf.data_ptr(), self.reward_buf.data_ptr(), self._dones.data_ptr()
            st.zero_action_on_reset = 1
            obs = self.sim.view(self._obs_field)
            st.obs_raw, st.obs_ld = obs.data_ptr(), obs.stride(0)
            self._xchg = nat.rollout_xchg_new(cm.cat._p_cstr.shape[1], self.obs_dim)
            st.xchg = self._xchg.data_ptr()
            self._xchg_views = nat.rollout_xchg_views(self._xchg, cm.cat._p_cstr.shape[1], self.obs_dim)
            self._xchg_all = None
            st.sim_state, st.sim_row_bytes = self.sim.cur.data_ptr(), self.sim.F * 4
            self._rstep_ref = C.byref(st)
        if action.dtype != torch.float32 or not action.is_contiguous():
            action = action.float().contiguous()
        st.action_in = action.data_ptr()
        st.sim_src = slab.data_ptr() if slab is not None else None
        cm.fill_rollout_step(st)
        sink.fill(st)
        lib, h, stream = nat.lib, nat.h, nat._stream()
        rc = lib.catppo_rollout_pre(h, self._rstep_ref, stream)
        if rc:
            nat._ok(rc)
        # env-sharded runs exchange the record rollout_pre just wrote {CaT column maxima | observation moment sums}.
        # The maxima travel only in exact mode (cm.dist_group, set by the trainer under dist_exact); the moment sums
        # whenever the consumer's normaliser is global (sink.obs_group) - its divisor obs_rows_total is then the global
        # env count, so the sums MUST be global too (with dist_exact=False they once stayed local while the divisor was
        # global: the running mean shrank by 1/world per update).  Both wanted (exact mode): ONE all-gather of the
        # record, folded by rollout_post; only one of them: an all-reduce of that half.
        par = self._parallel
        group, obs_group = cm.dist_group, getattr(sink, "obs_group", None)
        g_on = group is not None and par.active(group)
        o_on = obs_group is not None and par.active(obs_group)
        if g_on and o_on and group is obs_group:
            # exact mode: ONE collective per env step - all-gather this rank's record {colmax | sums}; rollout_post folds
            # the records of all ranks itself (MAX is exact, the sums run in rank order on every rank)
            w = par.world_size(group)
            if self._xchg_all is None or self._xchg_all.numel() != w * self._xchg.numel():
                self._xchg_all = torch.zeros(w * self._xchg.numel(), dtype=torch.uint8, device=self.device)
            # set on EVERY pass: a step through the other branch (another sink / trainer on the same env with a different
            # dist_exact or obs group) leaves xchg_records = 0, and rollout_post would then fold the local record only
            st.xchg_gathered, st.xchg_records = self._xchg_all.data_ptr(), w
            par.allgather_bytes_(self._xchg, self._xchg_all, group)
        else:
            st.xchg_records = 0
            if g_on:
                par.allreduce_max_(self._xchg_views[0], group)    # exact (max is order independent): masks stay bit-exact
            if o_on:
                par.allreduce_sum_(self._xchg_views[1], obs_group)   # fp64 [sum x | sum x^2]
        rc = lib.catppo_rollout_post(h, self._rstep_ref, stream)
        if rc:
            nat._ok(rc)
        # curriculum AFTER the CaT step, like _reset_idx (host scalars: the new max_p travels with the next step's
        # launch; the reference runs it whenever some env resets - with thousands of envs that is every step)
        cur = self.curriculum_manager
        cur.compute(env_ids=self.reset_buf)
        ex = self.extras
        ex["log"] = cm.latest_log(copy=False)
        ex["log_host"] = cur._state
        ex["log_packed"] = cm.log_packed
        return self.obs_buf, self.reward_buf, self._dones, self.reset_time_outs, ex

    def _reset_idx(self, env_ids: Sequence[int] | torch.Tensor):
        """reference: cat_env.py:149-200.  ``env_ids`` may be a bool mask (sync-free path)."""
        self.curriculum_manager.compute(env_ids=env_ids)
        log = {}
        log.update(self.action_manager.reset(env_ids))
        if hasattr(self.cfg, "constraints"):
            log.update(self.constraint_manager.reset(env_ids))
            self.extras["log_packed"] = self.constraint_manager.log_packed
        log.update(self.curriculum_manager.reset(env_ids))
        self.extras["log"] = log
        if isinstance(env_ids, torch.Tensor) and env_ids.dtype == torch.bool:
            self.episode_length_buf.masked_fill_(env_ids, 0)
        else:
            self.episode_length_buf[env_ids] = 0
