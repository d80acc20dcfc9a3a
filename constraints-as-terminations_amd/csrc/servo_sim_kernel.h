// The servo simulator's kernel template, its helpers and launch(): included by the six units that hold its instances, so
// that they compile side by side (servo_sim.hip lists them).  Everything here has internal linkage.
#pragma once
#include <type_traits>

#include "common.h"
#include "rng.h"
#include "servo_sim_host.h"

namespace {

constexpr int kThreads = 256;                                            // kEnvsPerBlock, kJoints, kPrivate, kRawObs: servo_sim_host.h
constexpr uint32_t kTagCommand = 0x434D4453u, kTagInit = 0x494E4954u;   // "CMDS", "INIT": fourth Philox counter word
constexpr uint32_t kTagObs = 0x4F42534Eu;                                // "OBSN": the observation noise
// "PUSH", "JVEL", "ROOT", "FRIC": the events ("Events")
constexpr uint32_t kTagPush = 0x50555348u, kTagJvel = 0x4A56454Cu, kTagRoot = 0x524F4F54u, kTagFric = 0x46524943u;
// "CMDD", "CMDT": command draws and resampling times of the configured command process ("Commands")
constexpr uint32_t kTagCmdDraw = 0x434D4444u, kTagCmdTime = 0x434D4454u;
constexpr uint32_t kTagActDelay = 0x41444C59u;                           // "ADLY": the actuator lag ("Actuators")
// "AGAN", "JPAR", "MASS": the randomised gains, joint parameters and base mass ("Randomisation")
constexpr uint32_t kTagGains = 0x4147414Eu, kTagJointPar = 0x4A504152u, kTagMass = 0x4D415353u;
// "PSHT", "WRNC": the timer of the timed push and the external wrench ("Disturbances")
constexpr uint32_t kTagPushTime = 0x50534854u, kTagWrench = 0x57524E43u;

// G[k][lane]: the fixed 5 x 12 matrix of the base model (rows vx, vy, wz, roll, pitch)
__device__ __forceinline__ float gain(int k, int lane) {
  if (lane >= kJoints) return 0.f;
  const int leg = lane / 3, part = lane - 3 * leg;
  const bool left = (leg & 1) == 0, front = leg < 2;
  switch (k) {
    case 0: return part == 1 ? 0.5f : 0.f;                          // vx: the four HFE offsets
    case 1: return part == 0 ? 0.5f : 0.f;                          // vy: the four HAA offsets
    case 2: return part == 0 ? (front ? 0.5f : -0.5f) : 0.f;        // wz: front against hind HAA
    case 3: return part == 1 ? (left ? 0.3f : -0.3f) : 0.f;         // roll: left against right HFE
    default: return part == 2 ? (front ? 0.3f : -0.3f) : 0.f;       // pitch: front against hind KFE
  }
}

__device__ __forceinline__ float tree16(float x) {
  x = x + __shfl_xor(x, 8, 16);
  x = x + __shfl_xor(x, 4, 16);
  x = x + __shfl_xor(x, 2, 16);
  x = x + __shfl_xor(x, 1, 16);
  return x;
}

__device__ __forceinline__ float tree4(float x) {
  x = x + __shfl_xor(x, 1, 16);
  x = x + __shfl_xor(x, 2, 16);
  return x;
}

// the descriptor of type T in the kernel's pack of extensions
template <typename T, typename U, typename... R>
__device__ __forceinline__ const T& ext_of(const U& u, const R&... r) {
  if constexpr (std::is_same_v<T, U>) return u;
  else return ext_of<T>(r...);
}

__device__ __forceinline__ float pick(const rng::u32x4& r, int w) { return rng::uniform_open(w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w); }

// the three instances of the kernel (see the kernel): what the launch's descriptor asks for
constexpr int kTrain = 0, kEvaluate = 1, kStepResponse = 2;

// command of (env, episode, resample index): uniform in the reference ranges, dead zone, standing fraction; with a
// fixed-command table the caller's row `e` as it stands, for every episode and resample index - in the step-response
// instance, of segment min(t / fixed_segment_steps, S - 1) when the table is a schedule of S > 1 segments, `t` being the
// episode length the command is for (one wave-uniform compare; the divide runs only for a schedule).  kMode: see the kernel
template <int kMode>
__device__ __forceinline__ void command_of(const catppo_servo_sim& d, int64_t e, uint32_t gid, uint32_t ep, uint32_t k,
                                           int64_t t, float c[3]) {
  if constexpr (kMode != kTrain) {
    if (d.fixed_command) {
      int64_t at = e;
      if constexpr (kMode == kStepResponse) {
        if (d.fixed_segments > 1) {
          int64_t seg = t / d.fixed_segment_steps;
          seg = seg < 0 ? 0 : seg < d.fixed_segments ? seg : d.fixed_segments - 1;
          at = seg * d.N + e;
        }
      }
      for (int i = 0; i < 3; ++i) c[i] = d.fixed_command[at * 3 + i];
      return;
    }
  }
  const rng::u32x4 r = rng::philox4x32_10(rng::u32x4{gid, ep, k, kTagCommand}, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
  c[0] = -0.3f + rng::uniform_open(r.x) * 1.3f;
  c[1] = -0.7f + rng::uniform_open(r.y) * 1.4f;
  c[2] = -0.78f + rng::uniform_open(r.z) * 1.56f;
  const float n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  const bool keep = n2 > d.command_deadzone * d.command_deadzone && !(rng::uniform_open(r.w) < d.standing_fraction);
  if (!keep) c[0] = c[1] = c[2] = 0.f;
}

// joint `lane` of the first pose of (env, episode): default + uniform noise; Philox block lane / 4, word lane % 4
__device__ __forceinline__ float init_q(const catppo_servo_sim& d, uint32_t gid, uint32_t ep, int lane, float def) {
  const rng::u32x4 r = rng::philox4x32_10(rng::u32x4{gid, ep, (uint32_t)(lane >> 2), kTagInit}, (uint32_t)d.seed,
                                          (uint32_t)(d.seed >> 32));
  return def + (pick(r, lane & 3) - 0.5f) * d.init_noise;
}

// the event block as the wave holds it: wave lane k < 32 has loaded word k, every lane reads word k through readlane, so
// all of this is wave-uniform (scalar registers)
struct Events {
  uint32_t flags;
  float p;
  int buckets;
  float push[10], jpos[2], jvel[2], rpos[4], rvel[6], fric[2];      // (lo, width) pairs
};

__device__ __forceinline__ float ev_word(float mine, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), k));
}

__device__ __forceinline__ Events events_of(float mine) {
  Events E;
  E.flags = (uint32_t)__float_as_int(ev_word(mine, 0));
  E.p = ev_word(mine, 1);
  E.buckets = __float_as_int(ev_word(mine, 2));
#pragma unroll
  for (int i = 0; i < 10; ++i) E.push[i] = ev_word(mine, 4 + i);
#pragma unroll
  for (int i = 0; i < 2; ++i) E.jpos[i] = ev_word(mine, 14 + i), E.jvel[i] = ev_word(mine, 16 + i), E.fric[i] = ev_word(mine, 28 + i);
#pragma unroll
  for (int i = 0; i < 4; ++i) E.rpos[i] = ev_word(mine, 18 + i);
#pragma unroll
  for (int i = 0; i < 6; ++i) E.rvel[i] = ev_word(mine, 22 + i);
  return E;
}

__device__ __forceinline__ rng::u32x4 ev_block(const catppo_servo_sim& d, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t tag) {
  return rng::philox4x32_10(rng::u32x4{c0, c1, c2, tag}, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
}

// joint `lane` of the first state of (env, episode) under the events: the built-in pose, or the joint-reset term's
__device__ __forceinline__ void first_joint(const catppo_servo_sim& d, const Events& E, uint32_t gid, uint32_t ep, int lane,
                                            float def, float& q0, float& qd0) {
  const float u = pick(ev_block(d, gid, ep, (uint32_t)(lane >> 2), kTagInit), lane & 3);
  qd0 = 0.f;
  if (E.flags & (CATPPO_SERVO_EVENT_JOINT_SCALE | CATPPO_SERVO_EVENT_JOINT_OFFSET)) {
    const float s = E.jpos[0] + u * E.jpos[1];
    q0 = (E.flags & CATPPO_SERVO_EVENT_JOINT_SCALE) ? def * s : def + s;
    if (E.flags & CATPPO_SERVO_EVENT_JOINT_OFFSET)
      qd0 = E.jvel[0] + pick(ev_block(d, gid, ep, (uint32_t)(lane >> 2), kTagJvel), lane & 3) * E.jvel[1];
  } else {
    q0 = def + (u - 0.5f) * d.init_noise;
  }
}

// root of the first state of (env, episode): position x y and velocities vx vy wz (zeros without the root-reset term)
__device__ __forceinline__ void first_root(const catppo_servo_sim& d, const Events& E, uint32_t gid, uint32_t ep, float xy[2],
                                           float v0[3]) {
  xy[0] = xy[1] = v0[0] = v0[1] = v0[2] = 0.f;
  if (E.flags & CATPPO_SERVO_EVENT_ROOT) {
    const rng::u32x4 a = ev_block(d, gid, ep, 0u, kTagRoot), b = ev_block(d, gid, ep, 1u, kTagRoot);
    xy[0] = E.rpos[0] + rng::uniform_open(a.x) * E.rpos[1];
    xy[1] = E.rpos[2] + rng::uniform_open(a.y) * E.rpos[3];
    v0[0] = E.rvel[0] + rng::uniform_open(b.x) * E.rvel[1];
    v0[1] = E.rvel[2] + rng::uniform_open(b.y) * E.rvel[3];
    v0[2] = E.rvel[4] + rng::uniform_open(b.z) * E.rvel[5];
  }
}

// traction of env `gid`: the friction of its bucket against the ground's 1.0, at most 1
__device__ __forceinline__ float traction_of(const catppo_servo_sim& d, const Events& E, uint32_t gid) {
  if (!(E.flags & CATPPO_SERVO_EVENT_FRICTION)) return 1.f;
  int bucket = (int)(rng::uniform_open(ev_block(d, gid, 0u, 0u, kTagFric).x) * (float)E.buckets);
  bucket = bucket < E.buckets - 1 ? bucket : E.buckets - 1;
  bucket = bucket > 0 ? bucket : 0;
  const float mu = E.fric[0] + rng::uniform_open(ev_block(d, (uint32_t)bucket, 0u, 1u, kTagFric).x) * E.fric[1];
  return mu < 1.f ? mu : 1.f;
}

// an event descriptor whose block is the extended one of CATPPO_SERVO_EVENT_FLOATS_EXT words (DESIGN section 9,
// "Disturbances"): a type of its own in the kernel's pack, so that the timed push and the wrench are a template parameter of
// the events path - the instances over catppo_servo_events itself compile without a line of them
struct ServoEventsExt {
  catppo_servo_events ev;
};

// what the wave keeps of words 32 .. 37 of an extended block (wave lane k < 64 has loaded word k), the three flag bits and the
// row offset of ev_state (0: the block keeps no timer, and the timed bit is ignored); empty without one
template <bool kOn>
struct DisturbRegs {};
template <>
struct DisturbRegs<true> {
  uint32_t flags = 0u;
  float timer[2] = {0.f, 0.f}, force[2] = {0.f, 0.f}, torque[2] = {0.f, 0.f};      // (lo, width) pairs
  int off_state = 0;
};

__device__ __forceinline__ DisturbRegs<true> disturb_of(float mine, int off_state) {
  DisturbRegs<true> X;
  X.flags = (uint32_t)__float_as_int(ev_word(mine, 0)) &
            (CATPPO_SERVO_EVENT_PUSH_TIMED | CATPPO_SERVO_EVENT_WRENCH | CATPPO_SERVO_EVENT_WRENCH_RESET);
  X.off_state = off_state;
  if (off_state == 0) X.flags &= ~CATPPO_SERVO_EVENT_PUSH_TIMED;
#pragma unroll
  for (int i = 0; i < 2; ++i) X.timer[i] = ev_word(mine, 32 + i), X.force[i] = ev_word(mine, 34 + i), X.torque[i] = ev_word(mine, 36 + i);
  return X;
}

// the time until the next timed push, drawn at the start of (env, episode) (third = 0) and after the push of the step that
// starts at episode length t (third = t + 1)
__device__ __forceinline__ float push_time(const catppo_servo_sim& d, const DisturbRegs<true>& X, uint32_t gid, uint32_t ep,
                                           uint32_t third) {
  return X.timer[0] + rng::uniform_open(ev_block(d, gid, ep, third, kTagPushTime).x) * X.timer[1];
}

// the event descriptor of the pack, plain or extended
template <bool kDist, typename... Ext>
__device__ __forceinline__ const catppo_servo_events& events_desc(const Ext&... ext) {
  if constexpr (kDist) return ext_of<ServoEventsExt>(ext...).ev;
  else return ext_of<catppo_servo_events>(ext...);
}

// the command block as the wave holds it: wave lane k < 16 has loaded word k, every lane reads word k through readlane, so
// every branch on a flag is wave-uniform
struct Commands {
  uint32_t flags;
  float dz, p_still, p_move, range[6], rel_standing, T[2];
};

__device__ __forceinline__ Commands commands_of(float mine) {
  Commands C;
  C.flags = (uint32_t)__float_as_int(ev_word(mine, 0));
  C.dz = ev_word(mine, 1), C.p_still = ev_word(mine, 2), C.p_move = ev_word(mine, 3);
#pragma unroll
  for (int i = 0; i < 6; ++i) C.range[i] = ev_word(mine, 4 + i);
  C.rel_standing = ev_word(mine, 10);
  C.T[0] = ev_word(mine, 11), C.T[1] = ev_word(mine, 12);
  return C;
}

// draw(third): the three commands from words 0..2, the standing decision from word 3
__device__ __forceinline__ void cmd_draw(const catppo_servo_sim& d, const Commands& C, uint32_t gid, uint32_t ep, uint32_t third,
                                         float c[3], bool& standing) {
  const rng::u32x4 r = ev_block(d, gid, ep, third, kTagCmdDraw);
  c[0] = C.range[0] + rng::uniform_open(r.x) * C.range[1];
  c[1] = C.range[2] + rng::uniform_open(r.y) * C.range[3];
  c[2] = C.range[4] + rng::uniform_open(r.z) * C.range[5];
  standing = rng::uniform_open(r.w) <= C.rel_standing;
}

// the dead-zone rule: no |c_i| above the dead zone zeroes the command
__device__ __forceinline__ void cmd_deadzone(const Commands& C, float c[3]) {
  if (C.flags & CATPPO_SERVO_COMMAND_DEADZONE) {
    const bool any = fabsf(c[0]) > C.dz || fabsf(c[1]) > C.dz || fabsf(c[2]) > C.dz;
    if (!any) c[0] = c[1] = c[2] = 0.f;
  }
}

// the first command of (env, episode): draw, dead zone, standing
__device__ __forceinline__ void first_command(const catppo_servo_sim& d, const Commands& C, uint32_t gid, uint32_t ep, float c[3]) {
  bool standing;
  cmd_draw(d, C, gid, ep, 0u, c, standing);
  cmd_deadzone(C, c);
  if ((C.flags & CATPPO_SERVO_COMMAND_STANDING) && standing) c[0] = c[1] = c[2] = 0.f;
}

// "any" over the 16 lanes of an env: the butterfly of tree16 with max in place of + (exact, so its order does not matter)
__device__ __forceinline__ float any16(float x) {
  x = fmaxf(x, __shfl_xor(x, 8, 16));
  x = fmaxf(x, __shfl_xor(x, 4, 16));
  x = fmaxf(x, __shfl_xor(x, 2, 16));
  x = fmaxf(x, __shfl_xor(x, 1, 16));
  return x;
}

// the length of a contact force, in the association of IsaacLab's norm over (x, y, z)
__device__ __forceinline__ float force_norm(float fx, float fy, float fz) { return sqrtf((fx * fx + fy * fy) + fz * fz); }

// what a lane keeps for the termination terms between the top of the kernel and their loop; empty without them
template <bool kOn>
struct TermRegs {};
template <>
struct TermRegs<true> {
  catppo_servo_term_entry entry = {0, 0u, 0.f, 0.f};      // lane k: entry k of the table
  int terms = 0;
  float rec0 = 0.f;                                        // lane k: float k of the env's record before this step
  uint32_t fired = 0u;                                     // bit k: term k fired in this step
  bool gone = false;                                       // some term that is no time-out fired
};

// what ends the episode besides the time-out: the model's roll-over flag, or the table's verdict
template <bool kOn>
__device__ __forceinline__ bool gone_of(const TermRegs<kOn>& tr, bool fallen) {
  if constexpr (kOn) return tr.gone;
  else return fallen;
}

// what lane j < 12 keeps of entry j of the action table, and the width of the action; empty without the table
template <bool kOn>
struct ActRegs {};
template <>
struct ActRegs<true> {
  catppo_servo_action_entry entry = {0, 0u, 0.f, 0.f, 0.f, 0.f, {0u, 0u}};
  int A = kJoints;
};

// what lane j < 12 keeps of entry j of the actuator table, the env's lag and the three history slots of the input row;
// empty without the table
template <bool kOn>
struct ActuRegs {};
template <>
struct ActuRegs<true> {
  catppo_servo_actuator_entry entry = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 0u, 0u};
  float h0 = 0.f, h1 = 0.f, h2 = 0.f;                      // slot k - 1: the processed action k control steps ago
  int L = 0;                                               // the lag of the joint's group, in physics steps
  float vl = 1.f;                                          // the velocity limit of a DC motor, 1.f for every other joint
};

// the servo torque of one substep before its clamp: the PD law on the target q_des, or the action term's (kind, processed
// action p) of the joint's table entry.  Selects, no branches: the kinds differ between the lanes of a wave
template <bool kOn>
__device__ __forceinline__ float servo_tau(const catppo_servo_sim& d, const ActRegs<kOn>& ar, float q_des, float p, float def,
                                           float q, float qd) {
  if constexpr (kOn) {
    const int kind = (int)(ar.entry.flags & CATPPO_SERVO_ACTION_KIND_MASK);
    const float tgt = kind == 1 ? p : kind == 2 ? p + q : def;
    const float pd = d.kp * (tgt - q) - d.kd * qd;
    const float vel = d.kd * (p - qd);
    return kind == 3 ? vel : kind == 4 ? p : pd;
  } else {
    return d.kp * (q_des - q) - d.kd * qd;
  }
}

// the joint's inertia: the descriptor's scalar, or lane j's entry of the actuator table
template <bool kOn>
__device__ __forceinline__ float inertia_of(const catppo_servo_sim& d, const ActuRegs<kOn>& ur) {
  if constexpr (kOn) return ur.entry.inertia;
  else return d.inertia;
}

// ... with the gains of the joint's actuator entry in the place of d.kp and d.kd
__device__ __forceinline__ float servo_tau(const ActRegs<true>& ar, const ActuRegs<true>& ur, float p, float def, float q,
                                           float qd) {
  const int kind = (int)(ar.entry.flags & CATPPO_SERVO_ACTION_KIND_MASK);
  const float tgt = kind == 1 ? p : kind == 2 ? p + q : def;
  const float pd = ur.entry.kp * (tgt - q) - ur.entry.kd * qd;
  const float vel = ur.entry.kd * (p - qd);
  return kind == 3 ? vel : kind == 4 ? p : pd;
}

// the processed action substep s acts on: this step's, or the history slot the lag reaches back to (at most the third)
__device__ __forceinline__ float delayed_p(const ActuRegs<true>& ur, int s, int decimation, float p) {
  int k = s >= ur.L ? 0 : (ur.L - s + decimation - 1) / decimation;
  k = k < 3 ? k : 3;
  return k == 0 ? p : k == 1 ? ur.h0 : k == 2 ? ur.h1 : ur.h2;
}

// the clamp of one substep's torque: +- effort_limit, or the DC motor's torque-speed bounds at the substep's qd
__device__ __forceinline__ float actuator_clamp(const ActuRegs<true>& ur, float tau, float qd) {
  const float eff = ur.entry.effort_limit, sat = ur.entry.saturation_effort;
  const float ideal = fminf(fmaxf(tau, -eff), eff);
  const float r = qd / ur.vl;
  float hi = sat * (1.f - r);
  hi = fminf(fmaxf(hi, 0.f), eff);
  float lo = sat * (-1.f - r);
  lo = fminf(fmaxf(lo, -eff), 0.f);
  const float dc = fminf(fmaxf(tau, lo), hi);
  return (ur.entry.flags & CATPPO_SERVO_ACTUATOR_DC_MOTOR) ? dc : ideal;
}

// what a lane keeps of the randomised robot of its env (lane j: joint j); empty without the randomisation block
template <bool kOn>
struct RndRegs {};
template <>
struct RndRegs<true> {
  float kp = 0.f, kd = 0.f, inertia = 1.f;                 // in the place of the actuator entry's
  float fr = 0.f, df = 0.f;                                // the Coulomb torque and the speed it takes off per substep
  float weight = 0.f, av = 0.f;                            // in the place of d.weight and d.vel_alpha
  float mine = 0.f, arm = 0.f;                             // wave lane k < 32: word k of the block; lane j: word 20 + j
};

// ... or the randomised one of the lane's joint
template <bool kActu>
__device__ __forceinline__ float inertia_of(const catppo_servo_sim& d, const ActuRegs<kActu>& ur, const RndRegs<true>& rr) {
  return rr.inertia;
}
template <bool kActu>
__device__ __forceinline__ float inertia_of(const catppo_servo_sim& d, const ActuRegs<kActu>& ur, const RndRegs<false>&) {
  return inertia_of(d, ur);
}

// the load the stance feet share and the gain of the base's velocity lags: the descriptor's, or the env's own
__device__ __forceinline__ float weight_of(const catppo_servo_sim& d, const RndRegs<false>&) { return d.weight; }
__device__ __forceinline__ float weight_of(const catppo_servo_sim&, const RndRegs<true>& rr) { return rr.weight; }
__device__ __forceinline__ float vel_alpha_of(const catppo_servo_sim& d, const RndRegs<false>&) { return d.vel_alpha; }
__device__ __forceinline__ float vel_alpha_of(const catppo_servo_sim&, const RndRegs<true>& rr) { return rr.av; }

// ... with randomised gains in the place of the entry's
__device__ __forceinline__ float servo_tau(const ActRegs<true>& ar, const RndRegs<true>& rr, float p, float def, float q, float qd) {
  const int kind = (int)(ar.entry.flags & CATPPO_SERVO_ACTION_KIND_MASK);
  const float tgt = kind == 1 ? p : kind == 2 ? p + q : def;
  const float pd = rr.kp * (tgt - q) - rr.kd * qd;
  const float vel = rr.kd * (p - qd);
  return kind == 3 ? vel : kind == 4 ? p : pd;
}

// one rounded operation on the nominal value x: 0 "scale", 1 "add", 2 "abs"
__device__ __forceinline__ float rnd_op(uint32_t op, float x, float s) { return op == 0u ? x * s : op == 1u ? x + s : s; }

// the robot of (env, episode): the actuator entry's gains and inertia, d.weight and d.vel_alpha, or what the randomisation
// block's terms make of them.  rr.mine: wave lane k < 32 has loaded word k; every branch on a flag is wave-uniform, a term that
// is off draws no Philox block.  rr.arm: the nominal armature of the lane's joint (word 20 + lane)
__device__ __forceinline__ void randomize(const catppo_servo_sim& d, const ActuRegs<true>& ur, uint32_t gid, uint32_t ep, int lane,
                                          RndRegs<true>& rr) {
  const float mine = rr.mine, arm = rr.arm;
  rr.kp = ur.entry.kp, rr.kd = ur.entry.kd, rr.inertia = ur.entry.inertia;
  rr.fr = 0.f, rr.df = 0.f, rr.weight = d.weight, rr.av = d.vel_alpha;
  const uint32_t flags = (uint32_t)__float_as_int(ev_word(mine, 0));
  if (!(flags & CATPPO_SERVO_RANDOMIZE_ENABLE)) return;
  const uint32_t ops = (uint32_t)__float_as_int(ev_word(mine, 1));
  if (flags & (CATPPO_SERVO_RANDOMIZE_KP | CATPPO_SERVO_RANDOMIZE_KD)) {
    const bool sel = (((uint32_t)__float_as_int(ev_word(mine, 2)) >> lane) & 1u) != 0u;
    const rng::u32x4 r = ev_block(d, gid, (flags & CATPPO_SERVO_RANDOMIZE_GAINS_RESET) ? ep : 0u, (uint32_t)lane, kTagGains);
    const float s0 = ev_word(mine, 6) + rng::uniform_open(r.x) * ev_word(mine, 7);
    const float s1 = ev_word(mine, 8) + rng::uniform_open(r.y) * ev_word(mine, 9);
    if ((flags & CATPPO_SERVO_RANDOMIZE_KP) && sel) rr.kp = rnd_op(ops & 0xFFu, ur.entry.kp, s0);
    if ((flags & CATPPO_SERVO_RANDOMIZE_KD) && sel) rr.kd = rnd_op(ops & 0xFFu, ur.entry.kd, s1);
  }
  if (flags & (CATPPO_SERVO_RANDOMIZE_FRICTION | CATPPO_SERVO_RANDOMIZE_ARMATURE)) {
    const bool sel = (((uint32_t)__float_as_int(ev_word(mine, 3)) >> lane) & 1u) != 0u;
    const rng::u32x4 r = ev_block(d, gid, (flags & CATPPO_SERVO_RANDOMIZE_JOINT_RESET) ? ep : 0u, (uint32_t)lane, kTagJointPar);
    const float s0 = ev_word(mine, 10) + rng::uniform_open(r.x) * ev_word(mine, 11);
    const float s1 = ev_word(mine, 12) + rng::uniform_open(r.y) * ev_word(mine, 13);
    const uint32_t op = (ops >> 8) & 0xFFu;
    if ((flags & CATPPO_SERVO_RANDOMIZE_FRICTION) && sel) rr.fr = rnd_op(op, 0.f, s0);
    if ((flags & CATPPO_SERVO_RANDOMIZE_ARMATURE) && sel) rr.inertia = ev_word(mine, 18) + rnd_op(op, arm, s1);
    rr.df = (rr.fr / rr.inertia) * d.dt;
  }
  if (flags & CATPPO_SERVO_RANDOMIZE_MASS) {
    const rng::u32x4 r = ev_block(d, gid, (flags & CATPPO_SERVO_RANDOMIZE_MASS_RESET) ? ep : 0u, 0u, kTagMass);
    const float m0 = ev_word(mine, 16);
    const float m = rnd_op((ops >> 16) & 0xFFu, m0, ev_word(mine, 14) + rng::uniform_open(r.x) * ev_word(mine, 15));
    rr.weight = m * ev_word(mine, 17);
    rr.av = fminf(d.vel_alpha / (m / m0), 1.f);
  }
}

// what a lane keeps of its env's row of the plant table (lane k < 8 of the env's 16: word k); empty without the table
template <bool kOn>
struct PlantRegs {};
template <>
struct PlantRegs<true> {
  float mine = 0.f;
};

// the pinned plant of the env ("Robustness"): the quantities whose bit is set in word 0 of the env's row
// stand where the lag draw and randomize() left theirs, on every joint.  Seven 16-wide shuffles up front (every lane of the env
// takes part), then branches that the env's 16 lanes take together; one rounded operation each
__device__ __forceinline__ void pin_plant(const catppo_servo_sim& d, const PlantRegs<true>& pr, ActuRegs<true>& ur, RndRegs<true>& rr) {
  const uint32_t bits = (uint32_t)__float_as_int(__shfl(pr.mine, 0, 16));
  const float t1 = __shfl(pr.mine, 1, 16), t2 = __shfl(pr.mine, 2, 16), t3 = __shfl(pr.mine, 3, 16);
  const float t4 = __shfl(pr.mine, 4, 16), t5 = __shfl(pr.mine, 5, 16);
  const uint32_t lag = (uint32_t)__float_as_int(__shfl(pr.mine, 6, 16));
  if (bits & CATPPO_SERVO_PLANT_KP) rr.kp = ur.entry.kp * t1;
  if (bits & CATPPO_SERVO_PLANT_KD) rr.kd = ur.entry.kd * t2;
  if (bits & CATPPO_SERVO_PLANT_FRICTION) rr.fr = t3;
  if (bits & CATPPO_SERVO_PLANT_ARMATURE) rr.inertia = ev_word(rr.mine, 18) + t4;
  if (bits & (CATPPO_SERVO_PLANT_FRICTION | CATPPO_SERVO_PLANT_ARMATURE)) rr.df = (rr.fr / rr.inertia) * d.dt;
  if (bits & CATPPO_SERVO_PLANT_MASS) {
    const float m0 = ev_word(rr.mine, 16);
    const float m = m0 * t5;
    rr.weight = m * ev_word(rr.mine, 17);
    rr.av = fminf(d.vel_alpha / (m / m0), 1.f);
  }
  if (bits & CATPPO_SERVO_PLANT_LAG) ur.L = (int)(lag < 255u ? lag : 255u);
}

// kMode = kTrain is the launch with all three evaluation pointers NULL: everything they add is compiled out of it, so
// that a training step runs the code it ran before the fields existed.  kEvaluate: a fixed-command table [N, 3] or an
// evaluation record, and nothing else - the evaluation that runs inside training keeps the code it had, too.
// kStepResponse: a command schedule or a step trace (either may be absent: two wave-uniform branches).  It is held to
// the 64 VGPRs the other two come out at: at 8 workgroups per CU 32768 envs are one resident round, at 7 they are two.
// kRew: the launch with reward_terms > 0 ("Rewards").  Orthogonal to the mode; with kRew false every
// line it adds is compiled out, so the three instances above keep their instruction streams.  The reward terms are
// evaluated in a wave-uniform loop over the table (lane k loads entry k up front, the loop reads it with readlane), every
// lane ends up with the same bits of every term, lane k keeps term k for the record.  The rewards-on instances are not held to 64 VGPRs
// Obs: empty, or catppo_servo_obs for the launch with an observation table ("Observations"): a post-pass
// over the finished LDS row fills the row's second observation field.  Orthogonal to both; only the obs-on launch carries
// the second kernel argument, and with the pack empty every line it adds is compiled out.  LDS (16 rows of about 356
// floats) admits 7 workgroups of the obs-on instances per CU, so they are not held to 64 VGPRs either.
// The pack may also hold catppo_servo_events, alone or behind catppo_servo_obs ("Events"): pushes, the
// first state's reset terms and the traction.  Orthogonal to the rest; only the events-on launch carries that kernel
// argument, and without it every line it adds is compiled out.  24 instances in all.
// catppo_servo_commands, last in the pack ("Commands"): the velocity command is the stateful process of the
// command block instead of command_of's draws, at its three call sites.  Orthogonal to the rest, compiled out without it:
// 24 more instances, none of which is held to 64 VGPRs.
// catppo_servo_terminations, last in the pack ("Terminations"): the table's terms decide when an episode
// is over; `terminated` (the OR of the fired terms that are no time-out) stands where `fallen` stood in `ends`, hard_reset,
// reward kinds 15 / 16, the evaluation record and the trace.  Orthogonal to the rest, compiled out without it: 32 more
// instances (their evaluation mode launches the step-response one, see launch()), none of which is held to 64 VGPRs.
// catppo_servo_actions, last in the pack ("Actions"): lane j's entry of the action table says which action
// column drives joint j, through which scale, offset and clip, and as what kind of target; the raw action by column stands
// where `a` stood.  Orthogonal to the rest, compiled out without it: 64 more instances (16 packs, evaluation folded as
// above), compiled in servo_sim_actions.hip.
// catppo_servo_actuators, last in the pack and only behind catppo_servo_actions ("Actuators"): lane j's entry
// of the actuator table stands where d.kp, d.kd, d.inertia and d.tau_max stand, a DC motor's clamp follows the substep's qd,
// and the processed action may act late by the env's lag, out of three history slots of the row.  Orthogonal to the rest,
// compiled out without it: 64 more instances (16 packs, evaluation folded as above), compiled in servo_sim_actuators.hip.
// catppo_servo_randomize, last in the pack and only behind catppo_servo_actuators ("Randomisation"): the
// env's own gains, joint inertia, joint friction, foot load and velocity-lag gain, re-derived in every step from stateless
// draws, stand where the actuator entry's and the descriptor's stand.  Orthogonal to the rest, compiled out without it: 64
// more instances (16 packs, evaluation folded as above), compiled in servo_sim_randomize.hip.
// catppo_servo_history, last in the pack and only behind catppo_servo_randomize and with catppo_servo_obs (DESIGN section 9,
// "History"): after the observation post-pass the env's 16 lanes write the row's second policy field, T floats outside the
// LDS-staged part of the row: per float the current frame's (the first frame of an episode fills every slot) or the input
// row's float one slot later.  Selects and copies, no arithmetic.  Orthogonal to the rest, compiled out without it: 32 more
// instances (8 packs, evaluation folded as above), compiled in servo_sim_history.hip.
// catppo_servo_plant, last in the pack and only behind catppo_servo_randomize, with or without catppo_servo_history (DESIGN
// section 9, "Robustness"): the quantities that the env's row of the plant table pins stand where the lag draw and randomize()
// left theirs.  An evaluation input: launch() takes the step-response instance whatever the mode.  Orthogonal to the rest,
// compiled out without it: 48 more instances (16 packs without a history, 8 with one), compiled in servo_sim_plant.hip.
// ServoEventsExt in the place of catppo_servo_events ("Disturbances"): the event block has
// CATPPO_SERVO_EVENT_FLOATS_EXT words and carries a timed push (the env's own timer, kept in the row field ev.reserved names) and
// an external wrench on the base.  A template parameter of the events path: every instance over catppo_servo_events compiles
// without a line of it; inside, the branches on the flag word are wave-uniform, and a block with neither bit set computes the
// bytes of the 32-word launch.  168 more instances (every events-on pack, evaluation folded as above), compiled in
// servo_sim_disturb.hip and servo_sim_disturb_robot.hip.
template <int kMode, bool kRew, typename... Ext>
__global__ __launch_bounds__(kThreads, (kMode == kStepResponse && !kRew && sizeof...(Ext) == 0) ? 8 : 1) void servo_sim_kernel(
    const catppo_servo_sim d, const Ext... ext) {
  constexpr bool kObs = (std::is_same_v<Ext, catppo_servo_obs> || ...);
  constexpr bool kDist = (std::is_same_v<Ext, ServoEventsExt> || ...);
  constexpr bool kEv = (std::is_same_v<Ext, catppo_servo_events> || ...) || kDist;
  constexpr bool kCmd = (std::is_same_v<Ext, catppo_servo_commands> || ...);
  constexpr bool kTerm = (std::is_same_v<Ext, catppo_servo_terminations> || ...);
  constexpr bool kAct = (std::is_same_v<Ext, catppo_servo_actions> || ...);
  constexpr bool kActu = (std::is_same_v<Ext, catppo_servo_actuators> || ...);
  static_assert(kAct || !kActu, "the actuator descriptor comes only behind the action descriptor");
  constexpr bool kRnd = (std::is_same_v<Ext, catppo_servo_randomize> || ...);
  static_assert(kActu || !kRnd, "the randomisation descriptor comes only behind the actuator descriptor");
  constexpr bool kHist = (std::is_same_v<Ext, catppo_servo_history> || ...);
  static_assert((kRnd && kObs) || !kHist, "the history descriptor comes only behind the randomisation descriptor, with observations");
  constexpr bool kPlant = (std::is_same_v<Ext, catppo_servo_plant> || ...);
  static_assert((kRnd && kMode == kStepResponse) || !kPlant,
                "the plant descriptor comes only behind the randomisation descriptor, in the step-response instance");
  constexpr bool kEval = kMode != kTrain;
  RndRegs<kRnd> RR;                      // declared first: further down it reorders register initialisations of older instances
  ActuRegs<kActu> UR;                    // likewise
  extern __shared__ float4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  const int tid = threadIdx.x, lane = tid & 15, grp = tid >> 4;
  // wave lane k < 32 loads word k of the event block (every lane of the wave its word of an extended one), long before the
  // first use
  float ev_mine = 0.f;
  if constexpr (kDist) ev_mine = events_desc<true>(ext...).block[tid & 63];
  else if constexpr (kEv)
    if ((tid & 63) < CATPPO_SERVO_EVENT_FLOATS) ev_mine = ext_of<catppo_servo_events>(ext...).block[tid & 63];
  // wave lane k < 16 loads word k of the command block
  float cmd_mine = 0.f;
  if constexpr (kCmd)
    if ((tid & 63) < CATPPO_SERVO_COMMAND_FLOATS) cmd_mine = ext_of<catppo_servo_commands>(ext...).block[tid & 63];
  // lane j < 12 loads entry j of the action table (two 16-byte loads), long before the substep loop reads it
  ActRegs<kAct> AR;
  if constexpr (kAct) {
    const catppo_servo_actions& ac = ext_of<catppo_servo_actions>(ext...);
    AR.A = ac.width;
    if (lane < kJoints && d.init == 0) AR.entry = ac.table[lane];
  }
  const int F = d.row_floats, D = d.obs_dim, B3 = d.B * 3;
  const int64_t e0 = (int64_t)blockIdx.x * kEnvsPerBlock;
  // rows past N recompute the last env and are dropped at the store: no divergence around the shuffles and barriers
  const int64_t e = e0 + grp < d.N ? e0 + grp : d.N - 1;
  float* row = lds + grp * F;
  for (int i = lane; i < F; i += 16) row[i] = 0.f;
  __syncthreads();

  const float* in = d.state_in + e * d.row_stride;
  const float* xin = in + d.off_servo;
  const bool init = d.init != 0;
  const bool rst = init || d.reset[e] != 0;
  const int64_t t = d.episode_length[e];
  const uint32_t gid = (uint32_t)(d.env_offset + e);
  const uint32_t ep = init ? 0u : (uint32_t)xin[13];
  const bool isj = lane < kJoints;
  const int f = lane & 3, foot_body = 4 * f + 4;
  const float def = isj ? d.default_joint_pos[lane] : 0.f;
  float cmd[3];
  // commands on: the time left until the timed resample, what the trace says of this step's update, and whether the
  // generator runs at all (a fixed-command table wins)
  Commands CM = {};
  float cmd_tl = 0.f, cmd_mark = 0.f;
  bool cmd_gen = true;
  if constexpr (kCmd) {
    CM = commands_of(cmd_mine);
    if constexpr (kMode != kTrain) cmd_gen = d.fixed_command == nullptr;
    if (!cmd_gen) {
      if constexpr (kMode != kTrain) command_of<kMode>(d, e, gid, ep, 0u, t, cmd);
    } else if (rst) {
      first_command(d, CM, gid, ep, cmd);
      cmd_tl = CM.T[0] + rng::uniform_open(ev_block(d, gid, ep, 0u, kTagCmdTime).x) * CM.T[1];
    } else {
      // the update of IsaacLab's command term, at the start of the step it applies to; D: the step's time block, whose
      // words 2 and 3 are its two decisions
      for (int i = 0; i < 3; ++i) cmd[i] = in[d.off_command + i];
      cmd_tl = in[ext_of<catppo_servo_commands>(ext...).off_cmd_state];
      const uint32_t third = ((uint32_t)t + 1u) << 1;
      const rng::u32x4 D = ev_block(d, gid, ep, third, kTagCmdTime);
      cmd_tl = cmd_tl - d.dt * (float)d.decimation;
      if (cmd_tl <= 0.f) {
        bool standing;
        cmd_draw(d, CM, gid, ep, third, cmd, standing);
        if ((CM.flags & CATPPO_SERVO_COMMAND_STANDING) && standing) cmd[0] = cmd[1] = cmd[2] = 0.f;
        cmd_tl = CM.T[0] + rng::uniform_open(D.x) * CM.T[1];
        cmd_mark = 1.f;
      }
      cmd_deadzone(CM, cmd);
      if (CM.flags & CATPPO_SERVO_COMMAND_RANDOM_RESAMPLE) {
        const bool still = sqrtf((cmd[0] * cmd[0] + cmd[1] * cmd[1]) + cmd[2] * cmd[2]) < CM.dz;
        if (rng::uniform_open(D.z) < (still ? CM.p_still : CM.p_move)) {
          bool standing;
          cmd_draw(d, CM, gid, ep, third | 1u, cmd, standing);       // meets the dead zone in the next step
          cmd_tl = CM.T[0] + rng::uniform_open(ev_block(d, gid, ep, third | 1u, kTagCmdTime).x) * CM.T[1];
          cmd_mark = 1.f;
        }
      }
      if ((CM.flags & CATPPO_SERVO_COMMAND_YAW_FLIP) && rng::uniform_open(D.w) < CM.p_move) {
        cmd[2] = -cmd[2];
        cmd_mark = cmd_mark + 2.f;
      }
    }
  } else {
    command_of<kMode>(d, e, gid, ep, (uint32_t)(t / d.resample_steps), t, cmd);
  }
  Events E = {};
  if constexpr (kEv) E = events_of(ev_mine);
  DisturbRegs<kDist> DX;
  if constexpr (kDist) DX = disturb_of(ev_mine, events_desc<true>(ext...).reserved);
  float* obs = row + d.off_obs;
  // (episode, episode length) of the state the observation describes: the key of its noise
  uint32_t obs_ep = 0u, obs_t = 0u;
  // history: the frame the post-pass produces is the first of an episode and fills every slot
  bool hist_fill = init;
  // evaluation record: lane k < 12 of a live lane group owns field k of its env (one 48-byte access per env); the spare
  // groups past N, which recompute env N - 1, neither read nor write it
  const bool rec = kEval && d.eval != nullptr && e0 + grp < d.N && isj;
  const int64_t rec_at = e * CATPPO_SERVO_EVAL_FLOATS + lane;
  float rec0 = 0.f;
  if constexpr (kEval)
    if (rec && !init) rec0 = d.eval[rec_at];
  // reward record: lane k of a live lane group owns floats k and 16 + k of its env (two 64-byte accesses per env)
  const bool rrec = kRew && e0 + grp < d.N;
  const int64_t rrec_at = e * CATPPO_SERVO_REWARD_FLOATS + lane;
  float run0 = 0.f, done0 = 0.f, a_prev = 0.f;
  // lane k holds entry k of the table (one 16-byte load per lane, issued here, long before the loop that reads it through
  // readlane: the loop then waits for no memory)
  catppo_servo_reward_term mine_tm = {0, 0u, 0.f, 0.f};
  if constexpr (kRew) {
    if (!init && lane < d.reward_terms) mine_tm = d.reward_table[lane];
    if (rrec && !init) run0 = d.reward_rec[rrec_at], done0 = d.reward_rec[rrec_at + 16];
    // the last-action block of the input row: the action manager's history (zero after a step that ended an episode)
    if (isj && !rst && D >= 45) a_prev = in[d.off_obs + 33 + lane];
  }
  // termination table and record: lane k holds entry k (one 16-byte load, long before the loop that reads it through
  // readlane); lane k of a live lane group owns float k of its env's record (one 64-byte access per env)
  TermRegs<kTerm> TR;
  if constexpr (kTerm) {
    const catppo_servo_terminations& tm = ext_of<catppo_servo_terminations>(ext...);
    TR.terms = tm.terms;
    if (!init && lane < TR.terms) TR.entry = tm.table[lane];
    if (e0 + grp < d.N && !init) TR.rec0 = tm.rec[e * CATPPO_SERVO_TERM_FLOATS + lane];
  }
  // lane j < 12 loads entry j of the actuator table (two 16-byte loads), long before the substep loop reads it
  if constexpr (kActu)
    if (lane < kJoints && d.init == 0) UR.entry = ext_of<catppo_servo_actuators>(ext...).table[lane];
  // wave lane k < 32 loads word k of the randomisation block, lane j < 12 the nominal armature of its joint as well
  if constexpr (kRnd) {
    const float* blk = ext_of<catppo_servo_randomize>(ext...).block;
    if ((tid & 63) < CATPPO_SERVO_RANDOMIZE_FLOATS && d.init == 0) RR.mine = blk[tid & 63];
    if (lane < kJoints && d.init == 0) RR.arm = blk[20 + lane];
  }
  // lane k < 8 loads word k of its env's row of the plant table: 32 bytes per env; the spare lane groups past N read the row
  // of env N - 1, which they recompute
  PlantRegs<kPlant> PR;
  if constexpr (kPlant)
    if (lane < CATPPO_SERVO_PLANT_FLOATS && d.init == 0)
      PR.mine = ext_of<catppo_servo_plant>(ext...).table[e * CATPPO_SERVO_PLANT_FLOATS + lane];

  if (init) {
    // the first state of episode 0: default pose + noise, at rest, four feet on the ground
    if constexpr (kEv) {
      // with events the first state may move: the joint-reset term's pose and velocity
      if (isj) {
        float q0 = 0.f, qd0 = 0.f;
        first_joint(d, E, gid, 0u, lane, def, q0, qd0);
        row[d.off_joint_pos + lane] = q0;
        row[d.off_joint_vel + lane] = qd0;
        if (9 + lane < D) obs[9 + lane] = q0 - def;
        if (21 + lane < D) obs[21 + lane] = qd0;
      } else {
        row[d.off_servo + 9 + f] = 1.f;
      }
    } else {
      const float q0 = isj ? init_q(d, gid, 0u, lane, def) : 0.f;
      if (isj) {
        row[d.off_joint_pos + lane] = q0;
        if (9 + lane < D) obs[9 + lane] = q0 - def;
      } else {
        row[d.off_servo + 9 + f] = 1.f;
      }
    }
    if (lane == 12) {
      row[d.off_projected_gravity + 2] = -1.f;
      row[d.off_root_pos + 2] = d.stand_height;
      if (5 < D) obs[5] = -1.f;
      if constexpr (kEv) {
        float xy[2], fv[3];
        first_root(d, E, gid, 0u, xy, fv);
        row[d.off_root_pos] = xy[0], row[d.off_root_pos + 1] = xy[1];
        for (int k = 0; k < 3; ++k) row[d.off_servo + k] = fv[k];
        if (2 < D) obs[2] = fv[2];
      }
    }
    if (lane == 13) {
      for (int k = 0; k < 3; ++k) {
        row[d.off_command + k] = cmd[k];
        if (6 + k < D) obs[6 + k] = cmd[k];
      }
      if constexpr (kCmd) row[ext_of<catppo_servo_commands>(ext...).off_cmd_state] = cmd_gen ? cmd_tl : 0.f;
      // the timer of episode 0 (without the timed push the field stays the zeros the row was filled with)
      if constexpr (kDist)
        if (DX.flags & CATPPO_SERVO_EVENT_PUSH_TIMED) row[DX.off_state] = push_time(d, DX, gid, 0u, 0u);
    }
    if constexpr (kEval)
      if (rec) d.eval[rec_at] = 0.f;
    if constexpr (kRew)
      if (rrec) d.reward_rec[rrec_at] = 0.f, d.reward_rec[rrec_at + 16] = 0.f;
    // term_state is part of the zero-filled row
    if constexpr (kTerm)
      if (e0 + grp < d.N) ext_of<catppo_servo_terminations>(ext...).rec[e * CATPPO_SERVO_TERM_FLOATS + lane] = 0.f;
  } else {
    // ---- the state this step starts from: the row, or the first state of episode `ep` re-derived from the counter
    float q = 0.f, qd = 0.f, a = 0.f;
    if (isj) {
      if constexpr (kEv) {
        q = in[d.off_joint_pos + lane], qd = in[d.off_joint_vel + lane];
        if (rst) first_joint(d, E, gid, ep, lane, def, q, qd);
      } else {
        q = rst ? init_q(d, gid, ep, lane, def) : in[d.off_joint_pos + lane];
        qd = rst ? 0.f : in[d.off_joint_vel + lane];
      }
      if constexpr (!kAct) a = d.action[e * kJoints + lane];
    }
    // the processed action of the joint's column; `a` is the raw action by column from here on (zero past the width)
    float act_p = 0.f;
    if constexpr (kAct) {
      if (lane < AR.A) a = d.action[e * AR.A + lane];
      const int col = AR.entry.col < 0 ? 0 : AR.entry.col < AR.A ? AR.entry.col : AR.A - 1;
      act_p = __shfl(a, col, 16) * AR.entry.scale + AR.entry.offset;
      if (AR.entry.flags & CATPPO_SERVO_ACTION_CLIP) {
        act_p = act_p < AR.entry.clip_lo ? AR.entry.clip_lo : act_p;
        act_p = act_p > AR.entry.clip_hi ? AR.entry.clip_hi : act_p;
      }
    }
    // actuators: the three history slots of the input row (three loads up front, chosen by selects in the loop; after a
    // reset, or behind an init launch, all three count as this step's p) and the lag of the joint's group
    if constexpr (kActu) {
      const float* hin = in + ext_of<catppo_servo_actuators>(ext...).off_act_hist;
      const float s0 = hin[lane], s1 = hin[16 + lane], s2 = hin[32 + lane];
      const bool fresh = rst || hin[12] == 0.f;
      UR.h0 = fresh ? act_p : s0, UR.h1 = fresh ? act_p : s1, UR.h2 = fresh ? act_p : s2;
      const int mn = (int)(UR.entry.delay & 0xFFu), mx = (int)((UR.entry.delay >> 8) & 0xFFu);
      UR.L = mn;
      if (mx > mn) {
        const float u = rng::uniform_open(ev_block(d, gid, ep, (UR.entry.delay >> 16) & 0xFFu, kTagActDelay).x);
        const int l = mn + (int)(u * (float)(mx - mn + 1));
        UR.L = l < mx ? l : mx;
      }
      if (UR.entry.flags & CATPPO_SERVO_ACTUATOR_DC_MOTOR) UR.vl = UR.entry.velocity_limit;
    }
    // randomisation: the robot of this env and episode
    if constexpr (kRnd) randomize(d, UR, gid, ep, lane, RR);
    // pinned plant: after the lag draw and the randomisation
    if constexpr (kPlant) pin_plant(d, PR, UR, RR);
    // ---- joints: `decimation` substeps of the clamped PD servo, semi-implicit Euler; the substep of largest |tau| is reported
    const float q_des = def + d.action_scale * a;
    float tau_w = 0.f;
    for (int s = 0; s < d.decimation; ++s) {
      float tau, qdd;
      if constexpr (kRnd) {
        tau = actuator_clamp(UR, servo_tau(AR, RR, delayed_p(UR, s, d.decimation, act_p), def, q, qd), qd);
        qdd = tau / RR.inertia;
      } else if constexpr (kActu) {
        tau = actuator_clamp(UR, servo_tau(AR, UR, delayed_p(UR, s, d.decimation, act_p), def, q, qd), qd);
        qdd = tau / UR.entry.inertia;
      } else {
        tau = servo_tau(d, AR, q_des, act_p, def, q, qd);
        tau = fminf(fmaxf(tau, -d.tau_max), d.tau_max);
        qdd = tau / d.inertia;
      }
      qd = qd + qdd * d.dt;
      // joint friction: an impulse that cannot reverse the joint within the substep
      if constexpr (kRnd) qd = RR.fr > 0.f ? qd - fminf(fmaxf(qd, -RR.df), RR.df) : qd;
      q = q + qd * d.dt;
      if (fabsf(tau) > fabsf(tau_w)) tau_w = tau;
    }
    const float dq = q - def;
    // ---- base: five joint reductions, first-order lags
    float red[5];
    if constexpr (kEv) {
      // the velocity rows feel the env's traction: one more rounded multiply
      const float m = traction_of(d, E, gid);
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k] = k < 3 ? tree16((gain(k, lane) * m) * dq) : tree16(gain(k, lane) * dq);
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k] = tree16(gain(k, lane) * dq);
    }
    // the external wrench of (env, episode) - or of the env, once for all episodes: a force shifts the velocity the legs ask
    // for by F / W m/s, a torque the yaw rate and the tilt by T / (W * stand_height), Fz lifts the load off the stance feet
    float load = weight_of(d, RR);                       // what the stance feet share
    if constexpr (kDist) {
      if (DX.flags & CATPPO_SERVO_EVENT_WRENCH) {
        const uint32_t we = (DX.flags & CATPPO_SERVO_EVENT_WRENCH_RESET) ? ep : 0u;
        const rng::u32x4 a = ev_block(d, gid, we, 0u, kTagWrench), b = ev_block(d, gid, we, 1u, kTagWrench);
        const float W = load, L = W * d.stand_height;
        const float Fx = DX.force[0] + rng::uniform_open(a.x) * DX.force[1], Fy = DX.force[0] + rng::uniform_open(a.y) * DX.force[1];
        const float Fz = DX.force[0] + rng::uniform_open(a.z) * DX.force[1];
        const float Tx = DX.torque[0] + rng::uniform_open(b.x) * DX.torque[1], Ty = DX.torque[0] + rng::uniform_open(b.y) * DX.torque[1];
        const float Tz = DX.torque[0] + rng::uniform_open(b.z) * DX.torque[1];
        red[0] = red[0] + Fx / W;
        red[1] = red[1] + Fy / W;
        red[2] = red[2] + Tz / L;
        red[3] = red[3] + Tx / L;
        red[4] = red[4] + Ty / L;
        load = fmaxf(W - Fz, 0.f);
      }
    }
    const float step_dt = d.dt * (float)d.decimation;
    // events: the root of a first state, and the push of this step on the state the step starts from (after the reset
    // select).  roll_k, pitch_k: the kicked tilt the lags start from; the rates keep differentiating against roll0, pitch0
    float first_xy[2] = {0.f, 0.f}, first_v[3] = {0.f, 0.f, 0.f}, push_v[3] = {0.f, 0.f, 0.f}, kick[2] = {0.f, 0.f};
    bool pushed = false;
    float ev_tl = 0.f;                                   // timed push: the time left, as the output row keeps it
    if constexpr (kEv) {
      if (rst) first_root(d, E, gid, ep, first_xy, first_v);
      if (E.flags & CATPPO_SERVO_EVENT_PUSH) {
        const rng::u32x4 r = ev_block(d, gid, ep, (uint32_t)t << 1, kTagPush);
        pushed = rng::uniform_open(r.x) < E.p;
        if (pushed) {
          push_v[0] = E.push[0] + rng::uniform_open(r.y) * E.push[1];
          push_v[1] = E.push[2] + rng::uniform_open(r.z) * E.push[3];
          push_v[2] = E.push[4] + rng::uniform_open(r.w) * E.push[5];
          const rng::u32x4 r1 = ev_block(d, gid, ep, ((uint32_t)t << 1) | 1u, kTagPush);
          kick[0] = (E.push[6] + rng::uniform_open(r1.x) * E.push[7]) * step_dt;
          kick[1] = (E.push[8] + rng::uniform_open(r1.y) * E.push[9]) * step_dt;
        }
      }
    }
    // the timed push: IsaacLab's interval rule on the env's own timer.  A reset step draws the timer and runs no update; a
    // push ADDS its samples to the velocities (such a step is no reset step: xin is what it starts from).  With both push
    // bits set the per-step push above wins and the timer keeps running
    if constexpr (kDist) {
      bool fire = false;
      if (DX.flags & CATPPO_SERVO_EVENT_PUSH_TIMED) {
        if (rst) {
          ev_tl = push_time(d, DX, gid, ep, 0u);
        } else {
          ev_tl = in[DX.off_state] - step_dt;
          fire = ev_tl < 1e-6f;
          if (fire) ev_tl = push_time(d, DX, gid, ep, (uint32_t)t + 1u);
        }
      } else if (DX.off_state != 0) {
        ev_tl = in[DX.off_state];                        // the bit cleared at run time: carried over
      }
      if (fire && !(E.flags & CATPPO_SERVO_EVENT_PUSH)) {
        const rng::u32x4 r = ev_block(d, gid, ep, (uint32_t)t << 1, kTagPush);
        const rng::u32x4 r1 = ev_block(d, gid, ep, ((uint32_t)t << 1) | 1u, kTagPush);
        pushed = true;
        push_v[0] = xin[0] + (E.push[0] + rng::uniform_open(r.y) * E.push[1]);
        push_v[1] = xin[1] + (E.push[2] + rng::uniform_open(r.z) * E.push[3]);
        push_v[2] = xin[2] + (E.push[4] + rng::uniform_open(r.w) * E.push[5]);
        kick[0] = (E.push[6] + rng::uniform_open(r1.x) * E.push[7]) * step_dt;
        kick[1] = (E.push[8] + rng::uniform_open(r1.y) * E.push[9]) * step_dt;
      }
    }
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v0 = rst ? 0.f : xin[k];
      if constexpr (kEv) v0 = pushed ? push_v[k] : rst ? first_v[k] : xin[k];
      v[k] = v0 + vel_alpha_of(d, RR) * (red[k] - v0);
    }
    const float roll0 = rst ? 0.f : xin[3], pitch0 = rst ? 0.f : xin[4];
    float roll_k = roll0, pitch_k = pitch0;
    if constexpr (kEv)
      if (pushed) roll_k = roll0 + kick[0], pitch_k = pitch0 + kick[1];
    const float roll = roll_k + d.tilt_beta * (red[3] - roll_k);
    const float pitch = pitch_k + d.tilt_beta * (red[4] - pitch_k);
    const float ang[3] = {(roll - roll0) / step_dt, (pitch - pitch0) / step_dt, v[2]};
    const float tilt2 = roll * roll + pitch * pitch;
    const bool fallen = tilt2 > d.tilt_max * d.tilt_max;
    const float nrm = sqrtf(tilt2 + 1.f);
    float grav[3] = {(0.f - pitch) / nrm, roll / nrm, -1.f / nrm};
    if (fallen) grav[0] = 0.f, grav[1] = 0.f, grav[2] = 1.f;
    // ---- feet (every lane: foot lane & 3), base height, contact forces, air times
    const float knee = __shfl(dq, 3 * f + 2, 16), knee_v = __shfl(qd, 3 * f + 2, 16), hfe = __shfl(dq, 3 * f + 1, 16);
    const float con = (0.f - d.foot_clearance * knee) < d.contact_threshold ? 1.f : 0.f;
    const float ncon = tree4(con);
    const float zleg = d.stand_height - d.height_drop * fabsf(hfe);
    const float nsafe = fmaxf(ncon, 1.f);
    const float zsum = tree4(con * zleg);
    const float z = ncon > 0.f ? zsum / nsafe : d.floor_height;
    const float con_prev = rst ? 1.f : xin[9 + f];
    const float air0 = rst ? 0.f : xin[5 + f];
    const float last_air0 = rst ? 0.f : in[d.off_last_air_time + foot_body];
    const bool touch = con > 0.f && !(con_prev > 0.f);
    const float fz = con > 0.f ? load / nsafe + (touch ? d.impact_gain * fabsf(knee_v) : 0.f) : 0.f;
    const float last_air = touch ? air0 : last_air0;
    const float air = con > 0.f ? 0.f : air0 + step_dt;
    const float fbase = z < d.min_height ? d.base_stiffness * (d.min_height - z) : 0.f;
    float x0 = rst ? 0.f : in[d.off_root_pos], y0 = rst ? 0.f : in[d.off_root_pos + 1];
    if constexpr (kEv)
      if (rst) x0 = first_xy[0], y0 = first_xy[1];
    // ---- termination terms: bit k of `fired` is term k of the table; a wave-uniform loop, every lane ends with the same bits
    if constexpr (kTerm) {
      bool gone = false;
      uint32_t fired = 0u;
      // the projected gravity before the roll-over override: what the orientation terms read
      const float g_pre[3] = {(0.f - pitch) / nrm, roll / nrm, -1.f / nrm};
      for (int k = 0; k < TR.terms; ++k) {
        catppo_servo_term_entry te;
        te.kind = __builtin_amdgcn_readlane(TR.entry.kind, k);
        te.mask = (uint32_t)__builtin_amdgcn_readlane((int)TR.entry.mask, k);
        te.p0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(TR.entry.p0), k));
        te.p1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(TR.entry.p1), k));
        const bool mj = isj && ((te.mask >> lane) & 1u);
        bool fire = false;
        switch (te.kind) {
          case 1: fire = t + 1 >= d.max_episode_length; break;
          case 2: {
            // slot 0, this step: base_link (body 0) on every lane, foot lane & 3 (body 4 f + 4); slots 1 .. H - 1 are slots
            // 0 .. H - 2 of the input row (none after a reset): lane l takes body l, lane 0 body 16 as well
            float hit = (te.mask & 1u) && force_norm(0.f, 0.f, fbase) > te.p0 ? 1.f : 0.f;
            if (((te.mask >> foot_body) & 1u) && force_norm(0.f, 0.f, fz) > te.p0) hit = 1.f;
            if (!rst) {
              for (int h = 0; h + 1 < d.H; ++h) {
                const float* fr = in + d.off_forces + h * B3;
                if (((te.mask >> lane) & 1u) && force_norm(fr[lane * 3], fr[lane * 3 + 1], fr[lane * 3 + 2]) > te.p0) hit = 1.f;
                if (lane == 0 && ((te.mask >> 16) & 1u) && force_norm(fr[48], fr[49], fr[50]) > te.p0) hit = 1.f;
              }
            }
            fire = any16(hit) > 0.f;
            break;
          }
          case 3: fire = sqrtf(g_pre[0] * g_pre[0] + g_pre[1] * g_pre[1]) > te.p0; break;
          case 4: fire = (0.f - g_pre[2]) < te.p0; break;
          case 5: fire = z < te.p0; break;
          case 6: fire = any16(mj && (q < te.p0 || q > te.p1) ? 1.f : 0.f) > 0.f; break;
          case 7: fire = any16(mj && fabsf(qd) > te.p0 ? 1.f : 0.f) > 0.f; break;
          case 8: fire = tilt2 > d.tilt_max * d.tilt_max; break;
          default: break;                                  // the table's writer admits no other kind
        }
        if (fire) {
          fired |= 1u << k;
          if (te.kind != 1) gone = true;
        }
      }
      TR.fired = fired, TR.gone = gone;
    }
    // ---- reward: rational stand-ins for the two exp tracking rewards
    const float ex = cmd[0] - v[0], ey = cmd[1] - v[1], ew = cmd[2] - v[2];
    const float reward = 1.f / (1.f + (ex * ex + ey * ey) / d.reward_scale) + 0.5f / (1.f + (ew * ew) / d.reward_scale);
    // ---- does this step end the episode?  Then `obs` already shows the first state of the next one.
    const bool ends = t + 1 >= d.max_episode_length || gone_of(TR, fallen);
    const uint32_t ep_out = ep + (ends ? 1u : 0u);
    if constexpr (kObs) obs_ep = ep_out, obs_t = ends ? 0u : (uint32_t)(t + 1);
    if constexpr (kHist) hist_fill = ends;
    // ---- reward terms: value_k = (raw_k * weight_k) * step_dt in table order, summed from 0.f; lane k keeps value_k
    float rsum = 0.f, mine = 0.f;
    if constexpr (kRew) {
      const float acc = tau_w / inertia_of(d, UR, RR), da = a - a_prev;
      const float moving = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1]) > 0.1f ? 1.f : 0.f;
      for (int k = 0; k < d.reward_terms; ++k) {
        // lanes 0 .. 15 of the wave are its first lane group: lane k of the wave holds entry k
        catppo_servo_reward_term tm;
        tm.kind = __builtin_amdgcn_readlane(mine_tm.kind, k);
        tm.joint_mask = (uint32_t)__builtin_amdgcn_readlane((int)mine_tm.joint_mask, k);
        tm.weight = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_tm.weight), k));
        tm.param = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_tm.param), k));
        const float m = ((tm.joint_mask >> lane) & 1u) ? 1.f : 0.f;
        float raw = 0.f;
        switch (tm.kind) {
          case 1: raw = expf(0.f - (ex * ex + ey * ey) / tm.param); break;
          case 2: raw = expf(0.f - (ew * ew) / tm.param); break;
          case 3: raw = 1.f / (1.f + (ex * ex + ey * ey) / tm.param); break;
          case 4: raw = 1.f / (1.f + (ew * ew) / tm.param); break;
          case 5: raw = ang[0] * ang[0] + ang[1] * ang[1]; break;
          case 6: raw = grav[0] * grav[0] + grav[1] * grav[1]; break;
          case 7: raw = tree16(m * (tau_w * tau_w)); break;
          case 8: raw = tree16(m * (acc * acc)); break;
          case 9: raw = tree16(m * (qd * qd)); break;
          case 10: raw = tree16(m * fabsf(dq)); break;
          case 11: raw = tree16(da * da); break;
          case 12: raw = tree16(a * a); break;
          case 13: raw = tree4((last_air - tm.param) * (touch ? 1.f : 0.f)) * moving; break;
          case 14: raw = (z - tm.param) * (z - tm.param); break;
          case 15: raw = gone_of(TR, fallen) ? 1.f : 0.f; break;
          case 16: raw = gone_of(TR, fallen) ? 0.f : 1.f; break;
          default: break;                                // the table's writer admits no other kind
        }
        const float value = (raw * tm.weight) * step_dt;
        rsum = rsum + value;
        if (lane == k) mine = value;
      }
      // the record: lane 15 owns the zero float 15 and the count of ended episodes (float 31)
      const float s = run0 + mine;
      if (rrec) {
        d.reward_rec[rrec_at] = ends ? 0.f : s;
        if (ends) d.reward_rec[rrec_at + 16] = done0 + (lane == 15 ? 1.f : s);
      }
    }

    // ---- step trace: one row of CATPPO_SERVO_TRACE_FLOATS per traced env, at the slot its record had counted before
    // this step (field 0, held by lane 0); registers to memory, neighbouring lanes write neighbouring floats
    if constexpr (kMode == kStepResponse) {
      const float slot = __shfl(rec0, 0, 16);
      // a float below (float)capacity is an integer below capacity: no float lies between an int and its rounding
      if (d.trace != nullptr && e0 + grp < d.N && e < d.trace_envs && slot >= 0.f && slot < (float)d.trace_capacity) {
        float* tr = d.trace + ((int64_t)slot * d.trace_envs + e) * CATPPO_SERVO_TRACE_FLOATS;
        float head = 0.f;
        switch (lane) {
          case 0: head = (float)t; break;
          case 1: head = ends ? 1.f : 0.f; break;
          case 2: head = gone_of(TR, fallen) ? 1.f : 0.f; break;
          case 3: head = reward; break;
          case 4: head = cmd[0]; break;
          case 5: head = cmd[1]; break;
          case 6: head = cmd[2]; break;
          case 7: head = v[0]; break;
          case 8: head = v[1]; break;
          case 9: head = v[2]; break;
          case 10: head = roll; break;
          case 11: head = pitch; break;
          case 12: head = z; break;
          case 13: head = ncon; break;
          default: break;
        }
        if constexpr (kEv)
          if (lane == 14) head = pushed ? 1.f : 0.f;
        if constexpr (kCmd)
          if (lane == 15) head = cmd_mark;
        tr[lane] = head;
        if (lane < 8) tr[16 + lane] = lane < 4 ? con : fz;      // lanes 0..3 and 4..7 both carry feet 0..3
        if (isj) {
          tr[24 + lane] = q;
          tr[36 + lane] = qd;
          tr[48 + lane] = tau_w;
          tr[60 + lane] = a;
        }
      }
    }

    // ---- assemble the next row
    if (isj) {
      row[d.off_joint_pos + lane] = q;
      row[d.off_joint_vel + lane] = qd;
      row[d.off_joint_acc + lane] = tau_w / inertia_of(d, UR, RR);
      row[d.off_applied_torque + lane] = tau_w;
      float o_q = dq, o_v = qd, o_a = a;
      if constexpr (kEv) {
        if (ends) {
          first_joint(d, E, gid, ep_out, lane, def, o_q, o_v);
          o_q = o_q - def, o_a = 0.f;
        }
      } else {
        if (ends) o_q = init_q(d, gid, ep_out, lane, def) - def, o_v = 0.f, o_a = 0.f;
      }
      if (9 + lane < D) obs[9 + lane] = o_q;
      if (21 + lane < D) obs[21 + lane] = o_v;
      if (33 + lane < D) obs[33 + lane] = o_a;
    } else {
      row[d.off_last_air_time + foot_body] = last_air;
      row[d.off_first_contact + foot_body] = touch ? 1.f : 0.f;
      row[d.off_forces + foot_body * 3 + 2] = fz;
      row[d.off_servo + 5 + f] = air;
      row[d.off_servo + 9 + f] = con;
    }
    if (lane == 12) {
      for (int k = 0; k < 3; ++k) row[d.off_projected_gravity + k] = grav[k];
      row[d.off_root_pos] = x0 + v[0] * step_dt;
      row[d.off_root_pos + 1] = y0 + v[1] * step_dt;
      row[d.off_root_pos + 2] = z;
      row[d.off_forces + 2] = fbase;                    // base_link is body 0
    }
    if (lane == 13) {
      for (int k = 0; k < 3; ++k) row[d.off_command + k] = cmd[k];
      row[d.off_reward] = kRew ? rsum : reward;
      row[d.off_hard_reset] = gone_of(TR, fallen) ? 1.f : 0.f;
      if constexpr (kCmd) row[ext_of<catppo_servo_commands>(ext...).off_cmd_state] = cmd_gen ? cmd_tl : 0.f;
      if constexpr (kDist)
        if (DX.off_state != 0) row[DX.off_state] = ev_tl;
    }
    if constexpr (kTerm) {
      const catppo_servo_terminations& tm = ext_of<catppo_servo_terminations>(ext...);
      // the fired terms as a float (exact: fewer than 16 bits); lane k counts term k over the steps that end an episode,
      // lane 15 those steps
      if (lane == 12) row[tm.off_term_state] = (float)TR.fired;
      if (e0 + grp < d.N && ends)
        tm.rec[e * CATPPO_SERVO_TERM_FLOATS + lane] = TR.rec0 + (lane == 15 || ((TR.fired >> lane) & 1u) ? 1.f : 0.f);
    }
    // the history moves one slot back: p | old slot 0 | old slot 1; float 12 of slot 0 says that a step wrote the row
    if constexpr (kActu) {
      float* hout = row + ext_of<catppo_servo_actuators>(ext...).off_act_hist;
      hout[lane] = isj ? act_p : lane == 12 ? 1.f : 0.f;
      hout[16 + lane] = isj ? UR.h0 : 0.f;
      hout[32 + lane] = isj ? UR.h1 : 0.f;
    }
    if (lane == 14) {
      for (int k = 0; k < 3; ++k) row[d.off_servo + k] = v[k];
      row[d.off_servo + 3] = roll;
      row[d.off_servo + 4] = pitch;
      row[d.off_servo + 13] = (float)ep_out;
    }
    if (lane == 15) {
      float head[9] = {ang[0], ang[1], ang[2], grav[0], grav[1], grav[2], cmd[0], cmd[1], cmd[2]};
      if (ends) {
        float cn[3];
        if constexpr (kCmd) {
          if (cmd_gen) first_command(d, CM, gid, ep_out, cn);
          else if constexpr (kMode != kTrain) command_of<kMode>(d, e, gid, ep_out, 0u, 0, cn);
        } else {
          command_of<kMode>(d, e, gid, ep_out, 0u, 0, cn);
        }
        head[0] = head[1] = head[2] = head[3] = head[4] = 0.f;
        head[5] = -1.f, head[6] = cn[0], head[7] = cn[1], head[8] = cn[2];
        if constexpr (kEv) {
          float nxy[2], nv[3];
          first_root(d, E, gid, ep_out, nxy, nv);
          head[2] = nv[2];
        }
      }
      for (int k = 0; k < 9; ++k)
        if (k < D) obs[k] = head[k];
    }
    // ---- evaluation record: every lane holds all twelve terms of this step, lane k adds term k to field k
    if (kEval && d.eval != nullptr) {
      const float torque2 = tree16(tau_w * tau_w);
      const float ret = __shfl(rec0, 9, 16) + reward;      // this episode's return so far (field 9 + this step)
      float term = 1.f, acc = rec0;
      switch (lane) {
        case 1: term = ends ? 1.f : 0.f; break;
        case 2: term = gone_of(TR, fallen) ? 1.f : 0.f; break;
        case 3: term = reward; break;
        case 4: term = ex * ex + ey * ey; break;
        case 5: term = ew * ew; break;
        case 6: term = tilt2; break;
        case 7: term = torque2; break;
        case 8: term = ncon; break;
        case 9: term = reward; break;
        case 10: term = ends ? ret : 0.f; break;
        case 11: term = ends ? (float)(t + 1) : 0.f; break;
        default: break;
      }
      acc = acc + term;
      if (lane == 9 && ends) acc = 0.f;
      if (rec) d.eval[rec_at] = acc;
    }
    // the force history moves one slot back (slot 0 is this step)
    if (!rst)
      for (int i = lane; i < (d.H - 1) * B3; i += 16) row[d.off_forces + B3 + i] = in[d.off_forces + i];
  }
  __syncthreads();

  // ---- policy observation: float j = scale((clip(noise(bias(raw[src_j]))))) in IsaacLab's ObservationManager order.  Lane l
  // of the env's group produces floats 4 l .. 4 l + 3 from one Philox block and writes one float4; the floats past `width`
  // of the padded field stay the zeros the row was filled with
  if constexpr (kObs) {
    const catppo_servo_obs& o = ext_of<catppo_servo_obs>(ext...);
    if (4 * lane < o.width) {
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      catppo_servo_obs_entry en[4];
      uint32_t noisy = 0u;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int j = 4 * lane + w;
        en[w] = o.table[j < o.width ? j : o.width - 1];
        noisy |= en[w].flags & 2u;
      }
      rng::u32x4 r = {0u, 0u, 0u, 0u};
      if (noisy)
        r = rng::philox4x32_10(rng::u32x4{gid, obs_ep, (obs_t << 4) | (uint32_t)lane, kTagObs}, (uint32_t)d.seed,
                               (uint32_t)(d.seed >> 32));
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const catppo_servo_obs_entry& E = en[w];
        const int src = E.src < 0 ? 0 : E.src < kRawObs ? E.src : kRawObs - 1;
        float v = obs[src];
        if (E.flags & 1u) v = v + E.bias;
        if (E.flags & 2u) v = (v + pick(r, w) * E.noise_width) + E.noise_lo;
        if (E.flags & 4u) {
          v = v < E.clip_lo ? E.clip_lo : v;
          v = v > E.clip_hi ? E.clip_hi : v;
        }
        v = v * E.scale;
        if (4 * lane + w < o.width) x[w] = v;
      }
      *reinterpret_cast<float4*>(row + o.off_policy_obs + 4 * lane) = float4{x[0], x[1], x[2], x[3]};
    }
    __syncthreads();
  }

  // ---- observation history: float i of the field is the current frame's float cur(i) when the frame fills every slot or i
  // lies in its term's newest slot, else the input row's float one slot later; registers to memory, neighbouring lanes write
  // neighbouring floats, the spare lane groups past N write nothing.  cur and i + w are clamped: the launch stays in its row
  if constexpr (kHist) {
    const catppo_servo_history& hs = ext_of<catppo_servo_history>(ext...);
    const catppo_servo_obs& o = ext_of<catppo_servo_obs>(ext...);
    if (e0 + grp < d.N) {
      const float* hin = in + hs.off_hist;
      const float* frame = row + o.off_policy_obs;
      float* hout = d.state_out + e * d.row_stride + hs.off_hist;
      const int T = hs.floats, T4 = (T + 3) / 4 * 4;
      for (int i = lane; i < T4; i += 16) {
        float v = 0.f;                                   // the floats past T of the padded field
        if (i < T) {
          const uint32_t m = hs.map[i];
          int c = (int)(m & 0xFFu), nx = i + (int)((m >> 8) & 0xFFu);
          c = c < o.width ? c : o.width - 1;
          nx = nx < T ? nx : T - 1;
          if (hist_fill || (m & CATPPO_SERVO_HISTORY_NEWEST)) v = frame[c];
          else v = hin[nx];
        }
        hout[i] = v;
      }
    }
  }

  const int F4 = F >> 2;
  const int64_t stride4 = d.row_stride >> 2;
  float4* out4 = reinterpret_cast<float4*>(d.state_out);
  for (int idx = tid; idx < kEnvsPerBlock * F4; idx += kThreads) {
    const int r = idx / F4, c = idx - r * F4;
    if (e0 + r < d.N) out4[(e0 + r) * stride4 + c] = lds4[idx];
  }
}

// the launch: the pack of extensions decides the kernel's signature, (mode, rewards) the instance among its six
template <typename... Ext>
void launch(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream, const catppo_servo_sim& d, const Ext&... ext) {
  using Kernel = void (*)(const catppo_servo_sim, const Ext...);
  // packs with terminations fold the evaluation instances into the step-response ones (which take a NULL trace and a plain
  // command table through two wave-uniform branches and compute the same bits): a third fewer instances to compile
  // (packs with an action table likewise)
  constexpr int kEvalAs = ((std::is_same_v<Ext, catppo_servo_terminations> || std::is_same_v<Ext, catppo_servo_actions> ||
                            std::is_same_v<Ext, catppo_servo_actuators> || std::is_same_v<Ext, catppo_servo_randomize> ||
                            std::is_same_v<Ext, catppo_servo_history> || std::is_same_v<Ext, ServoEventsExt>) || ...)
                              ? kStepResponse : kEvaluate;
  // a plant table is an evaluation input (the entry point has checked that an evaluation pointer is set): its packs have the
  // step-response instances only
  if constexpr ((std::is_same_v<Ext, catppo_servo_plant> || ...)) {
    const Kernel pinned[2] = {servo_sim_kernel<kStepResponse, false, Ext...>, servo_sim_kernel<kStepResponse, true, Ext...>};
    hipLaunchKernelGGL(pinned[rew ? 1 : 0], dim3(nblk), dim3(kThreads), lds_bytes, stream, d, ext...);
  } else {
    const Kernel table[3][2] = {{servo_sim_kernel<kTrain, false, Ext...>, servo_sim_kernel<kTrain, true, Ext...>},
                                {servo_sim_kernel<kEvalAs, false, Ext...>, servo_sim_kernel<kEvalAs, true, Ext...>},
                                {servo_sim_kernel<kStepResponse, false, Ext...>, servo_sim_kernel<kStepResponse, true, Ext...>}};
    hipLaunchKernelGGL(table[mode][rew ? 1 : 0], dim3(nblk), dim3(kThreads), lds_bytes, stream, d, ext...);
  }
}

}  // namespace

// the launches of the five other units (servo_sim.hip lists them): of a pack that ends with the descriptors the unit is named
// after, and holds whichever of the optional ones before them are present.  The entry point has checked everything
void catppo_internal_servo_sim_launch_actions(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                              const catppo_servo_sim& d, const ServoExts& x);
void catppo_internal_servo_sim_launch_actuators(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                                const catppo_servo_sim& d, const ServoExts& x);
void catppo_internal_servo_sim_launch_randomize(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                                const catppo_servo_sim& d, const ServoExts& x);
void catppo_internal_servo_sim_launch_history(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                              const catppo_servo_sim& d, const ServoExts& x);
void catppo_internal_servo_sim_launch_plant(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                            const catppo_servo_sim& d, const ServoExts& x);
// ... and of every pack whose event block is the extended one (x.ev->floats == CATPPO_SERVO_EVENT_FLOATS_EXT): without a
// randomisation descriptor, and with one
void catppo_internal_servo_sim_launch_disturb(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                              const catppo_servo_sim& d, const ServoExts& x);
void catppo_internal_servo_sim_launch_disturb_robot(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t stream,
                                                    const catppo_servo_sim& d, const ServoExts& x);
