// The program of tests/test_servo_sim_host.py: csrc/servo_sim_host.h on its own, without HIP and without a device.  The
// addresses are made up and never dereferenced.  Prints one line per expectation that does not hold, then "checks N bad M".
#include <cstdio>
#include <cstring>
#include <vector>

#include "catppo.h"
#include "servo_sim_host.h"

namespace {

int g_checks = 0, g_bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    ++g_checks;                                                   \
    if (!(cond)) ++g_bad, printf("line %d: %s\n", __LINE__, #cond); \
  } while (0)

constexpr int kN = 16, kH = 1, kB = 17, kObsDim = 45, kPolicy = 45, kHistFloats = 135;
enum { kObs = 1, kEv = 2, kCm = 4, kTm = 8, kAllOptional = 15 };
const int32_t kMagic[9] = {0, CATPPO_SERVO_EXT_OBS, CATPPO_SERVO_EXT_EVENTS, CATPPO_SERVO_EXT_COMMANDS,
                           CATPPO_SERVO_EXT_TERMINATIONS, CATPPO_SERVO_EXT_ACTIONS, CATPPO_SERVO_EXT_ACTUATORS,
                           CATPPO_SERVO_EXT_RANDOMIZE, CATPPO_SERVO_EXT_HISTORY};

template <typename P>
void point(P& field, uintptr_t at) { field = reinterpret_cast<P>(at); }
uintptr_t at(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// what servo_sim_host.h makes of a descriptor: the condition that failed, or nullptr
const char* verdict(const catppo_servo_sim_history& h, ServoExts* exts = nullptr) {
  ServoExts x;
  const char* why = servo_exts_of(&h.sim, x);
  if (!why) why = servo_sim_check(h.sim, x);
  if (exts) *exts = x;
  return why;
}

// one buffer of the launch: the pointer's place in the descriptor, its extent (restated from the issue's table, not taken
// from the header) and where make() put it
struct Buffer { const char* name; size_t field; uintptr_t bytes, base; };

struct Desc {
  catppo_servo_sim_history h;
  std::vector<Buffer> buffers;
  void set(const Buffer& b, uintptr_t to) { memcpy(reinterpret_cast<char*>(&h) + b.field, &to, sizeof(to)); }
};

// the descriptor of level `level` (index of `reserved` in kMagic) with the optional blocks of `mask` present, laid out as
// Solo12ServoSim lays it out; `extras`: a command schedule, the evaluation record, a trace and reward terms, too
Desc make(int level, int mask, bool extras = false) {
  Desc D;
  memset(&D.h, 0, sizeof(D.h));
  catppo_servo_sim& d = D.h.sim;
  const bool obs = level >= 1 && (mask & kObs), ev = level >= 2 && (mask & kEv), cm = level >= 3 && (mask & kCm),
             tm = level >= 4 && (mask & kTm), ac = level >= 5, au = level >= 6, rn = level >= 7, hs = level >= 8;
  int o = 0;
  const auto field = [&](int width) { const int at = o; o += width; return at; };
  d.off_joint_pos = field(12), d.off_joint_vel = field(12), d.off_joint_acc = field(12), d.off_applied_torque = field(12);
  d.off_projected_gravity = field(3), d.off_root_pos = field(3), d.off_command = field(3);
  d.off_last_air_time = field(kB), d.off_first_contact = field(kB), d.off_forces = field(kH * kB * 3);
  d.off_reward = field(1), d.off_hard_reset = field(1), d.off_obs = field(kObsDim), d.off_servo = field(14);
  o = (o + 3) / 4 * 4;
  if (obs) D.h.obs.off_policy_obs = field((kPolicy + 3) / 4 * 4), D.h.obs.width = kPolicy;
  if (cm) D.h.cmd.off_cmd_state = field(4), D.h.cmd.floats = CATPPO_SERVO_COMMAND_FLOATS;
  if (tm) D.h.term.off_term_state = field(4), D.h.term.terms = 8;
  if (au) D.h.actu.off_act_hist = field(CATPPO_SERVO_ACT_HIST_FLOATS);
  d.row_floats = o;
  if (hs) D.h.hist.off_hist = field((kHistFloats + 3) / 4 * 4), D.h.hist.floats = kHistFloats;
  d.row_stride = o;
  if (ev) D.h.ev.floats = CATPPO_SERVO_EVENT_FLOATS;
  if (ac) D.h.act.width = 8;
  d.N = kN, d.H = kH, d.B = kB, d.obs_dim = kObsDim, d.reserved = kMagic[level];
  d.max_episode_length = 1000, d.decimation = 4, d.resample_steps = 100, d.seed = 7;
  d.dt = 0.005f, d.inertia = 0.01f, d.reward_scale = 1.f;
  if (extras) d.fixed_segments = 3, d.fixed_segment_steps = 50, d.trace_envs = 4, d.trace_capacity = 6, d.reward_terms = 5;

  uintptr_t next = 0x10000000;
  const auto buffer = [&](bool there, const char* name, size_t fld, uintptr_t bytes) {
    if (!there) return;
    D.buffers.push_back({name, fld, bytes, next});
    D.set(D.buffers.back(), next);
    next += (bytes + 255) / 256 * 256 + 256;                           // 256-byte aligned, a gap behind each
  };
#define FIELD(path) offsetof(catppo_servo_sim_history, path)
  const uintptr_t n = kN;
  buffer(true, "state_in", FIELD(sim.state_in), n * d.row_stride * 4);
  buffer(true, "state_out", FIELD(sim.state_out), n * d.row_stride * 4);
  buffer(true, "action", FIELD(sim.action), n * 4 * (ac ? 8 : 12));
  buffer(true, "reset", FIELD(sim.reset), n);
  buffer(true, "episode_length", FIELD(sim.episode_length), n * 8);
  buffer(extras, "fixed_command", FIELD(sim.fixed_command), 3 * n * 12);
  buffer(extras, "eval", FIELD(sim.eval), n * 12 * 4);
  buffer(extras, "trace", FIELD(sim.trace), 6 * 4 * 72 * 4);
  buffer(extras, "reward_rec", FIELD(sim.reward_rec), n * 32 * 4);
  buffer(extras, "reward_table", FIELD(sim.reward_table), 15 * 16);
  buffer(obs, "obs.table", FIELD(obs.table), kPolicy * 32);
  buffer(ev, "ev.block", FIELD(ev.block), 32 * 4);
  buffer(cm, "cmd.block", FIELD(cmd.block), 16 * 4);
  buffer(tm, "term.table", FIELD(term.table), 15 * 16);
  buffer(tm, "term.rec", FIELD(term.rec), n * 16 * 4);
  buffer(ac, "act.table", FIELD(act.table), 12 * 32);
  buffer(au, "actu.table", FIELD(actu.table), 12 * 32);
  buffer(rn, "rnd.block", FIELD(rnd.block), 32 * 4);
  buffer(hs, "hist.map", FIELD(hist.map), kHistFloats * 4);
#undef FIELD
  return D;
}

#define ACCEPTED(D) EXPECT(verdict((D).h) == nullptr)
// the descriptor D with one edit is refused; D stays what it is
#define REFUSED(D, edit)             \
  do {                               \
    Desc m = D;                      \
    catppo_servo_sim_history& h = m.h; \
    edit;                            \
    EXPECT(verdict(h) != nullptr);   \
  } while (0)

// ------------------------------------------------------------------------------------------ well-formed descriptors
void well_formed() {
  int made = 0;
  for (int level = 0; level <= 8; ++level)
    for (int mask = 0; mask <= kAllOptional; ++mask) {
      // a block is optional from the level behind its own on; below its own level it does not exist; a history needs obs
      const int own[4] = {1, 2, 3, 4};
      bool allowed = true;
      for (int b = 0; b < 4; ++b) {
        const bool on = mask >> b & 1;
        if (level < own[b] && on) allowed = false;                     // counted once, as the mask without the bit
        if (level == own[b] && !on) allowed = false;                   // the announced level's own block is there
      }
      if (level == 8 && !(mask & kObs)) allowed = false;
      if (!allowed) continue;
      for (int extras = 0; extras < 2; ++extras) {
        const Desc D = make(level, mask, extras != 0);
        ServoExts x;
        const char* why = verdict(D.h, &x);
        EXPECT(why == nullptr);
        if (why) printf("  level %d mask %d: %s\n", level, mask, why);
        EXPECT(x.obs == (mask & kObs ? &D.h.obs : nullptr) && x.ev == (mask & kEv ? &D.h.ev : nullptr));
        EXPECT(x.cm == (mask & kCm ? &D.h.cmd : nullptr) && x.tm == (mask & kTm ? &D.h.term : nullptr));
        EXPECT(x.ac == (level >= 5 ? &D.h.act : nullptr) && x.au == (level >= 6 ? &D.h.actu : nullptr));
        EXPECT(x.rn == (level >= 7 ? &D.h.rnd : nullptr) && x.hs == (level >= 8 ? &D.h.hist : nullptr));
      }
      ++made;
    }
  EXPECT(made == 1 + 1 + 2 + 4 + 8 + 16 + 16 + 16 + 8);
  // "empty means absent" holds from the level behind a block's own on: the announced level's own block is never absent, nor are
  // the action, actuator and randomisation descriptors at any level, nor the observations under a history
  for (int level = 1; level <= 8; ++level) {
    const Desc D = make(level, kAllOptional);
    if (level == 1 || level == 8) REFUSED(D, memset(&h.obs, 0, sizeof(h.obs)));
    if (level == 2) REFUSED(D, memset(&h.ev, 0, sizeof(h.ev)));
    if (level == 3) REFUSED(D, memset(&h.cmd, 0, sizeof(h.cmd)));
    if (level == 4) REFUSED(D, memset(&h.term, 0, sizeof(h.term)));
    if (level >= 5) REFUSED(D, memset(&h.act, 0, sizeof(h.act)));
    if (level >= 6) REFUSED(D, memset(&h.actu, 0, sizeof(h.actu)));
    if (level >= 7) REFUSED(D, memset(&h.rnd, 0, sizeof(h.rnd)));
    if (level == 8) REFUSED(D, memset(&h.hist, 0, sizeof(h.hist)));
  }
  const Desc full = make(8, kAllOptional, true);
  EXPECT(full.h.sim.row_floats == 308 && full.h.sim.row_stride == 444 && full.h.obs.off_policy_obs == 204);
  EXPECT(full.h.cmd.off_cmd_state == 252 && full.h.term.off_term_state == 256 && full.h.actu.off_act_hist == 260);
  EXPECT(full.buffers.size() == 19);
}

// ------------------------------------------------------------------------------------------ aliasing
void aliasing() {
  const Desc full = make(8, kAllOptional, true);
  ACCEPTED(full);
  for (const Buffer& mine : full.buffers)
    for (const Buffer& other : full.buffers) {
      if (&mine == &other) continue;
      Desc m = full;
      m.set(mine, other.base);                                         // 256-byte aligned: only the overlap is wrong
      const char* why = verdict(m.h);
      EXPECT(why != nullptr && strstr(why, "do not overlap") != nullptr);
      if (!why || !strstr(why, "do not overlap")) printf("  %s = %s: %s\n", mine.name, other.name, why ? why : "accepted");
      m.set(mine, other.base + other.bytes - 1);                       // its last byte (the alignment rule may refuse it first)
      EXPECT(verdict(m.h) != nullptr);
      m.set(mine, other.base + (other.bytes - 1) / 16 * 16);           // its last bytes, aligned
      EXPECT(verdict(m.h) != nullptr);
      m.set(mine, other.base - 16);                                    // my own end on its first bytes
      if (mine.bytes > 16) EXPECT(verdict(m.h) != nullptr);
    }
  // back to back is fine, one 16 bytes into the other is not
  for (size_t i = 0; i + 1 < full.buffers.size(); ++i) {
    const Buffer &mine = full.buffers[i], &other = full.buffers[i + 1];
    const uintptr_t far = 0x20000000, behind = far + (mine.bytes + 15) / 16 * 16;
    Desc m = full;
    m.set(mine, far), m.set(other, behind);
    ACCEPTED(m);
    m.set(other, behind - 16);
    EXPECT(verdict(m.h) != nullptr);
  }
  Desc first = full;
  first.h.sim.init = 1, first.h.sim.state_out = const_cast<float*>(first.h.sim.state_in);
  ACCEPTED(first);                                                     // an init launch writes the slab it was given
  REFUSED(first, h.sim.init = 0);
  REFUSED(first, point(h.sim.state_out, at(h.sim.state_in) + 16));     // partly on it is not the exception
  for (const Buffer& other : full.buffers)                             // ... nor is anything else on an init launch
    if (other.field != offsetof(catppo_servo_sim_history, sim.state_in) && other.field != offsetof(catppo_servo_sim_history, sim.state_out))
      REFUSED(first, point(h.sim.state_out, other.base));
}

// ------------------------------------------------------------------------------------------ row fields
void row_fields() {
  const Desc full = make(8, kAllOptional, true);
  const catppo_servo_sim& d = full.h.sim;
  const int32_t base[14] = {d.off_joint_pos, d.off_joint_vel, d.off_joint_acc, d.off_applied_torque, d.off_projected_gravity,
                            d.off_root_pos, d.off_command, d.off_last_air_time, d.off_first_contact, d.off_forces, d.off_reward,
                            d.off_hard_reset, d.off_obs, d.off_servo};
  struct Ext { size_t field; int width; bool state; };
  const Ext ext[4] = {{offsetof(catppo_servo_sim_history, obs.off_policy_obs), 48, false},
                      {offsetof(catppo_servo_sim_history, cmd.off_cmd_state), 4, true},
                      {offsetof(catppo_servo_sim_history, term.off_term_state), 4, true},
                      {offsetof(catppo_servo_sim_history, actu.off_act_hist), 48, true}};
  const auto off = [](Desc& m, const Ext& e) -> int32_t& { return *reinterpret_cast<int32_t*>(reinterpret_cast<char*>(&m.h) + e.field); };
  for (const Ext& e : ext) {
    Desc m = full;
    const int32_t good = off(m, e);
    for (int32_t b : base) {
      off(m, e) = b / 4 * 4;                                           // aligned, inside the row, on the base field
      if (e.state) EXPECT(verdict(m.h) != nullptr);
    }
    // the policy observation is held clear of the raw observation alone: on joint_pos it passes, as it always has
    if (!e.state) {
      off(m, e) = 0;
      ACCEPTED(m);
      off(m, e) = d.off_obs / 4 * 4;
      EXPECT(verdict(m.h) != nullptr);
      off(m, e) = (d.off_obs + 40) / 4 * 4;
      EXPECT(verdict(m.h) != nullptr);
    }
    for (const Ext& other : ext) {
      if (&other == &e) continue;
      off(m, e) = off(m, other);
      EXPECT(verdict(m.h) != nullptr);
      off(m, e) = off(m, other) + other.width - 4;                     // on its last four floats
      EXPECT(verdict(m.h) != nullptr);
    }
    off(m, e) = good + 2;
    EXPECT(verdict(m.h) != nullptr);
    Desc roomy = full;                                                 // 56 free floats at the end of the row: there the
    roomy.h.sim.row_floats += 56, roomy.h.sim.row_stride += 56, roomy.h.hist.off_hist += 56;   // alignment alone decides
    roomy.set(roomy.buffers[1], 0x20000000);                           // (the longer slabs: the second one out of the way)
    off(roomy, e) = d.row_floats;
    ACCEPTED(roomy);
    off(roomy, e) = d.row_floats + 2;
    EXPECT(verdict(roomy.h) != nullptr);
    off(m, e) = d.row_floats - e.width + 4;
    EXPECT(verdict(m.h) != nullptr);
    off(m, e) = -4;
    EXPECT(verdict(m.h) != nullptr);
    off(m, e) = good;
    ACCEPTED(m);
  }
  REFUSED(full, h.hist.off_hist = d.row_floats - 4);                   // inside the part that is staged in LDS
  REFUSED(full, h.hist.off_hist = d.row_floats + 2);
  REFUSED(full, h.hist.off_hist = d.row_floats + 4);                   // past the stride
  REFUSED(full, h.hist.off_hist = 0);
  REFUSED(full, h.hist.off_hist = -4);
  // the 14 base fields lie in the row and are not compared with each other
  REFUSED(full, h.sim.off_obs = d.row_floats - 3);
  REFUSED(full, h.sim.off_reward = -1);
  Desc shared = full;
  shared.h.sim.off_reward = shared.h.sim.off_hard_reset;
  ACCEPTED(shared);
}

// ------------------------------------------------------------------------------------------ the refusals of tests/test_gpu_servo_*.py
void gpu_suite_refusals() {
  {  // test_gpu_servo_sim, _eval, _trace, _reward: the base descriptor
    const Desc D = make(0, 0, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    REFUSED(D, h.sim.state_out = const_cast<float*>(h.sim.state_in));
    REFUSED(D, h.sim.off_obs = d.row_stride - 3);
    REFUSED(D, point(h.sim.eval, at(d.eval) + 4));
    REFUSED(D, h.sim.eval = h.sim.state_out);
    REFUSED(D, h.sim.fixed_command = h.sim.state_in);
    REFUSED(D, h.sim.fixed_segment_steps = 0);
    REFUSED(D, h.sim.fixed_segment_steps = -3);
    REFUSED(D, h.sim.fixed_command = nullptr);                         // a schedule without a table
    REFUSED(D, h.sim.fixed_segments = -1);
    REFUSED(D, h.sim.eval = nullptr);                                  // a trace without the record
    REFUSED(D, point(h.sim.trace, at(d.trace) + 4));
    REFUSED(D, h.sim.trace_envs = 0);
    REFUSED(D, h.sim.trace_envs = kN + 1);
    REFUSED(D, h.sim.trace_capacity = 0);
    REFUSED(D, h.sim.trace_capacity = -1);
    REFUSED(D, h.sim.trace = const_cast<float*>(h.sim.state_in));
    REFUSED(D, h.sim.trace = h.sim.state_out);
    REFUSED(D, h.sim.trace = h.sim.eval);
    REFUSED(D, h.sim.trace = const_cast<float*>(h.sim.fixed_command));
    Desc untraced = D;                                                 // without a trace its sizes are not read
    untraced.h.sim.trace = nullptr, untraced.h.sim.trace_envs = -5, untraced.h.sim.trace_capacity = -5;
    ACCEPTED(untraced);
    REFUSED(D, h.sim.reward_terms = 16);
    REFUSED(D, h.sim.reward_terms = -1);
    REFUSED(D, h.sim.reward_rec = nullptr);
    REFUSED(D, point(h.sim.reward_rec, at(d.reward_rec) + 4));
    REFUSED(D, h.sim.reward_rec = h.sim.state_out);
    REFUSED(D, h.sim.reward_rec = const_cast<float*>(h.sim.state_in));
    REFUSED(D, h.sim.reward_table = nullptr);
    REFUSED(D, point(h.sim.reward_table, at(d.reward_table) + 4));
    REFUSED(D, h.sim.reward_rec = h.sim.eval);
  }
  {  // test_gpu_servo_obs
    const Desc D = make(1, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    for (int width : {0, 65, -1}) REFUSED(D, h.obs.width = width);
    REFUSED(D, h.obs.off_policy_obs += 2);
    REFUSED(D, h.obs.off_policy_obs = -4);
    REFUSED(D, h.obs.off_policy_obs += 4);                             // the padded field leaves the row
    REFUSED(D, h.obs.off_policy_obs = d.off_obs / 4 * 4);
    REFUSED(D, h.obs.width = 4; h.obs.off_policy_obs = (d.off_obs + 40) / 4 * 4);
    REFUSED(D, h.obs.table = nullptr);
    REFUSED(D, point(h.obs.table, at(h.obs.table) + 4));
    REFUSED(D, point(h.obs.table, at(d.state_out)));
    REFUSED(D, point(h.obs.table, at(d.state_in)));
    REFUSED(D, point(h.obs.table, at(d.reward_table)));
    REFUSED(D, h.sim.reserved = 1);                                    // neither 0 nor an announcement
    REFUSED(D, h.sim.max_episode_length = int64_t(1) << 27);
    REFUSED(D, h.sim.obs_dim = 44);
  }
  {  // test_gpu_servo_events
    const Desc D = make(2, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    REFUSED(D, h.ev.block = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.ev.block, at(h.ev.block) + by));
    for (const void* p : {(const void*)d.state_in, (const void*)d.state_out, (const void*)d.eval, (const void*)d.reward_rec,
                          (const void*)d.reward_table, (const void*)D.h.obs.table})
      REFUSED(D, point(h.ev.block, at(p)));
    REFUSED(D, h.ev.floats = 16);
    REFUSED(D, h.ev.floats = 0);
    REFUSED(D, h.ev.reserved = 1);
    REFUSED(D, h.sim.max_episode_length = int64_t(1) << 27);
    REFUSED(D, h.sim.reserved = 2);
    REFUSED(D, h.obs.width = 0);                                       // width 0 goes with a NULL table only
  }
  {  // test_gpu_servo_commands
    const Desc D = make(3, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    REFUSED(D, h.cmd.block = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.cmd.block, at(h.cmd.block) + by));
    for (const void* p : {(const void*)d.state_in, (const void*)d.state_out, (const void*)d.eval, (const void*)d.reward_rec,
                          (const void*)d.reward_table, (const void*)D.h.obs.table, (const void*)D.h.ev.block})
      REFUSED(D, point(h.cmd.block, at(p)));
    for (int floats : {0, 15, 32}) REFUSED(D, h.cmd.floats = floats);
    const int cs = D.h.cmd.off_cmd_state;
    // negative, not a multiple of 4, past the row, on the policy field, on the raw observation, on servo, on joint_pos
    for (int off : {-4, cs + 1, cs + 2, cs + 4, 1000, cs - 4, (int)D.h.obs.off_policy_obs, d.off_obs / 4 * 4, d.off_servo / 4 * 4, 0})
      REFUSED(D, h.cmd.off_cmd_state = off);
    REFUSED(D, h.sim.max_episode_length = int64_t(1) << 27);
    REFUSED(D, h.ev.floats = 0);                                       // floats 0 goes with a NULL block only
  }
  {  // test_gpu_servo_terminations
    const Desc D = make(4, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, D.h.obs.table, D.h.ev.block, D.h.cmd.block};
    REFUSED(D, h.term.table = nullptr);
    REFUSED(D, h.term.rec = nullptr);
    for (int by : {4, 8}) {
      REFUSED(D, point(h.term.table, at(h.term.table) + by));
      REFUSED(D, point(h.term.rec, at(h.term.rec) + by));
    }
    REFUSED(D, point(h.term.table, at(h.term.rec)));
    REFUSED(D, point(h.term.rec, at(h.term.table)));
    for (const void* p : others) {
      REFUSED(D, point(h.term.table, at(p)));
      REFUSED(D, point(h.term.rec, at(p)));
    }
    for (int terms : {0, 16, -1}) REFUSED(D, h.term.terms = terms);
    const int ts = D.h.term.off_term_state;
    for (int off : {-4, ts + 1, ts + 2, ts + 4, 1000, (int)D.h.cmd.off_cmd_state, (int)D.h.obs.off_policy_obs, d.off_obs / 4 * 4,
                    d.off_servo / 4 * 4, 0})
      REFUSED(D, h.term.off_term_state = off);
  }
  {  // test_gpu_servo_actions
    const Desc D = make(5, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, D.h.obs.table, D.h.ev.block,
                            D.h.cmd.block, D.h.term.table, D.h.term.rec};
    REFUSED(D, h.act.table = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.act.table, at(h.act.table) + by));
    for (const void* p : others) REFUSED(D, point(h.act.table, at(p)));
    for (int width : {0, 13, -1}) REFUSED(D, h.act.width = width);
    REFUSED(D, h.act.reserved = 1);
    ACCEPTED(make(5, 0));                                              // actions and nothing before them
  }
  {  // test_gpu_servo_actuators
    const Desc D = make(6, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    const uintptr_t act = at(D.h.act.table);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, D.h.obs.table, D.h.ev.block,
                            D.h.cmd.block, D.h.term.table, D.h.term.rec, D.h.act.table, (const void*)(act + 32), (const void*)(act - 32)};
    REFUSED(D, h.actu.table = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.actu.table, at(h.actu.table) + by));
    for (const void* p : others) REFUSED(D, point(h.actu.table, at(p)));
    const int hist = D.h.actu.off_act_hist, F = d.row_floats;
    for (int off : {-4, hist + 2, hist + 4, F - 44, F, (int)d.off_joint_pos, d.off_obs - 44, (int)D.h.obs.off_policy_obs,
                    (int)D.h.cmd.off_cmd_state, D.h.term.off_term_state - 44})
      REFUSED(D, h.actu.off_act_hist = off);
    REFUSED(D, h.actu.reserved = 1);
    REFUSED(D, h.act.table = nullptr);                                 // under this value the action table is never absent
    Desc older = D;                                                    // every older value of `reserved` keeps its meaning
    older.h.sim.reserved = CATPPO_SERVO_EXT_ACTIONS;
    ACCEPTED(older);
  }
  {  // test_gpu_servo_randomize
    const Desc D = make(7, kAllOptional, true);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    const uintptr_t actu = at(D.h.actu.table);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.reward_rec, d.reward_table, d.action, D.h.obs.table, D.h.ev.block,
                            D.h.cmd.block, D.h.term.table, D.h.term.rec, D.h.act.table, D.h.actu.table, (const void*)(actu + 32),
                            (const void*)(actu - 64), (const void*)(at(D.h.ev.block) + 64), (const void*)(at(D.h.cmd.block) - 64)};
    REFUSED(D, h.rnd.block = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.rnd.block, at(h.rnd.block) + by));
    for (const void* p : others) REFUSED(D, point(h.rnd.block, at(p)));
    REFUSED(D, h.rnd.reserved[0] = 1);
    REFUSED(D, h.rnd.reserved[1] = 1);
    REFUSED(D, h.actu.table = nullptr);                                // under this value the actuator table is never absent
    Desc older = D;
    older.h.sim.reserved = CATPPO_SERVO_EXT_ACTUATORS;
    ACCEPTED(older);
  }
  {  // test_gpu_servo_history
    const Desc D = make(8, kObs | kTm, false);
    const catppo_servo_sim& d = D.h.sim;
    ACCEPTED(D);
    const uintptr_t in = at(d.state_in), out = at(d.state_out), obs = at(D.h.obs.table), rnd = at(D.h.rnd.block), act = at(D.h.act.table);
    const void* others[] = {d.state_in, d.state_out, (const void*)(in + 64), (const void*)(out + 4 * d.row_stride), d.action,
                            D.h.obs.table, (const void*)(obs + 32), D.h.term.table, D.h.term.rec, D.h.act.table, D.h.actu.table,
                            D.h.rnd.block, (const void*)(rnd + 64), (const void*)(act + 32)};
    REFUSED(D, h.hist.map = nullptr);
    for (int by : {4, 8}) REFUSED(D, point(h.hist.map, at(h.hist.map) + by));
    for (const void* p : others) REFUSED(D, point(h.hist.map, at(p)));
    for (int floats : {0, -4, 513, kHistFloats + 4}) REFUSED(D, h.hist.floats = floats);   // out of range, or past the stride
    REFUSED(D, h.obs.table = nullptr; h.obs.width = 0);                // under this value the observations are never absent
    Desc older = D;
    older.h.sim.reserved = CATPPO_SERVO_EXT_RANDOMIZE;
    ACCEPTED(older);
  }
}

// ------------------------------------------------------------------------------------------ with_present
template <int K>
struct Tag { int id = K; };

void dispatch() {
  const Tag<1> a;
  const Tag<2> b;
  const Tag<3> c;
  const Tag<4> e;
  for (int mask = 0; mask < 16; ++mask) {
    std::vector<int> got, want;
    for (int k = 0; k < 4; ++k)
      if (mask >> k & 1) want.push_back(k + 1);
    int calls = 0;
    with_present([&](const auto&... present) { ++calls; (got.push_back(present.id), ...); },
                 mask & 1 ? &a : nullptr, mask & 2 ? &b : nullptr, mask & 4 ? &c : nullptr, mask & 8 ? &e : nullptr);
    EXPECT(calls == 1 && got == want);
  }
}

}  // namespace

int main() {
  well_formed();
  aliasing();
  row_fields();
  gpu_suite_refusals();
  dispatch();
  printf("checks %d bad %d\n", g_checks, g_bad);
  return g_bad != 0;
}
