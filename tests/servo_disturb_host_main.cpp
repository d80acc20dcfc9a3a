// The program of tests/test_servo_disturb_host.py: the extended event block and its timer field in csrc/servo_sim_host.h, without
// HIP and without a device ("Disturbances").  The addresses are made up and never dereferenced.  Prints one
// line per expectation that does not hold, then "checks N bad M".
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

constexpr int kN = 16, kH = 1, kB = 17, kObsDim = 45, kPolicy = 45;

uintptr_t at(const void* p) { return reinterpret_cast<uintptr_t>(p); }

const char* verdict(const catppo_servo_sim_actuators& h) {
  ServoExts x;
  const char* why = servo_exts_of(&h.sim, x);
  if (!why) why = servo_sim_check(h.sim, x);
  return why;
}

struct Buffer { const char* name; size_t field; uintptr_t bytes, base; };
struct Field { const char* name; int off, width; };

struct Desc {
  catppo_servo_sim_actuators h;
  std::vector<Buffer> buffers;
  std::vector<Field> fields, base;          // the other row fields of the extensions; the base fields
  int spare = 0;                            // a free 4-float slot of the row
  void set(const Buffer& b, uintptr_t to) { memcpy(reinterpret_cast<char*>(&h) + b.field, &to, sizeof(to)); }
};

// the descriptor of the actuator level with every optional block present and an event block of `floats` words; `timer`: the
// row has the ev_state field and the descriptor names it.  Laid out as Solo12ServoSim lays it out
Desc make(int floats, bool timer) {
  Desc D;
  memset(&D.h, 0, sizeof(D.h));
  catppo_servo_sim& d = D.h.sim;
  int o = 0;
  const auto field = [&](int width) { const int a = o; o += width; return a; };
  const auto base = [&](const char* name, int width) { const int a = field(width); D.base.push_back({name, a, width}); return a; };
  d.off_joint_pos = base("joint_pos", 12), d.off_joint_vel = base("joint_vel", 12), d.off_joint_acc = base("joint_acc", 12);
  d.off_applied_torque = base("applied_torque", 12), d.off_projected_gravity = base("projected_gravity", 3);
  d.off_root_pos = base("root_pos", 3), d.off_command = base("command", 3), d.off_last_air_time = base("last_air_time", kB);
  d.off_first_contact = base("first_contact", kB), d.off_forces = base("forces", kH * kB * 3), d.off_reward = base("reward", 1);
  d.off_hard_reset = base("hard_reset", 1), d.off_obs = base("obs", kObsDim), d.off_servo = base("servo", 14);
  o = (o + 3) / 4 * 4;
  D.h.obs.off_policy_obs = field((kPolicy + 3) / 4 * 4), D.h.obs.width = kPolicy;
  D.fields.push_back({"policy_obs", D.h.obs.off_policy_obs, (kPolicy + 3) / 4 * 4});
  D.h.cmd.off_cmd_state = field(4), D.h.cmd.floats = CATPPO_SERVO_COMMAND_FLOATS;
  D.fields.push_back({"cmd_state", D.h.cmd.off_cmd_state, 4});
  D.h.term.off_term_state = field(4), D.h.term.terms = 8;
  D.fields.push_back({"term_state", D.h.term.off_term_state, 4});
  D.h.actu.off_act_hist = field(CATPPO_SERVO_ACT_HIST_FLOATS);
  D.fields.push_back({"act_hist", D.h.actu.off_act_hist, CATPPO_SERVO_ACT_HIST_FLOATS});
  const int state = field(4);
  D.spare = field(4);
  d.row_floats = d.row_stride = o;
  D.h.ev.floats = floats, D.h.ev.reserved = timer ? state : 0;
  D.h.act.width = 12;
  d.N = kN, d.H = kH, d.B = kB, d.obs_dim = kObsDim, d.reserved = CATPPO_SERVO_EXT_ACTUATORS;
  d.max_episode_length = 1000, d.decimation = 4, d.resample_steps = 100, d.seed = 7;
  d.dt = 0.005f, d.inertia = 0.01f, d.reward_scale = 1.f;

  uintptr_t next = 0x10000000;
  const auto buffer = [&](const char* name, size_t fld, uintptr_t bytes) {
    D.buffers.push_back({name, fld, bytes, next});
    D.set(D.buffers.back(), next);
    next += (bytes + 255) / 256 * 256 + 256;                           // 256-byte aligned, a gap behind each
  };
#define FIELD(path) offsetof(catppo_servo_sim_actuators, path)
  const uintptr_t n = kN;
  buffer("state_in", FIELD(sim.state_in), n * d.row_stride * 4);
  buffer("state_out", FIELD(sim.state_out), n * d.row_stride * 4);
  buffer("action", FIELD(sim.action), n * 4 * 12);
  buffer("reset", FIELD(sim.reset), n);
  buffer("episode_length", FIELD(sim.episode_length), n * 8);
  buffer("eval", FIELD(sim.eval), n * 12 * 4);
  buffer("obs.table", FIELD(obs.table), kPolicy * 32);
  buffer("cmd.block", FIELD(cmd.block), 16 * 4);
  buffer("term.table", FIELD(term.table), 15 * 16);
  buffer("term.rec", FIELD(term.rec), n * 16 * 4);
  buffer("act.table", FIELD(act.table), 12 * 32);
  buffer("actu.table", FIELD(actu.table), 12 * 32);
  buffer("ev.block", FIELD(ev.block), (uintptr_t)(floats > 0 ? floats : 32) * 4);   // last: the one that is moved about
#undef FIELD
  return D;
}

#define ACCEPTED(D) EXPECT(verdict((D).h) == nullptr)
#define REFUSED(D, edit)                 \
  do {                                   \
    Desc m = D;                          \
    catppo_servo_sim_actuators& h = m.h; \
    edit;                                \
    EXPECT(verdict(h) != nullptr);       \
  } while (0)

void sizes_and_reserved() {
  EXPECT(CATPPO_SERVO_EVENT_FLOATS == 32 && CATPPO_SERVO_EVENT_FLOATS_EXT == 64 && sizeof(catppo_servo_events) == 16);
  EXPECT(CATPPO_SERVO_EVENT_PUSH_TIMED == 32u && CATPPO_SERVO_EVENT_WRENCH == 64u);
  const Desc plain = make(32, false), ext = make(64, false), timed = make(64, true);
  ACCEPTED(plain);
  ACCEPTED(ext);                                                       // 64 words without off_ev_state
  ACCEPTED(timed);                                                     // ... and with it
  const char* why = verdict(ext.h);
  if (why) printf("  64 words: %s\n", why);
  why = verdict(timed.h);
  if (why) printf("  64 words with a timer: %s\n", why);
  for (int floats : {0, 16, 31, 33, 48, 63, 65, 128, -32}) REFUSED(plain, h.ev.floats = floats);
  // a non-zero reserved under 32 words: the timer field of a well-formed row, and 1
  REFUSED(plain, h.ev.reserved = timed.h.ev.reserved);
  REFUSED(plain, h.ev.reserved = 1);
  REFUSED(ext, h.ev.reserved = 1);
  REFUSED(plain, h.ev.reserved = -4);
  REFUSED(ext, h.ev.reserved = -4);
  // the spare slot of the row serves as well; anything off a 16-byte boundary or past the row does not
  Desc moved = timed;
  moved.h.ev.reserved = timed.spare;
  ACCEPTED(moved);
  for (int by : {1, 2, 3}) REFUSED(timed, h.ev.reserved += by);
  REFUSED(timed, h.ev.reserved = h.sim.row_floats);
  REFUSED(timed, h.ev.reserved = h.sim.row_floats - 2);
  REFUSED(timed, h.ev.reserved = h.sim.row_floats + 4);
}

void field_overlaps() {
  const Desc timed = make(64, true);
  // on each other row field of the extensions: its first and its last four floats
  for (const Field& f : timed.fields) {
    REFUSED(timed, h.ev.reserved = f.off);
    REFUSED(timed, h.ev.reserved = f.off + f.width - 4);
  }
  EXPECT(timed.fields.size() == 4);
  // on each base field: the aligned slot that holds its first float
  for (const Field& f : timed.base) REFUSED(timed, h.ev.reserved = f.off / 4 * 4 == 0 ? 4 : f.off / 4 * 4);
  REFUSED(timed, h.ev.reserved = 8);                                   // inside joint_pos (offset 0 itself means "no field")
  EXPECT(timed.base.size() == 14);
}

void block_overlaps() {
  for (int floats : {32, 64}) {
    const Desc D = make(floats, floats == 64);
    const Buffer& blk = D.buffers.back();
    EXPECT(strcmp(blk.name, "ev.block") == 0 && blk.bytes == (uintptr_t)floats * 4);
    for (size_t i = 0; i + 1 < D.buffers.size(); ++i) {
      const Buffer& b = D.buffers[i];
      // the block's first word on the buffer's last 16 bytes, and its last 16 bytes on the buffer's first
      Desc m = D;
      m.set(blk, (b.base + b.bytes - 1) / 16 * 16);
      EXPECT(verdict(m.h) != nullptr);
      m.set(blk, b.base - blk.bytes + 16);
      EXPECT(verdict(m.h) != nullptr);
      // right behind the buffer and right in front of it: disjoint
      m.set(blk, (b.base + b.bytes + 15) / 16 * 16);
      EXPECT(verdict(m.h) == nullptr);
      m.set(blk, b.base - blk.bytes);
      EXPECT(verdict(m.h) == nullptr);
    }
  }
  // the extent is floats * 4: the second half of a 64-word block counts (a 32-word block at the same place is clear of the buffer)
  const Desc ext = make(64, false), plain = make(32, false);
  const Buffer& b = ext.buffers[0];
  Desc m = ext;
  m.set(ext.buffers.back(), b.base - 32 * 4);
  EXPECT(verdict(m.h) != nullptr);
  Desc p = plain;
  p.set(plain.buffers.back(), plain.buffers[0].base - 32 * 4);
  EXPECT(verdict(p.h) == nullptr);
  REFUSED(ext, h.ev.block = reinterpret_cast<const float*>(at(h.ev.block) + 4));      // misaligned
  REFUSED(ext, h.ev.block = nullptr);
}

}  // namespace

int main() {
  sizes_and_reserved();
  field_overlaps();
  block_overlaps();
  printf("checks %d bad %d\n", g_checks, g_bad);
  return g_bad == 0 ? 0 : 1;
}
