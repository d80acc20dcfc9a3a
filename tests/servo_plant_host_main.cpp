// The program of tests/test_servo_plant_host.py: the plant level of csrc/servo_sim_host.h on its own, without HIP and without a
// device ("Robustness").  The addresses are made up and never dereferenced.  Prints one line per expectation
// that does not hold, then "checks N bad M".
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
constexpr int kCommandTable = 1, kRecord = 2, kTrace = 4;              // the evaluation pointers that are set

template <typename P>
void point(P& field, uintptr_t at) { field = reinterpret_cast<P>(at); }
uintptr_t at(const void* p) { return reinterpret_cast<uintptr_t>(p); }

const char* verdict(const catppo_servo_sim_plant& h, ServoExts* exts = nullptr) {
  ServoExts x;
  const char* why = servo_exts_of(&h.sim, x);
  if (!why) why = servo_sim_check(h.sim, x);
  if (exts) *exts = x;
  return why;
}

struct Buffer { const char* name; size_t field; uintptr_t bytes, base; };

struct Desc {
  catppo_servo_sim_plant h;
  std::vector<Buffer> buffers;
  void set(const Buffer& b, uintptr_t to) { memcpy(reinterpret_cast<char*>(&h) + b.field, &to, sizeof(to)); }
};

// the descriptor of the plant level with the optional blocks of `mask` and, with `hist`, the history present, laid out as
// Solo12ServoSim lays it out; `eval`: which evaluation pointers are set (a trace needs the record)
Desc make(int mask, bool hist, int eval = kRecord, bool rewards = false) {
  Desc D;
  memset(&D.h, 0, sizeof(D.h));
  catppo_servo_sim& d = D.h.sim;
  const bool obs = mask & kObs, ev = mask & kEv, cm = mask & kCm, tm = mask & kTm;
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
  D.h.actu.off_act_hist = field(CATPPO_SERVO_ACT_HIST_FLOATS);
  d.row_floats = o;
  if (hist) D.h.hist.off_hist = field((kHistFloats + 3) / 4 * 4), D.h.hist.floats = kHistFloats;
  d.row_stride = o;
  if (ev) D.h.ev.floats = CATPPO_SERVO_EVENT_FLOATS;
  D.h.act.width = 8;
  d.N = kN, d.H = kH, d.B = kB, d.obs_dim = kObsDim, d.reserved = CATPPO_SERVO_EXT_PLANT;
  d.max_episode_length = 1000, d.decimation = 4, d.resample_steps = 100, d.seed = 7;
  d.dt = 0.005f, d.inertia = 0.01f, d.reward_scale = 1.f;
  if (eval & kTrace) d.trace_envs = 4, d.trace_capacity = 6;
  if (rewards) d.reward_terms = 5;

  uintptr_t next = 0x10000000;
  const auto buffer = [&](bool there, const char* name, size_t fld, uintptr_t bytes) {
    if (!there) return;
    D.buffers.push_back({name, fld, bytes, next});
    D.set(D.buffers.back(), next);
    next += (bytes + 255) / 256 * 256 + 256;                           // 256-byte aligned, a gap behind each
  };
#define FIELD(path) offsetof(catppo_servo_sim_plant, path)
  const uintptr_t n = kN;
  buffer(true, "state_in", FIELD(sim.state_in), n * d.row_stride * 4);
  buffer(true, "state_out", FIELD(sim.state_out), n * d.row_stride * 4);
  buffer(true, "action", FIELD(sim.action), n * 4 * 8);
  buffer(true, "reset", FIELD(sim.reset), n);
  buffer(true, "episode_length", FIELD(sim.episode_length), n * 8);
  buffer(eval & kCommandTable, "fixed_command", FIELD(sim.fixed_command), n * 12);
  buffer(eval & (kRecord | kTrace), "eval", FIELD(sim.eval), n * 12 * 4);
  buffer(eval & kTrace, "trace", FIELD(sim.trace), 6 * 4 * 72 * 4);
  buffer(rewards, "reward_rec", FIELD(sim.reward_rec), n * 32 * 4);
  buffer(rewards, "reward_table", FIELD(sim.reward_table), 15 * 16);
  buffer(obs, "obs.table", FIELD(obs.table), kPolicy * 32);
  buffer(ev, "ev.block", FIELD(ev.block), 32 * 4);
  buffer(cm, "cmd.block", FIELD(cmd.block), 16 * 4);
  buffer(tm, "term.table", FIELD(term.table), 15 * 16);
  buffer(tm, "term.rec", FIELD(term.rec), n * 16 * 4);
  buffer(true, "act.table", FIELD(act.table), 12 * 32);
  buffer(true, "actu.table", FIELD(actu.table), 12 * 32);
  buffer(true, "rnd.block", FIELD(rnd.block), 32 * 4);
  buffer(hist, "hist.map", FIELD(hist.map), kHistFloats * 4);
  buffer(true, "plant.table", FIELD(plant.table), n * 8 * 4);           // the issue's extent: N rows of 8 fp32 words
#undef FIELD
  return D;
}

#define ACCEPTED(D) EXPECT(verdict((D).h) == nullptr)
#define REFUSED(D, edit)             \
  do {                               \
    Desc m = D;                      \
    catppo_servo_sim_plant& h = m.h; \
    edit;                            \
    EXPECT(verdict(h) != nullptr);   \
  } while (0)

// ------------------------------------------------------------------------------------------ accepted
void well_formed() {
  int made = 0;
  for (int hist = 0; hist < 2; ++hist)
    for (int mask = 0; mask <= kAllOptional; ++mask) {
      if (hist && !(mask & kObs)) continue;                            // a history needs its observations
      for (int eval : {kCommandTable, kRecord, kRecord | kTrace, kCommandTable | kRecord | kTrace})
        for (int rewards = 0; rewards < 2; ++rewards) {
          const Desc D = make(mask, hist != 0, eval, rewards != 0);
          ServoExts x;
          const char* why = verdict(D.h, &x);
          EXPECT(why == nullptr);
          if (why) printf("  hist %d mask %d eval %d: %s\n", hist, mask, eval, why);
          EXPECT(x.obs == (mask & kObs ? &D.h.obs : nullptr) && x.ev == (mask & kEv ? &D.h.ev : nullptr));
          EXPECT(x.cm == (mask & kCm ? &D.h.cmd : nullptr) && x.tm == (mask & kTm ? &D.h.term : nullptr));
          EXPECT(x.ac == &D.h.act && x.au == &D.h.actu && x.rn == &D.h.rnd && x.pl == &D.h.plant);
          EXPECT(x.hs == (hist ? &D.h.hist : nullptr));
        }
      ++made;
    }
  EXPECT(made == 16 + 8);
  EXPECT(sizeof(catppo_servo_plant) == 16 && offsetof(catppo_servo_sim_plant, plant) == sizeof(catppo_servo_sim_history));
  EXPECT(sizeof(catppo_servo_sim_plant) == 520 && ServoExts().pl == nullptr);
  // an init launch of the level writes the slab it was given, like any other
  Desc first = make(kAllOptional, true);
  first.h.sim.init = 1, first.h.sim.state_out = const_cast<float*>(first.h.sim.state_in);
  ACCEPTED(first);
}

// ------------------------------------------------------------------------------------------ refused
void refusals() {
  for (int hist = 0; hist < 2; ++hist) {
    const Desc D = make(kAllOptional, hist != 0, kCommandTable | kRecord | kTrace, true);
    ACCEPTED(D);
    REFUSED(D, h.plant.table = nullptr);
    for (int by : {4, 8, 12}) REFUSED(D, point(h.plant.table, at(h.plant.table) + by));
    REFUSED(D, h.plant.reserved[0] = 1);
    REFUSED(D, h.plant.reserved[1] = 1);
    REFUSED(D, h.plant.reserved[1] = -1);
    // act, actu and rnd are never absent; the randomisation descriptor's reserved words stay zero
    REFUSED(D, memset(&h.act, 0, sizeof(h.act)));
    REFUSED(D, memset(&h.actu, 0, sizeof(h.actu)));
    REFUSED(D, memset(&h.rnd, 0, sizeof(h.rnd)));
    REFUSED(D, h.rnd.reserved[0] = 1);
    REFUSED(D, h.rnd.reserved[1] = CATPPO_SERVO_EXT_PLANT);
  }
  // a plant table is an evaluation input: some evaluation pointer is set
  for (int hist = 0; hist < 2; ++hist) {
    for (int eval : {kCommandTable, kRecord}) {
      const Desc D = make(kAllOptional, hist != 0, eval);
      ACCEPTED(D);
      REFUSED(D, h.sim.fixed_command = nullptr; h.sim.eval = nullptr);
    }
    Desc train = make(kAllOptional, hist != 0, 0);
    EXPECT(verdict(train.h) != nullptr);
    train.h.sim.init = 1, train.h.sim.state_out = const_cast<float*>(train.h.sim.state_in);
    EXPECT(verdict(train.h) != nullptr);                               // ... on an init launch, too
  }
  // a history that is present needs its observations and a map; an empty one is absent
  {
    const Desc D = make(kAllOptional, true);
    REFUSED(D, h.obs.table = nullptr; h.obs.width = 0);
    REFUSED(D, h.hist.map = nullptr);
    REFUSED(D, h.hist.floats = 0);
    for (int floats : {-4, 513, kHistFloats + 4}) REFUSED(D, h.hist.floats = floats);
    Desc gone = D;                                                     // the stride keeps the room, nobody writes it
    memset(&gone.h.hist, 0, sizeof(gone.h.hist));
    ServoExts x;
    EXPECT(verdict(gone.h, &x) == nullptr && x.hs == nullptr && x.obs == &gone.h.obs && x.pl == &gone.h.plant);
    Desc bare = make(0, false);                                        // no history: the observations may be absent, too
    EXPECT(verdict(bare.h, &x) == nullptr && x.hs == nullptr && x.obs == nullptr);
  }
}

// ------------------------------------------------------------------------------------------ aliasing
void aliasing() {
  for (int hist = 0; hist < 2; ++hist) {
    const Desc full = make(kAllOptional, hist != 0, kCommandTable | kRecord | kTrace, true);
    ACCEPTED(full);
    EXPECT(full.buffers.size() == (hist ? 20u : 19u));
    const Buffer& table = full.buffers.back();
    EXPECT(strcmp(table.name, "plant.table") == 0);
    for (const Buffer& other : full.buffers) {
      if (&other == &table) continue;
      for (int way = 0; way < 2; ++way) {                              // the table on the other range, and the other way round
        const Buffer &mine = way ? other : table, &onto = way ? table : other;
        Desc m = full;
        m.set(mine, onto.base);                                        // 256-byte aligned: only the overlap is wrong
        const char* why = verdict(m.h);
        EXPECT(why != nullptr && strstr(why, "do not overlap") != nullptr && strstr(why, "plant.table") != nullptr);
        if (!why || !strstr(why, "do not overlap")) printf("  %s = %s: %s\n", mine.name, onto.name, why ? why : "accepted");
        m.set(mine, onto.base + (onto.bytes - 1) / 16 * 16);           // its last bytes, aligned
        EXPECT(verdict(m.h) != nullptr);
        m.set(mine, onto.base - 16);                                   // my own end on its first bytes
        if (mine.bytes > 16) EXPECT(verdict(m.h) != nullptr);
      }
    }
    // back to back behind the table is fine, 16 bytes into its last row is not: the extent is N rows of 32 bytes
    Desc m = full;
    const uintptr_t far = 0x20000000;
    m.set(table, far), m.set(full.buffers[0], far + kN * 32);
    ACCEPTED(m);
    m.set(full.buffers[0], far + kN * 32 - 16);
    EXPECT(verdict(m.h) != nullptr);
  }
}

// ------------------------------------------------------------------------------------------ older levels on the same bytes
void older_levels() {
  const int32_t older[] = {CATPPO_SERVO_EXT_HISTORY, CATPPO_SERVO_EXT_RANDOMIZE, CATPPO_SERVO_EXT_ACTUATORS, CATPPO_SERVO_EXT_ACTIONS,
                           CATPPO_SERVO_EXT_TERMINATIONS, CATPPO_SERVO_EXT_COMMANDS, CATPPO_SERVO_EXT_EVENTS, CATPPO_SERVO_EXT_OBS};
  const Desc D = make(kAllOptional, true, kRecord, true);
  ACCEPTED(D);
  for (int32_t magic : older) {
    Desc m = D;
    m.h.sim.reserved = magic;
    // what the plant descriptor holds is not read under an older value, nor is an evaluation pointer asked for
    m.h.plant.table = nullptr, m.h.plant.reserved[0] = 7, m.h.sim.eval = nullptr;
    ServoExts x;
    EXPECT(verdict(m.h, &x) == nullptr && x.pl == nullptr);
    EXPECT((x.hs != nullptr) == (magic == CATPPO_SERVO_EXT_HISTORY));
  }
  // under the history level an empty history descriptor is still refused, as before
  Desc hist = D;
  hist.h.sim.reserved = CATPPO_SERVO_EXT_HISTORY;
  memset(&hist.h.hist, 0, sizeof(hist.h.hist));
  EXPECT(verdict(hist.h) != nullptr);
  // without a history the same bytes run as the randomisation level
  Desc plain = make(kAllOptional, false);
  plain.h.sim.reserved = CATPPO_SERVO_EXT_RANDOMIZE;
  ACCEPTED(plain);
  Desc unknown = D;
  unknown.h.sim.reserved = CATPPO_SERVO_EXT_PLANT + 1;
  EXPECT(verdict(unknown.h) != nullptr);
}

// ------------------------------------------------------------------------------------------ the dispatch's order
template <int K>
struct Tag { int id = K; };

void dispatch() {
  // the plant unit's two calls: the optional descriptors that are present, then the unit's own, the plant last
  const Tag<1> obs;
  const Tag<2> ev;
  const Tag<3> cm;
  const Tag<4> tm;
  const Tag<9> pl;
  for (int mask = 0; mask < 16; ++mask) {
    std::vector<int> got, want;
    for (int k = 0; k < 4; ++k)
      if (mask >> k & 1) want.push_back(k + 1);
    want.push_back(9);
    int calls = 0;
    with_present([&](const auto&... present) { ++calls; (got.push_back(present.id), ...); got.push_back(pl.id); },
                 mask & 1 ? &obs : nullptr, mask & 2 ? &ev : nullptr, mask & 4 ? &cm : nullptr, mask & 8 ? &tm : nullptr);
    EXPECT(calls == 1 && got == want);
  }
}

}  // namespace

int main() {
  well_formed();
  refusals();
  aliasing();
  older_levels();
  dispatch();
  printf("checks %d bad %d\n", g_checks, g_bad);
  return g_bad != 0;
}
