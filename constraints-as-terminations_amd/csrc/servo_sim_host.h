// The servo simulator's host side ("Host side of the launch"): which descriptors lie behind a catppo_servo_sim, whether
// the launch they describe is sound, and the call of a launch with exactly the descriptors that are present.  Plain C++17,
// nothing from HIP: tests/test_servo_sim_host.py compiles it with a host compiler and runs it without a device.
// Everything but ServoExts has internal linkage.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/catppo.h"

// ---------------------------------------------------------------------------------------------- a. the extension walk
// the descriptors behind the 368 bytes; null: absent.  Outside the unnamed namespace: the units pass it to each other
struct ServoExts {
  const catppo_servo_obs* obs = nullptr;
  const catppo_servo_events* ev = nullptr;
  const catppo_servo_commands* cm = nullptr;
  const catppo_servo_terminations* tm = nullptr;
  const catppo_servo_actions* ac = nullptr;
  const catppo_servo_actuators* au = nullptr;
  const catppo_servo_randomize* rn = nullptr;
  const catppo_servo_history* hs = nullptr;
  const catppo_servo_plant* pl = nullptr;
};

namespace {

constexpr int kEnvsPerBlock = 16, kJoints = 12, kPrivate = 14;
constexpr int kRawObs = 45;                                              // the raw observation a policy observation reads

// the level of `reserved` is its index here; it announces the descriptors of every level up to its own.
// catppo_servo_sim_plant is a superset of every shorter form (the static_asserts of servo_sim.hip)
enum { kLvNone, kLvObs, kLvEvents, kLvCommands, kLvTerminations, kLvActions, kLvActuators, kLvRandomize, kLvHistory, kLvPlant,
       kLevels };
constexpr struct { int32_t magic; size_t offset; } kServoExtTable[kLevels] = {
    {0, 0},
    {CATPPO_SERVO_EXT_OBS, offsetof(catppo_servo_sim_plant, obs)},
    {CATPPO_SERVO_EXT_EVENTS, offsetof(catppo_servo_sim_plant, ev)},
    {CATPPO_SERVO_EXT_COMMANDS, offsetof(catppo_servo_sim_plant, cmd)},
    {CATPPO_SERVO_EXT_TERMINATIONS, offsetof(catppo_servo_sim_plant, term)},
    {CATPPO_SERVO_EXT_ACTIONS, offsetof(catppo_servo_sim_plant, act)},
    {CATPPO_SERVO_EXT_ACTUATORS, offsetof(catppo_servo_sim_plant, actu)},
    {CATPPO_SERVO_EXT_RANDOMIZE, offsetof(catppo_servo_sim_plant, rnd)},
    {CATPPO_SERVO_EXT_HISTORY, offsetof(catppo_servo_sim_plant, hist)},
    {CATPPO_SERVO_EXT_PLANT, offsetof(catppo_servo_sim_plant, plant)}};

// fills `x` from what desc->reserved announces; returns nullptr, or the condition that failed
inline const char* servo_exts_of(const catppo_servo_sim* desc, ServoExts& x) {
  int level = -1;
  for (int i = 0; i < kLevels; ++i)
    if (desc->reserved == kServoExtTable[i].magic) level = i;
  if (level < 0) return "d.reserved is 0 or one of CATPPO_SERVO_EXT_*";
  const auto at = [&](int lv) -> const void* {
    return level >= lv ? reinterpret_cast<const char*>(desc) + kServoExtTable[lv].offset : nullptr;
  };
  x.obs = static_cast<const catppo_servo_obs*>(at(kLvObs));
  x.ev = static_cast<const catppo_servo_events*>(at(kLvEvents));
  x.cm = static_cast<const catppo_servo_commands*>(at(kLvCommands));
  x.tm = static_cast<const catppo_servo_terminations*>(at(kLvTerminations));
  x.ac = static_cast<const catppo_servo_actions*>(at(kLvActions));
  x.au = static_cast<const catppo_servo_actuators*>(at(kLvActuators));
  x.rn = static_cast<const catppo_servo_randomize*>(at(kLvRandomize));
  x.hs = static_cast<const catppo_servo_history*>(at(kLvHistory));
  x.pl = static_cast<const catppo_servo_plant*>(at(kLvPlant));
  // an empty descriptor below the announced level is an absent one; the action, actuator and randomisation descriptors are
  // never absent once announced, and a history needs its observations (servo_sim_check); the history descriptor itself may be
  // empty from the plant level on
  if (level >= kLvEvents && x.obs->width == 0 && x.obs->table == nullptr) x.obs = nullptr;
  if (level >= kLvCommands && x.ev->block == nullptr && x.ev->floats == 0) x.ev = nullptr;
  if (level >= kLvTerminations && x.cm->block == nullptr && x.cm->floats == 0) x.cm = nullptr;
  if (level >= kLvActions && x.tm->table == nullptr && x.tm->terms == 0) x.tm = nullptr;
  if (level >= kLvPlant && x.hs->map == nullptr && x.hs->floats == 0) x.hs = nullptr;
  return nullptr;
}

// ---------------------------------------------------------------------------------------------- b. the check
#define SERVO_REQUIRE(cond)      \
  do {                           \
    if (!(cond)) return #cond;   \
  } while (0)

// nullptr, or the first condition that failed.  What the device-resident tables and blocks hold is their writers' to check
// (Solo12ServoSim.set_*_table / set_*_block): the values are never addresses, and whatever they hold the launch stays
// inside its rows and records (the kernel clamps every index it takes from them)
inline const char* servo_sim_check(const catppo_servo_sim& d, const ServoExts& x) {
  const auto aligned16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };
  const auto pad4 = [](int64_t w) { return (w + 3) / 4 * 4; };
  SERVO_REQUIRE(d.N >= 1 && d.N < (int64_t(1) << 31) && d.env_offset >= 0 && d.env_offset + d.N < (int64_t(1) << 32));
  SERVO_REQUIRE(d.state_in && d.state_out && d.episode_length);
  SERVO_REQUIRE(d.init || (d.action && d.reset));
  SERVO_REQUIRE(d.row_floats >= 4 && d.row_floats % 4 == 0 && d.row_stride >= d.row_floats && d.row_stride % 4 == 0);
  SERVO_REQUIRE(aligned16(d.state_in) && aligned16(d.state_out));
  SERVO_REQUIRE((size_t)d.row_floats * kEnvsPerBlock * sizeof(float) <= 64 * 1024);
  SERVO_REQUIRE(d.H >= 1 && d.B == 17 && d.obs_dim >= 0);
  SERVO_REQUIRE(d.decimation >= 1 && d.resample_steps >= 1 && d.max_episode_length >= 1);
  SERVO_REQUIRE(d.inertia > 0.f && d.dt > 0.f && d.reward_scale > 0.f);
  SERVO_REQUIRE(aligned16(d.eval));
  SERVO_REQUIRE(d.fixed_segments >= 0);
  SERVO_REQUIRE(d.fixed_segments <= 1 || (d.fixed_segment_steps >= 1 && d.fixed_command != nullptr));
  if (d.trace) {
    SERVO_REQUIRE(d.eval != nullptr && aligned16(d.trace));
    SERVO_REQUIRE(d.trace_envs >= 1 && d.trace_envs <= d.N && d.trace_capacity >= 1);
  }
  SERVO_REQUIRE(d.reward_terms >= 0 && d.reward_terms <= CATPPO_SERVO_REWARD_MAX_TERMS);
  if (d.reward_terms > 0) {
    SERVO_REQUIRE(d.reward_rec != nullptr && aligned16(d.reward_rec));
    SERVO_REQUIRE(d.reward_table != nullptr && aligned16(d.reward_table));
  }
  // the step index is part of a Philox counter word of the observation noise, the events and the command process
  if (x.obs || x.ev || x.cm) SERVO_REQUIRE(d.max_episode_length < (int64_t(1) << 27));
  if (x.obs) {
    SERVO_REQUIRE(d.obs_dim == kRawObs);
    SERVO_REQUIRE(x.obs->width >= 1 && x.obs->width <= CATPPO_SERVO_OBS_MAX_WIDTH);
    SERVO_REQUIRE(x.obs->table != nullptr && aligned16(x.obs->table));
  }
  if (x.ev) {
    SERVO_REQUIRE(x.ev->floats == CATPPO_SERVO_EVENT_FLOATS || x.ev->floats == CATPPO_SERVO_EVENT_FLOATS_EXT);
    // reserved is off_ev_state: only an extended block keeps a timer in the row (the field itself: with the others below)
    SERVO_REQUIRE(x.ev->reserved == 0 || x.ev->floats == CATPPO_SERVO_EVENT_FLOATS_EXT);
    SERVO_REQUIRE(x.ev->block != nullptr && aligned16(x.ev->block));
  }
  if (x.cm) {
    SERVO_REQUIRE(x.cm->floats == CATPPO_SERVO_COMMAND_FLOATS);
    SERVO_REQUIRE(x.cm->block != nullptr && aligned16(x.cm->block));
  }
  if (x.tm) {
    SERVO_REQUIRE(x.tm->terms >= 1 && x.tm->terms <= CATPPO_SERVO_TERM_MAX_TERMS);
    SERVO_REQUIRE(x.tm->table != nullptr && aligned16(x.tm->table) && x.tm->rec != nullptr && aligned16(x.tm->rec));
  }
  if (x.ac) {
    SERVO_REQUIRE(x.ac->width >= 1 && x.ac->width <= kJoints && x.ac->reserved == 0);
    SERVO_REQUIRE(x.ac->table != nullptr && aligned16(x.ac->table));
  }
  if (x.au) {
    SERVO_REQUIRE(x.au->reserved == 0);
    SERVO_REQUIRE(x.au->table != nullptr && aligned16(x.au->table));
  }
  if (x.rn) {
    SERVO_REQUIRE(x.rn->reserved[0] == 0 && x.rn->reserved[1] == 0);
    SERVO_REQUIRE(x.rn->block != nullptr && aligned16(x.rn->block));
  }
  if (x.hs) {
    SERVO_REQUIRE(x.obs != nullptr);
    SERVO_REQUIRE(x.hs->floats >= 1 && x.hs->floats <= CATPPO_SERVO_OBS_HISTORY_MAX_FLOATS);
    SERVO_REQUIRE(x.hs->map != nullptr && aligned16(x.hs->map));
    // the field: pad4(T) floats of the row on a 16-byte boundary, behind the part that is staged in LDS, inside the stride
    const int64_t ho = x.hs->off_hist;
    SERVO_REQUIRE(ho % 4 == 0 && ho >= d.row_floats && ho + pad4(x.hs->floats) <= d.row_stride);
  }
  if (x.pl) {
    // a plant table is an evaluation input: the launch is the step-response instance of its pack
    SERVO_REQUIRE(d.fixed_command != nullptr || d.eval != nullptr || d.trace != nullptr);
    SERVO_REQUIRE(x.pl->reserved[0] == 0 && x.pl->reserved[1] == 0);
    SERVO_REQUIRE(x.pl->table != nullptr && aligned16(x.pl->table));
  }

  // every memory range the launch touches, by its byte extent (the tables of a variable number of entries by the most they
  // may hold); a NULL pointer is a buffer that is not there.  Every two of them are disjoint
  const uintptr_t n = (uintptr_t)d.N, f32 = sizeof(float);
  const struct { const void* p; uintptr_t bytes; const char* name; } ranges[] = {
      {d.state_in, n * (uintptr_t)d.row_stride * f32, "state_in"},     // the one exception: an init launch may write the
      {d.state_out, n * (uintptr_t)d.row_stride * f32, "state_out"},   // first state into the slab it was given (below)
      {d.action, n * f32 * (uintptr_t)(x.ac ? x.ac->width : kJoints), "action"},
      {d.reset, n, "reset"},
      {d.episode_length, n * sizeof(int64_t), "episode_length"},
      {d.fixed_command, (uintptr_t)(d.fixed_segments > 1 ? d.fixed_segments : 1) * n * 3 * f32, "fixed_command"},
      {d.eval, n * CATPPO_SERVO_EVAL_FLOATS * f32, "eval"},
      {d.trace, (uintptr_t)d.trace_capacity * (uintptr_t)d.trace_envs * CATPPO_SERVO_TRACE_FLOATS * f32, "trace"},
      // compared whenever they are set, as before: with reward_terms = 0 the launch does not touch them
      {d.reward_rec, n * CATPPO_SERVO_REWARD_FLOATS * f32, "reward_rec"},
      {d.reward_table, sizeof(catppo_servo_reward_term) * CATPPO_SERVO_REWARD_MAX_TERMS, "reward_table"},
      {x.obs ? x.obs->table : nullptr, sizeof(catppo_servo_obs_entry) * (uintptr_t)(x.obs ? x.obs->width : 0), "obs.table"},
      {x.ev ? x.ev->block : nullptr, f32 * (uintptr_t)(x.ev ? x.ev->floats : 0), "ev.block"},
      {x.cm ? x.cm->block : nullptr, f32 * CATPPO_SERVO_COMMAND_FLOATS, "cmd.block"},
      {x.tm ? x.tm->table : nullptr, sizeof(catppo_servo_term_entry) * CATPPO_SERVO_TERM_MAX_TERMS, "term.table"},
      {x.tm ? x.tm->rec : nullptr, n * CATPPO_SERVO_TERM_FLOATS * f32, "term.rec"},
      {x.ac ? x.ac->table : nullptr, sizeof(catppo_servo_action_entry) * kJoints, "act.table"},
      {x.au ? x.au->table : nullptr, sizeof(catppo_servo_actuator_entry) * kJoints, "actu.table"},
      {x.rn ? x.rn->block : nullptr, f32 * CATPPO_SERVO_RANDOMIZE_FLOATS, "rnd.block"},
      {x.hs ? x.hs->map : nullptr, sizeof(uint32_t) * (uintptr_t)(x.hs ? x.hs->floats : 0), "hist.map"},
      {x.pl ? x.pl->table : nullptr, n * CATPPO_SERVO_PLANT_FLOATS * f32, "plant.table"}};
  constexpr int kRanges = sizeof(ranges) / sizeof(ranges[0]);
  for (int i = 0; i < kRanges; ++i)
    for (int j = i + 1; j < kRanges; ++j) {
      const auto &a = ranges[i], &b = ranges[j];
      if (!a.p || !b.p) continue;
      if (i == 0 && j == 1 && d.init && a.p == b.p) continue;            // state_in == state_out on an init launch
      const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
      if (a0 < b0 + b.bytes && b0 < a0 + a.bytes) {
        static thread_local char why[96];
        snprintf(why, sizeof(why), "%s and %s do not overlap", a.name, b.name);
        return why;
      }
    }

  // every field the kernel writes lies inside the row (the base fields are not compared with each other)
  struct Field { int64_t off, width; };
  const Field base[] = {
      {d.off_joint_pos, kJoints}, {d.off_joint_vel, kJoints}, {d.off_joint_acc, kJoints}, {d.off_applied_torque, kJoints},
      {d.off_projected_gravity, 3}, {d.off_root_pos, 3}, {d.off_command, 3}, {d.off_last_air_time, d.B},
      {d.off_first_contact, d.B}, {d.off_forces, (int64_t)d.H * d.B * 3}, {d.off_reward, 1}, {d.off_hard_reset, 1},
      {d.off_obs, d.obs_dim}, {d.off_servo, kPrivate}};
  for (const Field& fl : base) SERVO_REQUIRE(fl.off >= 0 && fl.off + fl.width <= d.row_floats);
  // the fields of the extensions that are present: each on a 16-byte boundary inside the row, disjoint from the others; a
  // state field touches no base field, the policy observation stays clear of the raw one it is computed from
  const struct { bool present, state; Field f; } ext[] = {
      {x.obs != nullptr, false, {x.obs ? x.obs->off_policy_obs : 0, pad4(x.obs ? x.obs->width : 0)}},
      {x.cm != nullptr, true, {x.cm ? x.cm->off_cmd_state : 0, 4}},
      {x.tm != nullptr, true, {x.tm ? x.tm->off_term_state : 0, 4}},
      {x.au != nullptr, true, {x.au ? x.au->off_act_hist : 0, CATPPO_SERVO_ACT_HIST_FLOATS}},
      {x.ev != nullptr && x.ev->reserved != 0, true, {x.ev ? x.ev->reserved : 0, 4}}};
  const auto apart = [](const Field& a, const Field& b) { return a.off + a.width <= b.off || a.off >= b.off + b.width; };
  for (const auto& e : ext) {
    if (!e.present) continue;
    SERVO_REQUIRE(e.f.off >= 0 && e.f.off % 4 == 0 && e.f.off + e.f.width <= d.row_floats);
    if (e.state)
      for (const Field& fl : base) SERVO_REQUIRE(apart(e.f, fl));
    else
      SERVO_REQUIRE(apart(e.f, Field{d.off_obs, kRawObs}));
    for (const auto* o = ext; o != &e; ++o) SERVO_REQUIRE(!o->present || apart(e.f, o->f));
  }
  return nullptr;
}
#undef SERVO_REQUIRE

// ---------------------------------------------------------------------------------------------- c. the dispatch
// calls f with exactly the non-null descriptors, dereferenced, in the order given
template <typename F>
void with_present(F&& f) { f(); }
template <typename F, typename T, typename... R>
void with_present(F&& f, const T* p, const R*... r) {
  if (p) with_present([&](const auto&... x) { f(*p, x...); }, r...);
  else with_present(f, r...);
}

}  // namespace
