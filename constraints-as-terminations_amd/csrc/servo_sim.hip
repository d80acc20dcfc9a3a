// Solo12 servo surrogate: one control step of the closed-loop stand-in simulator in one launch (DESIGN section 9,
// include/catppo.h catppo_servo_sim).  tests/servo_twin.py restates this file statement by statement in numpy; the two
// agree bit for bit, so every expression here is part of the model: fp32, no fused multiply-add (the library is built
// with -ffp-contract=off), only + - * / sqrt min max abs compares and selects, reductions in a fixed order.
//
// 16 lanes per env, four envs per wave, 16 envs per workgroup.  Lane j < 12 is joint j (leg j / 3 in the order FL FR HL
// HR, part j % 3 in the order HAA HFE KFE) and integrates it in registers; every lane carries foot (lane & 3) and the
// whole base state redundantly (the joint sums are butterflies, all lanes end up with the same bits), so no lane waits
// for another except through the shuffles.  The next row is assembled in LDS and leaves as coalesced 16-byte stores.
//   tree16: x += xor-shuffle 8, 4, 2, 1 (width 16)     tree4 (feet): x += xor-shuffle 1, 2
// The kernel template is servo_sim_kernel.h; this unit holds the entry point and the instances of the packs without an action
// table, servo_sim_actions.hip those with one, servo_sim_actuators.hip those with an actuator table behind it,
// servo_sim_randomize.hip those with a randomisation block behind that, servo_sim_history.hip those with a history
// descriptor behind that.
#include "servo_sim_kernel.h"

// the descriptor's size is part of the ABI: cat_envs/native.py (ServoSimRewards) and tests/test_servo_reward_twin.py pin it
static_assert(sizeof(catppo_servo_sim) == 368, "catppo_servo_sim: 344 bytes up to trace_capacity + the 24-byte reward tail");
static_assert(sizeof(catppo_servo_reward_term) == 16 && CATPPO_SERVO_REWARD_FLOATS == 32, "reward table entry / record row");
static_assert(sizeof(catppo_servo_obs_entry) == 32 && CATPPO_SERVO_OBS_MAX_WIDTH == 64, "observation table entry: two 16-byte loads");
static_assert(offsetof(catppo_servo_sim_obs, obs) == sizeof(catppo_servo_sim) && sizeof(catppo_servo_obs) == 16,
              "catppo_servo_sim_obs: the observation descriptor lies right behind the 368 bytes");
static_assert(offsetof(catppo_servo_sim_events, obs) == 368 && offsetof(catppo_servo_sim_events, ev) == 384 &&
                  sizeof(catppo_servo_events) == 16 && sizeof(catppo_servo_sim_events) == 400 && CATPPO_SERVO_EVENT_FLOATS == 32,
              "catppo_servo_sim_events: observation and event descriptors behind the 368 bytes");
static_assert(offsetof(catppo_servo_sim_commands, obs) == 368 && offsetof(catppo_servo_sim_commands, ev) == 384 &&
                  offsetof(catppo_servo_sim_commands, cmd) == 400 && sizeof(catppo_servo_commands) == 16 &&
                  offsetof(catppo_servo_commands, floats) == 8 && offsetof(catppo_servo_commands, off_cmd_state) == 12 &&
                  sizeof(catppo_servo_sim_commands) == 416 && CATPPO_SERVO_COMMAND_FLOATS == 16,
              "catppo_servo_sim_commands: observation, event and command descriptors behind the 368 bytes");
static_assert(offsetof(catppo_servo_sim_terminations, cmd) == 400 && offsetof(catppo_servo_sim_terminations, term) == 416 &&
                  sizeof(catppo_servo_term_entry) == 16 && sizeof(catppo_servo_terminations) == 24 &&
                  offsetof(catppo_servo_terminations, rec) == 8 && offsetof(catppo_servo_terminations, terms) == 16 &&
                  offsetof(catppo_servo_terminations, off_term_state) == 20 && sizeof(catppo_servo_sim_terminations) == 440 &&
                  CATPPO_SERVO_TERM_FLOATS == 16 && CATPPO_SERVO_TERM_MAX_TERMS == 15,
              "catppo_servo_sim_terminations: observation, event, command and termination descriptors behind the 368 bytes");
static_assert(offsetof(catppo_servo_sim_actions, term) == 416 && offsetof(catppo_servo_sim_actions, act) == 440 &&
                  sizeof(catppo_servo_action_entry) == 32 && sizeof(catppo_servo_actions) == 16 &&
                  offsetof(catppo_servo_actions, width) == 8 && sizeof(catppo_servo_sim_actions) == 456,
              "catppo_servo_sim_actions: the action descriptor behind the termination descriptor");
static_assert(offsetof(catppo_servo_sim_actuators, act) == 440 && offsetof(catppo_servo_sim_actuators, actu) == 456 &&
                  sizeof(catppo_servo_actuator_entry) == 32 && offsetof(catppo_servo_actuator_entry, flags) == 24 &&
                  sizeof(catppo_servo_actuators) == 16 && offsetof(catppo_servo_actuators, off_act_hist) == 8 &&
                  sizeof(catppo_servo_sim_actuators) == 472 && CATPPO_SERVO_ACT_HIST_FLOATS == 48,
              "catppo_servo_sim_actuators: the actuator descriptor behind the action descriptor");
static_assert(offsetof(catppo_servo_sim_randomize, actu) == 456 && offsetof(catppo_servo_sim_randomize, rnd) == 472 &&
                  sizeof(catppo_servo_randomize) == 16 && offsetof(catppo_servo_randomize, reserved) == 8 &&
                  sizeof(catppo_servo_sim_randomize) == 488 && CATPPO_SERVO_RANDOMIZE_FLOATS == 32,
              "catppo_servo_sim_randomize: the randomisation descriptor behind the actuator descriptor");
static_assert(offsetof(catppo_servo_sim_history, rnd) == 472 && offsetof(catppo_servo_sim_history, hist) == 488 &&
                  sizeof(catppo_servo_history) == 16 && offsetof(catppo_servo_history, off_hist) == 8 &&
                  offsetof(catppo_servo_history, floats) == 12 && sizeof(catppo_servo_sim_history) == 504 &&
                  CATPPO_SERVO_OBS_HISTORY_MAX_FLOATS == 512 && CATPPO_SERVO_OBS_HISTORY_MAX_DEPTH == 16,
              "catppo_servo_sim_history: the history descriptor behind the randomisation descriptor");

extern "C" int catppo_servo_sim_step(catppo_ctx* ctx, const catppo_servo_sim* desc, void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  CATPPO_CHECK_ARG(ctx, desc != nullptr);
  const catppo_servo_sim& d = *desc;
  // reserved names what lies behind the descriptor: nothing, the observation descriptor of a catppo_servo_sim_obs, or the
  // observation and event descriptors of a catppo_servo_sim_events (whose observation descriptor may be empty)
  // ... or all three of a catppo_servo_sim_commands (whose event descriptor may be empty, too)
  // ... or all four of a catppo_servo_sim_terminations (whose command descriptor may be empty, too)
  // ... or all five of a catppo_servo_sim_actions (whose termination descriptor may be empty, too)
  // ... or all six of a catppo_servo_sim_actuators (whose action descriptor is never empty)
  // ... or all seven of a catppo_servo_sim_randomize (whose actuator descriptor is never empty)
  // ... or all eight of a catppo_servo_sim_history (whose observation and randomisation descriptors are never empty)
  const bool ext_hist = d.reserved == CATPPO_SERVO_EXT_HISTORY;
  const bool ext_rnd = d.reserved == CATPPO_SERVO_EXT_RANDOMIZE || ext_hist;
  const bool ext_actu = d.reserved == CATPPO_SERVO_EXT_ACTUATORS || ext_rnd;
  const bool ext_act = d.reserved == CATPPO_SERVO_EXT_ACTIONS || ext_actu;
  const bool ext_term = d.reserved == CATPPO_SERVO_EXT_TERMINATIONS || ext_act;
  const bool ext_cmd = d.reserved == CATPPO_SERVO_EXT_COMMANDS || ext_term;
  // d.reserved is one of the known values
  CATPPO_CHECK_ARG(ctx, d.reserved == 0 || d.reserved == CATPPO_SERVO_EXT_OBS || d.reserved == CATPPO_SERVO_EXT_EVENTS || ext_cmd);
  const catppo_servo_obs* obs = d.reserved != 0 ? &reinterpret_cast<const catppo_servo_sim_obs*>(desc)->obs : nullptr;
  const catppo_servo_events* ev = d.reserved == CATPPO_SERVO_EXT_EVENTS || ext_cmd
                                      ? &reinterpret_cast<const catppo_servo_sim_events*>(desc)->ev : nullptr;
  const catppo_servo_commands* cm = ext_cmd ? &reinterpret_cast<const catppo_servo_sim_commands*>(desc)->cmd : nullptr;
  if (ev && obs->width == 0 && obs->table == nullptr) obs = nullptr;
  const catppo_servo_terminations* tm = ext_term ? &reinterpret_cast<const catppo_servo_sim_terminations*>(desc)->term : nullptr;
  if (cm && ev->block == nullptr && ev->floats == 0) ev = nullptr;
  if (tm && cm->block == nullptr && cm->floats == 0) cm = nullptr;
  const catppo_servo_actions* ac = ext_act ? &reinterpret_cast<const catppo_servo_sim_actions*>(desc)->act : nullptr;
  if (ac && tm->table == nullptr && tm->terms == 0) tm = nullptr;
  const catppo_servo_actuators* au = ext_actu ? &reinterpret_cast<const catppo_servo_sim_actuators*>(desc)->actu : nullptr;
  const catppo_servo_randomize* rn = ext_rnd ? &reinterpret_cast<const catppo_servo_sim_randomize*>(desc)->rnd : nullptr;
  const catppo_servo_history* hs = ext_hist ? &reinterpret_cast<const catppo_servo_sim_history*>(desc)->hist : nullptr;
  CATPPO_CHECK_ARG(ctx, d.N >= 1 && d.N < (int64_t(1) << 31) && d.env_offset >= 0 && d.env_offset + d.N < (int64_t(1) << 32));
  CATPPO_CHECK_ARG(ctx, d.state_in && d.state_out && d.episode_length);
  CATPPO_CHECK_ARG(ctx, d.init || (d.action && d.reset && d.state_in != d.state_out));
  CATPPO_CHECK_ARG(ctx, d.row_floats >= 4 && d.row_floats % 4 == 0 && d.row_stride >= d.row_floats && d.row_stride % 4 == 0);
  CATPPO_CHECK_ARG(ctx, ((uintptr_t)d.state_in % 16) == 0 && ((uintptr_t)d.state_out % 16) == 0);
  CATPPO_CHECK_ARG(ctx, (size_t)d.row_floats * kEnvsPerBlock * sizeof(float) <= 64 * 1024);
  CATPPO_CHECK_ARG(ctx, d.H >= 1 && d.B == 17 && d.obs_dim >= 0);
  CATPPO_CHECK_ARG(ctx, d.decimation >= 1 && d.resample_steps >= 1 && d.max_episode_length >= 1);
  CATPPO_CHECK_ARG(ctx, d.inertia > 0.f && d.dt > 0.f && d.reward_scale > 0.f);
  CATPPO_CHECK_ARG(ctx, ((uintptr_t)d.eval % 16) == 0);
  CATPPO_CHECK_ARG(ctx, d.fixed_command == nullptr || (d.fixed_command != d.state_in && d.fixed_command != d.state_out));
  CATPPO_CHECK_ARG(ctx, d.eval == nullptr || (d.eval != d.state_in && d.eval != d.state_out));
  CATPPO_CHECK_ARG(ctx, d.fixed_segments >= 0);
  CATPPO_CHECK_ARG(ctx, d.fixed_segments <= 1 || (d.fixed_segment_steps >= 1 && d.fixed_command != nullptr));
  if (d.trace) {
    CATPPO_CHECK_ARG(ctx, d.eval != nullptr && ((uintptr_t)d.trace % 16) == 0);
    CATPPO_CHECK_ARG(ctx, d.trace_envs >= 1 && d.trace_envs <= d.N && d.trace_capacity >= 1);
    CATPPO_CHECK_ARG(ctx, d.trace != d.state_in && d.trace != d.state_out && d.trace != d.eval && d.trace != d.fixed_command);
  }
  CATPPO_CHECK_ARG(ctx, d.reward_terms >= 0 && d.reward_terms <= CATPPO_SERVO_REWARD_MAX_TERMS);
  if (d.reward_terms > 0) {
    CATPPO_CHECK_ARG(ctx, d.reward_rec != nullptr && ((uintptr_t)d.reward_rec % 16) == 0);
    CATPPO_CHECK_ARG(ctx, d.reward_rec != d.state_in && d.reward_rec != d.state_out && d.reward_rec != d.eval &&
                              d.reward_rec != d.trace && d.reward_rec != d.fixed_command);
    // the entries are device memory: their writer checks kinds, masks and params (Solo12ServoSim.set_reward_table)
    CATPPO_CHECK_ARG(ctx, d.reward_table != nullptr && ((uintptr_t)d.reward_table % 16) == 0);
    CATPPO_CHECK_ARG(ctx, (const void*)d.reward_table != d.state_in && (const void*)d.reward_table != d.state_out &&
                              (const void*)d.reward_table != d.reward_rec);
  }
  // every field the kernel writes lies inside the row
  const struct { int32_t off, width; } fields[] = {
      {d.off_joint_pos, kJoints}, {d.off_joint_vel, kJoints}, {d.off_joint_acc, kJoints}, {d.off_applied_torque, kJoints},
      {d.off_projected_gravity, 3}, {d.off_root_pos, 3}, {d.off_command, 3}, {d.off_last_air_time, d.B},
      {d.off_first_contact, d.B}, {d.off_forces, d.H * d.B * 3}, {d.off_reward, 1}, {d.off_hard_reset, 1},
      {d.off_obs, d.obs_dim}, {d.off_servo, kPrivate}};
  for (const auto& fl : fields) CATPPO_CHECK_ARG(ctx, fl.off >= 0 && (int64_t)fl.off + fl.width <= d.row_floats);
  if (obs) {
    const catppo_servo_obs& o = *obs;
    CATPPO_CHECK_ARG(ctx, d.obs_dim == kRawObs && d.max_episode_length < (int64_t(1) << 27));
    CATPPO_CHECK_ARG(ctx, o.width >= 1 && o.width <= CATPPO_SERVO_OBS_MAX_WIDTH);
    const int64_t padded = (o.width + 3) / 4 * 4;
    CATPPO_CHECK_ARG(ctx, o.off_policy_obs >= 0 && o.off_policy_obs % 4 == 0 && o.off_policy_obs + padded <= d.row_floats);
    CATPPO_CHECK_ARG(ctx, o.off_policy_obs + padded <= d.off_obs || o.off_policy_obs >= d.off_obs + kRawObs);
    // the entries are device memory: whatever they hold the launch stays inside the row (src is clamped in the kernel)
    const void* tb = o.table;
    CATPPO_CHECK_ARG(ctx, tb != nullptr && ((uintptr_t)tb % 16) == 0);
    CATPPO_CHECK_ARG(ctx, tb != d.state_in && tb != d.state_out && tb != d.eval && tb != d.trace && tb != d.fixed_command &&
                              tb != d.reward_rec && tb != (const void*)d.reward_table);
  }
  if (ev) {
    CATPPO_CHECK_ARG(ctx, d.max_episode_length < (int64_t(1) << 27));
    CATPPO_CHECK_ARG(ctx, ev->floats == CATPPO_SERVO_EVENT_FLOATS && ev->reserved == 0);
    // the block is device memory: its writer checks the values (Solo12ServoSim.set_event_block); they are never addresses
    const void* bl = ev->block;
    CATPPO_CHECK_ARG(ctx, bl != nullptr && ((uintptr_t)bl % 16) == 0);
    CATPPO_CHECK_ARG(ctx, bl != d.state_in && bl != d.state_out && bl != d.eval && bl != d.trace && bl != d.fixed_command &&
                              bl != d.reward_rec && bl != (const void*)d.reward_table && (!obs || bl != (const void*)obs->table));
  }
  if (cm) {
    CATPPO_CHECK_ARG(ctx, d.max_episode_length < (int64_t(1) << 27));
    CATPPO_CHECK_ARG(ctx, cm->floats == CATPPO_SERVO_COMMAND_FLOATS);
    // the block is device memory: its writer checks the values (Solo12ServoSim.set_command_block); they are never addresses
    const void* bl = cm->block;
    CATPPO_CHECK_ARG(ctx, bl != nullptr && ((uintptr_t)bl % 16) == 0);
    CATPPO_CHECK_ARG(ctx, bl != d.state_in && bl != d.state_out && bl != d.eval && bl != d.trace && bl != d.fixed_command &&
                              bl != d.reward_rec && bl != (const void*)d.reward_table && (!obs || bl != (const void*)obs->table) &&
                              (!ev || bl != (const void*)ev->block));
    // the state field: four floats of the row on a 16-byte boundary that no other field the kernel writes touches
    const int64_t cs = cm->off_cmd_state;
    CATPPO_CHECK_ARG(ctx, cs >= 0 && cs % 4 == 0 && cs + 4 <= d.row_floats);
    for (const auto& fl : fields) CATPPO_CHECK_ARG(ctx, cs + 4 <= fl.off || cs >= (int64_t)fl.off + fl.width);
    if (obs) {
      const int64_t padded = (obs->width + 3) / 4 * 4;
      CATPPO_CHECK_ARG(ctx, cs + 4 <= obs->off_policy_obs || cs >= obs->off_policy_obs + padded);
    }
  }
  if (tm) {
    CATPPO_CHECK_ARG(ctx, tm->terms >= 1 && tm->terms <= CATPPO_SERVO_TERM_MAX_TERMS);
    // the entries are device memory: their writer checks kinds, masks and params (Solo12ServoSim.set_termination_table);
    // whatever they hold the launch stays inside its row and its record: they are never addresses, and the history
    // slots a contact term reads are the input row's own
    const void* tb = tm->table;
    const void* rc = tm->rec;
    CATPPO_CHECK_ARG(ctx, tb != nullptr && ((uintptr_t)tb % 16) == 0 && rc != nullptr && ((uintptr_t)rc % 16) == 0);
    const uintptr_t tb0 = (uintptr_t)tb, tb1 = tb0 + sizeof(catppo_servo_term_entry) * CATPPO_SERVO_TERM_MAX_TERMS;
    const uintptr_t rc0 = (uintptr_t)rc, rc1 = rc0 + (uintptr_t)d.N * CATPPO_SERVO_TERM_FLOATS * sizeof(float);
    CATPPO_CHECK_ARG(ctx, tb1 <= rc0 || rc1 <= tb0);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.trace, d.fixed_command, d.reward_rec, (const void*)d.reward_table,
                            obs ? (const void*)obs->table : nullptr, ev ? (const void*)ev->block : nullptr,
                            cm ? (const void*)cm->block : nullptr};
    for (const void* o : others) CATPPO_CHECK_ARG(ctx, tb != o && rc != o);
    // the state field: four floats of the row on a 16-byte boundary that no other field the kernel writes touches
    const int64_t ts = tm->off_term_state;
    CATPPO_CHECK_ARG(ctx, ts >= 0 && ts % 4 == 0 && ts + 4 <= d.row_floats);
    for (const auto& fl : fields) CATPPO_CHECK_ARG(ctx, ts + 4 <= fl.off || ts >= (int64_t)fl.off + fl.width);
    if (obs) {
      const int64_t padded = (obs->width + 3) / 4 * 4;
      CATPPO_CHECK_ARG(ctx, ts + 4 <= obs->off_policy_obs || ts >= obs->off_policy_obs + padded);
    }
    if (cm) CATPPO_CHECK_ARG(ctx, ts + 4 <= cm->off_cmd_state || ts >= (int64_t)cm->off_cmd_state + 4);
  }
  if (ac) {
    CATPPO_CHECK_ARG(ctx, ac->width >= 1 && ac->width <= kJoints && ac->reserved == 0);
    // the entries are device memory: their writer checks them (Solo12ServoSim.set_action_table); whatever they hold the
    // launch stays inside the action's row (col is clamped in the kernel), the rest are values, never addresses
    const void* tb = ac->table;
    CATPPO_CHECK_ARG(ctx, tb != nullptr && ((uintptr_t)tb % 16) == 0);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.trace, d.fixed_command, d.reward_rec, (const void*)d.reward_table,
                            d.action, obs ? (const void*)obs->table : nullptr, ev ? (const void*)ev->block : nullptr,
                            cm ? (const void*)cm->block : nullptr, tm ? (const void*)tm->table : nullptr,
                            tm ? (const void*)tm->rec : nullptr};
    for (const void* o : others) CATPPO_CHECK_ARG(ctx, tb != o);
    if (tm) {
      // the table's 12 entries and the termination record do not overlap
      const uintptr_t tb0 = (uintptr_t)tb, tb1 = tb0 + sizeof(catppo_servo_action_entry) * kJoints;
      const uintptr_t rc0 = (uintptr_t)tm->rec, rc1 = rc0 + (uintptr_t)d.N * CATPPO_SERVO_TERM_FLOATS * sizeof(float);
      CATPPO_CHECK_ARG(ctx, tb1 <= rc0 || rc1 <= tb0);
    }
  }
  if (au) {
    CATPPO_CHECK_ARG(ctx, au->reserved == 0);
    // the entries are device memory: their writer checks them (Solo12ServoSim.set_actuator_table); they are values, never
    // addresses, and the kernel clamps the history slot a lag reaches back to
    const void* tb = au->table;
    CATPPO_CHECK_ARG(ctx, tb != nullptr && ((uintptr_t)tb % 16) == 0);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.trace, d.fixed_command, d.reward_rec, (const void*)d.reward_table,
                            d.action, obs ? (const void*)obs->table : nullptr, ev ? (const void*)ev->block : nullptr,
                            cm ? (const void*)cm->block : nullptr, tm ? (const void*)tm->table : nullptr,
                            tm ? (const void*)tm->rec : nullptr};
    for (const void* o : others) CATPPO_CHECK_ARG(ctx, tb != o);
    // the table's 12 entries overlap neither the action table's nor the termination record
    const uintptr_t tb0 = (uintptr_t)tb, tb1 = tb0 + sizeof(catppo_servo_actuator_entry) * kJoints;
    const uintptr_t at0 = (uintptr_t)ac->table, at1 = at0 + sizeof(catppo_servo_action_entry) * kJoints;
    CATPPO_CHECK_ARG(ctx, tb1 <= at0 || at1 <= tb0);
    if (tm) {
      const uintptr_t rc0 = (uintptr_t)tm->rec, rc1 = rc0 + (uintptr_t)d.N * CATPPO_SERVO_TERM_FLOATS * sizeof(float);
      CATPPO_CHECK_ARG(ctx, tb1 <= rc0 || rc1 <= tb0);
    }
    // the history field: 48 floats of the row on a 16-byte boundary that no other field the kernel writes touches
    const int64_t hs = au->off_act_hist, hw = CATPPO_SERVO_ACT_HIST_FLOATS;
    CATPPO_CHECK_ARG(ctx, hs >= 0 && hs % 4 == 0 && hs + hw <= d.row_floats);
    for (const auto& fl : fields) CATPPO_CHECK_ARG(ctx, hs + hw <= fl.off || hs >= (int64_t)fl.off + fl.width);
    if (obs) {
      const int64_t padded = (obs->width + 3) / 4 * 4;
      CATPPO_CHECK_ARG(ctx, hs + hw <= obs->off_policy_obs || hs >= obs->off_policy_obs + padded);
    }
    if (cm) CATPPO_CHECK_ARG(ctx, hs + hw <= cm->off_cmd_state || hs >= (int64_t)cm->off_cmd_state + 4);
    if (tm) CATPPO_CHECK_ARG(ctx, hs + hw <= tm->off_term_state || hs >= (int64_t)tm->off_term_state + 4);
  }
  if (rn) {
    CATPPO_CHECK_ARG(ctx, rn->reserved[0] == 0 && rn->reserved[1] == 0);
    // the words are device memory: their writer checks them (Solo12ServoSim.set_randomize_block); they are values and
    // masks, never addresses
    const void* bk = rn->block;
    CATPPO_CHECK_ARG(ctx, bk != nullptr && ((uintptr_t)bk % 16) == 0);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.trace, d.fixed_command, d.reward_rec, (const void*)d.reward_table,
                            d.action, d.reset, d.episode_length, obs ? (const void*)obs->table : nullptr,
                            tm ? (const void*)tm->table : nullptr};
    for (const void* o : others) CATPPO_CHECK_ARG(ctx, bk != o);
    // the block's 32 words overlap no other block, table or record
    const uintptr_t b0 = (uintptr_t)bk, b1 = b0 + sizeof(float) * CATPPO_SERVO_RANDOMIZE_FLOATS;
    const uintptr_t span[][2] = {
        {(uintptr_t)au->table, sizeof(catppo_servo_actuator_entry) * kJoints},
        {(uintptr_t)ac->table, sizeof(catppo_servo_action_entry) * kJoints},
        {ev ? (uintptr_t)ev->block : 0, sizeof(float) * CATPPO_SERVO_EVENT_FLOATS},
        {cm ? (uintptr_t)cm->block : 0, sizeof(float) * CATPPO_SERVO_COMMAND_FLOATS},
        {tm ? (uintptr_t)tm->rec : 0, (uintptr_t)d.N * CATPPO_SERVO_TERM_FLOATS * sizeof(float)}};
    for (const auto& sp : span) CATPPO_CHECK_ARG(ctx, sp[0] == 0 || b1 <= sp[0] || sp[0] + sp[1] <= b0);
  }
  if (hs) {
    CATPPO_CHECK_ARG(ctx, obs != nullptr);
    CATPPO_CHECK_ARG(ctx, hs->floats >= 1 && hs->floats <= CATPPO_SERVO_OBS_HISTORY_MAX_FLOATS);
    // the field: pad4(T) floats of the row on a 16-byte boundary, behind the part that is staged in LDS, inside the stride
    const int64_t ho = hs->off_hist, padded = ((int64_t)hs->floats + 3) / 4 * 4;
    CATPPO_CHECK_ARG(ctx, ho % 4 == 0 && ho >= d.row_floats && ho + padded <= d.row_stride);
    // the words are device memory: their writer checks them (Solo12ServoSim.set_history_table); whatever they hold the
    // launch stays inside its row (cur and i + w are clamped in the kernel)
    const void* mp = hs->map;
    CATPPO_CHECK_ARG(ctx, mp != nullptr && ((uintptr_t)mp % 16) == 0);
    const void* others[] = {d.state_in, d.state_out, d.eval, d.trace, d.fixed_command, d.reward_rec, (const void*)d.reward_table,
                            d.action, d.reset, d.episode_length, (const void*)obs->table, tm ? (const void*)tm->table : nullptr};
    for (const void* o : others) CATPPO_CHECK_ARG(ctx, mp != o);
    // the map's T words overlap no slab, block, table or record
    const uintptr_t m0 = (uintptr_t)mp, m1 = m0 + sizeof(uint32_t) * (uintptr_t)hs->floats;
    const uintptr_t slab = (uintptr_t)d.N * (uintptr_t)d.row_stride * sizeof(float);
    const uintptr_t span[][2] = {
        {(uintptr_t)d.state_in, slab},
        {(uintptr_t)d.state_out, slab},
        {(uintptr_t)obs->table, sizeof(catppo_servo_obs_entry) * (uintptr_t)obs->width},
        {(uintptr_t)rn->block, sizeof(float) * CATPPO_SERVO_RANDOMIZE_FLOATS},
        {(uintptr_t)au->table, sizeof(catppo_servo_actuator_entry) * kJoints},
        {(uintptr_t)ac->table, sizeof(catppo_servo_action_entry) * kJoints},
        {d.reward_terms > 0 ? (uintptr_t)d.reward_table : 0, sizeof(catppo_servo_reward_term) * CATPPO_SERVO_REWARD_MAX_TERMS},
        {d.reward_terms > 0 ? (uintptr_t)d.reward_rec : 0, (uintptr_t)d.N * CATPPO_SERVO_REWARD_FLOATS * sizeof(float)},
        {ev ? (uintptr_t)ev->block : 0, sizeof(float) * CATPPO_SERVO_EVENT_FLOATS},
        {cm ? (uintptr_t)cm->block : 0, sizeof(float) * CATPPO_SERVO_COMMAND_FLOATS},
        {tm ? (uintptr_t)tm->table : 0, sizeof(catppo_servo_term_entry) * CATPPO_SERVO_TERM_MAX_TERMS},
        {tm ? (uintptr_t)tm->rec : 0, (uintptr_t)d.N * CATPPO_SERVO_TERM_FLOATS * sizeof(float)},
        {(uintptr_t)d.eval, (uintptr_t)d.N * CATPPO_SERVO_EVAL_FLOATS * sizeof(float)},
        {(uintptr_t)d.trace, (uintptr_t)d.trace_capacity * (uintptr_t)d.trace_envs * CATPPO_SERVO_TRACE_FLOATS * sizeof(float)},
        {(uintptr_t)d.fixed_command, (uintptr_t)(d.fixed_segments > 1 ? d.fixed_segments : 1) * (uintptr_t)d.N * 3 * sizeof(float)}};
    for (const auto& sp : span) CATPPO_CHECK_ARG(ctx, sp[0] == 0 || m1 <= sp[0] || sp[0] + sp[1] <= m0);
  }
  const unsigned nblk = (unsigned)cdiv64(d.N, kEnvsPerBlock);
  const size_t lds_bytes = (size_t)d.row_floats * kEnvsPerBlock * sizeof(float);
  const int mode = (d.trace || d.fixed_segments > 1) ? kStepResponse : (d.fixed_command || d.eval) ? kEvaluate : kTrain;
  const bool rew = d.reward_terms > 0;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (hs) catppo_internal_servo_sim_launch_history(mode, rew, nblk, lds_bytes, st, d, *obs, ev, cm, tm, *ac, *au, *rn, *hs);
  else if (rn) catppo_internal_servo_sim_launch_randomize(mode, rew, nblk, lds_bytes, st, d, obs, ev, cm, tm, *ac, *au, *rn);
  else if (au) catppo_internal_servo_sim_launch_actuators(mode, rew, nblk, lds_bytes, st, d, obs, ev, cm, tm, *ac, *au);
  else if (ac) catppo_internal_servo_sim_launch_actions(mode, rew, nblk, lds_bytes, st, d, obs, ev, cm, tm, *ac);
  else if (tm && cm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *cm, *tm);
  else if (tm && cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *cm, *tm);
  else if (tm && cm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *cm, *tm);
  else if (tm && cm) launch(mode, rew, nblk, lds_bytes, st, d, *cm, *tm);
  else if (tm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *tm);
  else if (tm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *tm);
  else if (tm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *tm);
  else if (tm) launch(mode, rew, nblk, lds_bytes, st, d, *tm);
  else if (cm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *cm);
  else if (cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *cm);
  else if (cm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *cm);
  else if (cm) launch(mode, rew, nblk, lds_bytes, st, d, *cm);
  else if (obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev);
  else if (ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev);
  else if (obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs);
  else launch(mode, rew, nblk, lds_bytes, st, d);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}

