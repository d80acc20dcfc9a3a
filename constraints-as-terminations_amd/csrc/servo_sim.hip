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
// The kernel template is servo_sim_kernel.h, the host side of the launch servo_sim_host.h.  The instances compile in six
// units, by the last descriptor of their pack: this one (none behind the terminations; it holds the entry point, too),
// servo_sim_actions.hip, servo_sim_actuators.hip, servo_sim_randomize.hip, servo_sim_history.hip and servo_sim_plant.hip.
// The instances on an extended event block compile in two more, servo_sim_disturb.hip and servo_sim_disturb_robot.hip.
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
static_assert(offsetof(catppo_servo_sim_plant, hist) == 488 && offsetof(catppo_servo_sim_plant, plant) == 504 &&
                  sizeof(catppo_servo_plant) == 16 && offsetof(catppo_servo_plant, reserved) == 8 &&
                  sizeof(catppo_servo_sim_plant) == 520 && CATPPO_SERVO_PLANT_FLOATS == 8,
              "catppo_servo_sim_plant: the plant descriptor behind the history descriptor");

extern "C" int catppo_servo_sim_step(catppo_ctx* ctx, const catppo_servo_sim* desc, void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  CATPPO_CHECK_ARG(ctx, desc != nullptr);
  const catppo_servo_sim& d = *desc;
  ServoExts x;
  const char* failed = servo_exts_of(desc, x);
  if (!failed) failed = servo_sim_check(d, x);
  if (failed) return catppo_fail(ctx, CATPPO_E_ARG, "%s: bad argument: %s", __func__, failed);
  const unsigned nblk = (unsigned)cdiv64(d.N, kEnvsPerBlock);
  const size_t lds_bytes = (size_t)d.row_floats * kEnvsPerBlock * sizeof(float);
  const int mode = (d.trace || d.fixed_segments > 1) ? kStepResponse : (d.fixed_command || d.eval) ? kEvaluate : kTrain;
  const bool rew = d.reward_terms > 0;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  // the unit that holds the instance: of a pack with an extended event block ("Disturbances") one of two,
  // else by the last descriptor of the pack
  if (x.ev && x.ev->floats == CATPPO_SERVO_EVENT_FLOATS_EXT) {
    if (x.rn) catppo_internal_servo_sim_launch_disturb_robot(mode, rew, nblk, lds_bytes, st, d, x);
    else catppo_internal_servo_sim_launch_disturb(mode, rew, nblk, lds_bytes, st, d, x);
  } else if (x.pl) catppo_internal_servo_sim_launch_plant(mode, rew, nblk, lds_bytes, st, d, x);
  else if (x.hs) catppo_internal_servo_sim_launch_history(mode, rew, nblk, lds_bytes, st, d, x);
  else if (x.rn) catppo_internal_servo_sim_launch_randomize(mode, rew, nblk, lds_bytes, st, d, x);
  else if (x.au) catppo_internal_servo_sim_launch_actuators(mode, rew, nblk, lds_bytes, st, d, x);
  else if (x.ac) catppo_internal_servo_sim_launch_actions(mode, rew, nblk, lds_bytes, st, d, x);
  else with_present([&](const auto&... opt) { launch(mode, rew, nblk, lds_bytes, st, d, opt...); }, x.obs, x.ev, x.cm, x.tm);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}
