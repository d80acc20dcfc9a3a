// Solo12 servo surrogate: the instances of servo_sim_kernel whose event block is the extended one (DESIGN section 9,
// "Disturbances": a timed push and an external wrench), ServoEventsExt in the place of catppo_servo_events, without a
// randomisation descriptor: the 4 packs over {obs, commands, terminations} x {nothing, actions, actions + actuators} behind them
// x {train, step response} x {rewards off, on}.  A translation unit of their own, so that they compile beside the instances of
// the other units (servo_sim.hip lists them) and none of those changes.
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_disturb(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                              const catppo_servo_sim& d, const ServoExts& x) {
  const ServoEventsExt ev = {*x.ev};
  // the event descriptor is always there: it is passed by reference between the optional ones, so that no pack without it is
  // instantiated here
  with_present([&](const auto&... o) {
    with_present([&](const auto&... r) {
      if (x.au) launch(mode, rew, nblk, lds_bytes, st, d, o..., ev, r..., *x.ac, *x.au);
      else if (x.ac) launch(mode, rew, nblk, lds_bytes, st, d, o..., ev, r..., *x.ac);
      else launch(mode, rew, nblk, lds_bytes, st, d, o..., ev, r...);
    }, x.cm, x.tm);
  }, x.obs);
}
