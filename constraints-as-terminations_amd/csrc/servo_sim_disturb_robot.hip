// Solo12 servo surrogate: the instances of servo_sim_kernel whose event block is the extended one (DESIGN section 9,
// "Disturbances"), ServoEventsExt in the place of catppo_servo_events, behind a randomisation descriptor: the packs of
// servo_sim_randomize.hip, servo_sim_history.hip and servo_sim_plant.hip that hold an event descriptor.  A translation unit of
// their own, beside servo_sim_disturb.hip.
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_disturb_robot(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                                    const catppo_servo_sim& d, const ServoExts& x) {
  const ServoEventsExt ev = {*x.ev};
  // the event descriptor is always there: it is passed by reference between the optional ones, so that no pack without it is
  // instantiated here
  const auto behind_obs = [&](const auto&... o) {
    with_present([&](const auto&... r) {
      if (x.pl) launch(mode, rew, nblk, lds_bytes, st, d, o..., ev, r..., *x.ac, *x.au, *x.rn, *x.pl);
      else launch(mode, rew, nblk, lds_bytes, st, d, o..., ev, r..., *x.ac, *x.au, *x.rn);
    }, x.cm, x.tm);
  };
  if (x.hs)                                                        // a history needs its observations (servo_sim_check)
    with_present([&](const auto&... r) {
      if (x.pl) launch(mode, rew, nblk, lds_bytes, st, d, *x.obs, ev, r..., *x.ac, *x.au, *x.rn, *x.hs, *x.pl);
      else launch(mode, rew, nblk, lds_bytes, st, d, *x.obs, ev, r..., *x.ac, *x.au, *x.rn, *x.hs);
    }, x.cm, x.tm);
  else
    with_present(behind_obs, x.obs);
}
