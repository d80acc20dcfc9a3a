// Solo12 servo surrogate: the instances of servo_sim_kernel whose pack ends with the plant descriptor (DESIGN section 9,
// "Robustness"): behind the action, the actuator and the randomisation descriptors (16 packs), or behind those and the history
// descriptor, with the observation descriptor (8 packs), x {rewards off, on}; step-response instances only, a plant table is
// an evaluation input.  A translation unit of their own, so that they compile beside the instances of the other units
// (servo_sim.hip lists them), not behind them.
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_plant(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                            const catppo_servo_sim& d, const ServoExts& x) {
  if (x.hs)
    with_present([&](const auto&... opt) { launch(mode, rew, nblk, lds_bytes, st, d, *x.obs, opt..., *x.ac, *x.au, *x.rn, *x.hs, *x.pl); },
                 x.ev, x.cm, x.tm);
  else
    with_present([&](const auto&... opt) { launch(mode, rew, nblk, lds_bytes, st, d, opt..., *x.ac, *x.au, *x.rn, *x.pl); },
                 x.obs, x.ev, x.cm, x.tm);
}
