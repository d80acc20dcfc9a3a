// Solo12 servo surrogate: the instances of servo_sim_kernel whose pack ends with the action, the actuator and the
// randomisation descriptors ("Randomisation"): 16 packs x {train, step response} x {rewards off, on}.  A
// translation unit of their own, so that they compile beside the instances of the other units (servo_sim.hip lists them).
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_randomize(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                                const catppo_servo_sim& d, const ServoExts& x) {
  with_present([&](const auto&... opt) { launch(mode, rew, nblk, lds_bytes, st, d, opt..., *x.ac, *x.au, *x.rn); }, x.obs, x.ev, x.cm, x.tm);
}
