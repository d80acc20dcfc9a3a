// Solo12 servo surrogate: the instances of servo_sim_kernel whose pack holds the observation descriptor and ends with the
// action, the actuator, the randomisation and the history descriptors ("History"): 8 packs x {train, step
// response} x {rewards off, on}.  A translation unit of their own, so that they compile beside the instances of the four
// other units, not behind them.
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_history(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                              const catppo_servo_sim& d, const catppo_servo_obs& obs,
                                              const catppo_servo_events* ev, const catppo_servo_commands* cm,
                                              const catppo_servo_terminations* tm, const catppo_servo_actions& act,
                                              const catppo_servo_actuators& actu, const catppo_servo_randomize& rnd,
                                              const catppo_servo_history& hist) {
  if (tm && cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, obs, *ev, *cm, *tm, act, actu, rnd, hist);
  else if (tm && cm) launch(mode, rew, nblk, lds_bytes, st, d, obs, *cm, *tm, act, actu, rnd, hist);
  else if (tm && ev) launch(mode, rew, nblk, lds_bytes, st, d, obs, *ev, *tm, act, actu, rnd, hist);
  else if (tm) launch(mode, rew, nblk, lds_bytes, st, d, obs, *tm, act, actu, rnd, hist);
  else if (cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, obs, *ev, *cm, act, actu, rnd, hist);
  else if (cm) launch(mode, rew, nblk, lds_bytes, st, d, obs, *cm, act, actu, rnd, hist);
  else if (ev) launch(mode, rew, nblk, lds_bytes, st, d, obs, *ev, act, actu, rnd, hist);
  else launch(mode, rew, nblk, lds_bytes, st, d, obs, act, actu, rnd, hist);
}
