// Solo12 servo surrogate: the instances of servo_sim_kernel whose pack ends with the action descriptor (DESIGN section 9,
// "Actions"): 16 packs x {train, step response} x {rewards off, on}.  They are a translation unit of their own so that they
// compile beside the 80 instances of servo_sim.hip, not behind them.
#include "servo_sim_kernel.h"

void catppo_internal_servo_sim_launch_actions(int mode, bool rew, unsigned nblk, size_t lds_bytes, hipStream_t st,
                                              const catppo_servo_sim& d, const catppo_servo_obs* obs,
                                              const catppo_servo_events* ev, const catppo_servo_commands* cm,
                                              const catppo_servo_terminations* tm, const catppo_servo_actions& act) {
  if (tm && cm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *cm, *tm, act);
  else if (tm && cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *cm, *tm, act);
  else if (tm && cm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *cm, *tm, act);
  else if (tm && cm) launch(mode, rew, nblk, lds_bytes, st, d, *cm, *tm, act);
  else if (tm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *tm, act);
  else if (tm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *tm, act);
  else if (tm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *tm, act);
  else if (tm) launch(mode, rew, nblk, lds_bytes, st, d, *tm, act);
  else if (cm && obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, *cm, act);
  else if (cm && ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, *cm, act);
  else if (cm && obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *cm, act);
  else if (cm) launch(mode, rew, nblk, lds_bytes, st, d, *cm, act);
  else if (obs && ev) launch(mode, rew, nblk, lds_bytes, st, d, *obs, *ev, act);
  else if (ev) launch(mode, rew, nblk, lds_bytes, st, d, *ev, act);
  else if (obs) launch(mode, rew, nblk, lds_bytes, st, d, *obs, act);
  else launch(mode, rew, nblk, lds_bytes, st, d, act);
}
