"""Records the CPU learning curve the servo learning tests are measured against: PPOOracle on the closed-loop numpy
twin of the Solo12 servo surrogate (tests/servo_twin.py), sizes of servo_twin.LEARNING.

    python tools/servo_learning_oracle.py        ->  profiles/servo_learning_oracle.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "constraints-as-terminations_amd")):
    sys.path.insert(0, p)

import servo_twin as T  # noqa: E402

if __name__ == "__main__":
    reward, violation = T.run_oracle_learning(log=print)
    rec = dict(T.LEARNING, hidden=list(T.LEARNING["hidden"]), task=T.TASK,
               constraints=["joint_torque", "foot_contact_force", "base_orientation"],
               reward_per_step=reward, violation_share=violation, **T.learning_summary(reward, violation))
    with open(os.path.join(ROOT, T.LEARNING_PROFILE), "w") as f:
        json.dump(rec, f, indent=1)
    print({k: rec[k] for k in ("reward_gain", "violation_drop")})
