"""Records what the servo evaluation test is measured against: PPOOracle trained on the closed-loop numpy twin of the Solo12
servo surrogate (servo_twin.learning_cfgs()), its untrained and its trained deterministic policy evaluated with the eval
twin (tests/servo_eval_twin.py) on the fixed command grid and step count of servo_eval_twin.EVAL.  Runs on the CPU.

    python tools/servo_eval_oracle.py        ->  profiles/servo_eval_oracle.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "constraints-as-terminations_amd")):
    sys.path.insert(0, p)

import servo_eval_twin as E  # noqa: E402
import servo_twin as T  # noqa: E402

if __name__ == "__main__":
    before, after = E.run_oracle_eval_learning(log=print)
    rec = dict(T.LEARNING, hidden=list(T.LEARNING["hidden"]), task=T.TASK, eval=dict(E.EVAL, grid=list(E.EVAL["grid"])),
               constraints=["joint_torque", "foot_contact_force", "base_orientation"],
               untrained=before, trained=after, difference={k: (None if before[k] is None or after[k] is None
                                                               else after[k] - before[k]) for k in E.EVAL_KEYS},
               **E.eval_summary(before, after))
    with open(os.path.join(ROOT, E.EVAL_PROFILE), "w") as f:
        json.dump(rec, f, indent=1)
    print({k: rec[k] for k in ("reward_gain", "err_lin_drop")})
