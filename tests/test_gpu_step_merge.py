"""Env step in three launches: catppo_rollout_defer_tail mode 2 - catppo_rollout_post records the step, the next
catppo_policy_step carries it (step_fwd_kernel: the normalised observation rows go straight into the forward's LDS tile,
the post step's bookkeeping runs behind the critic's value head) - against the separate launches, bit for bit.

All cases run in ONE child process (tests/step_merge_cases.py; both arms of a case in that same process) that starts
with the 32-row rollout window pinned open; each test below asserts its own case."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("step_merge") / "results.json")
    env = dict(os.environ, CATPPO_FUSED_FWD_MIN_ROWS="17", CATPPO_FUSED_FWD_MAX_ROWS="4096", CATPPO_STEP16_FWD="0",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "constraints-as-terminations_amd"), HERE]))
    for k in ("CATPPO_STEP_MERGE", "CATPPO_ROLLOUT_DEFER_TAIL", "CATPPO_ROWS_FWD_ROLLOUT", "CATPPO_FUSED_ROLLOUT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "step_merge_cases.py"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["__process__"] = "ok" if r.returncode == 0 else (r.stdout[-2000:] + r.stderr[-4000:])
    return res


def _check(results, name):
    assert results["__process__"] == "ok" or name in results, results["__process__"]
    assert results.get(name) == "ok", results.get(name, results["__process__"])


@pytest.mark.parametrize("noise", ["eps", "philox"])
@pytest.mark.parametrize("rows", [33, 64, 300, 4096])
def test_four_env_steps_merged_equal_separate_launches_bitwise(results, rows, noise):
    """four env steps of the six-term Solo12 config, max_episode_length 2 (time-outs and resets in every tile): obs,
    actions, logprobs, values, rewards, dones, true_dones, normaliser mean / var / count, CaT running maxima, episode
    sums and lengths and the packed log, compared around every step; 33 rows = a ragged second tile"""
    _check(results, f"steps_{rows}_{noise}")


def test_full_iteration_64x24_identical_parameters(results):
    _check(results, "iteration")


def test_batch_outside_the_window_falls_back_and_flushes(results):
    _check(results, "outside_window")


def test_policy_step_on_other_rows_flushes_the_recorded_step(results):
    _check(results, "other_rows")


def test_state_is_current_for_a_checkpoint_after_an_armed_rollout(results):
    _check(results, "checkpoint")
