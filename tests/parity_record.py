"""Achieved parity errors of the config-size GPU tests (the whole-iteration tests printed their errors and
threw them away).  One entry per test name: max abs errors per tensor, sizes, seed.  The file is merged, not overwritten,
so one pytest run (or several) accumulate into it.  By default it is parity_out/parity.json at the repository root
(git-ignored: a test run leaves the tree clean); CATPPO_PARITY_RECORD=<path> writes elsewhere, e.g. the committed
profiles/r6_parity.json when a round's record is refreshed on purpose."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = [os.path.abspath(os.environ.get("CATPPO_PARITY_RECORD") or os.path.join(ROOT, "parity_out", "parity.json"))]


def record(name, errors, sizes=None, seed=None, note=None):
    def num(v):
        return v if isinstance(v, (list, str)) or v is None else float(v)
    entry = {"errors": {k: num(v) for k, v in errors.items()}, "sizes": sizes, "seed": seed}
    if note:
        entry["note"] = note
    for path in PATHS:
        try:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            data = {}
            if os.path.exists(path):
                with open(path) as f:
                    data = json.load(f)
            data[name] = entry
            with open(path, "w") as f:
                json.dump(data, f, indent=1, sort_keys=True)
        except OSError:
            pass
    return entry
