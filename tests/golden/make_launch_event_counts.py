#!/usr/bin/env python3
"""Writes tests/golden/launch_event_counts.json: for every case of tests/launch_event_cases.py, the event pairs one call records, in
total and per EvKind — what tests/test_gpu_launch_events.py holds the library to.  Needs the device; uses the public Engine API only.

The counts are a property of the host code's launch sites, not of the arithmetic: run this on the commit whose behaviour is to be kept,
commit the file unchanged, and a later change of the host code must reproduce it exactly."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import launch_event_cases as LC  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "launch_event_counts.json")


def main():
    models = LC.Models()
    try:
        out = {name: LC.measure(models, name, os.environ.__setitem__, lambda k: os.environ.pop(k, None)) for name in LC.CASES}
    finally:
        models.close()
    for name, c in out.items():
        print("%-28s %s" % (name, c))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
