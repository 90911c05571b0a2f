#!/usr/bin/env python3
"""How long must a stall be for a dropped wait to show?  The sweep behind STALL_USEC of tests/test_gpu_stall.py.

For each stall length the four controls of that module (one droppable wait dropped each: the door must return wrong bytes) run
in 5 fresh processes, one after the other.  A control that is not caught fails its test, so a run's outcome is read from pytest's
report.  The value to use is four times the smallest length at which all four controls were caught in all 5 runs (the headroom is
for a busy shared card, where the host's enqueue gaps widen).  Prints the table that profiles/stall_sensitivity.txt records.
Wrong bytes are the controls' purpose, never a fault; a child that ends in any other way than pass / fail stops the sweep."""
import os
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
LENGTHS, RUNS = (100, 300, 1000, 3000), 5
CONTROLS = ("batch_group", "chunk_band", "display_band", "copy_to_host")


def one_run(usec):
    env = dict(os.environ, S2SR_TEST_STALL_USEC=str(usec))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_stall.py", "-q", "-p", "no:cacheprovider", "-k", "test_control", "-rf"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=180)
    if r.returncode not in (0, 1):
        print(r.stdout[-3000:], r.stderr[-3000:])
        raise SystemExit(f"a control run ended with status {r.returncode}: the sweep stops here")
    missed = set(re.findall(r"FAILED \S+::test_control_(\w+?)_wait", r.stdout))
    if r.returncode == 1 and not missed:
        print(r.stdout[-3000:])
        raise SystemExit("a control run failed in a way this script does not know")
    return {c: c not in missed for c in CONTROLS}


def main():
    print(f"{'stall us':>8}  " + "  ".join(f"{c:>13}" for c in CONTROLS) + "   (runs of 5 in which the dropped wait was caught)")
    good = []
    for usec in LENGTHS:
        caught = dict.fromkeys(CONTROLS, 0)
        for _ in range(RUNS):
            for c, ok in one_run(usec).items():
                caught[c] += ok
        print(f"{usec:>8}  " + "  ".join(f"{caught[c]:>13}" for c in CONTROLS), flush=True)
        if all(v == RUNS for v in caught.values()):
            good.append(usec)
    if good:
        print(f"smallest length at which every control was caught in every run: {good[0]} us; STALL_USEC = 4 x {good[0]} = {4 * good[0]}")
    else:
        print("no length caught every control in every run")


if __name__ == "__main__":
    main()
