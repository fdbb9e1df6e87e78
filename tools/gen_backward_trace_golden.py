#!/usr/bin/env python3
"""Writes tests/golden/backward_launch_trace.json: the launch schedule (C entry, stream role, ngroups of a weight-gradient launch) of
every case of tests/backward_trace_cases.py, as the current tree issues it.  tests/test_gpu_backward_trace.py holds the autograd layer to
it.  Runs on the GPU.  Regenerate it in a change that alters the schedule ON PURPOSE, and say so there."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import backward_trace_cases as B
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "backward_launch_trace.json")
    traces = {name: B.record(name)[0] for name in B.CASES}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(t)}" for n, t in traces.items()) + "\n}\n")
    print(out, os.path.getsize(out), "bytes;", {n: len(t) for n, t in traces.items()})


if __name__ == "__main__":
    main()
