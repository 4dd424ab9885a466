"""GPU: repeated whole-program runs across service-thread counts, worker counts and the MEG stage on/off -- a bit-exact product must give the reference's files EVERY time.  tools/stress_parity.py does the
work and, on a mismatch, keeps what is needed to bisect it under gpurun_out/stress_test/ (both sides' files,
a diff, the environment, PINTRON_VERBOSE output, and the verdict of replaying the run's DP requests through
the oracle).  Round 2 saw one unexplained mismatch of the long-transcript input in eleven suite runs; this
test is the standing watch for it (36 runs of that input + 12 of the C3 sample per suite run; the tool's
full matrix -- 360 + 120 runs -- is in profiles/r03_stress_summary.json)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_repeated_runs_are_always_identical_to_the_reference(tmp_path):
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "est-fact-core")):
        pytest.skip("oracle/_ref/est-fact-core not present")
    import __graft_entry__ as g
    g.build()
    out = os.path.join(ROOT, "gpurun_out", "stress_test")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_parity.py"), "--long", "3", "--c3", "1", "--c3-ests", "1500",
                        "--poison", "255,165,0", "--out", out], capture_output=True, text=True, timeout=1500)
    summary = json.load(open(os.path.join(out, "summary.json")))
    runs = {x["input"]: (x["runs"], x["mismatches"]) for x in summary["results"]}
    assert r.returncode == 0 and runs["long"] == (36, 0) and runs["c3"] == (12, 0), (runs, r.stdout[-3000:])
