"""Makes tests/golden/option_calls.json: the trace of every case of tests/option_calls_ref.py -- what selfplay_batch, the loop and the match
wrappers hand to SelfPlayEngine / arena_batch / the device replay buffer, what they return and what they refuse -- on the commit checked
out when it runs, whose hash goes into the file.  It was run on the last commit before the wrappers' option handling was folded into
_lib.check_search_options / check_selfplay_options / search_kw / engine_kw and SelfPlayEngine.option_stats; run it again only on a commit
whose behaviour is to become the new record:  python tests/golden/gen_option_calls.py
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    import option_calls_ref as ref
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True, check=True).stdout.strip()
    traces = {case: ref.run_case(target, kw) for case, target, kw in ref.cases()}
    out = os.path.join(HERE, "option_calls.json")
    with open(out, "w") as f:
        json.dump(dict(commit=commit, cases=traces), f, sort_keys=True, separators=(",", ":"))
    print(out, os.path.getsize(out), "bytes,", len(traces), "cases,", sum("raised" in t for t in traces.values()), "refusals")
