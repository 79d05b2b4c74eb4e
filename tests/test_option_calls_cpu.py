"""The option wrappers against their record (tests/golden/option_calls.json, tests/option_calls_ref.py): every case hands SelfPlayEngine,
arena_batch and the device replay buffer the arguments it handed them on the recorded commit, makes the same later calls, returns the same
shape, leaves the same function attributes and refuses with the same exception and text; the real SelfPlayEngine makes the same
oz_selfplay_* calls in the same order.  No GPU, no library."""
import json
import os

import pytest

import option_calls_ref as ref

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "option_calls.json")) as _f:
    GOLDEN = json.load(_f)
CASES = ref.cases()


def test_the_record_holds_every_case():
    assert len(GOLDEN["commit"]) == 40 and sorted(GOLDEN["cases"]) == sorted(case for case, _, _ in CASES)
    refused = [case for case, t in GOLDEN["cases"].items() if "raised" in t]
    for group, prefix in ((ref.REFUSALS, "selfplay_batch-"), (ref.BATCH_REFUSALS, "selfplay_batch-"), (ref.TRAINING_REFUSALS, "training-")):
        assert all(prefix + name in refused for name in group), [name for name in group if prefix + name not in refused]
    assert all(GOLDEN["cases"][c]["raised"][0] == "ValueError" for c in refused), {c: GOLDEN["cases"][c]["raised"] for c in refused}


@pytest.mark.parametrize("case,target,kw", CASES, ids=[c[0] for c in CASES])
def test_option_calls(case, target, kw):
    got = json.loads(json.dumps(ref.run_case(target, kw)))
    want = GOLDEN["cases"][case]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for part in sorted(want):
        if part == "calls":
            assert len(got["calls"]) == len(want["calls"]), ([c[0] for c in got["calls"]], [c[0] for c in want["calls"]])
            for g, w in zip(got["calls"], want["calls"]):
                assert g == w
        else:
            assert got[part] == want[part], part
