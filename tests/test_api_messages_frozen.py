"""The argument errors of the batched calls, held to a recording: tests/golden/api_messages.json is what the api.py of the commit
before the front end was taken apart into helpers answered to each bad call of tests/golden/make_api_messages.py -- exception
type, exact sentence, and a call counter that did not move.  A helper that rewords a sentence, reports the second of two failing
checks first, or opens a device before an argument error, fails here.  No GPU; `api.engine` raises, as in test_ragged_api.py."""
import importlib.util
import os

import pytest

from esac_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_api_messages", os.path.join(GOLDEN, "make_api_messages.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "api_messages.json")) as f:
    RECORDED = gen.load(f)   # {case id: "<exception type>: <sentence>"}
CASES = gen.cases(api)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(api, "engine", gen.no_device)
    state = api.get_rng_state()
    yield
    api.set_seed(*state)


def test_the_recording_holds_exactly_the_table():
    assert sorted(RECORDED) == sorted(cid for cid, _, _ in CASES)
    assert {cid.split(":")[0].partition("+")[0] for cid in RECORDED} == {
        "forward_batch", "forward_batch_async", "backward", "backward_batch", "backward_batch_async", "backward_batch_shapes",
        "backward_batch_shapes_async", "verify_batch", "eval_batch"}
    assert sum(" & " in cid for cid in RECORDED) > 500   # the pairs that pin which of two failing checks speaks first


@pytest.mark.parametrize("key", gen.KEYS)
def test_messages_types_and_counter_are_the_recorded_ones(no_device, key):
    wrong = []
    for cid, k, muts in CASES:
        if k != key:
            continue
        got, want = gen.run_case(api, k, muts), RECORDED[cid]
        same = gen.outcome(got) == want or (want.endswith(": *") and got["type"] == want[:-3])
        if got["call_moved"] != 0 or not same:
            wrong.append("%s\n    recorded: %s\n    now:      %s (counter moved by %d)" % (cid, want, gen.outcome(got), got["call_moved"]))
    assert not wrong, "%d case(s) differ from the recording:\n%s" % (len(wrong), "\n".join(wrong[:20]))
