"""The event pairs one call records (csrc/host_request.hip.inc: launch / timed / LaunchTimer): for every case of
tests/launch_event_cases.py the total and the count per EvKind equal tests/golden/launch_event_counts.json, which
tests/golden/make_launch_event_counts.py recorded before the launch sites were moved onto the shared helpers.  Counts are integers:
there is no tolerance.  DM_DFM_TIME_LAUNCHES, DM_DR_TIME_LAUNCHES and DM_LONG_PIPELINE are read per call, so both states of a switch
run in this one process."""
import json
import os

import pytest

import launch_event_cases as LC

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_event_counts.json")))


@pytest.fixture(scope="module")
def models():
    m = LC.Models()
    yield m
    m.close()


def test_the_golden_file_has_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(LC.CASES)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_event_pairs_of_one_call(models, monkeypatch, name):
    got = LC.measure(models, name, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    print(name, got)
    assert got == GOLDEN[name]


@pytest.mark.parametrize("name", [n for n in sorted(LC.CASES) if n.startswith("dfm-") and not n.endswith("-timed")])
def test_deepfm_training_kinds_are_silent_without_the_switch(name):
    assert not any(str(k) in GOLDEN[name] for k in range(70, 77))


@pytest.mark.parametrize("name", [n for n in sorted(LC.CASES) if n.startswith("dr-") and not n.endswith("-timed")])
def test_deep_retrieval_kinds_are_silent_without_the_switch(name):
    assert not any(str(k) in GOLDEN[name] for k in list(range(10, 30)) + list(range(50, 56)) + list(range(60, 68)) + list(range(80, 89)))
