"""GPU: which check refuses a call of the list reductions -- gat_list_* and gat_sample_* of gat-distance, gat-local, gat-pairs,
gat-geneset and gat-profile -- when one argument is wrong, and which one wins when two are (tests/list_call_refusal_cases.py).
The return code and the whole text of gat_last_error are those recorded from the commit before these entry points were folded
into shared frames (tests/golden/list_call_refusals.json); a refused call, and one with nothing to write, leaves a
sentinel-filled out_host alone; and the same call with valid arguments succeeds behind it."""
import json

import pytest

import list_call_refusal_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    e = R.Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def recorded():
    with open(R.GOLDEN) as f:
        return json.load(f)["cases"]


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(c.id for c in R.CASES)
    assert set(R.SIGNATURES) == {c.entry for c in R.CASES} and len(R.SIGNATURES) == 10
    for c in R.CASES:
        assert (recorded[c.id]["rc"] == 0) == c.ok, c.id
    assert all(c.id.split("-", 1)[1].startswith("nothing-") for c in R.CASES if c.ok)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_refusal(env, recorded, case):
    want = recorded[case.id]
    rc, text, out = env.run(case)
    assert rc == want["rc"], (rc, text, want)
    if not case.ok:
        assert rc != 0 and text == want["error"]
    assert (out == R.SENTINEL).all()
    assert env.call(case.entry, {}) == 0, env.L.gat_last_error(env.ctx._h)
    assert (env.out != R.SENTINEL).any()                    # (the valid call does write)
