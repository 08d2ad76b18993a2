"""The UNet's host layer makes the calls it made when tests/golden/unet_walk.json was recorded: same C-ABI symbols in the same order with the
same arguments, null pointers and layer tags, no pack call in a second step, and bitwise the same output (tests/walk_recorder.py,
tests/golden/make_unet_walk.py)."""
import json

import pytest

import walk_recorder as wr
from pathlib import Path

pytestmark = pytest.mark.gpu

CONFIGS = wr.configs()


@pytest.fixture(scope="module")
def fixture():
    return json.loads((Path(__file__).resolve().parent / "golden" / "unet_walk.json").read_text())


def test_fixture_covers_every_configuration(fixture):
    assert sorted(fixture) == sorted(CONFIGS)
    assert all(v["digest"] is not None for v in fixture.values()), "every output was bitwise repeatable when the fixture was recorded"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_walk(fixture, name):
    want = fixture[name]
    got = wr.record(CONFIGS[name])
    second = got["trace"][got["trace"].index("--") + 1:]
    assert second and not [c for c in second if "pack" in c.split("|")[1]], "the second step packed weights again"
    assert got["trace"] == want["trace"]
    assert got["digest"] == want["digest"]
