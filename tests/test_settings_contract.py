"""The settings of the C ABI (rfwhip_set_setting / rfwhip_get_setting / rfwhip_get_settings, include/rfwhip.h), CPU tier: the
host-emulation library answers every probe of tests/golden/make_settings_contract.py exactly as the recorded fixture
tests/golden/settings_contract.json does — listed keys and their order, defaults, return codes, error texts, parse quirks and
print formats.  Strings and integers: no tolerance."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_settings_contract", os.path.join(GOLDEN, "make_settings_contract.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
with open(os.path.join(GOLDEN, "settings_contract.json")) as _f:
    WANT = json.load(_f)
KEYS = WANT["created"]["keys"] + G.UNLISTED


@pytest.fixture(scope="module")
def lib(emu_lib):
    G.declare(emu_lib)
    return emu_lib


def test_the_fixture_holds_the_probes_of_the_generator():
    assert WANT["values"] == G.VALUES and len(WANT["created"]["keys"]) == 31
    for state in G.STATES:
        assert WANT[state]["keys"] == WANT["created"]["keys"]
        assert list(WANT[state]["defaults"]) == KEYS and list(WANT[state]["sets"]) == KEYS
        assert all(len(rows) == len(G.VALUES) for rows in WANT[state]["sets"].values())


@pytest.mark.parametrize("state", G.STATES)
def test_listed_keys(lib, state):
    assert G.probe_keys(lib, state) == WANT[state]["keys"]


@pytest.mark.parametrize("state", G.STATES)
def test_defaults(lib, state):
    got = G.probe_defaults(lib, state, KEYS)
    for k in KEYS:
        assert got[k] == WANT[state]["defaults"][k], k


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("state", G.STATES)
def test_sets(lib, state, key):
    got = G.probe_sets(lib, state, key)
    for value, g, w in zip(G.VALUES, got, WANT[state]["sets"][key]):
        assert g == w, (key, value)
