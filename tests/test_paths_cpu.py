"""The conv dispatch table (csrc/conv_paths.hip): one mode per kernel family,
resolved from its environment variable when the library is loaded, changed by
vsrk_conv_set_path and read back by vsrk_conv_get_path.  Host only -- no
device calls."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from vsr_amd import _native

# name: (environment variable, mode when unset, largest settable mode)
TABLE = {
    "fast": ("VSRK_CONV_FAST", 1, 1),
    "pw": ("VSRK_CONV_PW", 1, 1),
    "pw_wide": ("VSRK_PW_WIDE", 1, 1),
    "roll": ("VSRK_CONV_ROLL", 2, 1),
    "roll_wr": ("VSRK_ROLL_WRES", 1, 2),
    "roll_fold": ("VSRK_ROLL_FOLD", 1, 1),
    "row": ("VSRK_CONV_ROW", -1, 1),
    "thin": ("VSRK_CONV_THIN", 1, 1),
    "stencil": ("VSRK_CONV_STENCIL", 1, 1),
    "wgrad_pipe": ("VSRK_WGRAD_PIPE", 1, 1),
    "wgrad_roll": ("VSRK_WGRAD_ROLL", 2, 1),
    "wgrad_row": ("VSRK_WGRAD_ROW", 1, 2),
}
NAMES = sorted(TABLE)


def get(lib, name):
    mode = C.c_int32(-99)
    assert lib.vsrk_conv_get_path(name.encode(), C.byref(mode)) == 0, lib.vsrk_last_error()
    return mode.value


def load_mode(name):
    """The mode the table rule gives this process's environment."""
    env, unset, _ = TABLE[name]
    v = os.environ.get(env)
    return unset if v is None else (0 if v.startswith("0") else 1)


# A fresh process that loads the library with ctypes only, applies the (name,
# mode) settings given as JSON and prints every path's mode.
_CHILD = """
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
for name, mode in json.loads(sys.argv[2]):
    assert lib.vsrk_conv_set_path(name.encode(), C.c_int32(mode)) == 0
out = {}
for name in json.loads(sys.argv[3]):
    m = C.c_int32(-99)
    assert lib.vsrk_conv_get_path(name.encode(), C.byref(m)) == 0
    out[name] = m.value
print(json.dumps(out))
"""


def child_modes(env_extra, sets=()):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VSRK_")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(_native.lib_path()), json.dumps(list(sets)),
                        json.dumps(NAMES)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def clean_modes(native):
    return child_modes({})


@pytest.mark.parametrize("name", NAMES)
def test_unset_default(clean_modes, name):
    assert clean_modes[name] == TABLE[name][1]


@pytest.mark.parametrize("name", NAMES)
def test_set_zero_and_restore(native, name):
    assert get(native, name) == load_mode(name)
    try:
        assert native.vsrk_conv_set_path(name.encode(), 0) == 0
        assert get(native, name) == 0
    finally:
        assert native.vsrk_conv_set_path(name.encode(), -1) == 0
    assert get(native, name) == load_mode(name)


@pytest.mark.parametrize("name", NAMES)
def test_mode_range(native, name):
    before = get(native, name)
    top = TABLE[name][2]
    assert top == (2 if name in ("roll_wr", "wgrad_row") else 1)
    for bad in [-2, 3] + ([2] if top == 1 else []):
        assert native.vsrk_conv_set_path(name.encode(), bad) != 0, (name, bad)
        assert name in native.vsrk_last_error().decode()
        assert get(native, name) == before
    try:
        assert native.vsrk_conv_set_path(name.encode(), top) == 0
        assert get(native, name) == top
    finally:
        assert native.vsrk_conv_set_path(name.encode(), -1) == 0
    assert get(native, name) == before


def test_unknown_name_lists_the_table(native):
    mode = C.c_int32(7)
    for rc in (native.vsrk_conv_set_path(b"rolled", 1), native.vsrk_conv_get_path(b"rolled", C.byref(mode))):
        assert rc != 0
        text = native.vsrk_last_error().decode()
        assert "rolled" in text
        listed = [s.strip() for s in text[text.rindex("(") + 1:text.rindex(")")].split(",")]
        assert sorted(listed) == NAMES
    assert mode.value == 7


def test_set_algo_is_path_fast(native):
    try:
        assert native.vsrk_conv_set_algo(0) == 0
        assert get(native, "fast") == 0
        assert native.vsrk_conv_set_algo(2) != 0
        assert get(native, "fast") == 0
    finally:
        assert native.vsrk_conv_set_algo(-1) == 0
    assert get(native, "fast") == load_mode("fast")


def test_environment_is_read_at_load(native):
    env = {"VSRK_CONV_ROLL": "0", "VSRK_CONV_ROW": "1", "VSRK_WGRAD_ROW": "0", "VSRK_ROLL_WRES": "0"}
    want = {"roll": 0, "row": 1, "wgrad_row": 0, "roll_wr": 0, "wgrad_roll": 2, "roll_fold": 1}
    for sets in ((), (("row", 0), ("row", -1))):
        got = child_modes(env, sets)
        assert {k: got[k] for k in want} == want, sets
    assert child_modes(env, (("row", 0),))["row"] == 0
