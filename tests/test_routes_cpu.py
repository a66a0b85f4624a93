"""CPU: the kernel family the library chooses for a descriptor, pinned against tests/golden/routes.json.

The table was recorded (tests/golden/make_routes.py) from a build of the commit named in it, before conv_route /
wgrad_route single-sourced the choice; the query entry points launch nothing and dereference no device pointer, so
the library as built must give the same variant name, stats rows, workspace bytes and act_out answer for every
recorded descriptor and environment.
"""

import importlib.util
import json
from collections import Counter
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"


def _make_routes():
    spec = importlib.util.spec_from_file_location("make_routes", GOLDEN / "make_routes.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    return json.loads((GOLDEN / "routes.json").read_text())


@pytest.fixture(scope="module")
def routes():
    M = _make_routes()
    path = M.L.library_path()
    assert path.exists(), "libunet_hip.so not built (run __graft_entry__.build())"
    return M, M.bind(path)


def test_table_covers_every_path(table):
    M = _make_routes()
    assert len(table["commit"]) >= 7
    assert table["envs"] == M.ENVS and [tuple(s) for s in table["shapes"]] == M.SHAPES
    v = table["variants"]
    conv = Counter(M.conv_path(v[c[9]]) for c in table["conv"])
    wgrad = Counter(M.wgrad_path(v[c[6]]) for c in table["wgrad"])
    for p in ("smallcin", "pw", "generic", "conv5w", "conv5", "conv5_splitk", "conv3", "conv2"):
        assert conv[p] >= 10, (p, conv)
    for p in ("smallcin", "pw", "wgrad5", "wgrad2", "wgrad"):
        assert wgrad[p] >= 10, (p, wgrad)
    used = {v[c[9]] for c in table["conv"]}
    assert any("+splitk" in s for s in used)
    assert any(s.startswith("conv5w_kernel<") and s.endswith(",4>") for s in used)
    assert any(s.startswith("conv5_kernel<") and s.endswith(",2>") for s in used)
    # every dtype, kernel size, shape, channel count, switch setting and descriptor state of the grid is in the table
    chans = {1, 3, 16, 20, 32, 48, 64, 128, 256, 512, 1024}
    for key in ("conv", "wgrad"):
        assert {c[1] for c in table[key]} == {M.L.F32, M.L.BF16, M.L.F16} and {c[2] for c in table[key]} == {1, 3}
        assert {c[3] for c in table[key]} == set(range(len(M.SHAPES)))
        assert chans <= {c[4] for c in table[key]} and chans <= {sum(s[1] for s in c[5]) for c in table[key]}
    assert any(len(c[5]) == 2 and c[5][0][1] % 16 for c in table["conv"])
    assert any(len(c[5]) == 2 and c[5][0][1] % 32 and not c[5][0][1] % 16 for c in table["conv"])
    assert {c[0] for c in table["conv"]} == set(M.CONV_ENVS) and {c[0] for c in table["wgrad"]} == set(M.WGRAD_ENVS)
    assert {c[7] for c in table["conv"]} == {0, 1} and {c[8] for c in table["conv"]} == {0, 1}
    assert {c[6] for c in table["conv"]} == {"y", "ys", "yb", "f", "fs", "fsa", "p", "s2", "fg"}
    assert {(s[0], s[2]) for c in table["conv"] for s in c[5]} == {(k, g) for k in M.KINDS for g in (0, 1)}


def _compare(M, table, key, ncase, query, monkeypatch):
    v = table["variants"]
    bad = []
    for env in range(len(table["envs"])):
        M.set_env(table["envs"][env], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
        for rec in table[key]:
            if rec[0] != env:
                continue
            want = [v[rec[ncase]]] + rec[ncase + 1:]
            got = query(rec[:ncase])
            if got != want:
                bad.append((table["envs"][env], rec[:ncase], want, got))
    assert not bad, f"{len(bad)} of {len(table[key])} routes differ from {table['commit']}; first: {bad[:5]}"


def test_conv_routes_match_parent(table, routes, monkeypatch):
    M, so = routes
    _compare(M, table, "conv", 9, lambda c: M.query_conv(so, c), monkeypatch)


def test_wgrad_routes_match_parent(table, routes, monkeypatch):
    M, so = routes
    _compare(M, table, "wgrad", 6, lambda c: M.query_wgrad(so, c), monkeypatch)
