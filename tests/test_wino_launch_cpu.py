"""What the Winograd host code of ops.py launches, on the CPU: every row of tests/golden/wino_launch_rows.json (cases, recorder and
replay: wino_launch_rows.py) replayed through the ops.py of the tree.  The table was written by the ops.py of the commit before
that host code was reshaped, so equality here is "issues what that code issued": the launches in order with their scalar
arguments, tile groups and descriptors, every pointer as (buffer, byte offset), the workspace and ops.empty requests in order,
and what the call returned."""
import os
import re

import pytest

import wino_launch_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wino_launch_rows.json")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from caesar_mrcnn_amd import _hip
    return _hip.lib()


def test_launches_equal_the_table(lib, monkeypatch):
    from caesar_mrcnn_amd import _hip, ops
    table = R.read_table(TABLE)
    cases = R.all_cases()
    assert [r["name"] for r in table] == [c["name"] for c in cases] and len(cases) >= 100
    bad = []
    for c, want in zip(cases, table):
        with monkeypatch.context() as m:
            events, returned = R.record(c, m, ops, _hip)
        if returned != want["returned"]:
            bad.append((c["name"], "returned", returned, want["returned"]))
        if len(events) != len(want["events"]):
            bad.append((c["name"], "events", [e[0] for e in events], [e[0] for e in want["events"]]))
        for k, (got, exp) in enumerate(zip(events, want["events"])):
            if got != exp:
                fields = [(i, g, w) for i, (g, w) in enumerate(zip(got, exp)) if g != w][:4] if len(got) == len(exp) else (got, exp)
                bad.append((c["name"], "event %d (%s)" % (k, exp[0]), fields))
                break
    assert not bad, "%d differences (row, what, got, table): %s" % (len(bad), bad[:6])


def test_table_covers_every_entry_status_and_tiling():
    """Every launching mrcnn_winograd_* entry ops.py names is in some row; the two one-launch entries are there accepted and
    refused; each of the five functions is there under each tiling; the refused shared weight-gradient launch goes one by one."""
    from caesar_mrcnn_amd import _hip
    table = R.read_table(TABLE)
    src = open(os.path.join(ROOT, "caesar-mrcnn_amd", "ops.py")).read()
    called = {n for n in re.findall(r"\.(mrcnn_winograd_\w+)\(", src) if not any(k in n for k in _hip._NO_RECORD)}
    assert len(called) >= 11, called
    launches = [(r["name"], e) for r in table for e in r["events"] if e[0].startswith("mrcnn_")]
    assert called <= {e[0] for _, e in launches}, called - {e[0] for _, e in launches}
    for entry in ("mrcnn_winograd_chain", "mrcnn_winograd_bwd_chain"):
        assert {e[1] for _, e in launches if e[0] == entry} == {0, R.UNSUPPORTED}, entry
    assert {e[1] for _, e in launches if e[0] == "mrcnn_conv2d_wgrad_multi"} == {0, R.UNSUPPORTED}
    assert {len(e[2]) - 1 for _, e in launches if e[0] == "mrcnn_conv2d_wgrad_multi"} == {16, 12}       # GEMMs per launch
    assert any(e[0] == "mrcnn_conv2d_wgrad" for _, e in launches)
    for fn in R.FUNCTIONS:
        assert {int(r["name"].split("/")[2][5:]) for r in table if r["name"].startswith(fn + "/")} == set(R.TILES), fn
    # the chain form requested without the mask from z never asks the one-launch entry
    rows = [r for r in table if "/chain_without_zmask" in r["name"]]
    assert len(rows) == 2 and not any(e[0] == "mrcnn_winograd_bwd_chain" for r in rows for e in r["events"])
    # pointers into the middle of a buffer: Mt of a stacked product, V, the channel-sum partials
    offsets = {e[0]: set() for _, e in launches}
    for _, e in launches:
        offsets[e[0]].update(a.split("+")[0] for a in e[2:] if isinstance(a, str) and not a.endswith("+0"))
    assert "ws:winograd_m" in offsets["mrcnn_winograd_output_g"] and "ws:winograd_m" in offsets["mrcnn_winograd_gemm"]
    assert "ws:winograd_bwd_sums" in offsets["mrcnn_winograd_output_bwd_zmask_g"] | offsets["mrcnn_winograd_output_bwd_g"]
    assert {"next_v", "ws:winograd_v", "keep_v"} <= offsets["mrcnn_winograd_input_g"] and "next_dm" in offsets["mrcnn_winograd_dy_g"]
