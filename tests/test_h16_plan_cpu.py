"""The 16-bit convolution planners, on the CPU: mrcnn_conv2d_fwd_h16_plan, mrcnn_conv2d_wgrad_h16_plan and
mrcnn_conv2d_wgrad_h16_workspace of the built tree against tests/golden/h16_plan_table.json (rows and replay: h16_plan_rows.py).
The table was recorded from the launch code as it stood before planning and launching were separated, with a record in place of
every launch, so equality here is "launches what that code launched": kernel and template arguments, grid, block, tiles owned,
remainder launch, epilogue form, pixel splits, reduction, workspace and status, row by row."""
import json
import os

import pytest

import h16_plan_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "h16_plan_table.json")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def lib(lib_path):
    return R.load(lib_path)


@pytest.fixture
def switches(monkeypatch):
    """The environment switches unset for the test and back to what they were afterwards (replay sets the per-call ones per row;
    answers() puts the tuning keys back)."""
    for k in R.PER_CALL + R.ONCE:
        monkeypatch.setenv(k, "0")          # registers the variable: monkeypatch restores whatever was there
        monkeypatch.delenv(k)


def test_table_rows_are_the_rows_of_the_generator():
    """The committed table holds exactly the inputs h16_plan_rows.all_rows() states (answers aside)."""
    table = R.read_table(TABLE)
    answers = ("status", "plan", "wsq")
    assert [{k: v for k, v in r.items() if k not in answers} for r in table] == json.loads(json.dumps(R.all_rows()))


def test_plans_and_workspace_equal_the_table(lib_path, lib, switches):
    table = R.read_table(TABLE)
    assert len(table) >= 1500
    bad = []
    for r, (rc, plan, query) in zip(table, R.answers(lib_path, table, lib=lib)):
        op = r.get("op", "fwd")
        if rc != r["status"]:
            bad.append((r["name"], "status", rc, r["status"]))
        if query != r["wsq"]:
            bad.append((r["name"], "workspace query", query, r["wsq"]))
        for f, want in zip(R.FIELDS[op], r["plan"]) if rc == 0 and r["plan"] else ():
            if plan[f] != want:
                bad.append((r["name"], f, plan[f], want))
    assert not bad, "%d differences (row, field, got, table): %s" % (len(bad), bad[:12])


def test_table_covers_every_kernel_reduction_and_status():
    from caesar_mrcnn_amd import _hip
    table = R.read_table(TABLE)
    fwd = [r for r in table if r.get("op", "fwd") == "fwd" and r["plan"]]
    wgrad = [r for r in table if r.get("op") == "wgrad" and r["plan"]]
    F, W = R.FIELDS["fwd"].index, R.FIELDS["wgrad"].index
    assert {r["plan"][F("kernel")] for r in fwd} == set(range(len(_hip.H16_KERNELS)))
    P, S = _hip.H16_KERNELS.index("PHASE"), _hip.H16_KERNELS.index("SLAB")
    assert {(r["plan"][F("kernel")], r["plan"][F("zout")]) for r in fwd if r["plan"][F("kernel")] in (P, S)} == {(P, 0), (P, 1), (S, 0), (S, 1)}
    assert {r["plan"][F("kernel")] for r in fwd if r["plan"][F("rem_grid")]} == {P, S}
    assert {r["plan"][F("fused_ep")] for r in fwd} == {0, 1} and {r["plan"][F("ep_vec")] for r in fwd} == {0, 1}
    # the phased weight gradient asks for aligned slabs and dw: its reduction is always the 16-byte one
    T, PH = _hip.H16_WGRAD_KERNELS.index("TABLE"), _hip.H16_WGRAD_KERNELS.index("PHASE")
    SC, V = _hip.H16_REDUCTIONS.index("SCALAR"), _hip.H16_REDUCTIONS.index("VEC")
    assert {(r["plan"][W("kernel")], r["plan"][W("reduce")]) for r in wgrad} == {(T, SC), (T, V), (PH, V)}
    assert {r["plan"][W("xcd_order")] for r in wgrad} == {0, 1, 2}
    assert {r["status"] for r in table if r.get("op", "fwd") == "fwd"} == {0, -1, -4}
    assert {r["status"] for r in table if r.get("op") == "wgrad"} == {0, -1, -3}


def _gpu_plans(lib_path, lib):
    """{row name: (row, status, plan)} of the rows h16_plan_rows states for tests/test_h16_gpu.py's launches."""
    rows = R.gpu_case_rows()
    return {r["name"]: (r, rc, plan) for r, (rc, plan, _) in zip(rows, R.answers(lib_path, rows, lib=lib))}


def test_gpu_suite_reaches_every_kernel(lib_path, lib, switches):
    """Every kernel id is what at least one launch of test_h16_gpu.py takes under that test's switches (a combination the test
    skips does not count), so a moved threshold cannot leave a kernel without a numerical test unnoticed."""
    import test_h16_gpu as T
    from caesar_mrcnn_amd import _hip
    plans = _gpu_plans(lib_path, lib)
    skipped = set()
    for dn in ("f16", "bf16"):
        for tile in ("small", "big", "phase", "slab", "wave128"):
            for i, case in enumerate(T.H16_CASES):
                if _fwd_h16_skips(case, tile):
                    skipped |= {"gpu/fwd_h16/%d/%s/%s" % (i, tile, dn), "gpu/fwd_h16/%d/%s/%s/dgrad" % (i, tile, dn)}
        skipped.add("gpu/deconv/big/%s" % dn)
        for i, case in enumerate(T.WGRAD_H16_CASES):
            if _wgrad_h16_skips(case, "phase"):
                skipped.add("gpu/wgrad/%d/phase/%s" % (i, dn))
    assert {n for n in skipped if not n.endswith("/dgrad")} <= set(plans)        # (not every forward row has a data-gradient row)
    fwd, wgrad = {}, {}
    for name, (r, rc, plan) in plans.items():
        if name in skipped:
            continue
        assert rc == 0, name
        if r.get("op") == "wgrad":
            wgrad.setdefault((_hip.H16_WGRAD_KERNELS[plan["kernel"]], _hip.H16_REDUCTIONS[plan["reduce"]]), []).append(name)
        else:
            fwd.setdefault(_hip.H16_KERNELS[plan["kernel"]], []).append(name)
            if plan["rem_grid"]:
                fwd.setdefault("remainder", []).append(name)
    assert set(fwd) == set(_hip.H16_KERNELS) - {"RING"} | {"remainder"}, {k: v[:2] for k, v in fwd.items()}     # the 3-slot ring has no test
    assert set(wgrad) == {("TABLE", "VEC"), ("PHASE", "VEC")}, {k: v[:2] for k, v in wgrad.items()}


def _fwd_h16_skips(case, tile):
    """test_conv_fwd_h16's skip conditions."""
    N, H, W, Cin, Cout, k, padding, act, bn = case
    if tile in ("big", "phase", "slab", "wave128") and (Cout % 256 or (tile in ("phase", "slab") and Cin % 64)):
        return True
    return tile == "slab" and not (k == 3 and padding == "same" and W <= 14 and Cin % 128 == 0)


def _wgrad_h16_skips(case, kernel):
    """test_conv_wgrad_h16's skip condition."""
    N, H, W, Cin, Cout, k, padding = case
    return bool(kernel == "phase" and (Cout % 256 or padding == "valid" and k > 1))


def test_skipped_gpu_combinations_would_not_take_the_named_kernel(lib_path, lib, switches):
    """The hand-written skip conditions of test_h16_gpu.py against the planner: a combination a test skips is one the planner
    would not send to the kernel the parameter names."""
    import test_h16_gpu as T
    from caesar_mrcnn_amd import _hip
    plans = _gpu_plans(lib_path, lib)
    named = {"big": ("BIG",), "phase": ("PHASE", "PHASE_DECONV"), "slab": ("SLAB",), "wave128": ("WAVE128",)}
    seen = 0
    for dn in ("f16", "bf16"):
        for tile in named:
            for i, case in enumerate(T.H16_CASES):
                if _fwd_h16_skips(case, tile):
                    r, rc, plan = plans["gpu/fwd_h16/%d/%s/%s" % (i, tile, dn)]
                    assert rc == 0 and _hip.H16_KERNELS[plan["kernel"]] not in named[tile], (case, tile, plan)
                    seen += 1
        # test_deconv_and_mask_output_stage_h16's skip is of another kind: MRCNN_H16_TILE=big DOES send the deconvolution to the
        # 4-stage ring kernel (so did the launch code the table was recorded from), which has no pixel-shuffle store -- the skip
        # hides a wrong result under an A/B switch, not a shape the selector declines.  Stated here so that it is known; the rule
        # goes with the ring kernel itself.
        r, rc, plan = plans["gpu/deconv/big/%s" % dn]
        assert rc == 0 and _hip.H16_KERNELS[plan["kernel"]] == "BIG"
        for tile, want in (("small", "T128"), ("phase", "PHASE_DECONV"), ("slab", "PHASE_DECONV"), ("wave128", "T128")):
            assert _hip.H16_KERNELS[plans["gpu/deconv/%s/%s" % (tile, dn)][2]["kernel"]] == want
        for i, case in enumerate(T.WGRAD_H16_CASES):
            r, rc, plan = plans["gpu/wgrad/%d/phase/%s" % (i, dn)]
            assert rc == 0 and (_hip.H16_WGRAD_KERNELS[plan["kernel"]] == "PHASE") == (not _wgrad_h16_skips(case, "phase")), (case, plan)
            r, rc, plan = plans["gpu/wgrad/%d/table/%s" % (i, dn)]
            assert rc == 0 and _hip.H16_WGRAD_KERNELS[plan["kernel"]] == "TABLE"
    assert seen == 2 * 9          # per type: Cout = 128 on four tiles, Cin = 32 on two, the slab on 7 x 7, 1 x 1 and Cin = 64


def test_ops_plan_wrappers(lib):
    """The thin wrappers on the mask head's layer (2048 ROIs): the phased kernel owns the six full rounds of 256 tiles, the small
    tile takes the 32 left; its weight gradient is the phased one.  Neither query is taped."""
    import torch
    from caesar_mrcnn_amd import _hip, ops
    d = ops.conv_desc((2048, 14, 14, 256), (3, 3, 256, 256), 1, "same", act=1)
    tape = _hip.tape_begin()
    try:
        rc, plan = ops.conv2d_h16_plan(d, torch.bfloat16, bias=32, scale=48, shift=64, z_out=80)
        rcw, wplan = ops.conv2d_wgrad_h16_plan(d)
    finally:
        _hip.tape_end()
    assert tape == [] and rc == 0 and rcw == 0
    M = 2048 * 14 * 14
    assert (_hip.H16_KERNELS[plan.kernel], plan.zout, plan.grid, plan.threads, plan.ptiles) == ("PHASE", 1, 256, 512, 6 * 256)
    assert plan.ptiles % 256 == 0 and plan.rem_mtile0 == plan.ptiles * 4 and plan.rem_grid == (M // 64 - plan.rem_mtile0) * (256 // 64) > 0
    assert (_hip.H16_WGRAD_KERNELS[wplan.kernel], _hip.H16_REDUCTIONS[wplan.reduce], wplan.itiles, wplan.ntiles) == ("PHASE", "VEC", 9, 1)
    assert wplan.grid == 9 * wplan.splits and wplan.chunk == 64 * wplan.nk and wplan.splits * wplan.chunk >= M
    assert ops.conv2d_h16_plan(d, x=20)[0] == -1 and ops.conv2d_wgrad_h16_plan(d, workspace_bytes=16)[0] == -3
