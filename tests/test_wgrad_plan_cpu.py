"""The float32 weight-gradient planner, on the CPU: mrcnn_conv2d_wgrad_plan, mrcnn_conv2d_wgrad_multi_plan and the two workspace
queries of the built tree against tests/golden/wgrad_plan_table.json (rows and replay: wgrad_plan_rows.py).  The table was recorded
from the launch code as it stood before planning and launching were separated, with a record in place of every launch, so equality
here is "launches what that code launched": kernel and tile shape, grid, dynamic LDS, pixel splits, pixel table, reduction, slab
offsets, block prefixes, workspace and status, row by row."""
import json
import os
import subprocess
import sys

import pytest

import wgrad_plan_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_plan_table.json")


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as ge
    return ge.build()


@pytest.fixture(scope="module")
def lib(lib_path):
    return R.load(lib_path)


@pytest.fixture
def flat_off(monkeypatch):
    """MRCNN_CONV_FLAT_GLDS unset for the test (the library of this process read it when it first planned a launch) and back to
    what it was afterwards."""
    monkeypatch.setenv("MRCNN_CONV_FLAT_GLDS", "1")         # registers the variable: monkeypatch restores whatever was there
    monkeypatch.delenv("MRCNN_CONV_FLAT_GLDS")


def test_table_rows_are_the_rows_of_the_generator():
    """The committed table holds exactly the inputs wgrad_plan_rows.all_rows() states (answers aside)."""
    table = R.read_table(TABLE)
    answers = ("status", "plan", "wsq")
    assert [{k: v for k, v in r.items() if k not in answers} for r in table] == json.loads(json.dumps(R.all_rows()))


def test_plans_and_workspace_equal_the_table(lib_path, lib, flat_off):
    table = R.read_table(TABLE)
    assert len(table) >= 635
    bad = []
    for r, (rc, plan, query) in zip(table, R.answers(lib_path, table, lib=lib)):
        op = r.get("op", "single")
        if rc != r["status"]:
            bad.append((r["name"], "status", rc, r["status"]))
        if query != r["wsq"]:
            bad.append((r["name"], "workspace query", query, r["wsq"]))
        for f, want in zip(R.FIELDS[op], r["plan"]) if rc == 0 and r["plan"] else ():
            if plan[f] != want:
                bad.append((r["name"], f, plan[f], want))
    assert not bad, "%d differences (row, field, got, table): %s" % (len(bad), bad[:12])


def test_table_covers_every_kernel_with_every_reduction_and_every_status():
    """Any of the four kernels can run with one split (no reduction), with the 16-byte reduction or -- dw or the workspace
    misaligned, or KH*KW*Cin*Cout % 4 != 0 -- the scalar one."""
    from caesar_mrcnn_amd import _hip
    table = R.read_table(TABLE)
    S = R.FIELDS["single"].index
    single = [r for r in table if r.get("op", "single") == "single"]
    multi = [r for r in table if r.get("op") == "multi"]
    seen = {(r["plan"][S("kernel")], r["plan"][S("reduce")]) for r in single if r["plan"]}
    assert seen == {(k, d) for k in range(len(_hip.WGRAD_KERNELS)) for d in range(len(_hip.WGRAD_REDUCTIONS))}
    tiles = {(r["plan"][S("bi")], r["plan"][S("bn")], r["plan"][S("fast")]) for r in single if r["plan"] and r["plan"][S("kernel")] == 0}
    assert tiles == {(128, 128, 1), (128, 64, 1), (128, 32, 1), (64, 128, 1), (64, 64, 1), (64, 32, 1), (64, 128, 0), (64, 64, 0), (64, 32, 0)}
    M = R.FIELDS["multi"].index
    assert {r["plan"][M("reduce_grid")] > 0 for r in multi if r["plan"]} == {False, True}
    assert {len(r["desc"]) for r in multi if r["plan"]} >= {1, 2, 3, 4, 12, 16}
    assert {r["status"] for r in single} == {0, -1, -3}
    assert {r["status"] for r in multi} == {0, -1, -3, -4}
    # the flat switch: the LDS-DMA shapes go to the flat kernel, the shared launch refuses while its query still answers
    flat = [r for r in table if r.get("flat")]
    assert {r["plan"][S("kernel")] for r in flat if r.get("op", "single") == "single" and r["plan"]} == {0, 3}
    assert {(r["status"], r["wsq"] > 0) for r in flat if r.get("op") == "multi"} == {(-4, True), (-4, False)}


def test_ops_plan_wrappers(lib):
    """The thin wrappers: the mask head's 3 x 3 layer (2048 ROIs) takes the LDS-DMA kernel through the pixel table with the 16-byte
    reduction; res4's block as engine.wgrad_group forms it is one launch of 16 + 36 + 16 tiles; neither query is taped."""
    from caesar_mrcnn_amd import _hip, ops
    d = ops.conv_desc((2048, 14, 14, 256), (3, 3, 256, 256), 1, "same")
    block = [ops.conv_desc((4, 16, 16, 256), (1, 1, 256, 1024), 1, "valid"), ops.conv_desc((4, 16, 16, 256), (3, 3, 256, 256), 1, "same"),
             ops.conv_desc((4, 16, 16, 1024), (1, 1, 1024, 256), 1, "valid")]
    tape = _hip.tape_begin()
    try:
        rc, plan = ops.conv2d_wgrad_plan(d)
        rcm, mplan = ops.conv2d_wgrad_multi_plan(block)
    finally:
        _hip.tape_end()
    assert tape == [] and rc == 0 and rcm == 0
    M = 2048 * 14 * 14
    assert (_hip.WGRAD_KERNELS[plan.kernel], _hip.WGRAD_REDUCTIONS[plan.reduce], plan.bi, plan.bn) == ("BLDS_TABLE", "VEC", 128, 128)
    assert plan.grid == 36 * plan.splits and plan.splits * plan.chunk >= M > (plan.splits - 1) * plan.chunk and plan.chunk % 32 == 0
    assert plan.table_grid == -(-(M + 16) // 256) and plan.workspace_bytes == plan.slab_bytes + plan.table_bytes
    assert _hip.WGRAD_KERNELS[ops.conv2d_wgrad_plan(d, workspace_bytes=plan.slab_bytes)[1].kernel] == "BLDS"
    assert ops.conv2d_wgrad_plan(d, workspace_bytes=plan.slab_bytes - 1)[0] == -3 and ops.conv2d_wgrad_plan(d, x=20)[0] == -1
    assert mplan.n == 3 and [mplan.first[g + 1] - mplan.first[g] for g in range(3)] == [t * s for t, s in zip((16, 36, 16), mplan.splits[:3])]
    assert mplan.grid == mplan.first[3] <= 1024 and mplan.workspace_bytes == mplan.slab_bytes + 256
    assert ops.conv2d_wgrad_multi_plan(block + [ops.conv_desc((4, 16, 16, 256), (1, 1, 256, 64), 1, "valid")])[0] == ops.ERR_UNSUPPORTED


def test_lds_pad_key_reaches_the_plan(lib):
    """The table was recorded with the tuning key at 0; the key is the dynamic LDS of the two buffer-addressed kernels only."""
    try:
        lib.mrcnn_tuning_set(b"wgrad_lds_pad", 4096)
        from caesar_mrcnn_amd import _hip
        got = {}
        for name, d in (("BLDS", R.gemm(1024, 128, 128)), ("BLDS_TABLE", R.wide(65536, 128, 128)), ("GLDS", R.gemm(4194288, 128, 128)), ("TILE", R.wide(1024, 64, 64))):
            plan = _hip.WgradPlan()
            desc = R._desc(R.pack_desc(d))
            import ctypes as C
            assert lib.mrcnn_conv2d_wgrad_plan(C.byref(desc), 16, 16, 16, 256, 1 << 40, C.byref(plan)) == 0 and _hip.WGRAD_KERNELS[plan.kernel] == name
            got[name] = plan.lds_bytes
        assert got == {"BLDS": 4096, "BLDS_TABLE": 4096, "GLDS": 0, "TILE": 0}
    finally:
        lib.mrcnn_tuning_set(b"wgrad_lds_pad", 0)


def _case_row(case):
    N, H, W, Cin, Cout, k, stride, padding = case
    return R.row("case", R.desc(N, H, W, Cin, Cout, k, stride, padding if isinstance(padding, str) else padding[0]))


def test_gpu_suites_reach_every_kernel(lib_path, lib, flat_off):
    """Every kernel id and each of the six conv_wgrad_kernel tile shapes is what at least one case of test_kernels_gpu's weight
    gradient tests launches (as ops.conv2d_wgrad calls: aligned tensors, the queried workspace or a larger one), so a moved
    threshold cannot leave a kernel without a numerical test unnoticed."""
    import test_kernels_gpu as T
    from caesar_mrcnn_amd import _hip
    S = R.FIELDS["single"].index
    reached, tiles, reductions = {}, {}, set()
    for case in T.WGRAD_CASES:
        for ws in ("query", 1 << 40):                         # ops.workspace only grows: a case may meet a larger buffer
            rc, plan, _ = R.replay(lib, dict(_case_row(case), ws=ws))
            assert rc == 0, case
            kernel = _hip.WGRAD_KERNELS[plan["kernel"]]
            reached.setdefault(kernel, []).append(case)
            reductions.add(_hip.WGRAD_REDUCTIONS[plan["reduce"]])
            if kernel == "TILE":
                tiles.setdefault((plan["bi"], plan["bn"]), []).append(case)
    assert set(tiles) == {(128, 128), (128, 64), (128, 32), (64, 128), (64, 64), (64, 32)}, {k: v[:2] for k, v in tiles.items()}
    # the two tile shapes that had no case, by the smallest shapes that reach them
    assert (2, 8, 8, 64, 32, 1, 1, "valid") in tiles[(64, 32)] and (2, 8, 8, 128, 192, 1, 1, "valid") in tiles[(128, 128)]
    # the WGRAD_CASES rows whose comments name a kernel
    named = {(3, 13, 11, 128, 256, 3, 1, "same"): "BLDS", (90, 13, 11, 128, 256, 3, 1, "same"): "BLDS", (459, 13, 11, 128, 128, 3, 1, "same"): "BLDS_TABLE"}
    for case, kernel in named.items():
        assert case in reached[kernel] and all(case not in v for k, v in reached.items() if k != kernel), (case, kernel)
    assert R.replay(lib, _case_row((40, 14, 14, 256, 256, 3, 1, "same")))[1]["splits"] > 1          # "several pixel splits"
    # conv_wgrad_glds_kernel serves tensors past a buffer descriptor's range; the suite reaches it through MRCNN_CONV_FLAT_GLDS
    # (read once per process) in test_flat_addressed_lds_dma_kernels: its shape, asked in a child process
    assert "(90, 13, 11, 128)" in T._FLAT_SCRIPT and "(3, 3, 128, 256), 1, \"same\"" in T._FLAT_SCRIPT
    script = ("import sys; sys.path.insert(0, %r); import wgrad_plan_rows as R; "
              "print('kernel', R.replay(R.load(%r), R.row('flat', R.desc(90, 13, 11, 128, 256, 3, 1, 'same'), flat=True))[1]['kernel'])"
              % (os.path.dirname(os.path.abspath(__file__)), lib_path))
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MRCNN_CONV_FLAT_GLDS="1"), capture_output=True, text=True)
    assert "kernel %d" % _hip.WGRAD_KERNELS.index("GLDS") in out.stdout, out.stderr[-2000:]
    assert set(reached) | {"GLDS"} == set(_hip.WGRAD_KERNELS), {k: v[:2] for k, v in reached.items()}
    # test_conv_wgrad_multi_launch: its four layers are one shared launch with a reduction; with the Cout = 64 layer it is refused
    N, H, W = 3, 9, 7
    layers = [R.desc(N, H, W, 256, 128), R.desc(N, H, W, 128, 128, 3, 1, "same"), R.desc(N, H, W, 128, 512), R.desc(N, 2 * H, 2 * W, 256, 512, 1, 2, "valid")]
    rc, plan, query = R.replay(lib, R.row("multi", layers, op="multi"))
    assert rc == 0 and plan["reduce_grid"] > 0 and all(s > 1 for s in plan["splits"]) and query > 256
    assert R.replay(lib, R.row("multi", [layers[0], R.desc(N, H, W, 256, 64)], op="multi"))[::2] == (-4, 0)
    # the reductions of the single launch: torch allocations are 256-byte aligned, so through ops the scalar one runs only where
    # KH*KW*Cin*Cout % 4 != 0, and every case has Cin % 4 == 0 or Cout % 4 == 0 (so has every layer of the model): WGRAD_CASES
    # cannot reach it.  The table's rows ptr/*/dw_misaligned and ws/tile_odd/* pin its selection; its arithmetic is
    # wgrad_reduce_vec_kernel's, element by element.
    assert all(case[3] % 4 == 0 or case[4] % 4 == 0 for case in T.WGRAD_CASES) and reductions == {"NONE", "VEC"}
    table = R.read_table(TABLE)
    assert any(r["plan"] and r["plan"][S("reduce")] == _hip.WGRAD_REDUCTIONS.index("SCALAR") for r in table if r["name"].startswith("ptr/"))
