"""The float32 convolution planner, on the CPU: mrcnn_conv2d_fwd_plan and mrcnn_conv2d_fwd_workspace of the built tree against
tests/golden/conv_plan_table.json (rows and replay: conv_plan_rows.py).  The table was written by the launch code as it stood
before planning and launching were separated, with a record in place of every launch, so equality here is "selects what that code
selected": kernel, tile, K slices, grid, reduction, tail split, slab bytes and status, row by row."""
import json
import os
import subprocess
import sys

import pytest

import conv_plan_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    return R.load(ge.build())


@pytest.fixture
def planner_state(lib, monkeypatch):
    """Tuning keys and the tail switch back to their defaults afterwards (replay sets them per row)."""
    monkeypatch.setenv("MRCNN_CONV_TAIL_SPLIT", "0")        # registers the variable: monkeypatch restores whatever was there
    yield
    lib.mrcnn_tuning_set(b"sk16", 0)
    lib.mrcnn_tuning_set(b"sk64", -1)


def test_table_rows_are_the_rows_of_the_generator():
    """The committed table holds exactly the inputs conv_plan_rows.all_rows() states (answers aside)."""
    table = R.read_table(TABLE)
    answers = ("status", "plan", "wsq")
    assert [{k: v for k, v in r.items() if k not in answers} for r in table] == json.loads(json.dumps(R.all_rows()))


def test_plan_and_workspace_equal_the_table(lib, planner_state):
    table = R.read_table(TABLE)
    assert len(table) >= 600
    bad = []
    for r in table:
        rc, plan, query = R.replay(lib, r)
        if rc != r["status"]:
            bad.append((r["name"], "status", rc, r["status"]))
        if query != r["wsq"]:
            bad.append((r["name"], "workspace query", query, r["wsq"]))
        for f, want in zip(R.PLAN_FIELDS, r["plan"]) if rc == 0 and r["plan"] else ():
            if plan[f] != want:
                bad.append((r["name"], f, plan[f], want))
    assert not bad, "%d differences (row, field, got, table): %s" % (len(bad), bad[:12])


def test_table_covers_every_kernel_with_every_reduction_it_can_have():
    from caesar_mrcnn_amd import _hip
    K, D = _hip.CONV_KERNELS.index, _hip.CONV_REDUCTIONS.index
    table = R.read_table(TABLE)
    seen = {(r["plan"][0], r["plan"][6]) for r in table if r["plan"]}          # R.PLAN_FIELDS: kernel, ..., reduce
    want = {(K(k), D("NONE")) for k in ("TILE", "BLDS", "GLDS", "SK", "SK16", "SK64")}
    want |= {(K(k), D(d)) for k in ("TILE", "BLDS_SPLITK", "BLDS_TAIL") for d in ("SCALAR", "VEC", "BWD")}
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    assert {r["status"] for r in table} == {0, -1, -4}


def test_ops_conv2d_plan(lib):
    """The thin wrapper: res4 2c of the training step takes conv_fwd_sk64_kernel; its data gradient with a misaligned epilogue
    operand is refused as the launch refuses it; the query is never taped."""
    from caesar_mrcnn_amd import _hip, ops
    d = ops.conv_desc((4, 16, 16, 256), (1, 1, 256, 1024), 1, "valid", act=1)
    tape = _hip.tape_begin()
    try:
        rc, plan = ops.conv2d_plan(d, bias=32, scale=48, shift=64, z_out=80)
    finally:
        _hip.tape_end()
    assert tape == [] and rc == 0
    assert (_hip.CONV_KERNELS[plan.kernel], _hip.CONV_REDUCTIONS[plan.reduce], plan.grid, plan.ksplit, plan.ksteps, plan.slab_bytes) == \
        ("SK64", "NONE", 256, 2, 4, 0)
    ep = _hip.BwdEpilogue(out=16, z=32, scale=48, mean=64, rstd=84, act=1)
    assert ops.conv2d_plan(ops.conv_desc((4, 16, 16, 1024), (1, 1, 1024, 256), 1, "valid"), ep=ep)[0] == ops.ERR_UNSUPPORTED
    ep.rstd = 80
    assert ops.conv2d_plan(ops.conv_desc((4, 16, 16, 1024), (1, 1, 1024, 256), 1, "valid"), ep=ep)[0] == 0


def _gpu_case_plans(lib):
    """(case, plan) of every forward case of the GPU suites, as those tests call ops.conv2d: tail split on and sk16 at 1 in
    test_conv_fwd; the sk64 key at 0 and at 1 in test_conv_shortk_gpu."""
    import test_conv_shortk_gpu as S
    import test_kernels_gpu as T
    rows = []
    for case in T.CONV_CASES:
        N, H, W, Cin, Cout, k, stride, padding, act, bn, res = case
        pad = padding if isinstance(padding, str) else padding[0]
        have = ("bias", "z_out") + (("scale", "shift") if bn else ()) + (("res",) if res else ())
        rows.append((case, R.row("case", R.desc(N, H, W, Cin, Cout, k, stride, pad, act, res), have=have, sk16=1, tail=1)))
    for case in S.FWD_CASES + S.DECLINED_CASES:
        N, H, W, Cin, Cout, stride, act, bn, res, z = case
        have = ("bias",) + (("scale", "shift") if bn else ()) + (("res",) if res else ()) + (("z_out",) if z else ())
        for key in (0, 1):
            rows.append((case + (key,), R.row("case", R.desc(N, H, W, Cin, Cout, 1, stride, "valid", act, 1 if res else 0), have=have, sk64=key)))
    plans = []
    for case, r in rows:
        rc, plan, _ = R.replay(lib, r)
        assert rc == 0, case
        plans.append((case, plan))
    return plans


def test_gpu_suites_reach_every_kernel(lib, planner_state):
    """Every kernel id is what at least one case of test_kernels_gpu.CONV_CASES or of test_conv_shortk_gpu's lists launches, so a
    moved threshold cannot leave a kernel without a numerical test unnoticed."""
    import test_kernels_gpu as T
    from caesar_mrcnn_amd import _hip
    reached = {}
    for case, plan in _gpu_case_plans(lib):
        reached.setdefault(_hip.CONV_KERNELS[plan["kernel"]], []).append(case)
    # conv_fwd_glds_kernel serves inputs past 2 GiB; the suite reaches it through MRCNN_CONV_FLAT_GLDS (read once per process) in
    # test_flat_addressed_lds_dma_kernels, whose forward shape is CONV_CASES' conv_fwd_blds_kernel case: asked in a child process
    assert reached["BLDS"] == [(10, 64, 64, 64, 256, 1, 1, "valid", 1, True, 0)] and "(10, 64, 64, 64)" in T._FLAT_SCRIPT
    script = ("import sys; sys.path.insert(0, %r); import conv_plan_rows as R; "
              "print('kernel', R.replay(R.load(%r), R.row('flat', R.desc(10, 64, 64, 64, 256)))[1]['kernel'])" % (os.path.dirname(__file__), lib._name))
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MRCNN_CONV_FLAT_GLDS="1"), capture_output=True, text=True)
    assert "kernel %d" % _hip.CONV_KERNELS.index("GLDS") in out.stdout, out.stderr[-2000:]
    assert set(reached) | {"GLDS"} == set(_hip.CONV_KERNELS), {k: v[:2] for k, v in reached.items()}


def test_conv_case_comments_name_the_kernel_taken(lib, planner_state):
    """The CONV_CASES rows whose comments name a kernel, against the query."""
    from caesar_mrcnn_amd import _hip
    named = {(8, 64, 64, 64, 256, 1, 1, "valid", 1, True, 0): ("TILE", 64, 128),
             (10, 64, 64, 64, 256, 1, 1, "valid", 1, True, 0): ("BLDS", 128, 128),
             (8, 64, 64, 64, 64, 3, 1, "same", 1, True, 0): ("TILE", 128, 64),
             (16, 64, 64, 256, 12, 1, 1, "valid", 0, False, 0): ("TILE", 128, 32),
             (1, 8, 8, 512, 6, 1, 1, "valid", 0, False, 0): ("TILE", 64, 32),
             (1, 33, 17, 64, 64, 3, 1, "same", 0, False, 0): ("SK16", 16, 16),
             (64, 14, 14, 256, 256, 3, 1, "same", 1, True, 1): ("BLDS_SPLITK", 128, 128),
             (90, 13, 11, 128, 256, 3, 1, "same", 1, False, 0): ("BLDS_SPLITK", 128, 128),
             (3, 64, 64, 256, 128, 1, 1, "valid", 0, False, 0): ("SK64", 64, 64),
             (457, 14, 14, 64, 256, 3, 1, "same", 1, True, 1): ("BLDS_TAIL", 128, 128),
             (1, 16, 16, 1024, 256, 1, 1, "valid", 1, True, 0): ("SK16", 16, 16),
             (1, 16, 16, 256, 256, 3, 1, "same", 1, True, 0): ("SK16", 16, 16),
             (1, 16, 16, 256, 1024, 1, 1, "valid", 1, True, 1): ("SK16", 16, 16),
             (1, 8, 8, 2048, 512, 1, 1, "valid", 1, True, 0): ("SK16", 16, 16),
             (1, 7, 9, 256, 128, 3, 1, "same", 0, False, 1): ("TILE", 64, 64),
             (3, 7, 9, 256, 128, 3, 1, "same", 0, False, 1): ("SK16", 16, 16),
             (4, 16, 16, 1024, 256, 1, 1, "valid", 1, True, 0): ("SK", 32, 32),
             (1, 16, 16, 512, 256, 1, 2, "valid", 1, True, 0): ("SK16", 16, 16)}
    got = {case: (_hip.CONV_KERNELS[p["kernel"]], p["bm"], p["bn"]) for case, p in _gpu_case_plans(lib) if case in named}
    assert got == named
