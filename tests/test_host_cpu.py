"""CPU-only checks: the C-ABI library loads and exports every symbol of include/mrcnn_hip.h, host
logic (config, parameter layout, FITS + zscale, weight files, data generator, facade error behaviour)
and the world_size-2 gradient reducer over gloo.  No compute call touches a GPU here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLD, "reference_numpy_helpers.npz"))


def test_cabi_library_exports_header_symbols():
    import ctypes
    import __graft_entry__ as ge
    lib_path = ge.build()
    assert os.path.exists(lib_path)
    header = open(os.path.join(ROOT, "include", "mrcnn_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(mrcnn_[a-z0-9_]+)\s*\(", header, re.M))
    assert len(declared) >= 30
    lib = ctypes.CDLL(lib_path)
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, "declared in mrcnn_hip.h but not exported: %s" % missing
    from caesar_mrcnn_amd import _hip
    assert set(_hip.exported_symbols()) <= declared
    lib.mrcnn_hip_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.mrcnn_hip_version()


def test_built_objects_have_no_store_data_hazard():
    """Machine-code check of the built kernel objects (caesar-mrcnn_amd/isa_check.py): a > 64-bit buffer store with an SGPR
    soffset must not be followed within two slots by a vector write of its data registers -- gfx950 loses that race on a
    cold instruction cache and LLVM's recogniser does not cover the SGPR form (the phased 16-bit convolution stored stray
    dwords that way).  The scanner itself is checked on the pattern that was found."""
    import glob
    import __graft_entry__ as ge
    from caesar_mrcnn_amd import isa_check
    listing = """
0000000000001000 <kern>:
	buffer_store_dwordx4 v[62:65], v82, s[40:43], s0 offen  // 00000001D84C: E07C1000
	v_mul_f32_e32 v62, v34, v66                              // 00000001D854: 0A7C8522
	buffer_store_dwordx4 v[58:61], v82, s[40:43], s0 offen
	v_readlane_b32 s0, v234, 2
	v_mul_f32_e32 v58, v42, v74
	buffer_store_dwordx4 v[58:61], v82, s[40:43], s0 offen
	s_nop 2
	v_mul_f32_e32 v58, v42, v74
	buffer_store_dwordx4 v[58:61], v82, s[40:43], 0 offen
	v_mul_f32_e32 v58, v42, v74
	buffer_store_dwordx4 v[58:61], v82, s[40:43], s0 offen
	v_mul_f32_e32 v57, v42, v74
	v_mul_f32_e32 v62, v42, v74
	v_cmp_gt_f32_e32 vcc, v58, v74
"""
    hits = isa_check.store_data_hazards(listing)
    assert [h[2] for h in hits] == ["v_mul_f32_e32 v62, v34, v66", "v_mul_f32_e32 v58, v42, v74"], hits
    if not isa_check.tools_available():
        pytest.skip("llvm-objcopy / clang-offload-bundler / llvm-objdump not found")
    ge.build()
    objs = sorted(glob.glob(os.path.join(ROOT, "caesar-mrcnn_amd", "build", "*.o")))
    assert len(objs) >= 10
    for o in objs:
        isa_check.check_object(o)


def test_product_path_has_no_cpu_fallback():
    import torch
    from caesar_mrcnn_amd import ops, _hip
    with pytest.raises(_hip.HipPathError):
        ops.conv2d(torch.zeros(1, 4, 4, 32), torch.zeros(1, 1, 32, 32))
    if not torch.cuda.is_available():
        from caesar_mrcnn_amd.config import run_py_config
        from caesar_mrcnn_amd.model import MaskRCNN
        with pytest.raises(_hip.HipPathError):
            MaskRCNN("inference", run_py_config(mode="inference"), "/tmp/x")
    # nothing under the package imports the oracle
    pkg = os.path.join(ROOT, "caesar-mrcnn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "mrcnn_oracle" not in open(os.path.join(pkg, fn)).read(), fn


@pytest.mark.parametrize("backbone", ["custom", "resnet50"])
def test_engine_cannot_be_built_on_cpu(backbone):
    """The training step is written for three streams and has no single-stream form: an engine on a device without streams
    must not come into being (MaskRCNNEngine.__init__ raises before it returns)."""
    import model_cases as T
    from caesar_mrcnn_amd import _hip
    from caesar_mrcnn_amd.engine import MaskRCNNEngine
    with pytest.raises(_hip.HipPathError):
        MaskRCNNEngine(T._small_cfg(backbone, 128), "cpu")


def test_same_padding_is_tf_asymmetric():
    from caesar_mrcnn_amd.ops import same_padding
    assert same_padding(128, 3, 2) == (64, 0)       # stem max-pool: pad 0 before / 1 after
    assert same_padding(127, 3, 2) == (64, 1)
    assert same_padding(64, 3, 1) == (64, 1)
    assert same_padding(64, 1, 2) == (32, 0)


def test_winograd_path_selection_and_buffer_sizes():
    """Host logic of the Winograd path: which shapes take it, which tile a training layer gets (a pure function of the shape:
    forward, data gradient and weight gradient must agree), and the buffer sizes the C-ABI reports -- (tile + 2)^2 matrices of
    whole 128-row tiles, tile 4 with tiles that hang over a 14 x 14 map (no GPU call: mrcnn_winograd_buffer_floats is host code)."""
    from caesar_mrcnn_amd import ops, _hip
    w = (3, 3, 256, 256)
    assert ops.winograd_ok((2048, 14, 14, 256), w) and ops.winograd_ok((100, 14, 14, 256), w)
    assert not ops.winograd_ok((10, 14, 14, 256), w)                      # too few rows to fill the chip
    assert not ops.winograd_ok((2048, 14, 14, 256), (1, 1, 256, 256))     # 3 x 3 only
    assert not ops.winograd_ok((2048, 14, 14, 256), w, stride=2)
    assert not ops.winograd_ok((2048, 15, 14, 256), w)                    # odd extent (the engine's rule; tile 4 alone would take it)
    assert not ops.winograd_ok((2048, 14, 14, 256), (3, 3, 256, 64))      # Cout % 128
    if ops._WINO_TILE == 4:
        big = ops.TILE_MIXED if ops._WINO_MIXED else 4              # 14 = 4 + 4 + 4 + 2: mixed groups instead of an overhanging 4th tile
        assert ops.winograd_tile((2048, 14, 14, 256)) == big and ops.winograd_tile((1024, 14, 14, 256)) == big
        assert ops.winograd_tile((512, 14, 14, 256)) == big and ops.winograd_tile((511, 14, 14, 256)) == 2
        assert ops.winograd_tile((2048, 16, 16, 256)) == 4
    gs = ops.winograd_groups(14, 14, ops.TILE_MIXED)
    assert [(g.oth, g.otw, g.th_n, g.tw_n, g.oh0, g.ow0) for g in gs] == [(4, 4, 3, 3, 0, 0), (4, 2, 3, 1, 0, 12), (2, 4, 1, 3, 12, 0),
                                                                          (2, 2, 1, 1, 12, 12)]
    covered = np.zeros((14, 14), int)                              # every output exactly once
    for g in gs:
        for th in range(g.th_n):
            for tw in range(g.tw_n):
                covered[g.oh0 + g.oth * th:g.oh0 + g.oth * (th + 1), g.ow0 + g.otw * tw:g.ow0 + g.otw * (tw + 1)] += 1
    assert (covered == 1).all()
    assert ops.winograd_v_floats((2048, 14, 14, 256), ops.TILE_MIXED) == (36 * 18432 + 2 * 24 * 6144 + 16 * 2048) * 256
    assert ops.winograd_tile((100, 14, 14, 256)) == 2
    lib = _hip.lib()
    assert lib.mrcnn_winograd_buffer_floats(2048, 14, 14, 256, 2) == 16 * 100352 * 256          # 2048 * 49 tiles: already whole row tiles
    assert lib.mrcnn_winograd_buffer_floats(2048, 14, 14, 256, 4) == 36 * 32768 * 256           # 2048 * 16 tiles
    assert lib.mrcnn_winograd_buffer_floats(37, 14, 14, 64, 2) == 16 * 1920 * 64                # 1813 tiles -> 15 row tiles of 128
    assert lib.mrcnn_winograd_buffer_floats(5, 7, 9, 32, 4) == 36 * 128 * 32                    # 5 * 2 * 3 tiles
    assert lib.mrcnn_winograd_buffer_floats(5, 7, 9, 32, 2) == 0                                # tile 2 wants even extents
    assert lib.mrcnn_winograd_buffer_floats(5, 8, 8, 32, 3) == 0                                # no such tile


def test_param_layout_counts_and_names():
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.params import ParamLayout, init_weights
    for bb, nconv, total in (("resnet50", 53, 44.6e6), ("resnet101", 104, 63.6e6)):
        L = ParamLayout(run_py_config(backbone=bb))
        backbone = [l for l in L.layers if l.name.startswith("res") or l.name == "conv1"]
        assert len(backbone) == nconv
        real = sum(s[2] for s in L.segments)
        assert abs(real - total) / total < 0.01
        offs = [s[1] for s in L.segments]
        assert offs == sorted(offs) and all(o % 64 == 0 for o in offs)
        ends = [s[1] + s[2] for s in L.segments]
        assert all(e <= o2 for e, o2 in zip(ends[:-1], offs[1:]))         # no overlap
    L = ParamLayout(run_py_config(backbone="resnet101"))
    assert "res4w_branch2c" in L.by_name and "res4x_branch2c" not in L.by_name
    assert L.by_name["mrcnn_class_conv1"].shape == (7, 7, 256, 1024)
    assert L.by_name["rpn_class_raw"].shape == (1, 1, 512, 6) and L.by_name["rpn_bbox_pred"].shape == (1, 1, 512, 12)
    assert L.by_name["mrcnn_bbox_fc"].shape == (1, 1, 1024, 16) and L.by_name["mrcnn_mask"].shape == (1, 1, 256, 4)
    # trainable presets (model.py:2432-2441)
    m = L.trainable_mask("heads")
    names = [s[0] for s in L.segments]
    assert all(bool(t) == bool(re.fullmatch(r"(mrcnn\_.*)|(rpn\_.*)|(fpn\_.*)", n.split("/")[0])) for n, t in zip(names, m))
    assert L.trainable_mask("all").all()
    assert not L.trainable_mask("5+")[names.index("res4a_branch2a/kernel")] and L.trainable_mask("5+")[names.index("bn5a_branch2a/gamma")]
    l2 = L.l2_coefficients(1e-4)
    assert l2[names.index("conv1/bias")] > 0 and l2[names.index("bn_conv1/gamma")] == 0
    w = init_weights(ParamLayout(run_py_config(backbone="custom")), seed=1)
    assert w["conv1/kernel"].shape == (7, 7, 3, 16) and float(w["bn_conv1/gamma"].min()) == 1.0


def test_weight_file_roundtrip_and_exclude_quirk(tmp_path):
    from caesar_mrcnn_amd import weights_io
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.params import ParamLayout, init_weights
    w = init_weights(ParamLayout(run_py_config(backbone="custom")), seed=2, perturb_bn=True)
    p = str(tmp_path / "rg-dataset20240101T0000" / "mask_rcnn_rg-dataset_0007.npz")
    weights_io.save(p, w)
    back = weights_io.load(p)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    # load_weights(exclude='conv1') is a substring test on the layer name in the reference
    kept = {k for k in back if k.split("/")[0] not in "conv1"}
    assert "conv1/kernel" not in kept and "bn_conv1/gamma" in kept and "mrcnn_mask_conv1/kernel" in kept


@pytest.mark.parametrize("num_classes", [2, 6, 17])
def test_param_layout_and_weight_files_follow_the_class_count(tmp_path, num_classes):
    """NUM_CLASSES (run.py --classdict) is the width of three layers: mrcnn_class_logits [1024, C], mrcnn_bbox_fc [1024, 4 C] (Dense
    layers, kept as 1 x 1 kernels) and mrcnn_mask [1, 1, 256, C].  Whatever C is, every tensor of the flat buffer starts on a 64-float
    granule, the buffer is a whole number of granules (the optimiser kernels' ABI), nothing overlaps, the granule table covers the
    three tensors, and both weight containers return the tensors bit for bit."""
    from caesar_mrcnn_amd import hdf5_min, weights_io
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.params import ALIGN, ParamLayout, deconv_gemm_to_keras, granule_coefficients, init_weights
    C_ = num_classes
    cfg = run_py_config(num_classes=C_, backbone="custom", imgsize=128)
    assert cfg.NUM_CLASSES == C_ and cfg.IMAGE_META_SIZE == 12 + C_
    L = ParamLayout(cfg)
    heads = {"mrcnn_class_logits": (1024, C_), "mrcnn_bbox_fc": (1024, 4 * C_), "mrcnn_mask": (256, C_)}
    for name, (cin, cout) in heads.items():
        assert L.by_name[name].shape == (1, 1, cin, cout)
        assert L.offsets[name + "/kernel"][1:] == (cin * cout, (1, 1, cin, cout)) and L.offsets[name + "/bias"][1:] == (cout, (cout,))
    assert ALIGN == 64 and L.total % 64 == 0 and L.gamma_offset % 64 == 0 and L.beta_offset % 64 == 0
    segs = sorted(L.segments, key=lambda s_: s_[1])
    assert all(s_[1] % 64 == 0 for s_ in segs)
    assert all(a[1] + a[2] <= b[1] for a, b in zip(segs[:-1], segs[1:])) and segs[-1][1] + segs[-1][2] <= L.total
    base = ParamLayout(run_py_config(num_classes=4, backbone="custom", imgsize=128))
    grow = lambda c: sum((n + 63) // 64 * 64 for n in (1024 * c, c, 1024 * 4 * c, 4 * c, 256 * c, c))
    assert L.total - base.total == grow(C_) - grow(4)                      # nothing but the three layers depends on C
    gran = granule_coefficients(L, 1e-4, L.trainable_mask("all"))
    assert gran.shape == (L.total // 64,)
    for name in heads:
        off, n, _ = L.offsets[name + "/kernel"]
        assert (gran[off // 64:(off + n + 63) // 64] == np.float32(2e-4 / n)).all()
        assert off + n == (off + n + 63) // 64 * 64 or gran[(off + n) // 64] == np.float32(2e-4 / n)      # a partial last granule is the tensor's
    w = init_weights(L, seed=3, perturb_bn=True)
    assert w["mrcnn_class_logits/kernel"].reshape(1024, C_).shape == (1024, C_) and w["mrcnn_class_logits/bias"].shape == (C_,)
    assert w["mrcnn_bbox_fc/kernel"].shape[-2:] == (1024, 4 * C_) and w["mrcnn_mask/kernel"].shape == (1, 1, 256, C_)
    assert all(np.abs(w[n + "/kernel"]).max() > 0 for n in heads)
    w["mrcnn_mask_deconv/kernel"] = deconv_gemm_to_keras(w["mrcnn_mask_deconv/kernel"])
    for ext in (".npz", ".h5"):
        p = str(tmp_path / ("mask_rcnn_c%d%s" % (C_, ext)))
        weights_io.save(p, w, L)
        back = weights_io.load(p)
        assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) and back[k].shape == w[k].shape for k in w)
    f = hdf5_min.H5File(str(tmp_path / ("mask_rcnn_c%d.h5" % C_)))
    assert f.read(f.get(f.root, "mrcnn_bbox_fc/mrcnn_bbox_fc/kernel:0")).shape[-2:] == (1024, 4 * C_)


def test_class_count_preconditions_of_gpu_cases():
    """The GPU parity tests at other class counts assert data-dependent preconditions from the reference side; here the same seeded
    inputs (tests/model_cases.py) go through the oracle alone, so the seeds are known to be good without a GPU: the detection layer
    keeps more than 10 detections per image at both confidence settings and every foreground class occurs among them; the class
    loss sees both active and inactive predictions, with a positive normaliser, and every class among its targets."""
    import mrcnn_oracle as orc
    import model_cases as M
    from caesar_mrcnn_amd.config import run_py_config
    for num_classes, seed, scale in [(4, 21, 2.0)] + M.DETECTION_CLASS_CASES:
        cfg = run_py_config(mode="inference", num_classes=num_classes)
        rois, probs, deltas, windows = M.detection_layer_inputs(num_classes, seed, scale)
        o = orc.OracleMaskRCNN(cfg, {})
        seen = set()
        for minconf in (0, 0.5):
            cfg.DETECTION_MIN_CONFIDENCE = minconf
            for b in range(rois.shape[0]):
                ref = o.refine_detections(rois[b], probs[b], deltas[b], windows[b])
                assert (ref[:, 4] > 0).sum() > 10, (num_classes, minconf, b)
                assert minconf == 0 or ref[ref[:, 4] > 0, 5].min() >= 0.5
                seen |= set(ref[ref[:, 4] > 0, 4].astype(int).tolist())
        assert seen == set(range(1, num_classes)), (num_classes, seen)
    for num_classes, cycle in ((4, False), (2, True), (5, True), (6, True), (17, True)):
        d = M.losses_inputs(num_classes, cycle)
        assert set(d["pred_active"].tolist()) == {0, 1} and d["pred_active"].sum() > 0, num_classes
        if cycle:
            assert set(d["tcls"].reshape(-1).tolist()) == set(range(num_classes))


def test_count_case_preconditions_of_gpu_cases():
    """The count-dependent GPU cases (tests/test_counts_gpu.py) assert their preconditions from the oracle side; here the same
    seeded inputs (tests/model_cases.py) go through the oracle alone.  Detection targets: the counts (P, N) every scene is built for
    -- the sweep's P = min(b, 66) with N and its float32 steps, P below the quota, scarce negatives, P = N = 0, R = 1, the caps --
    and the threshold scene's float32 IoUs of exactly 0.5 and either side of 0.001.  Detection layer: nvalid of every case, the zero
    tail, the cut inside a chunk.  Losses: which register groups of the RPN kernel hold positives, the emptied sides, the surplus."""
    import model_cases as M
    from caesar_mrcnn_amd.config import run_py_config
    for name in M.DT_SCENES:
        M.check_detection_target_case(name)
    for name in M.DT_MINI_SCENES:
        M.check_detection_target_case(name, True)
    seen = set()
    for R, n, maxi, minconf in M.DETECTION_COUNT_CASES:
        inp, cfg, ref, nvalid = M.detection_count_case(R, n, maxi, minconf)
        assert inp[0].shape == (2, R, 4) and (minconf != 0 or nvalid == list(n))
        seen |= set(nvalid)
    assert {0, 1, 63, 64, 65, 128, 129, 2048} <= seen
    cfg = run_py_config(num_classes=4)
    for A in M.RANK_CASE_ANCHORS:
        d = M.losses_rank_inputs(A)
        m = d["rpn_match"][:, :, 0]
        per_group = M.rank_case_group_positives(d)
        assert per_group.shape == (2, -(-A // M.LOSS_GROUP)) and (per_group.sum(0) > 0).all()          # every group, in some image
        assert per_group[0, 0] == 0 and (per_group[0, 1:] > 0).all()                                     # empty first group
        assert per_group[1, -1] == 0 and (per_group[1, :-1] > 0).all()                                   # empty last group
        assert ((m == 1).sum(1) <= 256).all() and ((m != 0).sum(1) <= 512).all() and (m != 0).sum() > 900
        for a in (0, 32767, 32768, 65535, 65536, 98303, 98304, A - 1):
            if a < A:
                assert (m[:, a] == 1).any() and (m[:, a] != 0).all(), a
        assert len(np.unique(d["rpn_bbox_t"], axis=1)[0]) == d["rpn_bbox_t"].shape[1] >= (m == 1).sum(1).max()
    for case in M.EMPTY_SIDE_CASES:
        d = M.losses_empty_inputs(case)
        ls, grads = M.losses_reference(cfg, d)
        zero = {"a": [1], "b": [0, 1], "c": [], "d": [3, 4], "e": [], "f": [], "g": []}[case]
        assert all(ls[i] == 0 for i in zero) and all(ls[i] > 0 for i in range(5) if i not in zero and not (case == "g" and i == 2))
        assert np.isnan(ls[2]) == (case == "g") and np.isnan(grads["logits"]).all() == (case == "g")
        assert int((d["tcls"] > 0).sum()) == {"d": 0, "e": 1, "f": d["tcls"].size}.get(case, 40)
    d, match_box = M.losses_surplus_inputs()
    npos = (d["rpn_match"][:, :, 0] == 1).sum(1)
    assert npos.max() == d["rpn_bbox_t"].shape[1] + 3 and ((match_box[:, :, 0] == 1).sum(1) <= d["rpn_bbox_t"].shape[1]).all()
    ls, grads = M.losses_reference(cfg, d, rpn_match_box=match_box)
    assert np.isfinite(ls).all() and (grads["rpn_bbox"][match_box[:, :, 0] != 1] == 0).all()


@pytest.mark.parametrize("A", [33797, 98309])
def test_rank_carry_perturbation_fails_the_loss_comparison(A):
    """The multi-group loss case can see a lost rank carry: a float64 statement of the RPN box loss with the ranks written out
    (model_cases.rpn_bbox_loss_statement) passes the GPU test's comparison with the oracle; the same statement with the ranks of
    the second register group shifted by one fails it, in the loss and in the gradient."""
    import model_cases as M
    from caesar_mrcnn_amd.config import run_py_config
    d = M.losses_rank_inputs(A)
    ls, grads = M.losses_reference(run_py_config(num_classes=4), d)

    def compare(shift_group):
        l1, g = M.rpn_bbox_loss_statement(d, shift_group)
        got = ls.copy(); got[1] = l1
        M.assert_losses_close(got, {"rpn_bbox": g}, ls, grads, names=["rpn_bbox"], which=[1])
        return l1, g

    compare(None)
    with pytest.raises(AssertionError):
        compare(1)
    l1, g = M.rpn_bbox_loss_statement(d, 1)
    assert abs(l1 - ls[1]) > 100 * (M.LOSS_TOL["atol"] + M.LOSS_TOL["rtol"] * abs(ls[1]))               # not a near miss
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(g, grads["rpn_bbox"], **M.GRAD_TOL)


@pytest.mark.parametrize("mini", [False, True])
def test_compacted_mask_plane_perturbation_changes_the_targets(mini):
    """The layout scene can see a kernel that reads GT mask plane g of the compacted order instead of the original row gorig[g]:
    with the planes moved that way the oracle's mask targets change (and nothing else does)."""
    import mrcnn_oracle as orc
    import model_cases as M
    s, cfg, ref = M.detection_target_case("layout", mini)
    wrong = M.layout_compacted_planes(s)
    o = orc.OracleMaskRCNN(cfg, {})
    for b, r in enumerate(ref):
        p = o.detection_targets(s["props"][b], s["gt_cls"][b], s["gt_boxes"][b], wrong[b].astype(bool), s["keys"][b])
        P = r[4][0]
        assert p[4] == r[4] and np.array_equal(p[0], r[0]) and np.array_equal(p[1], r[1]) and np.array_equal(p[2], r[2])
        differs = (p[3][:P] != r[3][:P]).any(axis=(1, 2))
        assert differs.mean() > 0.9, differs.mean()                  # (almost) every positive row: random planes


def test_oracle_training_graph_at_six_classes():
    """OracleMaskRCNN.forward_training on the small test configuration at NUM_CLASSES = 6 (the reference's documented 1 + 5): five
    finite losses, head outputs C / 4 C / C wide, target class ids of more than one foreground class below C."""
    import torch
    import mrcnn_oracle as orc
    import model_cases as T
    cfg = T._small_cfg("custom", 128, num_classes=6)
    w = T._weights(cfg, 11)
    inputs, keys = T._train_inputs(cfg, 2, 5)
    images, meta, rpn_match, rpn_bbox_t, gt_cls, gt_boxes, gt_masks = inputs
    assert meta.shape == (2, 18) and set(np.unique(gt_cls)) <= set(range(6)) and len(set(gt_cls[gt_cls > 0].tolist())) == 5
    o = orc.OracleMaskRCNN(cfg, w)
    with torch.no_grad():
        ref = o.forward_training(images, rpn_match, rpn_bbox_t.astype(np.float32), gt_cls, gt_boxes, gt_masks,
                                 meta[:, 12:].astype(np.int32), orc.get_anchors(cfg, images.shape[1:]), keys)
    losses = np.array([float(l) for l in ref["losses"]])
    assert losses.shape == (5,) and np.isfinite(losses).all() and (losses > 0).all(), losses
    assert tuple(ref["mrcnn_class_logits"].shape) == (2, cfg.TRAIN_ROIS_PER_IMAGE, 6)
    assert tuple(ref["mrcnn_bbox"].shape) == (2, cfg.TRAIN_ROIS_PER_IMAGE, 6, 4) and tuple(ref["mrcnn_mask"].shape[2:]) == (28, 28, 6)
    tc = ref["target_class_ids"]
    assert sum(c[0] for c in ref["counts"]) > 0 and tc.max() < 6 and len(set(tc[tc > 0].tolist())) > 1


def test_set_log_dir_epoch_parsing():
    from caesar_mrcnn_amd.model import MaskRCNN
    from caesar_mrcnn_amd.config import run_py_config
    m = MaskRCNN.__new__(MaskRCNN)
    m.config, m.model_dir = run_py_config(), "/tmp/logs"
    m.set_log_dir("/tmp/logs/rg-dataset20171029T2315/mask_rcnn_rg-dataset_0012.h5")
    assert m.epoch == 12 and m.log_dir.endswith("rg-dataset20171029T2315")
    assert m.checkpoint_path.endswith("mask_rcnn_rg-dataset_{epoch:04d}.h5")
    m.set_log_dir("/somewhere/else.h5")
    assert m.epoch == 0


# ---- FITS + zscale ------------------------------------------------------------------------------------
def test_fits_reader_on_reference_cutouts():
    from caesar_mrcnn_amd import fits
    data, hdr = fits.read_primary_hdu(os.path.join(GOLD, "galaxy0002.fits"))
    assert data.shape == (132, 132) and data.dtype == np.float32
    assert int(np.isnan(data).sum()) == 288                     # SURVEY: galaxy0002 has 288 NaN pixels
    assert hdr["BITPIX"] == -32 and hdr["NAXIS1"] == 132 and "BMAJ" in hdr and "CDELT1" not in hdr
    assert fits.get_fits_size(os.path.join(GOLD, "sidelobe0001.fits")) == (132, 132)
    img, hdr = fits.read_fits(os.path.join(GOLD, "galaxy0002.fits"))
    assert img.shape == (132, 132, 3) and img.dtype == np.uint8 and img.max() == 255
    assert np.array_equal(img[..., 0], img[..., 1])             # equal contrasts -> equal channels
    tile, _ = fits.read_fits(os.path.join(GOLD, "galaxy0002.fits"), xmin=10, xmax=74, ymin=20, ymax=52)
    assert tile.shape == (32, 64, 3)
    assert fits.read_fits(os.path.join(GOLD, "galaxy0002.fits"), xmin=10, xmax=5, ymin=0, ymax=4) is None
    assert fits.read_fits("/nonexistent.fits") is None
    raw, _ = fits.read_fits(os.path.join(GOLD, "sidelobe0001.fits"), stretch=False, normalize=False, convertToRGB=False)
    assert raw.dtype == np.float32 and not np.isnan(raw).any()


def test_fits_writer_roundtrip_and_zscale_properties(tmp_path):
    from caesar_mrcnn_amd import fits
    rng = np.random.RandomState(0)
    img = rng.normal(0, 1, (90, 70)).astype(np.float32)
    img[40:50, 30:40] += 50.0
    img[0, :5] = np.nan
    p = str(tmp_path / "t.fits")
    fits.write_fits(p, img, {"BUNIT": "JY/BEAM", "BMAJ": 0.0025})
    back, hdr = fits.read_primary_hdu(p)
    assert np.array_equal(np.isnan(back), np.isnan(img)) and np.array_equal(back[~np.isnan(back)], img[~np.isnan(img)])
    assert hdr["BUNIT"] == "JY/BEAM" and abs(hdr["BMAJ"] - 0.0025) < 1e-12
    clean = np.nan_to_num(img, nan=np.nanmin(img))
    vmin, vmax = fits.zscale_limits(clean, 0.25)
    assert clean.min() <= vmin < vmax <= clean.max()
    assert vmax < 10.0                                            # the bright source is clipped away by zscale
    lo2, hi2 = fits.zscale_limits(clean, 0.5)
    assert (hi2 - lo2) <= (vmax - vmin) + 1e-9                    # higher contrast -> narrower interval
    s = fits.stretch_img(clean, 0.25)
    assert s.min() == 0.0 and s.max() == 1.0
    flat = np.full((20, 20), 3.0)
    assert np.all(fits.stretch_img(flat) == 0.0)                  # degenerate interval: (x - vmin), no division
    assert np.allclose(fits.stretch_img_biasconstrast(np.array([0.0, 0.5, 1.0]), 2.0, 0.5), [0.0, 0.5, 1.0])
    rgb = fits.gray2rgb([s, s, s], True)
    assert rgb.dtype == np.uint8 and rgb.shape == (90, 70, 3)


def test_generate_tiles_matches_reference():
    from caesar_mrcnn_amd import fits
    assert np.array_equal(np.array(fits.generate_tiles(0, 999, 0, 799, 256, 256, 0.5, 1.0)), G["tiles_a"])
    assert np.array_equal(np.array(fits.generate_tiles(10, 521, 5, 300, 128, 100, 1.0, 0.75)), G["tiles_b"])
    assert fits.generate_tiles(0, 10, 0, 10, 64, 64, 1, 1) is None
    assert fits.generate_tiles(0, 100, 0, 100, 64, 64, 0, 1) is None


# ---- data generator -------------------------------------------------------------------------------------
class _ToyDataset(object):
    """Duck-typed like mrcnn.utils.Dataset as the generator uses it (model.py:1302-1366, 1766, 1791)."""

    def __init__(self, n=6, size=128, seed=0):
        self.rng = np.random.RandomState(seed)
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.size = size
        self._cache = {}

    def _make(self, i):
        if i not in self._cache:
            r = np.random.RandomState(100 + i)
            img = r.randint(0, 40, (self.size, self.size, 3)).astype(np.uint8)
            k = r.randint(1, 4)
            mask = np.zeros((self.size, self.size, k), bool)
            ids = np.zeros(k, np.int32)
            for g in range(k):
                y, x = r.randint(5, self.size - 40, 2)
                h, w = r.randint(8, 30, 2)
                mask[y:y + h, x:x + w, g] = True
                img[y:y + h, x:x + w] = 200
                ids[g] = r.randint(1, 4)
            self._cache[i] = (img, mask, ids)
        return self._cache[i]

    def load_image(self, i):
        return self._make(i)[0]

    def load_mask(self, i):
        return self._make(i)[1], self._make(i)[2]


def _gen_cfg():
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(backbone="custom", imgsize=128)
    cfg.MAX_GT_INSTANCES = 10
    cfg.RPN_TRAIN_ANCHORS_PER_IMAGE = 64
    return cfg


def test_data_generator_batches_and_rank_sharding():
    from caesar_mrcnn_amd.datagen import data_generator, load_image_gt
    from caesar_mrcnn_amd import utils
    cfg, ds = _gen_cfg(), _ToyDataset()
    gen = data_generator(ds, cfg, shuffle=False, batch_size=2)
    inputs, outputs = next(gen)
    images, meta, rpn_match, rpn_bbox, gt_ids, gt_boxes, gt_masks = inputs
    A = utils.get_anchors(cfg, (128, 128, 3)).shape[0]
    assert images.shape == (2, 128, 128, 3) and images.dtype == np.float32 and outputs == []
    assert meta.shape == (2, cfg.IMAGE_META_SIZE) and rpn_match.shape == (2, A, 1) and rpn_match.dtype == np.int32
    assert rpn_bbox.shape == (2, 64, 4) and gt_ids.shape == (2, 10) and gt_boxes.shape == (2, 10, 4)
    assert gt_masks.shape == (2, 128, 128, 10) and gt_masks.dtype == bool
    assert set(np.unique(rpn_match)) <= {-1, 0, 1} and (rpn_match == 1).sum() > 0
    assert (np.abs(rpn_match).sum(axis=(1, 2)) <= 64).all()
    # the first image of the batch is dataset image 0, boxes agree with the masks
    _, m0, ids0, b0, mk0 = load_image_gt(ds, cfg, 0)
    assert np.array_equal(gt_boxes[0, :len(b0)], b0) and np.array_equal(utils.extract_bboxes(mk0), b0)
    # two ranks see disjoint strides of the same order
    g0 = data_generator(ds, cfg, shuffle=True, batch_size=1, rank=0, world_size=2, seed=5)
    g1 = data_generator(ds, cfg, shuffle=True, batch_size=1, rank=1, world_size=2, seed=5)
    ids_r0 = [int(next(g0)[0][1][0, 0]) for _ in range(3)]
    ids_r1 = [int(next(g1)[0][1][0, 0]) for _ in range(3)]
    assert not set(ids_r0) & set(ids_r1) and len(set(ids_r0 + ids_r1)) == 6


def test_augmentation_callable_keeps_shapes():
    from caesar_mrcnn_amd.datagen import load_image_gt
    cfg, ds = _gen_cfg(), _ToyDataset()
    flip = lambda im, mk: (np.fliplr(im), np.fliplr(mk))
    img, meta, ids, boxes, masks = load_image_gt(ds, cfg, 1, augmentation=flip)
    img0, _, _, boxes0, _ = load_image_gt(ds, cfg, 1)
    assert np.array_equal(img, np.fliplr(img0))
    assert np.array_equal(np.sort(128 - boxes0[:, [3, 1]], axis=1), np.sort(boxes[:, [1, 3]], axis=1))


# ---- data-parallel gradient reduction over gloo (world_size 2, CPU tensors) ----------------------------
_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from caesar_mrcnn_amd.parallel import GradReducer, init_distributed, allreduce_mean_scalars
rank, local_rank, world = init_distributed(backend="gloo")
assert world == 2
g = torch.arange(1000, dtype=torch.float32) * (rank + 1)
red = GradReducer(g, world)
for lo, hi in ((600, 1000), (200, 600), (0, 200)):      # ranges arrive in backward order
    red.ready(lo, hi)
red.finish()
assert torch.equal(g, torch.arange(1000, dtype=torch.float32) * 3), g[:5]
assert red.mode == "torch"
# ranges cut into <= 256-float messages (MRCNN_ALLREDUCE_MAX_MB): same sums, more, smaller exchanges
g2 = torch.arange(1000, dtype=torch.float32) * (rank + 1)
red2 = GradReducer(g2, world, max_mb=256 * 4 / 2 ** 20, timing=True)     # the byte log is only kept for a caller that drains it
for lo, hi in ((600, 1000), (200, 600), (0, 200)):
    red2.ready(lo, hi)
assert len(red2.pending) == 2 + 2 + 1
red2.finish()
assert torch.equal(g2, torch.arange(1000, dtype=torch.float32) * 3)
assert red2.range_log == [1600, 1600, 800] and red2.bytes_moved == 4000
assert red.range_log == [] and red.bytes_moved == 0
# a recorded step replays its exchange: the launch tape holds the reducer's calls (gloo: the torch transport's)
from caesar_mrcnn_amd import _hip
g3 = torch.arange(1000, dtype=torch.float32) * (rank + 1)
red3 = GradReducer(g3, world)
_hip._tape, _hip._tape_owner = [], __import__("threading").get_ident()
red3.ready(0, 1000)
red3.finish()
tape = _hip.tape_end()
assert torch.equal(g3, torch.arange(1000, dtype=torch.float32) * 3) and len(tape) == 2
g3.copy_(torch.arange(1000, dtype=torch.float32) * (rank + 1))
_hip.tape_replay(tape)
assert torch.equal(g3, torch.arange(1000, dtype=torch.float32) * 3) and red3.pending == []
l = allreduce_mean_scalars(torch.full((5,), float(rank)), world)
assert torch.allclose(l, torch.full((5,), 0.5))
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_split_range():
    from caesar_mrcnn_amd.parallel import split_range
    assert split_range(0, 1000, None) == [(0, 1000)]
    assert split_range(64, 1000, 5000) == [(64, 1000)]
    assert split_range(0, 1000, 300) == [(0, 256), (256, 512), (512, 768), (768, 1000)]     # pieces are granule multiples
    assert split_range(128, 256, 10) == [(128, 192), (192, 256)]


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_direct_allreduce_plan_indexing(world):
    """The direct reduce-scatter + all-gather (csrc/allreduce.hip) as data: mrcnn_allreduce_direct_plan returns, for a rank
    and a phase, what it sends to / receives from every peer -- the function mrcnn_allreduce_grad itself walks.  Executed
    here in NumPy for every rank of the world: each ncclSend meets a receive of the same length on the other side (a
    mismatch hangs a real node), scratch slots stay inside mrcnn_allreduce_scratch() and never overlap, and every rank ends
    with the rank-ordered float32 sum, bit for bit.  Ranges that are not multiples of 64 * world, ranges shorter than the
    world (empty trailing chunks), a range of one float, an offset start."""
    import ctypes as C
    from caesar_mrcnn_amd import _hip
    L = _hip.lib()
    rng = np.random.default_rng(world)
    total = 5000
    for start, end in ((0, total), (64, 64 + 64 * world * 3), (128, 128 + 641), (0, 1), (7, 7 + world - 1), (100, 163), (3, 3 + 64 * world + 1)):
        n = end - start
        nbytes = L.mrcnn_allreduce_scratch(world, n, 1)
        grads = [rng.standard_normal(total).astype(np.float32) for _ in range(world)]
        before = [g.copy() for g in grads]
        want = before[0][start:end].copy()
        for r in range(1, world):
            want = want + before[r][start:end]                                  # rank order, float32
        scratch = [np.full(nbytes // 4, np.nan, np.float32) for _ in range(world)]

        def plan(rank, phase):
            buf = (C.c_int64 * (4 * world))()
            o, l, st = C.c_int64(), C.c_int64(), C.c_int64()
            assert L.mrcnn_allreduce_direct_plan(world, rank, start, end, phase, buf, C.byref(o), C.byref(l), C.byref(st)) == 0
            return np.array(buf[:], np.int64).reshape(world, 4), o.value, l.value, st.value
        for phase in (0, 1):
            plans = [plan(r, phase) for r in range(world)]
            staged = []
            for a in range(world):
                pa, own_off, own_len, stride = plans[a]
                assert pa[a].tolist() == [0, 0, 0, 0]
                assert start <= own_off <= end and own_off + own_len <= end
                assert stride % 64 == 0 and stride * world >= n
                slots = []
                for b in range(world):
                    if a == b:
                        continue
                    so, sl, _, _ = pa[b]
                    _, _, ro, rl = plans[b][0][a]
                    assert sl == rl, (world, start, end, phase, a, b)           # the pair agrees on the length
                    assert start <= so and so + sl <= end
                    if phase == 0:
                        assert ro + rl <= nbytes // 4
                    else:
                        assert start <= ro and ro + rl <= end
                    staged.append((b, phase, ro, grads[a][so:so + sl].copy()))
                    if phase == 0 and pa[b][3]:
                        slots.append((pa[b][2], pa[b][2] + pa[b][3]))
                slots.sort()
                assert all(x[1] <= y[0] for x, y in zip(slots, slots[1:]))      # my scratch slots do not overlap
            for b, ph, ro, data in staged:                                      # all transfers of a group land together
                (scratch[b] if ph == 0 else grads[b])[ro:ro + data.size] = data
            if phase == 0:
                for r in range(world):
                    _, own_off, own_len, stride = plans[r]
                    acc = None
                    for q in range(world):                                      # allreduce_sum_chunks_kernel's order
                        v = grads[r][own_off:own_off + own_len] if q == r else \
                            scratch[r][(q if q < r else q - 1) * stride:(q if q < r else q - 1) * stride + own_len]
                        acc = v.copy() if acc is None else acc + v
                    grads[r][own_off:own_off + own_len] = acc
        for r in range(world):
            assert np.array_equal(grads[r][start:end], want), (world, start, end, r)
            assert np.array_equal(grads[r][:start], before[r][:start]) and np.array_equal(grads[r][end:], before[r][end:])
    assert L.mrcnn_allreduce_direct_plan(world, world, 0, 10, 0, (C.c_int64 * (4 * world))(), None, None, None) != 0


def test_grad_reducer_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT})
    port = 29600 + (os.getpid() % 300)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs)


def test_keras_h5_weights_roundtrip_and_by_name_semantics(tmp_path):
    """Minimal HDF5 writer/reader (h5py absent): Keras save_weights layout, nested rpn_model group,
    TimeDistributed names, Conv2DTranspose kernel in the Keras (2,2,out,in) layout."""
    from caesar_mrcnn_amd import hdf5_min, weights_io
    from caesar_mrcnn_amd.config import run_py_config
    from caesar_mrcnn_amd.params import ParamLayout, init_weights, deconv_gemm_to_keras
    L = ParamLayout(run_py_config(backbone="custom"))
    w = init_weights(L, seed=4, perturb_bn=True)
    w["mrcnn_mask_deconv/kernel"] = deconv_gemm_to_keras(w["mrcnn_mask_deconv/kernel"])
    p = str(tmp_path / "rg-dataset20200127T1200" / "mask_rcnn_rg-dataset_0003.h5")
    weights_io.save(p, w, L)
    assert open(p, "rb").read(8) == b"\x89HDF\r\n\x1a\n"
    back = weights_io.load(p)
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) and back[k].dtype == np.float32 for k in w)
    f = hdf5_min.H5File(p)
    assert "rpn_model" in f.root.children and "rpn_conv_shared" not in f.root.children
    names = [n.decode() for n in f.root.attrs["layer_names"]]
    assert "conv1" in names and "mrcnn_mask_deconv" in names and "rpn_model" in names
    wn = [n.decode() for n in f.get(f.root, "mrcnn_class_bn1").attrs["weight_names"]]
    assert wn == ["mrcnn_class_bn1/gamma:0", "mrcnn_class_bn1/beta:0", "mrcnn_class_bn1/moving_mean:0",
                  "mrcnn_class_bn1/moving_variance:0"]
    assert f.read(f.get(f.root, "conv1/conv1/kernel:0")).shape == (7, 7, 3, 16)
    assert f.read(f.get(f.root, "mrcnn_mask_deconv/mrcnn_mask_deconv/kernel:0")).shape == (2, 2, 256, 256)
    with pytest.raises(KeyError):
        f.get(f.root, "no_such_layer")
    bad = tmp_path / "bad.h5"
    bad.write_bytes(b"not an hdf5 file at all")
    with pytest.raises(ValueError):
        hdf5_min.H5File(str(bad))


def test_prefetcher_order_errors_and_shutdown():
    """Loader threads in front of the batch generators (fit_generator(workers=...), model.py:2497-2510)."""
    import itertools
    import time
    from caesar_mrcnn_amd.datagen import Prefetcher

    def gen(k, n=None, fail_at=None):
        for i in itertools.count():
            if n is not None and i >= n:
                return
            if fail_at is not None and i == fail_at:
                raise ValueError("boom %d" % k)
            time.sleep(0.001)
            yield (k, i)

    p = Prefetcher([gen(0)], depth=3)
    assert [next(p) for _ in range(20)] == [(0, i) for i in range(20)]         # one worker: the generator's order
    p.close()
    p = Prefetcher([gen(k) for k in range(3)], depth=4)
    got = [next(p) for _ in range(60)]
    for k in range(3):
        mine = [i for kk, i in got if kk == k]
        assert mine == list(range(len(mine))) and len(mine) > 0                # every worker's own order is kept
    p.close()
    p = Prefetcher([gen(0, n=5), gen(1, n=3)], depth=2)
    assert sorted(p) == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2)]   # finite generators end the stream
    p = Prefetcher([gen(7, fail_at=2)], depth=2)
    assert next(p) == (7, 0) and next(p) == (7, 1)
    with pytest.raises(ValueError, match="boom 7"):
        next(p)


def test_resize_plan_matches_resize_image():
    """utils.resize_plan (the scalar half of resize_image that the device mold path works from) against resize_image itself:
    same scale, window, padding and scaled size for square / pad64 / none, up-scaled and unscaled, odd sizes."""
    from caesar_mrcnn_amd import utils
    rng = np.random.default_rng(3)
    for mode, min_dim, max_dim in (("square", 256, 256), ("square", 128, 192), ("pad64", 128, 1024), ("none", 256, 256)):
        for h, w in ((132, 132), (256, 256), (100, 180), (77, 201), (256, 130), (33, 47), (300, 200)):
            if mode == "square" and max(h, w) > max_dim and min(h, w) >= min_dim:
                continue                                        # scale < 1 never happens on this path (scale = max(1, ...)) unless max_dim caps it
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            out, window, scale, padding, crop = utils.resize_image(img, min_dim=min_dim, max_dim=max_dim, min_scale=0, mode=mode)
            s2, (oh, ow), pad2, win2 = utils.resize_plan(img.shape, min_dim, max_dim, 0, mode)
            assert s2 == scale and tuple(win2) == tuple(window) and [tuple(p) for p in pad2] == [tuple(p) for p in padding], (mode, h, w)
            assert out.shape[:2] == (oh + pad2[0][0] + pad2[0][1], ow + pad2[1][0] + pad2[1][1])


def test_bench_dump_outputs_and_step_count(tmp_path):
    """bench.py --dump-outputs: float32 .npy files within 64 MB, the same seeded sample positions run after run; --steps < 1
    is refused before any GPU work."""
    import types
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 3 * bench.DUMP_SAMPLE
    eng = types.SimpleNamespace(params=torch.arange(n, dtype=torch.float32), grads=-torch.arange(n, dtype=torch.float32))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]))
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["grads_sample.npy", "losses.npy", "params_sample.npy"]
    total = 0
    for f in names:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype == np.float32 and np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 << 20
    p = np.load(str(tmp_path / "a" / "params_sample.npy"))
    assert 0.8 * bench.DUMP_SAMPLE < p.size <= bench.DUMP_SAMPLE and np.all(np.diff(p) > 0)
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "grads_sample.npy")), -p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr
