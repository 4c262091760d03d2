"""csrc/outline.hip (ops.bitmap_outlines / mask_plane_outlines) against analyze.find_contours on the 1-padded mask and np.argwhere,
and the switches built on it (Analyzer.results_device, SFinder.results_device) against the host statement: exact equality
throughout.  Frames are at most 132 x 132; the case of n = 100 sources runs at 3 x 33.

A contour is a closed walk over 4-adjacent cells of the (bipartite) cell grid, one segment per cell visit, so its segment count is
even: the counts around a power of two that a loop can have are 2^k - 2, 2^k and 2^k + 2 (outline_cases.loop_of), not 2^k +- 1."""
import ctypes
import json

import numpy as np
import pytest
import torch

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import _hip, analyze, ops

import analyze_post_cases as post
import outline_cases as cases

pytestmark = pytest.mark.gpu

FORMS = [("lds", 1536), ("global", 0)]               # the ranking's two forms, by the "outline_lds_segs" threshold


@pytest.fixture(params=FORMS, ids=[f[0] for f in FORMS])
def form(request):
    ops.tuning_set("outline_lds_segs", request.param[1])
    yield request.param[0]
    ops.tuning_set("outline_lds_segs", 1536)


def _outlines(masks, dev, seed=None):
    pool, desc = cases.pack_sources(masks, seed)
    pool_t, desc_t = ops.tile_upload(pool, desc, dev) if all(m.size for m in masks) else (
        torch.from_numpy(pool.view(np.int32)).to(dev), torch.from_numpy(desc).to(dev))
    return ops.bitmap_outlines(pool_t, desc_t, desc)


def test_sizes(dev, form):
    """Widths 1 .. 132 with heights 1 .. 132: random, empty and full masks, one call per width."""
    grid = cases.size_grid()
    for w in cases.WIDTHS:
        masks = [m for _, m in grid if m.shape[1] == w]
        assert len(masks) == 3 * len(cases.HEIGHTS)
        cases.assert_outlines(_outlines(masks, dev).host(), masks, "width %d" % w)


@pytest.mark.parametrize("name,mask", cases.shapes(), ids=[s[0] for s in cases.shapes()])
def test_shapes(dev, form, name, mask):
    got = _outlines([mask], dev).host()
    cases.assert_outlines(got, [mask], name)
    lengths = np.diff(got["contour_offsets"]) - 1
    if name.startswith("loop_"):
        assert lengths.tolist() == [int(name[5:])]
    if name == "serpentine":
        assert lengths.size == 1 and lengths[0] > 4096            # one loop, past the LDS form's size: the global form by itself
    if name.startswith("diagonal_"):
        assert lengths.tolist() == [4, 4]                         # the saddle keeps the two pixels apart
    if name == "isolated_pixels":
        assert lengths.size == 17 * 34 and set(lengths.tolist()) == {4}
    if name == "ring_island":
        assert lengths.size == 4                                  # ring, its hole, the island, the island's hole


def test_full_mask_runs_along_the_frame(dev):
    got = _outlines([np.ones((3, 33), np.uint8)], dev).host()
    pts = got["points"]
    assert pts.shape[0] == 2 * (3 + 33) + 1 and np.array_equal(pts[0], pts[-1])
    assert pts[:, 0].min() == -0.5 and pts[:, 0].max() == 32.5 and pts[:, 1].min() == -0.5 and pts[:, 1].max() == 2.5


@pytest.mark.parametrize("n", [1, 2, 9, 100])
def test_source_counts(dev, form, n):
    shape = (3, 33) if n == 100 else (40, 70)
    masks = [cases.random_mask(shape[0], shape[1], 7 * n + k, 0.45) for k in range(n)]
    cases.assert_outlines(_outlines(masks, dev).host(), masks, "n = %d" % n)
    # the same masks as the bit planes of one frame
    stack = np.ascontiguousarray(np.stack(masks, axis=-1))
    planes = ops.mask_planes_pack(torch.from_numpy(stack).to(dev))
    cases.assert_outlines(ops.mask_plane_outlines(planes).host(), masks, "planes, n = %d" % n)


def _mixed():
    return [cases.random_mask(5, 70, 1, 0.5), cases.serpentine(20, 33), np.ones((2, 64), np.uint8), cases.random_mask(132, 31, 2, 0.2),
            np.zeros((4, 40), np.uint8), cases.random_mask(1, 132, 3, 0.5), cases.blobs((60, 100), 1, 8)[0]]


def test_mixed_sources_in_one_call(dev, form):
    """Different sizes, nonzero x0 / y0 and word_offset, words_per_row larger than needed, garbage in every padding bit."""
    masks = _mixed()
    pool, desc = cases.pack_sources(masks, seed=11)
    assert (desc[:, 4] > 0).all() and (desc[:, 5] > (desc[:, 2] + 31) // 32).any() and (desc[:, :2] != 0).any()
    cases.assert_outlines(_outlines(masks, dev, seed=11).host(), masks, "mixed")


def test_zero_sized_source_between_two_others(dev, form):
    a, b = cases.random_mask(9, 40, 21, 0.5), cases.random_mask(6, 33, 22, 0.5)
    pool, desc = cases.pack_sources([a, b])
    for w, h in ((0, 0), (0, 5), (7, 0), (-3, 4)):
        table = np.array([desc[0], (3, 4, w, h, 0, 0), desc[1]], np.int32)
        got = ops.bitmap_outlines(torch.from_numpy(pool.view(np.int32)).to(dev), torch.from_numpy(table).to(dev), table).host()
        assert got["source_contours"][1] == got["source_contours"][2] and got["pixel_offsets"][1] == got["pixel_offsets"][2]
        keep = {k: v for k, v in got.items()}
        keep["source_contours"] = np.delete(got["source_contours"], 1)
        keep["pixel_offsets"] = np.delete(got["pixel_offsets"], 1)
        cases.assert_outlines(keep, [a, b], "zero-sized %r" % ((w, h),))


def test_desc_is_read_back_when_no_host_copy_is_given(dev):
    masks = _mixed()[:3]
    pool, desc = cases.pack_sources(masks, seed=5)
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    cases.assert_outlines(ops.bitmap_outlines(pool_t, desc_t).host(), masks, "desc read back")


def test_device_tensors_and_repeat_are_bitwise_equal(dev, form):
    masks = _mixed()
    first, second = _outlines(masks, dev, seed=3), _outlines(masks, dev, seed=3)
    host = first.host()
    for name in ("points", "contour_offsets", "source_contours", "pixels", "pixel_offsets"):
        a, b = getattr(first, name), getattr(second, name)
        assert a.is_cuda and a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert np.array_equal(a.cpu().numpy().view(np.int32), np.ascontiguousarray(host[name]).view(np.int32)), name
    assert first.points.dtype == torch.float32 and first.points.shape[1] == 2 and first.pixels.shape[1] == 2


# ---- refusals: in the table only -- nothing large is allocated, nothing is launched -------------------------------------------
def _table(*rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def _status(table, pool_words, totals=None):
    L = _hip.lib()
    t = None if totals is None else np.ascontiguousarray(totals, np.int32)
    return L.mrcnn_outline_check(table.ctypes.data_as(ctypes.c_void_p), table.shape[0], int(pool_words),
                                 None if t is None else t.ctypes.data_as(ctypes.c_void_p))


def _refused_cases():
    ok = (0, 0, 40, 5, 0, 2)
    big = 2 ** 31 - 1
    yield "no source", _table(ok)[:0], 10, None, -1
    yield "negative pool", _table(ok), -1, None, -1
    yield "past the pool", _table(ok), 9, None, -1
    yield "second source past the pool", _table(ok, (0, 0, 40, 5, 1, 2)), 10, None, -1
    yield "negative offset", _table((0, 0, 40, 5, -1, 2)), 10, None, -1
    yield "row pitch too small", _table((0, 0, 65, 5, 0, 2)), 100, None, -1
    yield "negative total", _table(ok), 10, [[-1, 0]], -1
    yield "width cap + 1", _table((0, 0, 8193, 1, 0, 257)), 257, None, -4
    yield "height cap + 1", _table((0, 0, 1, 8193, 0, 1)), 8193, None, -4
    yield "sources cap + 1", np.tile(_table(ok), (65536, 1)), 10, None, -4
    yield "pool cap + 1", _table(ok), big + 1, None, -4
    yield "segments cap + 1", _table((0, 0, 8192, 8192, 0, 256)), 8192 * 256, [[2 ** 22 + 1, 0]], -4
    # 410 sources: S = 1717986919 segments need S + S / 4 = 2^31 points; one segment fewer fits
    seg = [2 ** 22] * 409 + [1717986919 - 409 * 2 ** 22]
    yield "points cap + 1", np.tile(_table((0, 0, 8192, 8192, 0, 256)), (410, 1)), 8192 * 256, [[s, 0] for s in seg], -4
    yield "pixels cap + 1", np.tile(_table((0, 0, 8192, 8192, 0, 256)), (64, 1)), 8192 * 256, [[0, 2 ** 25]] * 64, -4


def _accepted_cases():
    ok = (0, 0, 40, 5, 0, 2)
    big = 2 ** 31 - 1
    yield "plain", _table(ok), 10, None
    yield "at the width and height caps", _table((0, 0, 8192, 8192, 0, 256)), 8192 * 256, [[2 ** 22, 8192 * 8192]]
    yield "65535 sources", np.tile(_table(ok), (65535, 1)), 10, None
    yield "pool at its cap", _table(ok), big, None
    seg = [2 ** 22] * 409 + [1717986918 - 409 * 2 ** 22]
    yield "points at their cap", np.tile(_table((0, 0, 8192, 8192, 0, 256)), (410, 1)), 8192 * 256, [[s, 0] for s in seg]
    yield "pixels at their cap", np.tile(_table((0, 0, 8192, 8192, 0, 256)), (64, 1)), 8192 * 256, [[0, 2 ** 25]] * 63 + [[0, 2 ** 25 - 1]]
    yield "empty sources only", _table((0, 0, 0, 0, -5, 0), (0, 0, -1, 9, 0, 0)), 0, [[0, 0], [0, 0]]


def test_check_entry_refuses_and_accepts():
    for name, table, words, totals, want in _refused_cases():
        assert _status(table, words, totals) == want, name
    for name, table, words, totals in _accepted_cases():
        assert _status(table, words, totals) == 0, name
        size = _hip.lib().mrcnn_outline_workspace(table.ctypes.data_as(ctypes.c_void_p), table.shape[0], int(words), None)
        assert size > 0, name


def test_real_entries_refuse_without_launching(dev):
    """The C entries answer with the check's status before they read a pointer: the buffers here are 64 ints."""
    L = _hip.lib()
    t = torch.full((64,), 7, dtype=torch.int32, device=dev)
    p, s = t.data_ptr(), _hip.current_stream()
    for name, table, words, totals, want in _refused_cases():
        host = table.ctypes.data_as(ctypes.c_void_p)
        assert L.mrcnn_outline_workspace(host, table.shape[0], int(words), None) == 0 or totals is not None, name
        if totals is None:
            assert L.mrcnn_outline_count(p, int(words), host, p, table.shape[0], p, 256, p, p, s) == want, name
        th = np.ascontiguousarray(totals if totals is not None else np.zeros((max(table.shape[0], 1), 2)), np.int32)
        assert L.mrcnn_outline_emit(p, int(words), host, p, table.shape[0], th.ctypes.data_as(ctypes.c_void_p), p, 256, p, 256, p, p, 16,
                                    p, 16, p, p, 16, s) == want, name
    torch.cuda.synchronize()
    assert bool((t == 7).all())                                   # nothing was written
    # the wrappers: ValueError for a malformed table, OutlineUnsupported past a cap -- before anything is allocated
    pool = torch.zeros(16, dtype=torch.int32, device=dev)
    for table, err in ((_table((0, 0, 40, 5, 8, 2)), ValueError), (_table((0, 0, 40, 5, 0, 1)), ValueError),
                       (_table((0, 0, 8193, 1, 0, 257)), ValueError), (_table((0, 0, 40, 5, 0, 2))[:0], ValueError)):
        with pytest.raises(err):
            ops.bitmap_outlines(pool, torch.from_numpy(np.ascontiguousarray(table).reshape(-1, 6)).to(dev), table)
    wide = torch.zeros(257, dtype=torch.int32, device=dev)
    with pytest.raises(ops.OutlineUnsupported):
        ops.bitmap_outlines(wide, torch.from_numpy(_table((0, 0, 8193, 1, 0, 257))).to(dev), _table((0, 0, 8193, 1, 0, 257)))
    assert issubclass(ops.OutlineUnsupported, _hip.HipPathError)
    with pytest.raises(_hip.HipPathError):
        ops.tuning_set("outline_lds_segs", 1537)


# ---- the switches: Analyzer.results_device, SFinder.results_device -------------------------------------------------------------
def _blob_objs(shape, n, seed):
    rng = np.random.default_rng(seed)
    return [(m.astype(bool), int(rng.integers(1, 4)), float(rng.uniform(0.7, 1.0))) for m in cases.blobs(shape, n, seed)]


def _analyzer_cases():
    by_name = {s[0]: s for s in post.scenarios()}
    out = [by_name[k] for k in ("chain_of_three", "other_classes_touch_and_diagonal", "split_two_islands", "merge_and_select_off",
                                "one_row_and_empty", "one_detection", "one_pixel_frame", "discs_24")]
    out.append(("blobs_with_holes", (100, 132), _blob_objs((100, 132), 10, 8), {"merge_overlapped_masks": False}))
    out.append(("boxes_not_polygons", (70, 100), by_name["chain_of_three"][2], {"use_polygon_regions": False}))
    return out


def _run_analyzer(case, tmp_path, tag, results_device, postprocess_device):
    name, shape, objs, settings = case
    an = post.analyzer(objs, shape, settings, device=postprocess_device)
    an.write_to_json = an.write_to_ds9 = True
    an.outfile_json, an.outfile_ds9 = str(tmp_path / (tag + ".json")), str(tmp_path / (tag + ".reg"))
    an.results_device, an.results_device_min_masks = results_device, 1         # (the class default is to hold a measured break-even)
    return post.run(an, shape)                                    # xmin = 7, ymin = 11


@pytest.mark.parametrize("postprocess_device", [True, False], ids=["planes_reused", "masks_uploaded"])
@pytest.mark.parametrize("case", _analyzer_cases(), ids=lambda c: c[0])
def test_analyzer_results_device_equals_host(dev, tmp_path, case, postprocess_device):
    ref = _run_analyzer(case, tmp_path, "host", False, postprocess_device)
    got = _run_analyzer(case, tmp_path, "device", True, postprocess_device)
    n = len(ref.masks_final)
    assert n >= 1 and ref.results_timing == {}
    assert got.results_timing["masks"] == n                       # the device form ran ...
    assert got.results_timing["mask_uploads"] == (0 if postprocess_device else 1)      # ... on the planes already there, or one upload
    post.assert_same(got, ref, case[0])
    assert json.dumps(got.results, sort_keys=True) == json.dumps(ref.results, sort_keys=True)
    assert len(ref.obj_regions) >= 1 and ("box(" if case[3].get("use_polygon_regions") is False else "polygon(") in ref.obj_regions[0]
    for ext in (".json", ".reg"):
        a, b = (tmp_path / ("device" + ext)).read_bytes(), (tmp_path / ("host" + ext)).read_bytes()
        assert len(b) > 0 and a == b, (case[0], ext)


def test_analyzer_results_device_with_nothing_detected(dev, tmp_path):
    for objs in ([], [(post.rect((70, 100), 5, 15, 5, 15), post.COMPACT, 0.5)]):             # no detection; none above the score cut
        case = ("nothing", (70, 100), objs, {})
        got, ref = _run_analyzer(case, tmp_path, "device", True, True), _run_analyzer(case, tmp_path, "host", False, True)
        assert got.results == ref.results and got.obj_regions == ref.obj_regions == [] and got.results_timing == {}
        assert not (tmp_path / "device.reg").exists() and not (tmp_path / "host.reg").exists()


def test_analyzer_results_device_threshold_and_other_values(dev, tmp_path):
    case = [s for s in post.scenarios() if s[0] == "chain_of_three"][0]
    an = _run_analyzer(case, tmp_path, "a", True, False)
    ref = an.results
    assert an.results_timing["masks"] == len(an.masks_final) == 2
    an.results_device_min_masks = 3                               # fewer final masks than the threshold: the host statement
    an.make_json_results()
    assert an.results_timing == {} and an.results == ref
    an.results_device_min_masks = 1
    an.masks_final = [np.asarray(m).astype(np.int32) * 2 for m in an.masks_final]      # values other than 0 / 1: the host statement
    an.make_json_results()
    got = an.results
    assert an.results_timing == {} and all(o["pixels"] == [] for o in got["objs"])       # `mask == 1` finds nothing ...
    assert [o["vertexes"] for o in got["objs"]] != [o["vertexes"] for o in ref["objs"]]  # ... and 0.5 between 0 and 2 lies elsewhere
    an.make_json_results_host()
    assert an.results == got


def _ring_scenario():
    """A 128 x 64 mosaic of two 64-tiles; a ring that the border x = 64 cuts in two (the merged source has a hole), a bar cut in
    two below it, and an interior source."""
    import sfinder_cases as S
    sc = S._scenario("ring", [], nx=128, ny=64, tile=64)
    tiles = S.tiles_of(sc)
    ring = S.union(S.rect(10, 13, 50, 80), S.rect(27, 30, 50, 80), S.rect(10, 30, 50, 53), S.rect(10, 30, 77, 80))
    bar = S.rect(40, 44, 60, 70)
    dets = [(tid, 3, 0.9, S.clip(ring, tiles[tid])) for tid in (0, 1)] + [(tid, 2, 0.8, S.clip(bar, tiles[tid])) for tid in (0, 1)]
    dets.append((0, 2, 0.95, S.rect(50, 55, 10, 20)))
    sc["dets"] = sorted(dets, key=lambda d: d[0])
    return sc


def test_sfinder_results_device_equals_host(dev, monkeypatch):
    import sfinder_cases as S
    from caesar_mrcnn_amd import sfinder
    sc = _ring_scenario()
    calls = []
    real = ops.bitmap_outlines
    monkeypatch.setattr(ops, "bitmap_outlines", lambda *a, **k: calls.append(1) or real(*a, **k))

    def run(results_device, merge):
        cfg = S.make_config()
        sf = sfinder.SFinder(None, cfg)
        sf.results_device = results_device
        _, sources = S.drive(sf, sc, cfg, merge=getattr(sf, merge))
        return S.canon(sources), sources
    host, _ = run(False, "merge_edge_sources_host")
    off, _ = run(False, "merge_edge_sources_device")
    assert calls == []
    on, raw = run(True, "merge_edge_sources_device")
    assert calls == [1]                                           # all unions in one call
    assert on == off == host
    assert json.dumps(on, sort_keys=True) == json.dumps(host, sort_keys=True)
    merged = [s for s in on if s["merged"]]
    assert len(merged) == 2 and sorted(len(s["vertexes"]) for s in merged) == [1, 2]          # the ring: its outline and its hole
    for s in raw:                                                 # plain Python values, as the host path leaves them
        assert all(type(v[0]) is float and type(v[1]) is float for c in s["vertexes"] for v in c)
