"""Connected components of bit planes without a GPU: the library exports the entry points, mrcnn_mask_components_check /
_workspace answer as include/mrcnn_hip.h says (every cap just inside and just past it), min_area_rect is its two halves, and a
NumPy statement of the contract of csrc/components.hip -- run table from the words by the kernel's bit rules, union-find with
the smaller id as root, labels by the rank of the roots, pieces as planes, row extents -- agrees with analyze.label_components /
np.nonzero on every scene of tests/components_cases.py."""
import ctypes

import numpy as np
import pytest

import components_cases as cases
from caesar_mrcnn_amd import _hip, analyze

OK, ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -3, -4
NEW_SYMBOLS = ("mrcnn_mask_components_check", "mrcnn_mask_components_workspace", "mrcnn_mask_components_count",
               "mrcnn_mask_components_emit", "mrcnn_mask_row_extents")
MAX_SIDE, MAX_PLANES, MAX_RUNS, LDS_RUNS = 8192, 4096, 1 << 22, cases.LDS_RUNS


def _table(boxes):
    b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    return b, b.ctypes.data_as(ctypes.c_void_p)


def _check(n, H, W, conn, boxes, ws_bytes=None):
    L = _hip.lib()
    b, host = _table(boxes) if boxes is not None else (None, None)
    if ws_bytes is None:
        ws_bytes = L.mrcnn_mask_components_workspace(n, H, W, host)
    return L.mrcnn_mask_components_check(n, H, W, conn, host, ws_bytes)


def _words(box, H, W):
    """Workspace words of one box, as the header states them."""
    y1, x1, y2, x2 = max(box[0], 0), max(box[1], 0), min(box[2], H), min(box[3], W)
    bh, bw = (y2 - y1, x2 - x1) if y2 > y1 and x2 > x1 else (0, 0)
    cap = bh * ((bw + 1) // 2)
    return bh + 1 + (3 if cap > LDS_RUNS else 2) * cap


def test_library_exports_the_entry_points():
    assert set(NEW_SYMBOLS) <= set(_hip.exported_symbols())
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    from caesar_mrcnn_amd import ops
    assert issubclass(ops.ComponentsUnsupported, _hip.HipPathError)
    for name in ("mask_components", "mask_components_split", "mask_row_extents"):
        assert callable(getattr(ops, name))


def test_check_malformed_requests():
    box = [[0, 0, 4, 4]]
    assert _check(1, 8, 8, 4, box) == OK and _check(1, 8, 8, 8, box) == OK
    for n, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8)):
        assert _check(n, H, W, 4, box, 1 << 20) == ERR_ARG
    for conn in (0, 1, 3, 5, 6, 9, -4):
        assert _check(1, 8, 8, conn, box, 1 << 20) == ERR_ARG
    assert _check(1, 8, 8, 4, None, 1 << 20) == ERR_ARG
    assert _hip.lib().mrcnn_mask_components_workspace(0, 8, 8, _table(box)[1]) == 0


def test_check_caps_just_inside_and_just_past():
    L = _hip.lib()
    small = [[0, 0, 2, 2]]
    assert _check(1, MAX_SIDE, MAX_SIDE, 4, small) == OK
    assert _check(1, MAX_SIDE + 1, 8, 4, small, 1 << 20) == ERR_UNSUPPORTED and _check(1, 8, MAX_SIDE + 1, 8, small, 1 << 20) == ERR_UNSUPPORTED
    assert _check(MAX_PLANES, 8, 8, 4, small * MAX_PLANES) == OK
    assert _check(MAX_PLANES + 1, 8, 8, 4, small * (MAX_PLANES + 1), 1 << 30) == ERR_UNSUPPORTED
    # run capacity of one box: rows * ceil(columns / 2) <= 2^22
    assert 2048 * (4096 // 2) == MAX_RUNS
    assert _check(1, MAX_SIDE, MAX_SIDE, 4, [[0, 0, 2048, 4096]]) == OK
    assert _check(1, MAX_SIDE, MAX_SIDE, 4, [[0, 0, 2048, 4097]], 1 << 40) == ERR_UNSUPPORTED
    assert _check(1, MAX_SIDE, MAX_SIDE, 4, [[0, 0, 2049, 4096]], 1 << 40) == ERR_UNSUPPORTED
    assert _check(1, MAX_SIDE, MAX_SIDE, 4, [[5, 7, 2053, 4103]]) == OK                      # the same box elsewhere
    assert _check(1, 2048, 4096, 4, [[-9, -9, 1 << 20, 1 << 20]]) == OK                      # a box is cut to the frame first
    # workspace words of the whole table <= 2^31 - 1
    big = [0, 0, 2048, 4096]
    per = _words(big, MAX_SIDE, MAX_SIDE)
    most = (2 ** 31 - 1) // per
    assert 1 < most < MAX_PLANES
    assert _check(most, MAX_SIDE, MAX_SIDE, 4, [big] * most) == OK
    assert L.mrcnn_mask_components_workspace(most, MAX_SIDE, MAX_SIDE, _table([big] * most)[1]) == 4 * per * most
    assert _check(most + 1, MAX_SIDE, MAX_SIDE, 4, [big] * (most + 1), 1 << 40) == ERR_UNSUPPORTED
    assert L.mrcnn_mask_components_workspace(most + 1, MAX_SIDE, MAX_SIDE, _table([big] * (most + 1))[1]) == 0
    # the workspace itself
    boxes = [[0, 0, 40, 40], [3, 3, 4, 4], [0, 0, 0, 0]]
    need = L.mrcnn_mask_components_workspace(3, 64, 64, _table(boxes)[1])
    assert need == 4 * sum(_words(b, 64, 64) for b in boxes)
    assert _check(3, 64, 64, 4, boxes, need) == OK and _check(3, 64, 64, 4, boxes, need + 4) == OK
    assert _check(3, 64, 64, 4, boxes, need - 4) == ERR_WORKSPACE and _check(3, 64, 64, 4, boxes, 0) == ERR_WORKSPACE


def test_workspace_is_monotone_in_the_boxes():
    L = _hip.lib()
    H, W = 300, 260
    last = 0
    for grow in range(0, 300, 7):
        boxes = [[10, 10, 10 + grow, 10 + grow], [0, 0, grow, W], [H - grow, 0, H, 3]]
        got = L.mrcnn_mask_components_workspace(3, H, W, _table(boxes)[1])
        assert got == 4 * sum(_words(b, H, W) for b in boxes) and got >= last
        last = got
    # across the size at which a box gets its parent table in the workspace
    rows = LDS_RUNS // 128
    a = L.mrcnn_mask_components_workspace(1, 512, 256, _table([[0, 0, rows, 256]])[1])
    b = L.mrcnn_mask_components_workspace(1, 512, 256, _table([[0, 0, rows + 1, 256]])[1])
    assert a == 4 * (rows + 1 + 2 * LDS_RUNS) and b == 4 * (rows + 2 + 3 * (LDS_RUNS + 128))


# ---- the NumPy statement of the contract ---------------------------------------------------------------------------------
def _masked(word, k, x1, x2):
    lo, hi = x1 - 32 * k, x2 - 32 * k
    if lo > 0:
        word &= (0xFFFFFFFF << lo) & 0xFFFFFFFF
    if hi < 32:
        word &= (1 << hi) - 1
    return word


def run_table(words, box):
    """(row_off [bh + 1], start, end) of the runs of one plane [H, wpr] inside box, by the kernel's rules: a start is a set bit
    whose left neighbour is clear, an end one whose right neighbour is clear, and the j-th start of a row pairs with its j-th end."""
    y1, x1, y2, x2 = (int(v) for v in box)
    row_off, start, end = [0], [], []
    if y2 > y1 and x2 > x1:
        k0, k1 = x1 >> 5, (x2 - 1) >> 5
        for y in range(y1, y2):
            row = [_masked(int(words[y, k]), k, x1, x2) for k in range(k0, k1 + 1)] + [0]
            prev = 0
            for q, w in enumerate(row[:-1]):
                k = k0 + q
                starts = w & ~(((w << 1) & 0xFFFFFFFF) | prev)
                ends = w & ~((w >> 1) | ((row[q + 1] & 1) << 31))
                start.extend(32 * k + b for b in range(32) if starts >> b & 1)
                end.extend(32 * k + b for b in range(32) if ends >> b & 1)
                prev = w >> 31
            assert len(start) == len(end)
            row_off.append(len(start))
    return row_off, start, end


def label_runs(row_off, start, end, connectivity):
    """label per run (1..k, by the rank of the component's smallest run id) and k."""
    c = 1 if connectivity == 8 else 0
    parent = list(range(len(start)))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for r in range(1, len(row_off) - 1):
        i, j = row_off[r - 1], row_off[r]
        i1, j1 = j, row_off[r + 1]
        while i < i1 and j < j1:
            if start[i] <= end[j] + c and start[j] <= end[i] + c:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            if end[i] < end[j]:
                i += 1
            else:
                j += 1
    roots = [find(a) for a in range(len(parent))]
    rank = {root: q + 1 for q, root in enumerate(sorted(set(roots)))}
    return [rank[root] for root in roots], len(rank)


def emit_pieces(shape, box, row_off, start, end, label, wanted):
    """The planes [len(wanted), H, wpr] of the components `wanted`, with count and box, as mrcnn_mask_components_emit lays them out."""
    H, W = shape
    wpr = (W + 31) // 32
    out = np.zeros((len(wanted), H, wpr), np.uint32)
    count, obox = np.zeros(len(wanted), np.int32), np.zeros((len(wanted), 4), np.int32)
    for q, comp in enumerate(wanted):
        ys, xs = [], []
        for r in range(len(row_off) - 1):
            for j in range(row_off[r], row_off[r + 1]):
                if label[j] != comp:
                    continue
                for x in range(start[j], end[j] + 1):
                    out[q, box[0] + r, x >> 5] |= np.uint32(1 << (x & 31))
                count[q] += end[j] - start[j] + 1
                ys.append(box[0] + r)
                xs.extend((start[j], end[j]))
        if ys:
            obox[q] = (min(ys), min(xs), max(ys) + 1, max(xs) + 1)
    return out, count, obox


def row_extents(words, box):
    y1, x1, y2, x2 = (int(v) for v in box)
    out = []
    for y in range(y1, y2):
        first = last = -1
        for k in range(x1 >> 5, ((x2 - 1) >> 5) + 1):
            w = _masked(int(words[y, k]), k, x1, x2)
            if w:
                if first < 0:
                    first = 32 * k + (w & -w).bit_length() - 1
                last = 32 * k + w.bit_length() - 1
        out.append((first, last))
    return np.asarray(out, np.int32).reshape(-1, 2)


SMALL = [name for name, p in cases.scenes() if p.shape[1] * p.shape[2] <= 256 * 97]


@pytest.mark.parametrize("name", SMALL)
def test_statement_agrees_with_the_host_labelling(name):
    planes = cases.scene(name)
    n, H, W = planes.shape
    words = analyze.pack_mask_planes(np.moveaxis(planes, 0, -1))
    boxes = cases.boxes_of(planes)
    for conn in (4, 8):
        for p in range(n):
            labels, k = cases.reference(name, conn)[p]
            if conn == 8:
                assert k == analyze.count_islands(planes[p])
            row_off, start, end = run_table(words[p], boxes[p])
            label, got_k = label_runs(row_off, start, end, conn)
            assert got_k == k, (name, conn, p)
            # every run lies in one component of the host's map, numbered as the host numbers it
            for r in range(len(row_off) - 1):
                for j in range(row_off[r], row_off[r + 1]):
                    assert (labels[boxes[p][0] + r, start[j]:end[j] + 1] == label[j]).all(), (name, conn, p, j)
            assert sum(e - s + 1 for s, e in zip(start, end)) == int(planes[p].sum())
            if k <= 40:
                pieces, count, obox = emit_pieces((H, W), boxes[p], row_off, start, end, label, list(range(1, k + 1)))
                want = np.stack([labels == q + 1 for q in range(k)]) if k else np.zeros((0, H, W), bool)
                assert np.array_equal(analyze.unpack_mask_planes(pieces, W).astype(bool), want)
                want_count, want_box = cases.label_boxes(labels, k)
                assert np.array_equal(count, want_count) and np.array_equal(obox, want_box)
                assert np.array_equal(obox, cases.boxes_of(want))
    for p in range(n):
        ext = row_extents(words[p], boxes[p])
        ys, xs = np.nonzero(planes[p])
        for r, (first, last) in enumerate(ext):
            row = xs[ys == boxes[p][0] + r]
            assert (first, last) == ((row.min(), row.max()) if row.size else (-1, -1))


@pytest.mark.parametrize("name", SMALL)
def test_min_area_rect_is_its_two_halves(name):
    for plane in cases.scene(name):
        points = analyze.row_extreme_points(plane)
        ys, xs = np.nonzero(plane)
        if ys.size == 0:
            assert points is None and analyze.min_area_rect(plane) is None
            continue
        rows = np.unique(ys)
        want = [(xs[ys == y].min(), y) for y in rows] + [(xs[ys == y].max(), y) for y in rows]
        assert points.tolist() == [[int(x), int(y)] for x, y in want]
        assert analyze.min_area_rect_of_points(points) == analyze.min_area_rect(plane)
        # the same points from the row-extent table of the plane's box
        y1 = int(rows[0])
        table = np.full((int(rows[-1]) + 1 - y1, 2), -1, np.int32)
        for y in rows:
            table[y - y1] = (xs[ys == y].min(), xs[ys == y].max())
        again = analyze.row_extents_points(table, y1)
        assert np.array_equal(again, points) and analyze.min_area_rect_of_points(again) == analyze.min_area_rect(plane)
    assert analyze.row_extents_points(np.full((3, 2), -1, np.int32), 5) is None


def test_min_area_rect_keeps_its_values():
    """The rectangle of a plane whose hull is known: a 3 x 5 block, a single pixel, one row."""
    m = np.zeros((12, 20), bool)
    m[4:7, 8:13] = True
    centre, size, angle = analyze.min_area_rect(m)
    assert centre == (10.0, 5.0) and sorted(size) == [2.0, 4.0] and angle == 90.0
    m[:] = False
    m[3, 7] = True
    assert analyze.min_area_rect(m) == ((7.0, 3.0), (0.0, 0.0), 90.0)


def test_switch_is_off_by_default_and_handed_on(monkeypatch):
    import analyze_post_cases as post
    import tester_cases as T
    from caesar_mrcnn_amd import sfinder
    from caesar_mrcnn_amd.config import run_py_config
    an = analyze.Analyzer(post.StubModel(None), post.cfg())
    assert an.components_device is False and analyze.Analyzer.COMPONENTS_DEVICE is False and an.components_timing == {}
    # SFinder -> its tile tasks -> every tile's Analyzer
    cfg = run_py_config(num_classes=4, imgsize=64, mode="inference")
    cfg.IMG_PATH = "none.fits"
    assert sfinder.SFinder(None, cfg).components_device is False
    for want in (False, True):
        task = sfinder.TileTask((0, 9, 0, 9), None, cfg)
        assert task.components_device is False
        task.components_device = want
        assert task._analyzer().components_device is want
    # ModelTester -> every image's Analyzer (None: the Analyzer's own default)
    seen = []
    monkeypatch.setattr(analyze.Analyzer, "inspect_results", lambda self, image_id, path: seen.append(self.components_device) or -1)
    ds = T.StubDataset()
    ds.add(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 0), int), [], [])
    for want in (None, True, False):
        tester = analyze.ModelTester(None, T.cfg(), ds)
        assert tester.components_device is None
        tester.components_device = want
        monkeypatch.setattr(tester, "compute_performances", lambda: None)
        monkeypatch.setattr(tester, "save", lambda: None)
        assert tester.test() == 0
    assert seen == [False, True, False]


def test_switch_on_without_gpu_takes_the_host_statement():
    """Where no GPU is there, split_gtmasks and split_masks with the switch on run the host statement (and give its lists anywhere)."""
    import analyze_post_cases as post
    import tester_cases as T
    from caesar_mrcnn_amd.utils import extract_bboxes
    sc = T.scenario("split_gt")
    runs = []
    for on in (True, False):
        an = analyze.Analyzer(None, T.cfg(), T.StubDataset(True), [], [])
        an.components_device = on
        T.drive(an, sc, extract_bboxes)
        runs.append(an)
    assert (runs[0].components_timing == {}) == (not analyze.Analyzer.has_gpu(None)) and len(runs[0].masks_gt_merged) == len(runs[1].masks_gt_merged) >= 2
    assert all(np.array_equal(a, b) for a, b in zip(runs[0].masks_gt_merged, runs[1].masks_gt_merged))
    name, shape, objs, settings = [c for c in post.scenarios() if c[0] == "split_two_islands"][0]
    outs = []
    for on in (True, False):
        an = post.analyzer(objs, shape, settings, device=False)
        an.components_device = on
        outs.append(post.run(an, shape))
    post.assert_same(outs[0], outs[1], name)
