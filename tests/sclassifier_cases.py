"""Hand-built catalogues, mosaics and planted detections of the source-classifier tests.  Not a test module: imported by
test_sclassifier_cpu.py, test_sclassifier_gpu.py and golden/make_sclassifier_fixtures.py (which runs the reference's
SClassifier.classify_source on the same scenarios and records what it did in golden/sclassifier.npz).

A scenario: ``size`` (scutout_size), ``sources`` [(name, x0, y0, xmin, xmax, ymin, ymax)], ``planted`` {cut-out name: (boxes,
scores, class ids) or "fail"} -- what the stand-in Analyzer answers for the cut-out of that source --, ``iou_thr``, ``n_max`` and
``image`` (a function returning the float32 mosaic).  In every scenario that goes to the reference a cut-out with a planted
detection has a second member, and no source is as large as the cut-out: the reference raises on both."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "sclassifier.npz")

CLASS_NAMES = ["bkg", "sidelobe", "source", "galaxy_C2", "galaxy_C3"]


class Cfg(object):
    NUM_CLASSES = len(CLASS_NAMES)
    CLASS_NAMES = CLASS_NAMES


def src(name, x0, y0, hw=2, hh=None):
    hh = hw if hh is None else hh
    return (name, x0, y0, x0 - hw, x0 + hw, y0 - hh, y0 + hh)


def plain_image(ny=120, nx=120, seed=3):
    def make():
        rng = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:ny, 0:nx]
        img = rng.normal(0.0, 1.0, (ny, nx)).astype(np.float32)
        img += (50 * np.exp(-0.5 * (((yy - 50) / 3.0) ** 2 + ((xx - 50) / 4.0) ** 2))).astype(np.float32)
        return img
    return make


def nan_image():
    """60 x 80: a pixel far below everything at (row 20, column 10) -- inside the first cut-out only --, NaNs in columns 28..34 of
    rows 15..25: the overlap of the first two cut-outs and beyond, and a NaN block the third cut-out shares with the second."""
    rng = np.random.RandomState(5)
    img = rng.normal(10.0, 1.0, (60, 80)).astype(np.float32)
    img[20, 10] = -40.0
    img[15:26, 28:35] = np.nan
    img[18:22, 40:46] = np.nan
    return img


def scenarios():
    """The scenarios the reference can run (the fixture)."""
    out = []
    # window of A at size 20: x, y in (40, 60).  Centres exactly on each edge are outside (strict comparisons); boxes exactly
    # touching each edge are cut (<= / >=); one pixel inside they are not.
    edge = [src("A", 50, 50),
            src("onL", 40, 50), src("onR", 60, 50), src("onT", 50, 40), src("onB", 50, 60), src("inL", 40.5, 50.5, 0.25),
            ("tL", 45, 50, 40, 47, 48, 52), ("tR", 55, 50, 53, 60, 48, 52), ("tT", 50, 45, 48, 52, 40, 47), ("tB", 50, 55, 48, 52, 53, 60),
            ("nL", 44, 44, 41, 46, 41, 46), ("nR", 56, 56, 54, 59, 54, 59)]
    out.append(dict(name="edges", size=20, sources=edge, iou_thr=0.6,
                    planted={"A": ([[8, 8, 12, 12], [1, 1, 6, 6], [30, 30, 35, 35]], [0.9, 0.8, 0.95], [2, 1, 3])}))
    # fractional centres: 51.2 - 10.5 = 40.7 -> 40 (rounding gives 41), 10.2 - 10.5 = -0.3 -> 0 (floor gives -1)
    out.append(dict(name="trunc", size=21, iou_thr=0.6,
                    sources=[src("A", 51.2, 49.5), src("in", 40.5, 45.25, 0.25), src("out", 61.9, 50, 0.5), src("E", 10.2, 30.7),
                             src("e2", 0.5, 25.5, 0.25), src("e3", 15.0, 20.3, 1)],
                    planted={"A": ([[8.5, 9.2, 12.5, 13.2]], [0.75], [2]), "E": ([[8, 8.2, 12, 12.2], [13, 13, 15, 15]], [0.8, 0.9], [1, 4])}))
    # two detections with equal IoU (0.6) to A: the later wins; one with IoU exactly 0.5 = iou_thr to B: not matched
    out.append(dict(name="ties", size=20, iou_thr=0.5, sources=[src("A", 50, 50), ("B", 54, 52, 50, 54, 50, 54)],
                    planted={"A": ([[8, 7, 12, 11], [8, 9, 12, 13], [10, 10, 14, 18]], [0.9, 0.8, 0.7], [1, 2, 3])}))
    # B is visited through A and skipped; C is cut in A's and in D's cut-out and classified in both (and has its own turn);
    # A and B share a detection (snames)
    visit = [src("A", 50, 50), src("B", 53, 50), ("C", 58, 50, 56, 63, 48, 52), src("D", 66, 50), src("far", 100, 100)]
    planted = {"A": ([[8, 8, 12, 15], [8, 16, 12, 23]], [0.9, 0.85], [2, 3]), "D": ([[8, 0, 12, 7], [8, 8, 12, 12]], [0.8, 0.99], [3, 1])}
    out.append(dict(name="visit", size=20, iou_thr=0.3, sources=visit, planted=planted))
    out.append(dict(name="nmax", size=20, iou_thr=0.3, sources=visit, planted=planted, n_max=2))
    # predict fails for A: nobody becomes visited through it, B gets a cut-out of its own
    out.append(dict(name="predfail", size=20, iou_thr=0.3, sources=visit, planted=dict(planted, A="fail", B=planted["A"])))
    # the in-place NaN fill: B's cut-out overlaps A's and sees A's fill value (-40), which lies below B's own minimum
    out.append(dict(name="nanfill", size=24, iou_thr=0.6, image=nan_image,
                    sources=[src("A", 20, 20), ("B", 30, 20, 25, 36, 18, 22), ("C", 44, 22, 38, 58, 20, 24), src("lone", 60, 45)],
                    planted={"A": ([[10, 10, 14, 14]], [0.9], [2]), "B": ([[10, 7, 14, 18]], [0.8], [3])}))
    for sc in out:
        sc.setdefault("n_max", -1)
        sc.setdefault("image", plain_image())
    return out


def departures():
    """Scenarios the reference raises on; the port's stated behaviour is tested instead."""
    def all_nan():
        img = plain_image(60, 60)()
        img[0:30, 0:30] = np.nan
        return img
    out = [
        # a source as wide as the cut-out: warned, bbox_cut, never visited through its own cut-out
        dict(name="oversized", size=20, iou_thr=0.5, sources=[("big", 50, 50, 40, 60, 48, 52), src("n", 53, 53)],
             planted={"big": ([[8, 0, 12, 20]], [0.9], [3])}),
        # a degenerate catalogue box and a degenerate detection: IoU 0 with everything
        dict(name="degenerate", size=20, iou_thr=0.5, sources=[("flat", 50, 50, 48, 52, 50, 50), src("n", 54, 54)],
             planted={"flat": ([[10, 8, 10, 12], [12, 12, 16, 16], [5, 5, 5, 9]], [0.9, 0.8, 0.7], [1, 2, 3])}),
        # a lone source with a detection (the reference's unbound bbox_j)
        dict(name="lone", size=20, iou_thr=0.5, sources=[src("L", 50, 50)], planted={"L": ([[8, 8, 12, 12]], [0.9], [2])}),
        # negative corner, a window past the far edge (empty), an all-NaN window: each fails alone, the neighbour "ok" is classified
        dict(name="windows", size=20, iou_thr=0.5, image=all_nan,
             sources=[src("neg", 5, 40), src("past", 80, 40), src("nan", 15, 15), src("ok", 40, 40), src("ok2", 43, 40)],
             planted={"ok": ([[8, 8, 12, 12]], [0.9], [2])}),
    ]
    for sc in out:
        sc.setdefault("n_max", -1)
        sc.setdefault("image", plain_image())
    return out


# ---- the stand-in Analyzer and the loop --------------------------------------------------------------------------------
def analyzer_class(planted, log):
    """An Analyzer whose predict answers the cut-out called image_id with what `planted` holds for it, and logs the call."""
    class StubAnalyzer(object):
        def __init__(self, model, config, *a, **k):
            self.iou_thr = self.score_thr = None
            self.write_to_json = self.write_to_ds9 = self.draw = True
            self.bboxes, self.scores_final, self.class_ids_final = [], [], []

        def predict(self, image, image_id='', bboxes_gt=[]):
            log.append({"name": image_id, "image": np.array(image), "boxes": np.array(bboxes_gt, dtype=np.float64).reshape(-1, 4),
                        "thr": (self.iou_thr, self.score_thr), "writes": (self.write_to_json, self.write_to_ds9, self.draw)})
            p = planted.get(image_id)
            if p == "fail":
                return -1
            if p:
                self.bboxes, self.scores_final, self.class_ids_final = [list(b) for b in p[0]], list(p[1]), list(p[2])
            return 0
    return StubAnalyzer


def setup(clf, sc, sdata_class):
    clf.sources = []
    for row in sc["sources"]:
        s = sdata_class()
        s.name, s.x0, s.y0, s.xmin, s.xmax, s.ymin, s.ymax = row
        clf.sources.append(s)
    clf.img_data = sc["image"]()
    clf.ny, clf.nx = clf.img_data.shape
    clf.scutout_size, clf.iou_thr, clf.n_max_sources = sc["size"], sc["iou_thr"], sc["n_max"]
    return clf


def drive(clf):
    """The loop of SClassifier.run over classify_source: (status per call, visited flags after every call)."""
    statuses, visited = [], []
    for i in range(len(clf.sources)):
        if clf.n_max_sources > 0 and i >= clf.n_max_sources:
            break
        statuses.append(clf.classify_source(i))
        visited.append([bool(s.visited) for s in clf.sources])
    return statuses, visited


def class_infos(clf):
    """[(source index, class_id, class_name, 'a,b' of snames)] in source order, entries in the order they were added."""
    return [(i, int(c.class_id), str(c.class_name), ",".join(c.snames)) for i, s in enumerate(clf.sources) for c in s.class_info]


def record(clf, log, statuses, visited):
    rec = {"statuses": np.array(statuses, np.int64), "visited": np.array(visited, bool).reshape(len(statuses), len(clf.sources)),
           "img_data": np.array(clf.img_data), "ncalls": np.array(len(log)), "call_names": np.array([e["name"] for e in log], dtype="U32")}
    for k, e in enumerate(log):
        rec["call%d_boxes" % k] = e["boxes"]
    ci = class_infos(clf)
    rec["ci_source"] = np.array([c[0] for c in ci], np.int64)
    rec["ci_class_id"] = np.array([c[1] for c in ci], np.int64)
    rec["ci_class_name"] = np.array([c[2] for c in ci], dtype="U32")
    rec["ci_snames"] = np.array([c[3] for c in ci], dtype="U64")
    return rec


def literal_members(sources, i, size):
    """The member scan as the double loop states it: (window, [j], [cut]) -- the slow statement the NumPy form is checked against."""
    _, x0, y0 = sources[i][:3]
    xmin, xmax, ymin, ymax = int(x0 - size / 2), int(x0 + size / 2), int(y0 - size / 2), int(y0 + size / 2)
    js, cut = [], []
    for j, (_, xj, yj, bx0, bx1, by0, by1) in enumerate(sources):
        if j == i or not (xj > xmin and xj < xmax and yj > ymin and yj < ymax):
            continue
        js.append(j)
        cut.append(bool(bx0 <= xmin or bx1 >= xmax or by0 <= ymin or by1 >= ymax))
    return (xmin, xmax, ymin, ymax), js, cut


def random_catalogue(S, extent, seed, frac=True):
    """S sources scattered over extent x extent pixels, boxes of 1 to 9 pixels half-width; float64 [S, 6] table."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0, extent, (S, 2))
    if not frac:
        c = np.floor(c)
    h = rng.randint(1, 10, (S, 2)).astype(np.float64)
    return np.stack([c[:, 0], c[:, 1], c[:, 0] - h[:, 0], c[:, 0] + h[:, 0], c[:, 1] - h[:, 1], c[:, 1] + h[:, 1]], axis=1)


def members_numpy(table, dx, dy):
    """(windows, offsets, members, cut) of a float64 [S, 6] table: one vectorised comparison per source (the statement
    ops.catalog_members is compared with)."""
    t = np.asarray(table, np.float64)
    S = t.shape[0]
    windows = np.zeros((S, 4), np.int32)
    offsets = np.zeros(S + 1, np.int64)
    mem, cut = [], []
    for i in range(S):
        xmin, xmax, ymin, ymax = int(t[i, 0] - dx / 2), int(t[i, 0] + dx / 2), int(t[i, 1] - dy / 2), int(t[i, 1] + dy / 2)
        windows[i] = (xmin, xmax, ymin, ymax)
        inside = (t[:, 0] > xmin) & (t[:, 0] < xmax) & (t[:, 1] > ymin) & (t[:, 1] < ymax)
        inside[i] = False
        js = np.nonzero(inside)[0]
        mem.append(js.astype(np.int32))
        cut.append(((t[js, 2] <= xmin) | (t[js, 3] >= xmax) | (t[js, 4] <= ymin) | (t[js, 5] >= ymax)).astype(np.uint8))
        offsets[i + 1] = offsets[i] + js.size
    return windows, offsets, np.concatenate(mem) if mem else np.zeros(0, np.int32), np.concatenate(cut) if cut else np.zeros(0, np.uint8)
