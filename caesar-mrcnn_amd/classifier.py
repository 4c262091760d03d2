"""Source classifier: give every source of a CAESAR catalogue the class and score of the Mask R-CNN detection that matches it
(reference: mrcnn/classifier.py ``SClassInfo``, ``SData``, ``SClassifier``; scripts/sclassifier.py).

For each source not yet visited a window of ``scutout_size`` pixels is cut around it, the model runs on the stretched cut-out,
and every catalogue source whose centre lies in the window (the members) is matched to the detections by box IoU.  Members
whose box is not cut by the window become visited and get no cut-out of their own.

The reference does all of this one source at a time and scans the whole catalogue for every cut-out.  Here the run is split:

  ``plan(failed)``            which cut-outs the loop would run, in order, with their windows, members, local boxes and cut flags:
                              a pure function of the catalogue, ``scutout_size`` and the cut-outs known to fail -- nothing the
                              network finds enters it.  Member lists: one NumPy comparison per source, or with ``plan_device`` the
                              whole catalogue in two launches (ops.catalog_members, csrc/catalog.hip).
  ``associate(cutout, an)``   the matching of one cut-out's members to one Analyzer's detections (a handful times a handful: host).
  ``classify_source(i)``      the literal statement -- one source, one crop_img, one Analyzer.predict -- through the two above.

``cutout_batch = N`` (default 0: the loop over classify_source) runs the pixel work of the planned cut-outs on the GPU: the mosaic
is uploaded once, one launch counts the finite and NaN pixels of every window, one pass applies crop_img's in-place NaN fills in
plan order (later overlapping cut-outs see earlier fill values, as in the reference), ops.fits_tiles_to_rgb stretches N windows
per call and model.detect takes them N at a time.  Same visited flags, class infos and catalogue as the loop.

Departures from the reference:
  1. what raises there and ends the whole run fails alone here or has a defined answer: the ``%d`` of a source name in the two
     "cutout size <=" warnings (here: the warning and bbox_cut = True); get_iou's asserts on a degenerate box (IoU 0); a window
     that is empty, has a negative corner or holds no finite pixel (that source: logged, -1, not visited, nothing written into the
     mosaic); the unbound ``bbox_j`` of a detection in a cut-out without a second member (matched like any other);
  2. SClassInfo.score is filled (the reference computes it and leaves 0);
  3. the per-cut-out out_<name>.json/.reg/.png files are off (``save_cutout_results``) and ``run`` ends by writing one catalogue,
     sclass_<image>.json and .dat.
Sources are told apart by index, not by name: read_scatalog warns once when names repeat.
"""
import json
import logging
import os

import numpy as np

from . import analyze, fits, utils
from .analyze import Analyzer

logger = logging.getLogger("mrcnn")


class SClassInfo(object):
    """One classification of a source: the detection it was matched to in one cut-out."""

    def __init__(self):
        self.class_id = -1
        self.class_name = ''
        self.score = 0
        self.snames = []           # the other sources matched to the same detection


class SData(object):
    def __init__(self):
        self.name = ''
        self.x0 = self.y0 = -1
        self.xmin = self.xmax = self.ymin = self.ymax = -1
        self.visited = False
        self.class_info = []

    def add_class_info(self, c):
        self.class_info.append(c)


class Cutout(object):
    """One entry of plan(): the cut-out around source `index`.  window = (xmin, xmax, ymin, ymax); members[0] == index, then the
    other sources inside in catalogue order; boxes[k] = [y1, x1, y2, x2] of members[k] in window pixels; cut[k]: its box is cut by
    the window; failed: the cut-out is known to fail (nobody becomes visited through it)."""
    __slots__ = ("index", "window", "members", "boxes", "cut", "failed")


class SClassifier(object):
    def __init__(self, model, config):
        self.model = model
        self.r = None
        self.config = config
        self.n_classes = self.config.NUM_CLASSES
        self.class_names = self.config.CLASS_NAMES
        self.image_path = ''
        self.img_data = None
        self.img_header = None
        self.nx = self.ny = -1
        self.scatalog_path = ''
        self.sources = []
        self.n_max_sources = -1
        self.scutout_size = 132
        self.iou_thr = 0.6
        self.score_thr = 0.7
        # classify_source's constants (classifier.py:212-214); the batched form applies only while all three are on
        self.stretch = self.normalize = self.convertToRGB = True
        self.save_cutout_results = False      # the Analyzer's out_<name>.json/.reg/.png per cut-out (the reference's are on)
        self.cutout_batch = 0                 # N >= 1: cut-outs N at a time on the GPU; 0: the loop over classify_source
        self.plan_device = False              # member lists of the whole catalogue on the GPU (ops.catalog_members)
        self.outdir = "."
        self.outfile_json = self.outfile_dat = ""
        self.timing = {}
        self._table_key, self._table_arr = None, None
        self._lists_key, self._lists_val = None, None

    # ---- run (classifier.py:117-156) --------------------------------------------------------------------------------------
    def run(self, image_path, scatalog_path):
        self.image_path, self.scatalog_path = image_path, scatalog_path
        logger.info("Reading input image %s ..." % self.image_path)
        if self.read_img() < 0:
            logger.error("Failed to read image %s!" % self.image_path)
            return -1
        logger.info("Reading input source catalog %s ..." % self.scatalog_path)
        if self.read_scatalog() < 0:
            logger.error("Failed to read source catalog %s!" % self.scatalog_path)
            return -1
        self.classify_all()
        return self.save()

    def classify_all(self):
        """The loop over the catalogue (classifier.py:137-151), or its batched form."""
        if self._batched():
            return self._run_batched()
        for i in range(len(self.sources)):
            if self.n_max_sources > 0 and i >= self.n_max_sources:
                logger.info("Max number of sources to be processed reached, stop here.")
                break
            sname = self.sources[i].name
            logger.info("Classifying source %s ..." % (sname))
            if self.classify_source(i) < 0:
                logger.warning("Failed to run source classification on source %s!" % (sname))
        return 0

    # ---- geometry -------------------------------------------------------------------------------------------------------------
    def _table(self):
        """The catalogue as float64 [S, 6]: x0, y0, xmin, xmax, ymin, ymax.  Built once per source list (and length): whoever
        changes a coordinate afterwards sets ``_table_key = None``."""
        key = (id(self.sources), len(self.sources))
        if self._table_key != key:
            self._table_arr = np.array([[s.x0, s.y0, s.xmin, s.xmax, s.ymin, s.ymax] for s in self.sources],
                                       dtype=np.float64).reshape(-1, 6)
            self._table_key = key
        return self._table_arr

    def window(self, i):
        """(xmin, xmax, ymin, ymax) of source i's cut-out: int() truncates toward zero (classifier.py:199-202)."""
        s, d = self.sources[i], self.scutout_size
        return (int(s.x0 - d / 2), int(s.x0 + d / 2), int(s.y0 - d / 2), int(s.y0 + d / 2))

    def members_host(self, i, window):
        """Indices j != i, ascending, of the sources whose centre is strictly inside `window`, and their cut flags: the member
        scan of classifier.py:230-260 as one vectorised comparison (the statement ops.catalog_members equals)."""
        t = self._table()
        xmin, xmax, ymin, ymax = window
        inside = (t[:, 0] > xmin) & (t[:, 0] < xmax) & (t[:, 1] > ymin) & (t[:, 1] < ymax)
        inside[i] = False
        js = np.nonzero(inside)[0]
        cut = (t[js, 2] <= xmin) | (t[js, 3] >= xmax) | (t[js, 4] <= ymin) | (t[js, 5] >= ymax)
        return js, cut

    def member_lists(self):
        """With plan_device: (windows, offsets, members, cut) of the whole catalogue from the GPU, computed once per catalogue and
        cut-out size; None where the host scan answers (switch off, no GPU, a refused catalogue, a failed device form)."""
        if not (self.plan_device and len(self.sources) and analyze.model_has_gpu(self.model)):
            return None
        key = (id(self.sources), len(self.sources), self.scutout_size)
        if self._lists_key != key:
            from . import ops
            d = self.scutout_size
            self._lists_val = analyze.device_or_host(
                "SClassifier.member_lists", lambda: ops.catalog_members(self._table(), d, d, analyze.model_device(self.model)),
                lambda: None, refusal=ops.CatalogUnsupported)
            self._lists_key = key
        return self._lists_val

    def _cutout(self, i, lists=None):
        """The cut-out around source i (classifier.py:170-260 without the pixels)."""
        s, d = self.sources[i], self.scutout_size
        bbox_cut = False
        if d <= s.xmax - s.xmin:
            logger.warning("Cutout size (%d pix) is <= source %s size (%s pix) along x dimension!" % (d, s.name, str(s.xmax - s.xmin)))
            bbox_cut = True
        if d <= s.ymax - s.ymin:
            logger.warning("Cutout size (%d pix) is <= source %s size (%s pix) along y dimension!" % (d, s.name, str(s.ymax - s.ymin)))
            bbox_cut = True
        if lists is not None:
            windows, offsets, members, cut = lists
            window = tuple(int(v) for v in windows[i])
            js, cuts = members[offsets[i]:offsets[i + 1]], cut[offsets[i]:offsets[i + 1]]
        else:
            window = self.window(i)
            js, cuts = self.members_host(i, window)
        xmin, xmax, ymin, ymax = window
        c = Cutout()
        c.index, c.window, c.failed = i, window, False
        c.members = [i]
        c.boxes = [[s.ymin - ymin, s.xmin - xmin, s.ymax - ymin, s.xmax - xmin]]
        c.cut = [bbox_cut]
        for j, cj in zip(js, cuts):
            sj = self.sources[int(j)]
            c.members.append(int(j))
            c.boxes.append([sj.ymin - ymin, sj.xmin - xmin, sj.ymax - ymin, sj.xmax - xmin])
            c.cut.append(bool(cj))
        return c

    @staticmethod
    def _mark(cutout, flags):
        """What a processed cut-out does to the visited flags: every member whose box is not cut (classifier.py:281-285, :338)."""
        for m, is_cut in zip(cutout.members, cutout.cut):
            if not is_cut:
                flags[m] = True

    def plan(self, failed=frozenset(), lists=None):
        """The cut-outs the loop over classify_source would run, in order, given the cut-outs (source indices) that fail:
        a failed one is run -- it is in the list, with failed = True -- but marks nobody."""
        if lists is None:
            lists = self.member_lists()
        visited = [bool(s.visited) for s in self.sources]
        out = []
        for i in range(len(self.sources)):
            if self.n_max_sources > 0 and i >= self.n_max_sources:
                break
            if visited[i]:
                continue
            c = self._cutout(i, lists)
            c.failed = i in failed
            out.append(c)
            if not c.failed:
                self._mark(c, visited)
        return out

    # ---- one source (classifier.py:167-375) -----------------------------------------------------------------------------------
    def classify_source(self, sindex):
        s = self.sources[sindex]
        if s.visited:
            logger.info("Source %s already visited, nothing to be done ..." % s.name)
            return 0
        c = self._cutout(sindex, self.member_lists())
        if self._run_cutout(c) < 0:
            return -1
        self._mark_sources(c)
        return 0

    def _mark_sources(self, cutout):
        flags = {}
        self._mark(cutout, flags)
        for m in flags:
            self.sources[m].visited = True

    def window_fails(self, window):
        """A window no cut-out can be made of: a negative corner, no pixel, or no finite pixel (where the reference raises)."""
        xmin, xmax, ymin, ymax = window
        if min(window) < 0:
            return True
        crop = self.img_data[ymin:ymax, xmin:xmax]
        return crop.size == 0 or not np.isfinite(crop).any()

    def _analyzer(self):
        an = Analyzer(self.model, self.config)
        an.iou_thr, an.score_thr = self.iou_thr, self.score_thr
        if not self.save_cutout_results:
            an.write_to_json = an.write_to_ds9 = an.draw = False
        return an

    def _run_cutout(self, c, sink=None):
        """Pixels, detection and matching of one cut-out on the host path: crop_img (fills the window's NaNs in the mosaic),
        Analyzer.predict, associate.  0 / -1."""
        s, d = self.sources[c.index], self.scutout_size
        if self.window_fails(c.window):
            logger.error("Cutout window [%d:%d, %d:%d] of source %s is empty or has no finite pixel!" % (
                c.window[2], c.window[3], c.window[0], c.window[1], s.name))
            return -1
        data_crop = fits.crop_img(self.img_data, s.x0, s.y0, d, d, self.stretch, self.normalize, self.convertToRGB)
        logger.info("Crop image for source %s has size: %d x %d ..." % (s.name, data_crop.shape[1], data_crop.shape[0]))
        analyzer = self._analyzer()
        if analyzer.predict(data_crop, s.name, c.boxes) < 0:
            logger.error("Failed to run model prediction on source %s!" % s.name)
            return -1
        self.associate(c, analyzer, sink)
        return 0

    def associate(self, cutout, analyzer, sink=None):
        """Match the cut-out's members to the analyzer's detections (classifier.py:290-367): per member the detection with
        iou > iou_thr and iou >= the best so far (the last of equal maxima), one SClassInfo per matched member.  The infos go
        to the sources' class_info, or as (source index, info) to `sink` when one is given."""
        bboxes_det, scores_det, classid_det = analyzer.bboxes, analyzer.scores_final, analyzer.class_ids_final
        sname = self.sources[cutout.index].name
        if len(bboxes_det) == 0:
            logger.warning("No object detected for source cutout %s, this source won't be classified..." % sname)
            return
        association_map, det_indices = {}, []
        for index, bbox_s in zip(cutout.members, cutout.boxes):
            index_best, iou_best = -1, 0
            for i, bbox_det in enumerate(bboxes_det):
                iou = utils.get_iou(bbox_det, bbox_s)
                if iou > self.iou_thr and iou >= iou_best:
                    index_best, iou_best = i, iou
            det_indices.append(index_best)
            if index_best != -1:
                association_map.setdefault(index_best, []).append(index)
        for index, det_index in zip(cutout.members, det_indices):
            sname_s = self.sources[index].name
            if det_index == -1:
                logger.info("Source %s was not associated to any detected object and so it won't be classified." % (sname_s))
                continue
            c = SClassInfo()
            c.class_id = classid_det[det_index]
            c.class_name = self.class_names[c.class_id]
            c.score = scores_det[det_index]
            c.snames = [self.sources[k].name for k in association_map[det_index] if k != index]
            logger.info("Source %s associated to class %s (class_id=%d) with score=%f ..." % (sname_s, c.class_name, c.class_id, c.score))
            if sink is None:
                self.sources[index].add_class_info(c)
            else:
                sink.append((index, c))

    # ---- cut-outs N at a time -------------------------------------------------------------------------------------------------
    def _batched(self):
        """True when classify_all takes the batched form: cutout_batch set, classify_source's flags all on (the device chain is
        that combination), a GPU, a float32 plane, and a cut-out within the tile chain's size limit."""
        if int(self.cutout_batch) < 1:
            return False
        why = ""
        if not (self.stretch and self.normalize and self.convertToRGB):
            why = "the crop_img flags are not stretch, normalize and RGB"
        elif not analyze.model_has_gpu(self.model):
            why = "no GPU"
        elif not (isinstance(self.img_data, np.ndarray) and self.img_data.ndim == 2 and self.img_data.dtype == np.float32):
            why = "the image is not a float32 plane"
        elif int(self.scutout_size) ** 2 > fits.DEVICE_TILE_MAX_PIXELS:
            why = "the cut-out is above the device chain's size limit"
        if why:
            logger.info("cutout_batch = %d ignored: %s; cut-outs are made and detected one at a time" % (self.cutout_batch, why))
        return not why

    def _detect_images(self, images):
        """One model.detect call on a group of cut-outs (device tensors).  The model takes exactly cutout_batch images: a short
        group is padded by repeating its last image and what the padding produced is dropped (as SFinder._detect_images)."""
        n, N = len(images), int(self.cutout_batch)
        padded = list(images) + [images[-1]] * (N - n)
        res = self.model.detect(padded, verbose=0)
        kept = getattr(self.model, "last_masks_device", None)
        if isinstance(kept, list) and len(kept) > n:
            del kept[n:]
        return [(tuple(int(v) for v in images[i].shape), res[i], kept[i] if kept and i < len(kept) else None) for i in range(n)]

    def _accept_cutout(self, c, det):
        """Analyzer + matching of a cut-out that was detected in a batch: (status, [(source index, SClassInfo), ...])."""
        shape, r, masks_device = det
        s = self.sources[c.index]
        analyzer = self._analyzer()
        if analyzer.accept_detection(shape, r, masks_device, s.name, c.boxes) < 0:
            logger.error("Failed to run model prediction on source %s!" % s.name)
            return -1, []
        sink = []
        self.associate(c, analyzer, sink)
        return 0, sink

    def _run_batched(self):
        """classify_all with the pixel work on the GPU; leaves sources[*].visited, class_info and img_data as the loop does.
        The plan depends on which cut-outs fail, and a window without a finite pixel may have got some from an earlier cut-out's
        fill by its turn, so: plan with what is known, fill in plan order from the pristine plane, compare what the fill found
        alive with what the plan assumed, correct the first difference and plan again; the same when a cut-out fails in the
        Analyzer.  Every round agrees with the loop up to its first correction, so the rounds end."""
        import torch
        from . import ops
        dev = analyze.model_device(self.model)
        N = int(self.cutout_batch)
        S = len(self.sources) if self.n_max_sources <= 0 else min(len(self.sources), int(self.n_max_sources))
        if S == 0:
            return 0
        lists = self.member_lists()
        windows = np.array([lists[0][i] if lists is not None else self.window(i) for i in range(S)], dtype=np.int64).reshape(-1, 4)
        pristine = torch.from_numpy(np.ascontiguousarray(self.img_data)).to(dev)
        plane = pristine.clone()
        ny, nx = self.img_data.shape
        flags = ops.catalog_window_flags(pristine, windows)               # (finite, NaN) pixels of every window that may be planned
        never = set(int(i) for i in np.nonzero((windows.min(axis=1) < 0) | ((flags[:, 0] == 0) & (flags[:, 1] == 0)))[0])
        dead = never | set(int(i) for i in np.nonzero((flags[:, 0] == 0) & (flags[:, 1] > 0))[0])      # assumed; the fill corrects
        afail, done, filled, alive = set(), {}, (), {}
        touched, synced, rounds = False, True, 0
        while True:
            rounds += 1
            cuts = self.plan(frozenset(dead | afail), lists)
            fill = [c for c in cuts if c.index not in never and flags[c.index, 1] > 0]
            key = tuple(c.index for c in fill)
            if key != filled:                                              # other fills, another plane: nothing made from it holds
                done.clear()
                if filled:
                    plane.copy_(pristine)
                alive = dict(zip(key, ops.catalog_nan_fill(plane, [c.window for c in fill])))
                filled, synced = key, False
                touched = touched or bool(key)
            wrong = [i for i in key if bool(alive[i]) == (i in dead)]      # (the plane is right either way: the fill decides alone)
            if wrong:
                dead.symmetric_difference_update(wrong[:1])
                continue
            if touched and not synced:
                self.img_data[...] = plane.cpu().numpy()                   # the host copy: what the loop's crop_img calls leave
                synced = True
            todo = [c for c in cuts if not c.failed and c.index not in done]
            failed_now = False
            for g0 in range(0, len(todo), N):
                group = todo[g0:g0 + N]
                dets = None
                try:
                    rects = [(c.window[0], c.window[2], min(c.window[1], nx) - c.window[0], min(c.window[3], ny) - c.window[2]) for c in group]
                    dets = self._detect_images(ops.fits_tiles_to_rgb(plane, rects))
                except Exception as e:
                    logger.error("Cut-outs of sources %s: batched stretch / detect raised %s: %s; taking them one at a time" % (
                        [self.sources[c.index].name for c in group], type(e).__name__, e))
                for k, c in enumerate(group):
                    if dets is not None:
                        status, infos = self._accept_cutout(c, dets[k])
                    else:
                        infos = []
                        status = self._run_cutout(c, infos)
                    done[c.index] = (status, infos)
                    if status < 0:
                        afail.add(c.index)
                        failed_now = True
                if failed_now:
                    break                                                  # what comes after may no longer be planned
            if not failed_now:
                break
        for c in cuts:
            sname = self.sources[c.index].name
            if c.failed:
                if c.index not in afail:
                    logger.error("Cutout window [%d:%d, %d:%d] of source %s is empty or has no finite pixel!" % (
                        c.window[2], c.window[3], c.window[0], c.window[1], sname))
                logger.warning("Failed to run source classification on source %s!" % (sname))
                continue
            for index, info in done[c.index][1]:
                self.sources[index].add_class_info(info)
            self._mark_sources(c)
        self.timing["batched_rounds"] = rounds
        self.timing["batched_cutouts"] = len(cuts)
        return 0

    # ---- input (classifier.py:381-431) ----------------------------------------------------------------------------------------
    def read_img(self):
        res = fits.read_fits(self.image_path, stretch=False, normalize=False, convertToRGB=False)
        if not res:
            logger.error("Failed to read image %s!" % self.image_path)
            return -1
        self.img_data, self.img_header = res[0], res[1]
        self.nx, self.ny = self.img_data.shape[1], self.img_data.shape[0]
        logger.info("Input image %s has size %d x %d..." % (self.image_path, self.nx, self.ny))
        return 0

    def read_scatalog(self):
        """Columns 0 (name), 5, 6 (x0, y0), 13-16 (xmin, xmax, ymin, ymax) of the CAESAR ascii catalogue."""
        t = fits.read_table(self.scatalog_path)
        if not t:
            logger.error("Failed to read table!")
            return -1
        if len(t[0]) < 17:
            logger.error("Source catalog %s has %d columns, 17 or more are needed!" % (self.scatalog_path, len(t[0])))
            return -1
        self.sources = []
        for item in t:
            sdata = SData()
            sdata.name = item[0] if isinstance(item[0], str) else str(item[0])
            sdata.x0, sdata.y0 = item[5], item[6]
            sdata.xmin, sdata.xmax, sdata.ymin, sdata.ymax = item[13], item[14], item[15], item[16]
            self.sources.append(sdata)
        names = [s.name for s in self.sources]
        if len(set(names)) != len(names):
            logger.warning("Source names repeat in %s: sources are told apart by their row, associated names may be ambiguous" % self.scatalog_path)
        logger.info("Read #%d sources from file %s ..." % (len(self.sources), self.scatalog_path))
        return 0

    # ---- output ---------------------------------------------------------------------------------------------------------------
    def catalogue_rows(self):
        """One row per source: name, the best entry's class (highest score, the earliest of equals), the number of entries and
        the names associated in any entry (first-seen order).  Unclassified: class_id -1, class_name '', score 0."""
        rows = []
        for s in self.sources:
            best = None
            for c in s.class_info:
                if best is None or c.score > best.score:
                    best = c
            snames = []
            for c in s.class_info:
                for n in c.snames:
                    if n not in snames:
                        snames.append(n)
            rows.append({"name": s.name, "class_id": int(best.class_id) if best else -1, "class_name": best.class_name if best else "",
                         "score": float(best.score) if best else 0.0, "nentries": len(s.class_info), "snames": ",".join(snames)})
        return rows

    def save(self):
        """sclass_<image base>.json and .dat under outdir ('-' stands for an empty field in the .dat, so it stays a table)."""
        base = os.path.splitext(os.path.basename(self.image_path))[0] if self.image_path else "image"
        self.outfile_json = os.path.join(self.outdir, "sclass_%s.json" % base)
        self.outfile_dat = os.path.join(self.outdir, "sclass_%s.dat" % base)
        rows = self.catalogue_rows()
        try:
            os.makedirs(self.outdir or ".", exist_ok=True)
            with open(self.outfile_json, "w") as f:
                json.dump({"image": os.path.basename(self.image_path), "scatalog": os.path.basename(self.scatalog_path), "sources": rows},
                          f, indent=2)
                f.write("\n")
            with open(self.outfile_dat, "w") as f:
                f.write("# name class_id class_name score nentries snames\n")
                for r in rows:
                    f.write("%s %d %s %.6f %d %s\n" % (r["name"], r["class_id"], r["class_name"] or "-", r["score"], r["nentries"],
                                                       r["snames"] or "-"))
        except OSError as e:
            logger.error("Failed to write the classified catalogue (%s)!" % e)
            return -1
        logger.info("Classified catalogue of %d sources written to %s and %s" % (len(rows), self.outfile_json, self.outfile_dat))
        return 0
