"""The batched tile front end of the tiled source finder (SFinder.tile_batch), without a GPU: grouping, padding and fall-back
logic with the "prepare" step of the seam replaced by fits.read_fits per tile and a stub model whose detections are a pure
function of the tile's bytes; run.py's --tile_batch; Analyzer.predict against Analyzer.accept_detection."""
import importlib.util
import json
import logging
import os

import numpy as np
import pytest

import sfinder_cases as cases
import sfinder_tiles_cases as tc

ROOT = tc.ROOT


@pytest.fixture(scope="module")
def mosaic_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tiles") / "mosaic.fits")
    tc.write_mosaic(path)
    return path


@pytest.fixture(scope="module")
def baseline(mosaic_path, tmp_path_factory):
    """tile_batch = 0 at both steps: (SFinder, canonical catalogue, JSON text, region text), computed once."""
    out = {}
    for step in (1.0, 0.5):
        d = str(tmp_path_factory.mktemp("base"))
        sf = tc.run(mosaic_path, 0, step, outdir=d)
        out[step] = (sf, cases.canon(sf.sources["sources"]), open(sf.outfile_json).read(), open(sf.outfile_ds9).read())
    return out


def _spy(sf, log, prepare=None):
    """Host "prepare" + records of what the run does: groups prepared (tile ids), tiles through find_sources, edge calls."""
    from caesar_mrcnn_amd.sfinder import TileTask
    host = prepare or tc.host_prepare(sf)

    def prepare_tile_images(tasks):
        log["groups"].append([t.tid for t in tasks])
        return host(tasks)

    real_edge = sf.find_sources_at_edge

    def find_sources_at_edge(j):
        log["edge"].append(j)
        return real_edge(j)

    sf.prepare_tile_images = prepare_tile_images
    sf.find_sources_at_edge = find_sources_at_edge
    real_find = TileTask.find_sources

    def find_sources(task):
        log["single"].append(task.tid)
        return real_find(task)
    return find_sources


def _new_log():
    return {"groups": [], "single": [], "edge": []}


def test_seed_gives_merged_and_edge_sources(baseline):
    """Seed 4 at step 1.0: 49 sources, 4 of them merged across tile borders, 5 edge-flagged (step 0.5: 35, 31 merged, 33 edge).
    Without these the catalogue comparisons below would say nothing about the edge bookkeeping."""
    src = baseline[1.0][0].sources["sources"]
    assert sum(1 for s in src if s["merged"]) >= 1 and sum(1 for s in src if s["edge"]) >= 1
    assert (len(src), sum(1 for s in src if s["merged"]), sum(1 for s in src if s["edge"])) == (49, 4, 5)
    src = baseline[0.5][0].sources["sources"]
    assert (len(src), sum(1 for s in src if s["merged"]), sum(1 for s in src if s["edge"])) == (35, 31, 33)


@pytest.mark.parametrize("step", [1.0, 0.5])
@pytest.mark.parametrize("batch", [1, 3, 4])
def test_groups_padding_and_catalogue(mosaic_path, baseline, tmp_path, monkeypatch, batch, step):
    """Groups in task order; a short last group padded to the model's batch and the padding dropped; find_sources_at_edge once
    per tile, in order; no tile through find_sources; catalogue, JSON and region file equal to the tile_batch = 0 ones.  (9 tiles
    at step 1.0, 30 at 0.5: batch 4 pads the last group at both steps.)"""
    from caesar_mrcnn_amd.sfinder import TileTask
    base_sf, base_canon, base_json, base_reg = baseline[step]
    ntiles = len(base_sf.tasks_per_worker[0])
    assert ntiles == (9 if step == 1.0 else 30)
    log = _new_log()

    def setup(sf):
        monkeypatch.setattr(TileTask, "find_sources", _spy(sf, log))
    sf = tc.run(mosaic_path, batch, step, outdir=str(tmp_path), setup=setup)
    tids = list(range(ntiles))
    assert log["groups"] == [tids[k:k + batch] for k in range(0, ntiles, batch)]
    assert sf.model.batches == [batch] * len(log["groups"])               # every detect call at the model's batch size
    if batch == 4:
        assert ntiles % batch != 0                                        # the padded case is really there
    assert log["single"] == []
    assert log["edge"] == tids
    assert cases.canon(sf.sources["sources"]) == base_canon
    assert open(sf.outfile_json).read() == base_json
    assert open(sf.outfile_ds9).read() == base_reg


def test_padded_results_are_dropped(mosaic_path):
    """_detect_images on a short group: the model sees tile_batch images, the caller gets the group's results only, and the
    model's last_masks_device loses the padding's entries."""
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = tc.config(mosaic_path)

    class Model(tc.ThresholdModel):
        def detect(self, images, verbose=0):
            self.last_masks_device = ["m%d" % i for i in range(len(images))]
            return tc.ThresholdModel.detect(self, images, verbose)
    sf = SFinder(Model(cfg), cfg)
    sf.tile_batch = 4
    a = np.zeros((5, 7, 3), np.uint8)
    b = np.full((6, 4, 3), 255, np.uint8)
    out = sf._detect_images([a, b])
    assert sf.model.batches == [4]
    assert [o[0] for o in out] == [(5, 7, 3), (6, 4, 3)]
    assert [o[1]["masks"].shape[-1] for o in out] == [0, 1]
    assert [o[2] for o in out] == ["m0", "m1"] and sf.model.last_masks_device == ["m0", "m1"]


def test_failing_prepare_sends_its_group_through_find_sources(mosaic_path, baseline, monkeypatch):
    """A "prepare" that raises for the second group: exactly that group's tiles take task.find_sources(), the others stay
    batched, the edge calls stay in order and the catalogue is the tile_batch = 0 one."""
    from caesar_mrcnn_amd.sfinder import TileTask
    log = _new_log()

    def setup(sf):
        host = tc.host_prepare(sf)

        def prepare(tasks):
            if tasks[0].tid == 4:
                raise RuntimeError("planted failure of the group that starts at tile 4")
            return host(tasks)
        monkeypatch.setattr(TileTask, "find_sources", _spy(sf, log, prepare))
    sf = tc.run(mosaic_path, 4, 1.0, setup=setup)
    assert log["groups"] == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
    assert log["single"] == [4, 5, 6, 7]
    assert log["edge"] == list(range(9))
    assert sf.model.batches == [4, 1, 1, 1, 1, 4]
    assert cases.canon(sf.sources["sources"]) == baseline[1.0][1]


def test_empty_tile_fails_alone(mosaic_path, monkeypatch):
    """A tile with xmax <= xmin fails as read_fits fails it today -- alone: its group's other tiles stay batched, it gets no
    edge call, and the catalogue equals that of the same grid at tile_batch = 0."""
    from caesar_mrcnn_amd.sfinder import SFinder, TileTask
    real_create = SFinder.create_tile_tasks

    def create(self):
        rc = real_create(self)
        t = self.tasks_per_worker[0][5]
        t.ix_max = t.ix_min
        return rc
    monkeypatch.setattr(SFinder, "create_tile_tasks", create)
    base = tc.run(mosaic_path, 0, 1.0)
    log = _new_log()

    def setup(sf):
        monkeypatch.setattr(TileTask, "find_sources", _spy(sf, log))
    sf = tc.run(mosaic_path, 4, 1.0, setup=setup)
    assert log["groups"] == [[0, 1, 2, 3], [4, 6, 7], [8]]
    assert log["single"] == []
    assert log["edge"] == [0, 1, 2, 3, 4, 6, 7, 8]
    assert sf.tasks_per_worker[0][5].det_sources == {}
    assert cases.canon(sf.sources["sources"]) == cases.canon(base.sources["sources"])
    assert len(sf.sources["sources"]) > 0


def test_other_flags_take_the_old_path(tmp_path, monkeypatch, caplog):
    """read_fits flags other than the run.py ones (here: every stretch off): tile_batch is ignored with one log line, every tile
    goes through find_sources, nothing is prepared."""
    from caesar_mrcnn_amd.sfinder import SFinder, TileTask
    labels, n = cases.planted_mosaic(3, nx=512, ny=256, n_try=80)          # two 256-tiles
    assert n >= 5
    path = str(tmp_path / "labels.fits")
    from caesar_mrcnn_amd import fits
    fits.write_fits(path, labels.astype(np.float32))
    runs = {}
    for batch in (0, 4):
        cfg = cases.label_map_config(path)
        sf = SFinder(cases.LabelMapModel(cfg), cfg)
        sf.merge_device = False
        sf.write_to_json = sf.write_to_ds9 = False
        sf.tile_batch = batch
        log = _new_log()
        monkeypatch.setattr(TileTask, "find_sources", _spy(sf, log))
        with caplog.at_level(logging.INFO, logger="mrcnn"):
            caplog.clear()
            assert sf.run_parallel() == 0
            said = [r.getMessage() for r in caplog.records if "tile_batch" in r.getMessage()]
        monkeypatch.undo()
        runs[batch] = (cases.canon(sf.sources["sources"]), log, said)
    assert runs[4][1]["groups"] == [] and runs[4][1]["single"] == [0, 1] and runs[4][1]["edge"] == [0, 1]
    assert len(runs[4][2]) == 1 and runs[0][2] == []
    assert runs[4][0] == runs[0][0] and len(runs[0][0]) == n


def test_plane_is_read_once(mosaic_path, monkeypatch):
    """fits.read_primary_hdu: one call in a batched run (header and plane come from it), one per tile and more in the loop."""
    from caesar_mrcnn_amd import fits
    calls = []
    real = fits.read_primary_hdu

    def counted(*a, **k):
        calls.append(a[0])
        return real(*a, **k)
    monkeypatch.setattr(fits, "read_primary_hdu", counted)

    def setup(sf):                                  # cut the tiles on the host from the plane the run holds
        def prepare(tasks):
            plane = sf._image_plane()
            out = []
            for t in tasks:
                cut = plane[t.iy_min:t.iy_max, t.ix_min:t.ix_max].astype(np.float32)
                cut[np.isnan(cut)] = np.nanmin(cut)
                c = fits.normalize_img(fits.stretch_img(cut, 0.25).astype(np.float32)).astype(np.float32)
                out.append(fits.gray2rgb([c, c, c]))
            return out
        sf.prepare_tile_images = prepare
    sf = tc.run(mosaic_path, 4, 1.0, setup=setup)
    assert len(calls) == 1
    assert sf._plane is None and sf._plane_dev is None                    # freed at the end of the run
    batched = cases.canon(sf.sources["sources"])
    del calls[:]
    sf0 = tc.run(mosaic_path, 0, 1.0)
    assert len(calls) == 1 + 9                                            # the header, then every tile
    assert cases.canon(sf0.sources["sources"]) == batched


# ---- run.py ------------------------------------------------------------------------------------------------------
def _load_run_py():
    spec = importlib.util.spec_from_file_location("_run_py_tiles_under_test", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_tile_batch(mosaic_path, tmp_path, monkeypatch):
    """--tile_batch: default 0; with N under --split_img_in_tiles --merge_tile_sources the inference model is configured for
    batches of N and the SFinder gets tile_batch = N; without the flag (or without the merge flags) IMAGES_PER_GPU stays 1."""
    run = _load_run_py()
    from caesar_mrcnn_amd import sfinder
    base = ["detect", "--image", mosaic_path, "--split_img_in_tiles", "--tile_xsize", "128", "--tile_ysize", "128",
            "--merge_tile_sources", "--detect_outfile_json", str(tmp_path / "out.json")]
    args = run.parse_args(base)
    assert args.tile_batch == 0
    cfg = run.build_config(args, {"source": 1})
    assert cfg.IMAGES_PER_GPU == 1 and cfg.BATCH_SIZE == 1
    assert run.build_config(run.parse_args(["detect", "--image", mosaic_path, "--tile_batch", "4"]), {"source": 1}).IMAGES_PER_GPU == 1
    seen = []
    real = sfinder.SFinder.run_parallel

    def run_parallel(self):
        self.merge_device = self.params_device = False
        self.prepare_tile_images = tc.host_prepare(self)
        seen.append(self.tile_batch)
        return real(self)
    monkeypatch.setattr(sfinder.SFinder, "run_parallel", run_parallel)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    model = tc.ThresholdModel(cfg)
    assert run.detect(args, model, cfg) == 0
    assert seen == [0] and set(model.batches) == {1}
    plain = json.load(open(str(tmp_path / "out.json")))
    args = run.parse_args(base + ["--tile_batch", "4"])
    assert args.tile_batch == 4
    cfg = run.build_config(args, {"source": 1})
    assert cfg.IMAGES_PER_GPU == 4 and cfg.BATCH_SIZE == 4
    model = tc.ThresholdModel(cfg)
    assert run.detect(args, model, cfg) == 0
    assert seen == [0, 4] and model.batches == [4, 4, 4]
    assert json.load(open(str(tmp_path / "out.json"))) == plain


# ---- Analyzer ----------------------------------------------------------------------------------------------------
def test_accept_detection_equals_predict(mosaic_path, tmp_path):
    """predict = detect + accept_detection: the same detection gives equal results, boxes and regions, whether the Analyzer is
    handed the image or only its shape."""
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.analyze import Analyzer
    cfg = tc.config(mosaic_path)
    image, header = fits.read_fits(mosaic_path, 64, 256, 0, 192)
    model = tc.ThresholdModel(cfg)

    def analyzer(tag):
        a = Analyzer(model, cfg)
        a.score_thr, a.iou_thr, a.obj_name_tag = 0.7, 0.6, "t3"
        a.outfile_json, a.outfile_ds9 = str(tmp_path / (tag + ".json")), str(tmp_path / (tag + ".reg"))
        return a
    a = analyzer("a")
    assert a.predict(image, "mosaic", header=header, xmin=64, ymin=0) == 0
    r = model.detect([image])[0]
    assert r["masks"].shape[-1] >= 2
    for tag, img in (("b", image), ("c", image.shape)):
        b = analyzer(tag)
        assert b.accept_detection(img, r, None, "mosaic", header=header, xmin=64, ymin=0) == 0
        assert b.results == a.results and len(b.results["objs"]) >= 2
        assert [list(map(int, x)) for x in b.bboxes] == [list(map(int, x)) for x in a.bboxes]
        assert b.obj_regions == a.obj_regions and b.scores_final == a.scores_final
        assert open(str(tmp_path / (tag + ".json"))).read() == open(str(tmp_path / "a.json")).read()
        assert open(str(tmp_path / (tag + ".reg"))).read() == open(str(tmp_path / "a.reg")).read()
    assert analyzer("d").accept_detection(None, r) == -1
