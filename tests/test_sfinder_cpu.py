"""Tiled source finding on the host: caesar-mrcnn_amd/sfinder.py against the reference's own SFinder (recorded in
tests/golden/sfinder_merge.npz by tests/golden/make_sfinder_fixtures.py), the tiling-invariance property on planted mosaics, the
two-rank gather, and the unchanged default of `run.py detect --split_img_in_tiles`."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sfinder_cases as cases

ROOT = cases.ROOT


def _fixture():
    return np.load(cases.GOLDEN)


def _names():
    return cases.fixture_names(_fixture())


def test_fixture_inputs_are_the_scenarios():
    """The committed inputs are what sfinder_cases builds today (a drifted scenario would silently test something else)."""
    z = _fixture()
    scs = {sc["name"]: sc for sc in cases.grid_scenarios() + cases.merge_scenarios()}
    assert sorted(scs) == cases.fixture_names(z)
    for name, sc in scs.items():
        got, _, _ = cases.decode(name, z)
        assert {k: got[k] for k in got if k != "dets"} == {k: sc[k] for k in sc if k != "dets"}
        assert len(got["dets"]) == len(sc["dets"])
        for a, b in zip(got["dets"], sc["dets"]):
            assert a[:3] == (b[0], b[1], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("name", _names())
def test_host_path_equals_reference(name):
    """Grid (tile ids, worker, coordinates, neighbour ids / indices / workers in order) and catalogue (order, names, boxes, edge,
    merged, class, score, pixels in order, vertexes): exact."""
    from caesar_mrcnn_amd.sfinder import SFinder
    sc, grid, want = cases.decode(name, _fixture())
    cfg = cases.make_config()
    sf = SFinder(None, cfg)
    got_grid, got = cases.drive(sf, sc, cfg, merge=sf.merge_edge_sources_host)
    assert got_grid == grid
    got = cases.canon(got)
    assert [s["name"] for s in got] == [s["name"] for s in want]
    assert got == want


def test_candidate_pairs_equal_the_double_loop():
    """The per-tile-pair enumeration of the device path hands over exactly the pairs (and in the order) of the reference's
    `j > i` double loop with its neighbour and box tests."""
    from caesar_mrcnn_amd.sfinder import SFinder
    z = _fixture()
    for name in ("all_w3", "overlap_w3", "interlock", "gap2"):
        sc, _, _ = cases.decode(name, z)
        cfg = cases.make_config()
        sf = SFinder(None, cfg)
        cases.drive(sf, sc, cfg, merge=lambda: None)
        todo = sf._split_edge_sources()
        tiles = sf.tile_sources["sources"]
        want = []
        for i in range(len(todo)):
            a = sf._edge_source(todo[i])
            for j in range(i + 1, len(todo)):
                b = sf._edge_source(todo[j])
                if tiles[todo[j].tindex]["tileId"] not in tiles[todo[i].tindex]["neighborTileIds"]:
                    continue
                if a["x2"] < b["x1"] or a["x1"] > b["x2"] or a["y2"] < b["y1"] or a["y1"] > b["y2"]:
                    continue
                want.append((i, j))
        assert sf.candidate_pairs(todo).tolist() == [list(p) for p in want], name
        assert want, name


def test_pack_sources_roundtrip():
    from caesar_mrcnn_amd.sfinder import pack_sources, unpack_bitmap
    rng = np.random.RandomState(3)
    lists = []
    for w, h in ((1, 1), (31, 2), (32, 3), (33, 1), (64, 2), (65, 5), (200, 3)):
        m = rng.rand(h, w) < 0.5
        m[0, 0] = m[-1, -1] = True
        lists.append((np.argwhere(m) + (7, 1000)).tolist())
    pool, desc = pack_sources(lists)
    assert pool.dtype == np.uint32 and desc.shape == (len(lists), 6)
    for pixels, (x0, y0, w, h, off, wpr) in zip(lists, desc.tolist()):
        assert wpr == (w + 31) // 32
        back = np.argwhere(unpack_bitmap(pool[off:off + h * wpr], h, w, wpr)) + (y0, x0)
        assert back.tolist() == pixels


# ---- tiling invariance ----------------------------------------------------------------------------------------
def _write_mosaic(path, labels):
    from caesar_mrcnn_amd import fits
    fits.write_fits(path, labels.astype(np.float32))


def _run_parallel(path, step, outfile):
    from caesar_mrcnn_amd.sfinder import SFinder
    cfg = cases.label_map_config(path)
    cfg.TILE_XSTEP = cfg.TILE_YSTEP = step
    sf = SFinder(cases.LabelMapModel(cfg), cfg)
    sf.merge_device = False
    sf.outfile_json = outfile
    sf.outfile_ds9 = os.path.splitext(outfile)[0] + ".reg"
    assert sf.run_parallel() == 0
    return sf


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("step", [1.0, 0.5])
def test_tiling_invariance(tmp_path, step, seed):
    """Whatever the tiling, every planted source comes out exactly once, with exactly its pixels."""
    labels, n = cases.planted_mosaic(seed)
    assert n >= 30
    path = str(tmp_path / "mosaic.fits")
    _write_mosaic(path, labels)
    sf = _run_parallel(path, step, str(tmp_path / "cat.json"))
    assert len(sf.tile_sources["sources"]) == (6 if step == 1.0 else 24)
    sources = sf.sources["sources"]
    found = {}
    for s in sources:
        p = np.asarray(s["pixels"])
        ids = np.unique(labels[p[:, 0], p[:, 1]])
        assert ids.size == 1 and ids[0] > 0, "a catalogue entry mixes planted sources or sky"
        assert len({(y, x) for y, x in s["pixels"]}) == len(s["pixels"]), "duplicate pixels"
        found.setdefault(int(ids[0]), []).append(s)
    for k in range(1, n + 1):                          # every planted source, none skipped
        assert len(found.get(k, [])) == 1, "planted source %d appears %d times" % (k, len(found.get(k, [])))
        got = {(y, x) for y, x in found[k][0]["pixels"]}
        assert got == {(int(y), int(x)) for y, x in np.argwhere(labels == k)}
    assert [s["name"] for s in sources] == ["S%d" % (i + 1) for i in range(len(sources))]
    assert any(s["merged"] for s in sources)
    written = json.load(open(str(tmp_path / "cat.json")))
    assert written["image_id"] == "mosaic" and len(written["objs"]) == len(sources)
    assert all("merged" in o for o in written["objs"])
    assert open(str(tmp_path / "cat.reg")).read().splitlines()[2] == "image"


# ---- two ranks ---------------------------------------------------------------------------------------------------
_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import sfinder_cases as cases
from caesar_mrcnn_amd import sfinder
rank = int(os.environ["RANK"])
if os.environ.get("SF_FAIL") == "1" and rank == 1:
    def boom(self):
        raise RuntimeError("planted failure in tile %%d" %% self.tid)
    sfinder.TileTask.find_sources = boom
cfg = cases.label_map_config(%(path)r)
sf = sfinder.SFinder(cases.LabelMapModel(cfg), cfg)
sf.merge_device = False
sf.outfile_json = %(out)r
sf.outfile_ds9 = %(out)r + ".reg"
rc = sf.run_parallel()
assert rc == 0, rc
assert sf.nproc == 2 and sf.procId == rank
print("ok", len(sf.sources["sources"]))
"""


def _run_world2(tmp_path, path, out, fail):
    script = tmp_path / ("worker%d.py" % fail)
    script.write_text(_WORKER % {"root": ROOT, "path": path, "out": out})
    port = 29900 + (os.getpid() % 300) + 301 * fail
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MRCNN_DIST_BACKEND="gloo", SF_FAIL=str(fail))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0].decode())      # the wall-clock limit: a rank left in the collective fails here
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ok" in o for o in outs), outs
    return json.load(open(out))


def _key(s):
    return (frozenset((y, x) for y, x in s["pixels"]), s["class_id"], s["score"], s["merged"], s["edge"], s["x1"], s["x2"], s["y1"], s["y2"])


def test_two_ranks_gloo(tmp_path):
    """Rank 0 of a two-process run holds the catalogue of a one-process run.  Two workers visit the tiles in another order (0, 2,
    4 then 1, 3, 5), which permutes the entries and the first-seen pixel order as in the reference, so entries are compared as
    sets: pixel set, class, score, flags, box.  Then: a tile that raises on rank 1 leaves nobody waiting in the gather."""
    labels, n = cases.planted_mosaic(5)
    path = str(tmp_path / "mosaic.fits")
    _write_mosaic(path, labels)
    one = _run_parallel(path, 1.0, str(tmp_path / "one.json")).sources["sources"]
    two = _run_world2(tmp_path, path, str(tmp_path / "two.json"), fail=0)["objs"]
    assert len(one) == len(two) == n
    assert {_key(s) for s in one} == {_key(s) for s in two}
    assert sorted(s["name"] for s in two) == sorted("S%d" % (i + 1) for i in range(n))
    assert not os.path.exists(str(tmp_path / "two_rank1.json"))
    failed = _run_world2(tmp_path, path, str(tmp_path / "failed.json"), fail=1)["objs"]
    tiles_rank0 = [(0, 256, 0, 256), (512, 768, 0, 256), (256, 512, 256, 512)]        # tiles 0, 2, 4
    want = set()
    for k in range(1, n + 1):
        p = np.argwhere(labels == k)
        if any(len(cases.clip(p, t)) for t in tiles_rank0):
            want.add(k)
    got = {int(labels[s["pixels"][0][0], s["pixels"][0][1]]) for s in failed}
    assert got == want                                      # rank 0's tiles are all there, rank 1's are reported lost, not waited for


# ---- CLI ---------------------------------------------------------------------------------------------------------
def _load_run_py():
    spec = importlib.util.spec_from_file_location("_run_py_under_test", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_default_tiles_path_unchanged(tmp_path, monkeypatch):
    """Without --merge_tile_sources `detect --split_img_in_tiles` takes today's path: one Analyzer.predict per tile, objects
    concatenated with their tile tag, no `merged` key; SFinder is not touched.  With the flag it goes through
    SFinder.run_parallel."""
    run = _load_run_py()
    from caesar_mrcnn_amd import sfinder
    from caesar_mrcnn_amd.analyze import Analyzer
    labels, n = cases.planted_mosaic(7)
    path = str(tmp_path / "mosaic.fits")
    _write_mosaic(path, labels)
    base = ["detect", "--image", path, "--split_img_in_tiles", "--tile_xsize", "256", "--tile_ysize", "256", "--no_zscale",
            "--no_norm_img", "--no_uint8"]
    args = run.parse_args(base + ["--detect_outfile_json", str(tmp_path / "plain.json")])
    assert args.merge_tile_sources is False
    assert run.parse_args(base + ["--merge_tile_sources"]).merge_tile_sources is True
    calls = {"predict": 0, "sfinder": 0}
    real_predict, real_run_parallel = Analyzer.predict, sfinder.SFinder.run_parallel

    def predict(self, *a, **k):
        calls["predict"] += 1
        return real_predict(self, *a, **k)

    def run_parallel(self):
        calls["sfinder"] += 1
        return real_run_parallel(self)

    monkeypatch.setattr(Analyzer, "predict", predict)
    monkeypatch.setattr(sfinder.SFinder, "run_parallel", run_parallel)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    cfg = run.build_config(args, {"source": 1})
    model = cases.LabelMapModel(cfg)
    assert run.detect(args, model, cfg) == 0
    assert calls == {"predict": 6, "sfinder": 0}
    plain = json.load(open(str(tmp_path / "plain.json")))["objs"]
    assert len(plain) > n and all("merged" not in o for o in plain)              # cut sources are reported per tile
    assert all(o["name"].split("_")[1] in ("t0", "t1", "t2", "t3", "t4", "t5") for o in plain)
    # the new flag
    args = run.parse_args(base + ["--merge_tile_sources", "--detect_outfile_json", str(tmp_path / "merged.json")])
    cfg = run.build_config(args, {"source": 1})
    model = cases.LabelMapModel(cfg)
    assert run.detect(args, model, cfg) == 0
    assert calls["sfinder"] == 1
    merged = json.load(open(str(tmp_path / "merged.json")))
    assert merged["image_id"] == "mosaic" and len(merged["objs"]) == n
    assert set(merged["objs"][0]) == set(plain[0]) | {"merged"}
    assert [o["name"] for o in merged["objs"]] == ["S%d" % (i + 1) for i in range(n)]
    assert os.path.exists(str(tmp_path / "merged.reg"))
