"""The device half of the tiled source finder: csrc/tilemerge.hip (ops.tile_adjacency / ops.tile_union) against brute-force
NumPy, SFinder's device path against its host statement and the reference fixture, and the command line."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sfinder_cases as cases

pytestmark = pytest.mark.gpu
ROOT = cases.ROOT


# ---- sources as (x0, y0, bool mask) ------------------------------------------------------------------------------
def _pixels(src):
    x0, y0, m = src
    return np.argwhere(m) + (y0, x0)


def _adjacent_brute(a, b):
    """The predicate of sfinder.py:797-799 over every pixel pair."""
    pa, pb = _pixels(a), _pixels(b)
    for k in range(0, len(pa), 256):
        d = np.abs(pa[k:k + 256, None, :] - pb[None, :, :])
        if np.any((d[..., 0] <= 1) & (d[..., 1] <= 1)):
            return 1
    return 0


def _pack(sources):
    """The header's layout, built directly from the masks (boxes as given, not tightened)."""
    desc, chunks, off = [], [], 0
    for x0, y0, m in sources:
        h, w = m.shape
        wpr = (w + 31) // 32
        padded = np.zeros((h, wpr * 32), np.uint8)
        padded[:, :w] = m
        chunks.append(np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(-1))
        desc.append((x0, y0, w, h, off, wpr))
        off += h * wpr
    return np.concatenate(chunks).astype(np.uint32), np.array(desc, np.int32)


def _rand(rng, w, h, density):
    m = rng.rand(h, w) < density
    m[rng.randint(h), 0] = True             # keep the box as stated: something in the first / last column and row
    m[rng.randint(h), w - 1] = True
    m[0, rng.randint(w)] = True
    m[h - 1, rng.randint(w)] = True
    return m


def _adjacency_cases():
    rng = np.random.RandomState(20240611)
    S, P = [], []

    def pair(a, b):
        S.extend([a, b])
        P.append((len(S) - 2, len(S) - 1))

    one = np.ones((1, 1), bool)
    # every relative bit offset 0..63 between the boxes, both signs, sparse masks of more than two words per row
    for off in range(64):
        for sign in (1, -1):
            for dy in (0, 3):
                pair((1000, 50, _rand(rng, 70, 6, 0.04)), (1000 + sign * off, 50 + dy, _rand(rng, 90, 5, 0.04)))
    # boxes that start / end on 32- and 64-bit boundaries
    for x0 in (0, 32, 64, 96, 128):
        for w in (32, 64, 96):
            pair((x0, 10, _rand(rng, w, 3, 0.05)), (x0 + w, 10, _rand(rng, 32, 3, 0.3)))          # touching at the boundary
            pair((x0, 10, _rand(rng, w, 3, 0.05)), (x0 + w + 1, 10, _rand(rng, 32, 3, 0.3)))      # one empty column between
    # widths x heights, random small displacements: both answers occur
    widths, heights = (1, 31, 32, 33, 64, 65, 130, 200), (1, 2, 7)
    for wa in widths:
        for wb in widths:
            for ha in heights:
                hb = heights[rng.randint(3)]
                dx, dy = rng.randint(-wb - 2, wa + 3), rng.randint(-hb - 2, ha + 3)
                pair((500, 500, _rand(rng, wa, ha, 0.08)), (500 + dx, 500 + dy, _rand(rng, wb, hb, 0.08)))
    # one-pixel sources: the 3 x 3 neighbourhood (adjacent) and the ring at distance 2 (not)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            for x in (31, 32, 63, 64, 200):
                pair((x, 40, one), (x + dx, 40 + dy, one))
    # contact only through the carry bit between two words: i ends in bit 31 of a word, j starts in bit 0 of the next
    for y in (0, 1, -1):
        a = np.zeros((3, 64), bool)
        a[1, 31] = True
        b = np.zeros((3, 64), bool)
        b[1 + y, 32] = True
        pair((320, 70, a), (320, 70, b))
        pair((320, 70, b), (320, 70, a))
        c = np.zeros((3, 64), bool)
        c[1, 33] = True                       # two columns away: no contact
        pair((320, 70, a), (320, 70, c))
    # contact only on the first / last row; and exactly distance 2 there
    top = np.zeros((4, 40), bool)
    top[3, 20] = True
    top[0, 0] = True
    for gap, dx in ((0, 1), (0, 0), (0, -1), (1, 0), (0, 2)):
        bot = np.zeros((3, 40), bool)
        bot[0, 20 + dx] = True
        bot[2, 39] = True
        pair((77, 100, top), (77, 104 + gap, bot))
        pair((77, 104 + gap, bot), (77, 100, top))
    # disjoint boxes far apart, identical sources, a source with itself
    big = _rand(rng, 150, 9, 0.1)
    pair((0, 0, big), (4000, 3000, big))
    pair((700, 700, big), (700, 700, big.copy()))
    S.append((900, 900, _rand(rng, 33, 2, 0.2)))
    P.append((len(S) - 1, len(S) - 1))
    # dense against dense with a diagonal corridor of width 2 between them (full product on the host, no contact)
    yy, xx = np.mgrid[0:60, 0:140]
    pair((2000, 2000, (xx - 2 * yy) <= -2), (2000, 2000, (xx - 2 * yy) >= 3))
    pair((2000, 2000, (xx - 2 * yy) <= -1), (2000, 2000, (xx - 2 * yy) >= 1))
    return S, np.array(P, np.int32)


def test_tile_adjacency_equals_brute_force(dev):
    import torch
    from caesar_mrcnn_amd import ops
    S, P = _adjacency_cases()
    want = np.array([_adjacent_brute(S[i], S[j]) for i, j in P], np.int32)
    assert 0.2 < want.mean() < 0.8, "the cases must exercise both answers"
    pool, desc = _pack(S)
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    got = ops.tile_adjacency(pool_t, desc_t, P).cpu().numpy()
    torch.cuda.synchronize()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "pairs %s: device %s, brute force %s" % (P[bad[:8]].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    # symmetric
    got_t = ops.tile_adjacency(pool_t, desc_t, P[:, ::-1].copy()).cpu().numpy()
    assert np.array_equal(got_t, want)
    # no pairs: nothing launched, empty answer
    assert ops.tile_adjacency(pool_t, desc_t, np.zeros((0, 2), np.int32)).numel() == 0


def test_tile_adjacency_rejects_bad_input(dev):
    from caesar_mrcnn_amd import _hip, ops
    S, _ = _adjacency_cases()
    pool, desc = _pack(S[:4])
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    with pytest.raises(_hip.HipPathError):
        ops.tile_adjacency(pool_t, desc_t, np.array([[0, 4]], np.int32))
    bad = desc.copy()
    bad[3, 4] = pool.size                        # points past the pool
    with pytest.raises(_hip.HipPathError):
        ops.tile_upload(pool, bad, dev)


def test_tile_union_equals_numpy(dev):
    import torch
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.sfinder import unpack_bitmap
    rng = np.random.RandomState(99)
    S, comps = [], []
    for c in range(40):
        k = rng.randint(1, 6)
        bx, by = rng.randint(0, 3000), rng.randint(0, 3000)
        ids = []
        for _ in range(k):
            w, h = [1, 31, 32, 33, 64, 65, 150][rng.randint(7)], rng.randint(1, 12)
            far = rng.rand() < 0.25          # a member whose box is disjoint from the others
            S.append((bx + rng.randint(-40, 40) + (400 if far else 0), by + rng.randint(-6, 6), _rand(rng, w, h, 0.3)))
            ids.append(len(S) - 1)
        comps.append(ids)
    # identical members, and a member listed twice
    S.append((10, 10, _rand(rng, 40, 4, 0.5)))
    S.append((10, 10, S[-1][2].copy()))
    comps.append([len(S) - 2, len(S) - 1, len(S) - 2])
    # boxes wider than their set bits: the union box must be tightened
    loose = np.zeros((6, 100), bool)
    loose[2:4, 37:70] = True
    S.append((64, 64, loose))
    S.append((64, 66, loose))
    comps.append([len(S) - 2, len(S) - 1])
    order = rng.permutation(len(comps))
    comps = [comps[i] for i in order]
    comp_offsets = np.concatenate([[0], np.cumsum([len(c) for c in comps])]).astype(np.int32)
    member_ids = np.concatenate(comps).astype(np.int32)
    pool, desc = _pack(S)
    pool_t, desc_t = ops.tile_upload(pool, desc, dev)
    u = ops.tile_union(pool_t, desc_t, desc, comp_offsets, member_ids)
    torch.cuda.synchronize()
    out_desc, out_count = u["out_desc"].cpu().numpy(), u["out_count"].cpu().numpy()
    out_pool, fresh_pool = u["out_pool"].cpu().numpy().view(np.uint32), u["fresh_pool"].cpu().numpy().view(np.uint32)
    q = 0
    for c, ids in enumerate(comps):
        pix = np.unique(np.concatenate([_pixels(S[i]) for i in ids]), axis=0)
        y0, x0 = pix.min(axis=0)
        y1, x1 = pix.max(axis=0)
        gx0, gy0, gw, gh, goff, gwpr = out_desc[c].tolist()
        assert (gx0, gy0, gw, gh) == (x0, y0, x1 - x0 + 1, y1 - y0 + 1), c
        assert goff == u["out_offsets"][c] and gwpr == (gw + 31) // 32
        assert out_count[c] == len(pix)
        got = np.argwhere(unpack_bitmap(out_pool[goff:goff + gh * gwpr], gh, gw, gwpr)) + (gy0, gx0)
        assert np.array_equal(got, pix[np.lexsort((pix[:, 1], pix[:, 0]))]), c
        padding = np.unpackbits(out_pool[goff:goff + gh * gwpr].view(np.uint8).reshape(gh, gwpr * 4), axis=1, bitorder="little")[:, gw:]
        assert not padding.any()
        seen = set()
        for i in ids:                          # fresh bitmaps: the first-seen order of the reference's list union
            x, y, m = S[i]
            h, w = m.shape
            wpr = (w + 31) // 32
            fo = int(u["fresh_offsets"][q])
            fresh = np.argwhere(unpack_bitmap(fresh_pool[fo:fo + h * wpr], h, w, wpr)) + (y, x)
            want = [p for p in map(tuple, _pixels(S[i]).tolist()) if p not in seen]
            assert [tuple(p) for p in fresh.tolist()] == want, (c, i)
            seen.update(want)
            q += 1
    assert q == len(member_ids)


# ---- SFinder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.fixture_names(np.load(cases.GOLDEN)))
def test_device_path_equals_host_and_reference(dev, name):
    from caesar_mrcnn_amd.sfinder import SFinder
    sc, grid, want = cases.decode(name, np.load(cases.GOLDEN))
    cfg = cases.make_config()
    out = {}
    for path in ("merge_edge_sources_device", "merge_edge_sources_host"):
        sf = SFinder(None, cfg)
        got_grid, got = cases.drive(sf, sc, cfg, merge=getattr(sf, path))
        assert got_grid == grid
        out[path] = cases.canon(got)
    assert out["merge_edge_sources_device"] == out["merge_edge_sources_host"]
    assert out["merge_edge_sources_device"] == want


@pytest.mark.parametrize("step", [1.0, 0.5])
def test_device_path_on_planted_mosaic(dev, tmp_path, step):
    """A few dozen ellipses, every one cut or seen several times at step 0.5: the switch `merge_device` picks the device path
    and it writes the host path's catalogue."""
    from caesar_mrcnn_amd import fits
    from caesar_mrcnn_amd.sfinder import SFinder
    labels, n = cases.planted_mosaic(11)
    path = str(tmp_path / "mosaic.fits")
    fits.write_fits(path, labels.astype(np.float32))
    got = {}
    for device in (True, False):
        cfg = cases.label_map_config(path)
        cfg.TILE_XSTEP = cfg.TILE_YSTEP = step
        sf = SFinder(cases.LabelMapModel(cfg), cfg)
        assert sf.merge_device is True                 # default: on where there is a GPU
        sf.merge_device = device
        called = []
        real = sf.merge_edge_sources_device
        sf.merge_edge_sources_device = lambda: (called.append(1), real())[1]
        sf.outfile_json = str(tmp_path / ("cat%d.json" % device))
        sf.outfile_ds9 = str(tmp_path / ("cat%d.reg" % device))
        assert sf.run_parallel() == 0
        assert bool(called) == device
        got[device] = cases.canon(sf.sources["sources"])
    assert len(got[True]) == n
    assert got[True] == got[False]


# ---- command line --------------------------------------------------------------------------------------------------
def test_cli_merge_tile_sources(dev, tmp_path):
    from caesar_mrcnn_amd import fits
    d = str(tmp_path)
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:256, 0:256]
    img = rng.normal(0, 1, (256, 256)).astype(np.float32)
    for cy, cx in ((128, 128), (60, 127), (200, 40), (128, 200)):            # blobs on the tile borders of a 2 x 2 grid
        img += 80 * np.exp(-0.5 * (((yy - cy) / 6.0) ** 2 + ((xx - cx) / 9.0) ** 2))
    fits.write_fits(os.path.join(d, "mosaic.fits"), img, {"BUNIT": "JY/BEAM"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "detect", "--imgsize", "128", "--backbone", "custom",
                        "--logs", os.path.join(d, "logs"), "--image", os.path.join(d, "mosaic.fits"), "--scoreThr", "0.0",
                        "--split_img_in_tiles", "--tile_xsize", "128", "--tile_ysize", "128", "--merge_tile_sources"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    assert glob.glob(os.path.join(d, "*.json")) == [os.path.join(d, "out_mosaic.json")]
    res = json.load(open(os.path.join(d, "out_mosaic.json")))
    assert res["image_id"] == "mosaic" and isinstance(res["objs"], list)
    keys = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "pixels", "vertexes", "edge", "merged"}
    for s in res["objs"]:
        assert set(s) == keys
    assert [s["name"] for s in res["objs"]] == ["S%d" % (i + 1) for i in range(len(res["objs"]))]
    assert "sources (" in out and "written to out_mosaic.json" in out
    if res["objs"]:
        assert open(os.path.join(d, "out_mosaic.reg")).read().splitlines()[2] == "image"
