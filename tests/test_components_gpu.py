"""Connected components of bit planes on the GPU (csrc/components.hip through ops.mask_components / mask_components_split /
mask_row_extents) against the host statement, exactly: on every scene of tests/components_cases.py and for both connectivities the
component counts, every piece as a plane (bits, count, box), the "first" mode, the bytes of a second run, the row extents; and on
the C entry points themselves that nothing outside the outputs and the workspace is written and that a refused table writes
nothing at all."""
import ctypes

import numpy as np
import pytest
import torch

import components_cases as cases
from caesar_mrcnn_amd import _hip, analyze, ops

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in cases.scenes()]
SENTINEL = 0x5A5A5A5A
GUARD = 64                       # int32 words of sentinel on either side of a buffer


def _planes(name, dev):
    planes = cases.scene(name)
    masks = np.ascontiguousarray(np.moveaxis(planes, 0, -1))
    return ops.mask_planes_pack(torch.from_numpy(masks.view(np.uint8)).to(dev))


def _label_maps(pieces, offs, n, H, W):
    """(label map, cover) [n, H, W] int32 on the device from the emitted pieces: the sum of (rank + 1) * piece and the number of
    pieces that hold a pixel.  cover <= 1 and a label map equal to the host's say that piece k IS labels == k, for every k."""
    dev = pieces.words.device
    labels = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
    cover = torch.zeros((n, H, W), dtype=torch.int32, device=dev)
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    for p in range(n):
        for first in range(int(offs[p]), int(offs[p + 1]), 256):
            last = min(first + 256, int(offs[p + 1]))
            bits = ((pieces.words[first:last].unsqueeze(-1) >> shifts) & 1).reshape(last - first, H, -1)
            assert int(bits[:, :, W:].sum()) == 0                                    # the bits past W stay zero
            bits = bits[:, :, :W]
            rank = torch.arange(first - int(offs[p]) + 1, last - int(offs[p]) + 1, dtype=torch.int32, device=dev)
            labels[p] += (bits * rank[:, None, None]).sum(0, dtype=torch.int32)
            cover[p] += bits.sum(0, dtype=torch.int32)
    return labels, cover


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_components_equal_the_host_labelling(dev, name, conn):
    scene = cases.scene(name)
    n, H, W = scene.shape
    ref = cases.reference(name, conn)
    planes = _planes(name, dev)
    handle = ops.mask_components(planes, conn)
    want_n = [k for _, k in ref]
    assert handle.ncomp.cpu().numpy().tolist() == want_n
    pieces, offs = ops.mask_components_split(handle)
    assert offs.tolist() == np.concatenate([[0], np.cumsum(want_n)]).tolist() and pieces.n == sum(want_n)
    assert (pieces.H, pieces.W, pieces.wpr) == (H, W, (W + 31) // 32)
    want_labels = np.stack([lab for lab, _ in ref])
    if pieces.n <= 1200:                                                             # the literal comparison: piece k == (labels == k)
        got = analyze.unpack_mask_planes(pieces.words.cpu().numpy(), W).astype(bool) if pieces.n else np.zeros((0, H, W), bool)
        want = [want_labels[p] == k + 1 for p in range(n) for k in range(want_n[p])]
        assert np.array_equal(got, np.stack(want) if want else np.zeros((0, H, W), bool))
    labels, cover = _label_maps(pieces, offs, n, H, W)
    assert np.array_equal(labels.cpu().numpy(), want_labels)
    assert np.array_equal(cover.cpu().numpy(), (scene != 0).astype(np.int32))
    stats = [cases.label_boxes(lab, k) for lab, k in ref]
    assert np.array_equal(pieces.count.cpu().numpy(), np.concatenate([s[0] for s in stats]))
    assert np.array_equal(pieces.box.cpu().numpy(), np.concatenate([s[1] for s in stats]))
    if 0 < pieces.n <= 1200:
        assert np.array_equal(pieces.box.cpu().numpy(), cases.boxes_of(got))      # utils.extract_bboxes itself
        assert np.array_equal(pieces.count.cpu().numpy(), got.reshape(pieces.n, -1).sum(1))

    # "first": component 1 of every plane that has one
    firsts, foffs = ops.mask_components_split(handle, first_only=True)
    assert foffs.tolist() == np.concatenate([[0], np.cumsum([min(k, 1) for k in want_n])]).tolist()
    sel = torch.as_tensor([int(offs[p]) for p in range(n) if want_n[p]], dtype=torch.long, device=dev)
    assert torch.equal(firsts.words, pieces.words.index_select(0, sel))
    assert torch.equal(firsts.count, pieces.count.index_select(0, sel)) and torch.equal(firsts.box, pieces.box.index_select(0, sel))

    # a second run: the same bytes
    again = ops.mask_components(planes, conn, boxes_host=handle.boxes_host)
    assert torch.equal(again.ncomp, handle.ncomp)                       # (the workspace's unused capacity is never written: not compared)
    pieces2, offs2 = ops.mask_components_split(again)
    assert offs2.tolist() == offs.tolist() and torch.equal(pieces2.words, pieces.words)
    assert torch.equal(pieces2.count, pieces.count) and torch.equal(pieces2.box, pieces.box)

    # the pieces are planes like any other: they go straight into the mask graph
    if 2 <= pieces.n <= 600:
        ids = np.arange(pieces.n)
        plane_of = np.searchsorted(offs, ids, side="right") - 1
        near = plane_of[:-1] == plane_of[1:]                                         # neighbours in the list that are pieces of one plane
        inter, _ = ops.mask_pair_stats(pieces, np.stack([ids[:-1][near], ids[1:][near]], axis=1).astype(np.int32))
        assert int(inter.sum()) == 0                                                 # ... are disjoint
        whole = ops.mask_union(pieces, offs, np.arange(pieces.n))
        assert torch.equal(whole.words, planes.words) and torch.equal(whole.count, planes.count)


@pytest.mark.parametrize("name", NAMES)
def test_row_extents_equal_the_host(dev, name):
    scene = cases.scene(name)
    planes = _planes(name, dev)
    boxes = cases.boxes_of(scene)
    extents, offs = ops.mask_row_extents(planes)
    assert offs.tolist() == np.concatenate([[0], np.cumsum(boxes[:, 2] - boxes[:, 0])]).tolist()
    got = extents.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (int(offs[-1]), 2)
    for p, plane in enumerate(scene):
        part = got[offs[p]:offs[p + 1]]
        idx = np.arange(plane.shape[1])
        rows = plane[boxes[p, 0]:boxes[p, 2]]
        any_ = rows.any(1)
        first = np.where(any_, np.where(rows, idx, plane.shape[1]).min(1), -1)
        last = np.where(any_, np.where(rows, idx, -1).max(1), -1)
        assert np.array_equal(part, np.stack([first, last], 1)), (name, p)
        points = analyze.row_extents_points(part, boxes[p, 0])
        want = analyze.row_extreme_points(plane)
        assert (points is None and want is None) or np.array_equal(points, want)
    again, _ = ops.mask_row_extents(planes, boxes_host=boxes)
    assert torch.equal(again, extents)


def test_a_smaller_box_hides_pixels(dev):
    """The labelling and the extents are those of the plane cut to its box: boxes other than the planes' own, one of them leaving
    the frame, one empty."""
    scene = cases.scene("mixed_70x67")
    n, H, W = scene.shape
    planes = _planes("mixed_70x67", dev)
    boxes = np.array([[5, 9, 60, 40], [0, 31, 70, 33], [-4, -4, 200, 200], [30, 40, 31, 41], [0, 0, 0, 0], [69, 66, 70, 67], [10, 0, 50, 67],
                      [3, 32, 64, 64], [60, 1, 70, 2]], np.int32)
    cut = np.zeros_like(scene)
    for p, (y1, x1, y2, x2) in enumerate(boxes):
        cut[p, max(y1, 0):y2, max(x1, 0):x2] = scene[p, max(y1, 0):y2, max(x1, 0):x2]
    planes.box = torch.from_numpy(boxes).to(dev)
    for conn in (4, 8):
        handle = ops.mask_components(planes, conn)
        pieces, offs = ops.mask_components_split(handle)
        want = [cases.label_host(c, conn) for c in cut]
        assert handle.ncomp_host.tolist() == [k for _, k in want]
        labels, cover = _label_maps(pieces, offs, n, H, W)
        assert np.array_equal(labels.cpu().numpy(), np.stack([lab for lab, _ in want])) and int(cover.max()) <= 1
    extents, offs = ops.mask_row_extents(planes)
    got = extents.cpu().numpy()
    for p, (y1, x1, y2, x2) in enumerate(boxes):
        rows = range(max(y1, 0), min(y2, H)) if x2 > x1 else []
        assert offs[p + 1] - offs[p] == len(rows)
        for r, y in enumerate(rows):
            xs = np.flatnonzero(cut[p, y])
            assert tuple(got[offs[p] + r]) == ((xs[0], xs[-1]) if xs.size else (-1, -1))


# ---- the C entry points, between sentinels ------------------------------------------------------------------------------------
def _guarded(words, dev):
    buf = torch.full((GUARD + max(words, 1) + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf.data_ptr() + 4 * GUARD


def _untouched(buf, words):
    words = max(words, 1)
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + words:] == SENTINEL).all())


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", ["seam", "mixed_70x67", "stripes_%d" % (cases.LDS_RUNS + 1), "full_and_empty"])
def test_nothing_is_written_outside_the_outputs(dev, name):
    scene = cases.scene(name)
    n, H, W = scene.shape
    wpr = (W + 31) // 32
    planes = _planes(name, dev)
    L = _hip.lib()
    stream = ops.current_stream()
    boxes, boxes_p = _host(cases.boxes_of(scene))
    ws_bytes = L.mrcnn_mask_components_workspace(n, H, W, boxes_p)
    ws, ws_p = _guarded(ws_bytes // 4, dev)
    ncomp, ncomp_p = _guarded(n, dev)
    assert L.mrcnn_mask_components_count(planes.words.data_ptr(), boxes_p, planes.box.data_ptr(), n, H, W, 4, ws_p, ws_bytes, ncomp_p, stream) == 0
    torch.cuda.synchronize()
    assert _untouched(ws, ws_bytes // 4) and _untouched(ncomp, n)
    nc = ncomp[GUARD:GUARD + n].cpu().numpy()
    assert nc.tolist() == [k for _, k in cases.reference(name, 4)]
    for mode, per in ((0, nc), (1, np.minimum(nc, 1))):
        offs, offs_p = _host(np.concatenate([[0], np.cumsum(per)]))
        P = int(offs[-1])
        offs_t = torch.from_numpy(offs).to(dev)
        out, out_p = _guarded(P * H * wpr, dev)
        count, count_p = _guarded(P, dev)
        box, box_p = _guarded(4 * P, dev)
        assert L.mrcnn_mask_components_emit(boxes_p, planes.box.data_ptr(), n, H, W, ws_p, ws_bytes, ncomp_p, offs_p, offs_t.data_ptr(), mode,
                                            out_p, count_p, box_p, stream) == 0
        torch.cuda.synchronize()
        assert _untouched(out, P * H * wpr) and _untouched(count, P) and _untouched(box, 4 * P)
        assert _untouched(ws, ws_bytes // 4) and _untouched(ncomp, n)
        assert int(count[GUARD:GUARD + P].sum()) == (int(scene.sum()) if mode == 0 else
                                                     sum(int((lab == 1).sum()) for lab, _ in cases.reference(name, 4)))
    rows, rows_p = _host(np.concatenate([[0], np.cumsum(boxes[:, 2] - boxes[:, 0])]))
    R = int(rows[-1])
    rows_t = torch.from_numpy(rows).to(dev)
    ext, ext_p = _guarded(2 * R, dev)
    assert L.mrcnn_mask_row_extents(planes.words.data_ptr(), boxes_p, planes.box.data_ptr(), n, H, W, rows_t.data_ptr(), R, ext_p, stream) == 0
    torch.cuda.synchronize()
    assert _untouched(ext, 2 * R) and not bool((ext[GUARD:GUARD + 2 * R] == SENTINEL).any())


def test_a_refused_table_launches_and_writes_nothing(dev):
    scene = cases.scene("mixed_70x67")
    n, H, W = scene.shape
    wpr = (W + 31) // 32
    planes = _planes("mixed_70x67", dev)
    L = _hip.lib()
    stream = ops.current_stream()
    boxes, boxes_p = _host(cases.boxes_of(scene))
    ws_bytes = L.mrcnn_mask_components_workspace(n, H, W, boxes_p)
    ws, ws_p = _guarded(ws_bytes // 4, dev)
    ncomp, ncomp_p = _guarded(n, dev)
    out, out_p = _guarded(4 * H * wpr, dev)
    small, small_p = _guarded(64, dev)
    offs, offs_p = _host([0, 1, 2, 3, 4, 4, 4, 4, 4, 4])
    offs_t = torch.from_numpy(offs).to(dev)
    bad_offs, bad_offs_p = _host([0, 2, 1, 3, 4, 4, 4, 4, 4, 4])
    two, two_p = _host([0, 2, 2, 3, 4, 4, 4, 4, 4, 4])
    count = lambda *a: L.mrcnn_mask_components_count(planes.words.data_ptr(), boxes_p, planes.box.data_ptr(), *a)
    emit = lambda host, mode, n_=n, H_=H: L.mrcnn_mask_components_emit(boxes_p, planes.box.data_ptr(), n_, H_, W, ws_p, ws_bytes, ncomp_p, host,
                                                                       offs_t.data_ptr(), mode, out_p, small_p, small_p + 64, stream)
    assert count(n, H, W, 6, ws_p, ws_bytes, ncomp_p, stream) == -1                   # no such connectivity
    assert count(0, H, W, 4, ws_p, ws_bytes, ncomp_p, stream) == -1
    assert count(n, H, W, 4, ws_p, ws_bytes - 4, ncomp_p, stream) == -3               # a workspace one word short
    assert count(n, 8193, W, 4, ws_p, 1 << 30, ncomp_p, stream) == -4                 # past a cap
    assert count(4097, H, W, 4, ws_p, 1 << 30, ncomp_p, stream) == -4
    assert emit(bad_offs_p, 0) == -1 and emit(two_p, 1) == -1 and emit(offs_p, 2) == -1 and emit(offs_p, 0, H_=8193) == -4
    rows, rows_p = _host(np.concatenate([[0], np.cumsum(boxes[:, 2] - boxes[:, 0])]))
    rows_t = torch.from_numpy(rows).to(dev)
    R = int(rows[-1])
    ext, ext_p = _guarded(2 * R, dev)
    assert L.mrcnn_mask_row_extents(planes.words.data_ptr(), boxes_p, planes.box.data_ptr(), n, H, W, rows_t.data_ptr(), R - 1, ext_p, stream) == -1
    assert L.mrcnn_mask_row_extents(planes.words.data_ptr(), boxes_p, planes.box.data_ptr(), 0, H, W, rows_t.data_ptr(), R, ext_p, stream) == -1
    torch.cuda.synchronize()
    for buf in (ws, ncomp, out, small, ext):
        assert bool((buf == SENTINEL).all())
    # and through ops: the exceptions of a refusal, before anything is launched
    with pytest.raises(ValueError):
        ops.mask_components(planes, 6)
    with pytest.raises(ops.ComponentsUnsupported):
        ops.mask_components(ops.MaskPlanes(torch.zeros((1, 8193, 1), dtype=torch.int32, device=dev), planes.count[:1], planes.box[:1], 8))
