"""analyze.outline_statement -- the closed-form rule the kernels of csrc/outline.hip follow -- against analyze.find_contours on the
1-padded mask and np.argwhere, and the Analyzer.results_device / SFinder.results_device switches where no GPU is there."""
import numpy as np
import pytest

import caesar_mrcnn_amd  # noqa: F401
from caesar_mrcnn_amd import _hip, analyze

import analyze_post_cases as post
import outline_cases as cases


def _assert_statement(mask, tag):
    contours, pixels = analyze.outline_statement(mask)
    want_c, want_p = cases.reference(mask)
    assert len(contours) == len(want_c), (tag, len(contours), len(want_c))
    for k, (a, b) in enumerate(zip(contours, want_c)):
        assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b), (tag, k)
    assert pixels.dtype == want_p.dtype and np.array_equal(pixels, want_p), tag


def test_outline_statement_on_the_kernel_cases():
    for name, mask in cases.size_grid() + cases.shapes():
        _assert_statement(mask, name)
        _assert_statement(mask.astype(bool), name + " (bool)")
    for k, mask in enumerate(cases.blobs((60, 100), 6, 8)):
        _assert_statement(mask, "blob %d" % k)


def test_outline_statement_on_random_masks():
    """300 seeded masks: random fill, XOR-ed rectangles, full frames with holes, thinned checkerboards (saddles of both kinds)."""
    rng = np.random.default_rng(2024)
    total = 0
    for t in range(300):
        h, w = (int(v) for v in rng.integers(1, 41, size=2))
        kind = t % 4
        if kind == 0:
            m = rng.uniform(size=(h, w)) < rng.uniform(0.05, 0.95)
        elif kind == 1:
            m = np.zeros((h, w), bool)
            for _ in range(int(rng.integers(1, 6))):
                y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
                m[y:y + int(rng.integers(1, 12)), x:x + int(rng.integers(1, 12))] ^= True
        elif kind == 2:
            m = np.ones((h, w), bool)
            m[int(rng.integers(0, h)), int(rng.integers(0, w))] = False
            m &= rng.uniform(size=(h, w)) < 0.97
        else:
            m = (np.indices((h, w)).sum(0) % 2 == int(rng.integers(0, 2))) & (rng.uniform(size=(h, w)) < 0.8)
        _assert_statement(m.astype(np.uint8), "random %d" % t)
        total += len(cases.reference(m.astype(np.uint8))[0])
    assert total > 5000


def test_outline_statement_refuses_other_ranks():
    with pytest.raises(ValueError):
        analyze.outline_statement(np.zeros((2, 2, 2), np.uint8))
    contours, pixels = analyze.outline_statement(np.zeros((0, 5), np.uint8))
    assert contours == [] and pixels.shape == (0, 2)


class _Cpu(object):
    type = "cpu"


class _CpuEngine(object):
    dev = _Cpu()


def _analyzer(objs, shape, results_device, tmp_path, tag):
    an = post.analyzer(objs, shape, {}, device=False)
    an.model.engine = _CpuEngine()                              # Analyzer.has_gpu(model) is False wherever this runs
    an.write_to_json = an.write_to_ds9 = True
    an.outfile_json, an.outfile_ds9 = str(tmp_path / (tag + ".json")), str(tmp_path / (tag + ".reg"))
    an.results_device = results_device
    return an


def test_switch_defaults():
    an = post.analyzer([], (4, 4), {}, device=False)
    assert analyze.Analyzer.RESULTS_DEVICE is False and an.results_device is False
    assert an.results_device_min_masks == analyze.Analyzer.RESULTS_DEVICE_MIN_MASKS and an.results_timing == {}
    from caesar_mrcnn_amd import sfinder
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=4, imgsize=64, mode="inference")
    cfg.IMG_PATH = "none.fits"
    sf = sfinder.SFinder(None, cfg)
    assert sf.results_device is False
    assert sfinder.TileTask((0, 9, 0, 9), None, cfg).results_device is False


def test_switch_on_without_gpu_takes_the_host_path(tmp_path):
    name, shape, objs, _ = post.scenarios()[0]
    on = post.run(_analyzer(objs, shape, True, tmp_path, "on"), shape)
    off = post.run(_analyzer(objs, shape, False, tmp_path, "off"), shape)
    assert analyze.Analyzer.has_gpu(on.model) is False
    assert len(off.results["objs"]) >= 2 and on.results_timing == {}
    post.assert_same(on, off, name)
    for ext in (".json", ".reg"):
        assert (tmp_path / ("on" + ext)).read_bytes() == (tmp_path / ("off" + ext)).read_bytes()


def test_other_values_and_failures_stay_on_the_host(tmp_path, monkeypatch):
    """Masks holding a value other than 0 / 1 never reach the device form, whatever the switch says; a device form that raises
    is logged once and left for good."""
    name, shape, objs, _ = post.scenarios()[0]
    an = post.run(_analyzer(objs, shape, False, tmp_path, "a"), shape)
    ref = an.results
    monkeypatch.setattr(analyze.Analyzer, "has_gpu", staticmethod(lambda model: True))
    calls = []
    monkeypatch.setattr(analyze.Analyzer, "make_json_results_device", lambda self: calls.append(1) or self.make_json_results_host())
    an.results_device = True
    assert an._results_masks_ok()
    an.make_json_results()
    assert calls == [1] and an.results == ref                     # eligible masks reach it ...
    keep = an.masks_final
    an.masks_final = [keep[0][None]] + list(keep[1:])
    assert not an._results_masks_ok()                             # (the host statement cannot take a 3-D mask either)
    for bad in (keep[0].astype(np.int32) * 2, keep[0].astype(np.float32), keep[0][:-1]):
        an.masks_final = [bad] + list(keep[1:])
        assert not an._results_masks_ok()
        an.make_json_results()
        assert calls == [1]                                       # ... any other array does not
    an.masks_final = keep
    an.results_device_min_masks = len(keep) + 1                   # below the threshold: host
    an.make_json_results()
    assert calls == [1]
    an.results_device_min_masks = 1

    def broken(self):
        calls.append(2)
        raise _hip.HipPathError("no library")
    monkeypatch.setattr(analyze, "device_forms_failed", set())
    monkeypatch.setattr(analyze.Analyzer, "make_json_results_device", broken)
    an.make_json_results()
    an.make_json_results()
    assert calls == [1, 2] and an.results == ref and analyze.device_forms_failed == {"make_json_results_device"}


def test_failed_device_forms_are_left_for_the_process(tmp_path, monkeypatch, caplog):
    """make_json_results_device, and the outlines of SFinder's merged sources (whose host answer is None: find_contours later)."""
    from caesar_mrcnn_amd import ops, sfinder
    from caesar_mrcnn_amd.config import run_py_config
    name, shape, objs, _ = post.scenarios()[0]
    an = post.run(_analyzer(objs, shape, False, tmp_path, "a"), shape)
    want = an.results
    monkeypatch.setattr(analyze.Analyzer, "has_gpu", staticmethod(lambda model: True))
    an.results_device = True

    def results():
        an.results = {}
        an.make_json_results()
        return an.results
    post.check_failure_policy(monkeypatch, caplog, "make_json_results_device",
                              lambda entered: monkeypatch.setattr(analyze.Analyzer, "make_json_results_device", post.planted_failure(entered)),
                              results, want)
    cfg = run_py_config(num_classes=4, imgsize=64, mode="inference")
    cfg.IMG_PATH = "none.fits"
    sf = sfinder.SFinder(None, cfg)
    post.check_failure_policy(monkeypatch, caplog, "bitmap_outlines",
                              lambda entered: monkeypatch.setattr(ops, "bitmap_outlines", post.planted_failure(entered)),
                              lambda: sf._union_outlines({"out_pool": None, "out_desc": None}, None), None)
