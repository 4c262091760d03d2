"""Class-weighted head losses (run.py --weight_classes) without a GPU: the float64 statement the GPU tests compare
the kernels with agrees with the oracle when every weight is one, compute_class_weights follows the reference's formula,
utils.class_weight_vector builds and refuses what it should, and run.py refuses a training class id the model does not have."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import class_weight_cases as CW
import model_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _run_py():
    spec = importlib.util.spec_from_file_location("_class_weights_run_py", os.path.join(ROOT, "scripts", "run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the statement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
@pytest.mark.parametrize("num_classes,cycle", [(4, False), (6, True)])
def test_statement_with_weights_of_one_is_the_oracle(num_classes, cycle, dice):
    """weighted_losses_statement with cw = None and with cw = ones against model_cases.losses_reference (the float32 oracle), at
    the tolerances of the kernel tests."""
    d = M.losses_inputs(num_classes, cycle)
    ref = M.losses_reference(CW.loss_cfg(dice, num_classes), d)
    for cw in (None, np.ones(num_classes, np.float32)):
        got = CW.weighted_losses_statement(d, dice, cw)
        fl, fg = M.tolerance_fractions(got[0], got[1], ref[0], ref[1])
        print("[statement C=%d dice=%s cw=%s] worst fraction of the tolerance: losses %.3g, gradients %.3g" % (
            num_classes, dice, "None" if cw is None else "ones", fl, fg))
        M.assert_losses_close(got[0], got[1], ref[0], ref[1])
        assert all(np.abs(got[1][n]).max() > 0 for n in M.LOSS_GRADS)


@pytest.mark.parametrize("dice", [False, True])
def test_statement_weights_act_on_the_head_losses_only(dice):
    """Non-trivial weights change the three head losses of the statement and leave its RPN side exactly alone; one weight for all
    classes scales the class, box and cross-entropy mask loss by it and leaves the Dice loss where it was (up to the smoothing
    term)."""
    d = M.losses_inputs(4, False)
    base = CW.weighted_losses_statement(d, dice)
    got = CW.weighted_losses_statement(d, dice, CW.case_weights(4))
    assert np.array_equal(got[0][:2], base[0][:2]) and all(np.array_equal(got[1][n], base[1][n]) for n in ("rpn_logits", "rpn_bbox"))
    assert all(got[0][i] != base[0][i] for i in (2, 3, 4))
    three = CW.weighted_losses_statement(d, dice, np.full(4, 3.0, np.float32))
    np.testing.assert_allclose(three[0][2:4], 3.0 * base[0][2:4], rtol=1e-12)
    np.testing.assert_allclose(three[0][4], base[0][4] if dice else 3.0 * base[0][4], rtol=1e-9)


# ---- 2. compute_class_weights ------------------------------------------------------------------------------------------------------------
def _dataset(nobjs):
    from caesar_mrcnn_amd.dataset import SourceDataset
    ds = SourceDataset()
    assert ds.set_class_dict('{"sidelobe":1,"source":2,"galaxy":3}') == 0
    ds.nobjs_per_class = list(nobjs)
    return ds


def test_compute_class_weights_counts_the_classes_that_have_objects():
    """nobjs / (nclasses_with_objects * nobjs_k), and 1.0 for a class without objects, the background included: with 30 + 60
    objects in two of three classes, 90 / (2 * 30) and 90 / (2 * 60)."""
    w = _dataset([0, 30, 60, 0]).compute_class_weights()
    assert w == {0: 1.0, 1: 1.5, 2: 0.75, 3: 1.0}
    w = _dataset([0, 10, 10, 20]).compute_class_weights()
    assert set(w) == {0, 1, 2, 3} and w[0] == 1.0
    np.testing.assert_allclose([w[1], w[2], w[3]], [4.0 / 3.0, 4.0 / 3.0, 2.0 / 3.0], rtol=1e-15)
    # the object-weighted mean of the weights is 1
    for nobjs in ([0, 30, 60, 0], [0, 10, 10, 20], [0, 1, 999, 7]):
        w = _dataset(nobjs).compute_class_weights()
        np.testing.assert_allclose(sum(w[k] * n for k, n in enumerate(nobjs)) / sum(nobjs), 1.0, rtol=1e-12)
    assert _dataset([0, 0, 0, 0]).compute_class_weights() == {0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0}


# ---- 3. class_weight_vector --------------------------------------------------------------------------------------------------------------
def test_class_weight_vector():
    from caesar_mrcnn_amd.utils import class_weight_vector
    v = class_weight_vector({1: 2.0, 3: 0.5}, 4)                  # a dict with gaps: missing ids weigh 1
    assert v.dtype == np.float32 and v.tolist() == [1.0, 2.0, 1.0, 0.5]
    assert class_weight_vector({np.int64(2): 4}, 3).tolist() == [1.0, 1.0, 4.0]
    assert class_weight_vector({}, 2).tolist() == [1.0, 1.0]
    v = class_weight_vector([0.25, 1.5, 3.0], 3)                    # a sequence
    assert v.dtype == np.float32 and v.tolist() == [0.25, 1.5, 3.0]
    assert class_weight_vector(np.array([2.0, 2.0]), 2).tolist() == [2.0, 2.0]
    assert class_weight_vector(_dataset([0, 30, 60, 0]).compute_class_weights(), 4).tolist() == [1.0, 1.5, 0.75, 1.0]


@pytest.mark.parametrize("bad", [{4: 1.0}, {-1: 1.0}, {1.5: 1.0}, [1.0, 2.0], [1.0] * 5, [[1.0] * 4], {1: 0.0}, {2: -1.0},
                                 {1: float("nan")}, {1: float("inf")}, [1.0, 0.0, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0],
                                 [1.0, 1e-50, 1.0, 1.0], [1.0, 1e39, 1.0, 1.0]],
                         ids=lambda b: repr(b).replace(" ", ""))
def test_class_weight_vector_refusals(bad):
    """An id outside [0, C), a sequence of another length, a weight that is not finite or not > 0 -- as float32, which is what the
    kernels read (1e-50 is 0 there and 1e39 infinite)."""
    from caesar_mrcnn_amd.utils import class_weight_vector
    with pytest.raises(ValueError):
        class_weight_vector(bad, 4)


# ---- 4. run.py -------------------------------------------------------------------------------------------------------------------------
def test_run_py_refuses_a_training_class_id_the_model_does_not_have(monkeypatch, caplog):
    """`train --weight_classes` with a --classdict id outside the classes of --classdict_model: refused before the model is built,
    with the id in the message; the same dictionaries pass the check without the flag and with ids in range."""
    run = _run_py()
    from caesar_mrcnn_amd import model as modellib

    class Built(Exception):
        pass

    def no_model(*a, **k):
        raise Built()
    monkeypatch.setattr(modellib, "MaskRCNN", no_model)
    base = ["train", "--datalist", "unused.dat", "--imgsize", "128", "--backbone", "custom"]
    wide = ['--classdict', '{"sidelobe":1,"source":2,"galaxy":3}', '--classdict_model', '{"sidelobe":1,"source":2}']
    with caplog.at_level("ERROR"):
        assert run.main(base + wide + ["--weight_classes"]) == 1
    assert any("--weight_classes" in r.getMessage() and "galaxy=3" in r.getMessage() for r in caplog.records)
    with pytest.raises(Built):                                     # without the flag nothing changes: the model is built
        run.main(base + wide)
    with pytest.raises(Built):                                     # ids in range: the model is built
        run.main(base + ['--classdict', '{"sidelobe":1,"source":2}', '--classdict_model', '{"sidelobe":1,"source":2,"galaxy":3}',
                         "--weight_classes"])
    assert run.weight_classes_refusal({"a": 1, "b": 2}, {"a": 1, "b": 2}) is None
    assert run.weight_classes_refusal({"bkg": 0, "a": 1}, {"a": 1}) is None
    assert "b=-1" in run.weight_classes_refusal({"a": 1, "b": -1}, {"a": 1, "b": 2})


def test_train_signature_and_config_default():
    """None is the default everywhere."""
    import inspect
    from caesar_mrcnn_amd import ops
    from caesar_mrcnn_amd.config import Config
    from caesar_mrcnn_amd.model import MaskRCNN
    assert Config.CLASS_WEIGHTS is None
    assert inspect.signature(MaskRCNN.train).parameters["class_weights"].default is None
    assert inspect.signature(ops.losses_fwd_bwd).parameters["class_weights"].default is None
    assert hasattr(MaskRCNN, "set_class_weights")
