"""Class-weighted head losses on the GPU (run.py --weight_classes): mrcnn_losses_fwd_bwd_weighted against the float64
statement of tests/class_weight_cases.py at the tolerances of the loss tests; weights of one, the RPN side and repeated calls bit
for bit; the refusals of ops.losses_fwd_bwd; the engine's step, its launch tape across a change of the weights, and
MaskRCNN.train()."""
import numpy as np
import pytest
import torch

import class_weight_cases as CW
import model_cases as M

pytestmark = pytest.mark.gpu


def _ops():
    from caesar_mrcnn_amd import ops
    return ops


def _run_losses(dev, d, dice, cw=None):
    """ops.losses_fwd_bwd on the NumPy operands d -> (losses[5], {name: gradient}) as NumPy.  cw: NumPy [C] or None."""
    D = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    out = _ops().losses_fwd_bwd(D(d["rpn_match"]), D(d["rpn_bbox_t"]), D(d["rpn_logits"]), D(d["rpn_bbox"]), D(d["tcls"]), D(d["tbbox"]),
                                D(d["tmask"]), D(d["active"][0].copy()), D(d["logits"]), D(d["mbbox"]), D(d["mmask"]), M.LOSS_WEIGHTS, dice,
                                class_weights=None if cw is None else D(np.asarray(cw, np.float32)))
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), {n: g.cpu().numpy() for n, g in zip(M.LOSS_GRADS, out[1:])}


def _report(tag, got, ref):
    fl, fg = M.tolerance_fractions(got[0], got[1], ref[0], ref[1])
    print("[%s] worst fraction of the tolerance: losses %.3g, gradients %.3g" % (tag, fl, fg))


def _same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and all(np.array_equal(a[1][n], b[1][n], equal_nan=True) for n in M.LOSS_GRADS)


# ---- 1. kernel parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
@pytest.mark.parametrize("num_classes", [2, 4, 6])
def test_weighted_losses_match_the_statement(dev, num_classes, dice):
    """The five losses and their gradients with class weights spread over [0.25, 4], none of them 1, at NUM_CLASSES = 2, 4, 6 and
    both mask losses, against the float64 statement at LOSS_TOL / GRAD_TOL.  Every foreground class occurs among the positive
    rows (two different ones at least, wherever the model has two: NUM_CLASSES = 2 has one foreground class, and there the
    two weights in play are the background rows' and the positive rows' in the class loss)."""
    d = M.losses_inputs(num_classes, True)
    cw = CW.case_weights(num_classes)
    pos_classes = set(d["tcls"][d["tcls"] > 0].tolist())
    assert len(pos_classes) >= min(2, num_classes - 1) and pos_classes == set(range(1, num_classes))
    counted = d["tcls"].reshape(-1)[d["pred_active"] > 0]             # rows the class loss counts
    assert len(set(cw[counted].tolist())) >= 2 and len(set(cw[sorted(pos_classes)].tolist())) == len(pos_classes)
    ref = CW.weighted_losses_statement(d, dice, cw)
    got = _run_losses(dev, d, dice, cw)
    _report("weighted losses C=%d dice=%s" % (num_classes, dice), got, ref)
    assert np.isfinite(got[0]).all() and all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in got[1].values())
    M.assert_losses_close(got[0], got[1], ref[0], ref[1])
    plain = CW.weighted_losses_statement(d, dice)                      # ... and the weights matter at these tolerances
    with pytest.raises(AssertionError):
        M.assert_losses_close(got[0], got[1], plain[0], plain[1], which=[2, 3, 4], names=("logits", "mbbox", "mmask"))


# ---- 2. weights of one ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
def test_weights_of_one_are_bit_identical_to_no_weights(dev, dice):
    d = M.losses_inputs(4, False)
    plain = _run_losses(dev, d, dice)
    ones = _run_losses(dev, d, dice, np.ones(4, np.float32))
    for i in range(5):
        assert np.array_equal(ones[0][i], plain[0][i]), i
    for n in M.LOSS_GRADS:
        assert np.array_equal(ones[1][n], plain[1][n]), n
    assert all(np.abs(plain[1][n]).max() > 0 for n in M.LOSS_GRADS)


# ---- 3. the RPN side ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
def test_rpn_losses_do_not_see_the_weights(dev, dice):
    d = M.losses_inputs(4, False)
    plain = _run_losses(dev, d, dice)
    got = _run_losses(dev, d, dice, CW.case_weights(4))
    assert np.array_equal(got[0][:2], plain[0][:2]) and (plain[0][:2] > 0).all()
    assert np.array_equal(got[1]["rpn_logits"], plain[1]["rpn_logits"]) and np.array_equal(got[1]["rpn_bbox"], plain[1]["rpn_bbox"])
    assert all(got[0][i] != plain[0][i] for i in (2, 3, 4))
    assert all(not np.array_equal(got[1][n], plain[1][n]) for n in ("logits", "mbbox", "mmask"))


# ---- 4. empty sides ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
@pytest.mark.parametrize("case", M.EMPTY_SIDE_CASES)
def test_weighted_losses_empty_sides(dev, case, dice):
    """model_cases.losses_empty_inputs with weights, against the statement: no positive anchor, no positive ROI, one positive ROI in
    the last row, every row positive, no active class (the class loss and its gradient are NaN on both sides) ..."""
    d = M.losses_empty_inputs(case)
    cw = CW.case_weights(4)
    ref = CW.weighted_losses_statement(d, dice, cw)
    got = _run_losses(dev, d, dice, cw)
    _report("weighted losses, empty side %s dice=%s" % (case, dice), got, ref)
    M.assert_losses_close(got[0], got[1], ref[0], ref[1])
    if case == "g":
        assert np.isnan(got[0][2]) and np.isnan(got[1]["logits"]).all() and np.isfinite(got[0][[0, 1, 3, 4]]).all()
    else:
        assert np.isfinite(got[0]).all() and all(np.isfinite(g).all() for g in got[1].values())
    if case == "d":
        assert got[0][3] == 0 and got[0][4] == 0 and (got[1]["mbbox"] == 0).all() and (got[1]["mmask"] == 0).all() and got[0][2] > 0


# ---- 5. run to run ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dice", [False, True])
def test_weighted_losses_run_to_run(dev, dice):
    d = M.losses_inputs(4, False)
    cw = CW.case_weights(4)
    a, b = _run_losses(dev, d, dice, cw), _run_losses(dev, d, dice, cw)
    assert _same_bits(a, b)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_ops_refuses_wrong_class_weights(dev):
    """A wrong length, a wrong dtype and a host tensor raise ValueError before any launch (the outputs are never allocated: the
    refusal comes first)."""
    d = M.losses_inputs(4, False)
    D = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    args = [D(d[n]) for n in ("rpn_match", "rpn_bbox_t", "rpn_logits", "rpn_bbox", "tcls", "tbbox", "tmask")] + [D(d["active"][0].copy())] + \
           [D(d[n]) for n in ("logits", "mbbox", "mmask")]
    for bad in (torch.ones(3, device=dev), torch.ones(5, device=dev), torch.ones((1, 4), device=dev),
                torch.ones(4, dtype=torch.float64, device=dev), torch.ones(4, dtype=torch.int32, device=dev), torch.ones(4),
                np.ones(4, np.float32)):
        with pytest.raises(ValueError):
            _ops().losses_fwd_bwd(*args, M.LOSS_WEIGHTS, False, class_weights=bad)
    out = _ops().losses_fwd_bwd(*args, M.LOSS_WEIGHTS, False, class_weights=torch.ones(4, device=dev))
    torch.cuda.synchronize()
    assert np.isfinite(out[0].cpu().numpy()).all()


# ---- 7. the engine ---------------------------------------------------------------------------------------------------------------------
def _loss_operands(model, di):
    eng = model.engine
    last = eng.last
    return (di[1], di[2], last["rpn_class_logits"], last["rpn_bbox"], last["target_class_ids"], last["target_bbox"], last["target_mask"],
            di[6], last["mrcnn_class_logits"], last["mrcnn_bbox"], last["mrcnn_mask"], eng.loss_weights(),
            model.config.MASK_LOSS_FUNCTION == "dice_coef_loss")


def test_engine_step_uses_the_class_weights(dev):
    """A training step after model.set_class_weights: the loss call of the step, repeated on the operands the step kept, gives the
    step's five losses bit for bit with the same weights and other head losses without them."""
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = M._small_cfg("custom", 128)
    model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=M._weights(cfg, 11))
    inputs, keys = M._train_inputs(cfg, 2, 5)
    weights = {1: 2.5, 2: 0.4, 3: 3.0}
    model.set_class_weights(weights)
    eng = model.engine
    assert eng.class_weights is not None and eng.class_weights.cpu().tolist() == pytest.approx([1.0, 2.5, 0.4, 3.0])
    losses = model.train_on_batch(inputs, rand_keys=keys, apply=False, keep_outputs=True)
    torch.cuda.synchronize()
    got = losses.cpu().numpy().copy()
    di = model._to_device(inputs, keys)                                # the step's rpn_match, rpn_bbox and active_class_ids again
    tcls = eng.last["target_class_ids"].cpu().numpy()
    assert (tcls > 0).sum() > 0 and len(set(tcls[tcls > 0].tolist())) >= 2, "the scene has no positives of two classes"
    operands = _loss_operands(model, di)
    again = _ops().losses_fwd_bwd(*operands, class_weights=eng.class_weights)[0].cpu().numpy()
    plain = _ops().losses_fwd_bwd(*operands)[0].cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(again, got)
    assert np.array_equal(plain[:2], got[:2]) and all(plain[i] != got[i] for i in (2, 3, 4))
    model.set_class_weights(None)                                      # and back to None
    assert eng.class_weights is None
    off = model.train_on_batch(inputs, rand_keys=keys, apply=False, keep_outputs=True).cpu().numpy()
    assert np.array_equal(off, plain)
    with pytest.raises(ValueError):
        model.set_class_weights([1.0, 2.0])
    with pytest.raises(ValueError):
        eng.set_class_weights(np.ones(5, np.float32))


# ---- 8. the launch tape -------------------------------------------------------------------------------------------------------------------
def test_taped_steps_follow_set_class_weights(dev):
    """Three optimiser steps from identical weights and inputs -- without class weights, with weights A, with weights B -- taped
    (engine.step_taped) against eager, compared as the tape tests compare the two (losses rtol 2e-4 / atol 1e-5, parameters to
    2e-4 of their largest).  The tape is recorded again when weights are switched on (the loss call is another C-ABI entry) and
    not when only their values change (the buffer is refreshed in place); a third eager run that keeps A in the last step shows
    that the comparison tells A from B."""
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = M._small_cfg("custom", 128)
    w = M._weights(cfg, 17)
    batches = [M._train_inputs(cfg, 2, 9), M._train_inputs(cfg, 2, 13), M._train_inputs(cfg, 2, 9)]
    A, B_ = {1: 3.0, 2: 0.5, 3: 2.0}, {1: 0.3, 2: 4.0, 3: 0.6}
    out = {}
    for run, plan in (("eager", (None, A, B_)), ("taped", (None, A, B_)), ("eager_AA", (None, A, A))):
        model = MaskRCNN("training", cfg, "/tmp/mrcnn_logs", device=dev, weights=w)
        eng = model.engine
        model.compile(0.01, 0.9)
        losses, tapes, ptr = [], [], None
        for s, weights in enumerate(plan):
            model.set_class_weights(weights)
            if weights is not None:
                assert ptr in (None, eng.class_weights.data_ptr())           # same buffer, new contents
                ptr = eng.class_weights.data_ptr()
            di = model._to_device(*batches[s])
            if run == "taped":
                ls = eng.step_taped(di, 0.01, 0.9)
            else:
                ls = eng.forward_backward(*di)
                eng.apply_gradients(0.01, 0.9, 1)
            losses.append(ls.cpu().numpy().copy())
            tapes.append(len(eng._train_tapes))
        torch.cuda.synchronize()
        out[run] = (np.stack(losses), eng.params.cpu().numpy().copy())
        if run == "taped":
            assert tapes == [1, 2, 2], tapes
            model.set_class_weights(None)                                  # and back: the first recording serves again
            eng.step_taped(model._to_device(*batches[0]), 0.01, 0.9)
            torch.cuda.synchronize()
            assert len(eng._train_tapes) == 2
    ref, got, other = out["eager"], out["taped"], out["eager_AA"]
    print("[tape] losses of step 3: eager %s taped %s eager with A kept %s" % (ref[0][2].tolist(), got[0][2].tolist(), other[0][2].tolist()))
    assert np.isfinite(ref[0]).all() and np.isfinite(got[0]).all()
    np.testing.assert_allclose(got[0], ref[0], rtol=2e-4, atol=1e-5)
    assert np.abs(got[1] - ref[1]).max() <= 2e-4 * np.abs(ref[1]).max()
    rel = np.abs(other[0][2, 2:] - ref[0][2, 2:]) / np.abs(ref[0][2, 2:])
    assert (rel > 2e-3).all(), rel                                       # A for B in step 3 is ten tolerances away in every head loss


# ---- 9. MaskRCNN.train ------------------------------------------------------------------------------------------------------------------
def test_maskrcnn_train_takes_class_weights(dev, tmp_path, capsys):
    from caesar_mrcnn_amd.model import MaskRCNN
    cfg = M._small_cfg("custom", 128)
    cfg.IMAGES_PER_GPU, cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 2, 2, 1
    ds = CW.ToyDataset(4, 128)
    model = MaskRCNN("training", cfg, str(tmp_path / "logs"), device=dev, seed=0)
    assert model.engine.class_weights is None
    model.train(ds, ds, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all", n_worker_threads=1, class_weights={1: 2.0, 2: 0.5})
    assert model.engine.class_weights.cpu().tolist() == [1.0, 2.0, 0.5, 1.0]
    assert len(model.history["loss"]) == 1 and np.isfinite(model.history["loss"][0]) and np.isfinite(model.history["val_loss"][0])
    assert "Class weights of the head losses: [1, 2, 0.5, 1]" in capsys.readouterr().out
    # Config.CLASS_WEIGHTS is the fall-back of train(class_weights=None)
    cfg.CLASS_WEIGHTS = [1.0, 0.5, 3.0, 1.5]
    model.epoch = 0
    model.train(ds, ds, learning_rate=cfg.LEARNING_RATE, epochs=1, layers="all", n_worker_threads=1)
    assert model.engine.class_weights.cpu().tolist() == [1.0, 0.5, 3.0, 1.5] and np.isfinite(model.history["loss"][0])
