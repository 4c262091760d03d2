"""Shared by tests/test_class_weights_cpu.py and tests/test_class_weights_gpu.py: the float64 statement of the five losses with
class weights on the three head losses, written from the definition, with its gradients from autograd; the
fixed weight vectors of the cases; a four-image in-memory dataset.  Pure NumPy + torch-CPU, like tests/model_cases.py."""
import numpy as np
import torch

import model_cases as M

# Keras evaluates K.binary_crossentropy in float32: its clip bounds are the float32 numbers next to 1e-7 and 1 - 1e-7 (the
# latter is 1 - 2^-23), and so are the kernel's.  The statement clips at exactly these two numbers and is float64 otherwise.
BCE_LO = float(np.float32(1e-7))
BCE_HI = float(np.float32(1.0) - np.float32(1e-7))
DICE_SMOOTH = 1e-7


def case_weights(C):
    """C fixed class weights spread over [0.25, 4] (geometric steps, background first), none equal to 1."""
    cw = np.geomspace(0.25, 4.0, C).astype(np.float32)
    assert cw.min() == 0.25 and cw.max() == 4.0 and not np.any(cw == 1.0) and len(set(cw.tolist())) == C
    return cw


def _smooth_l1(t, p):
    diff = torch.abs(t - p)
    return torch.where(diff < 1.0, 0.5 * diff * diff, diff - 0.5)


def weighted_losses_statement(d, dice, cw=None, weights=M.LOSS_WEIGHTS):
    """The five losses of the operands d (model_cases.losses_inputs) in float64 -> (losses[5], {name: gradient of
    sum_i weights[i] * loss_i}) as NumPy.  cw: [C] class weights, None = all one.  Every ROI row r carries u_r = cw[tcls_r]:
        mrcnn_class = sum_r(u_r ce_r pa_r) / sum_r(pa_r)
        mrcnn_bbox  = sum_{r positive}(u_r smooth_l1_r) / (4 npos)
        mrcnn_mask  = sum_{r positive}(u_r sum_pix bce) / (npos npix)                        (binary cross-entropy)
                      1 - (2 sum(u_r y q) + s) / (sum(u_r y) + sum(u_r q) + s), s = 1e-7      (Dice)
    and the two RPN losses carry no weights.  An empty side gives a loss of 0 with zero gradients; no active class gives 0 / 0."""
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    t = {n: f64(d[n]).requires_grad_(True) for n in M.LOSS_GRADS}
    zero = torch.zeros((), dtype=torch.float64)
    B = d["rpn_logits"].shape[0]
    C = d["logits"].shape[-1]
    # ---- RPN: class-agnostic ----
    rm = torch.tensor(d["rpn_match"]).reshape(B, -1)
    sel = rm != 0
    l1 = zero
    if sel.any():
        lg = t["rpn_logits"][sel]
        tgt = (rm[sel] == 1).long()
        l1 = (torch.logsumexp(lg, 1) - lg.gather(1, tgt[:, None])[:, 0]).mean()
    pos = rm == 1
    l2 = zero
    if pos.any():
        tgt = torch.cat([f64(d["rpn_bbox_t"][b])[:int(pos[b].sum())] for b in range(B)], 0)
        l2 = _smooth_l1(tgt, t["rpn_bbox"][pos]).mean()
    # ---- heads ----
    tc = torch.tensor(d["tcls"]).reshape(-1).long()
    u = torch.ones(tc.shape[0], dtype=torch.float64) if cw is None else f64(cw)[tc]
    lg = t["logits"].reshape(-1, C)
    pa = f64(d["active"][0])[lg.argmax(1)]
    ce = torch.logsumexp(lg, 1) - lg.gather(1, tc[:, None])[:, 0]
    l3 = (u * ce * pa).sum() / pa.sum()
    prow = torch.nonzero(tc > 0)[:, 0]
    l4 = l5 = zero
    if prow.numel():
        npos = float(prow.numel())
        up = u[prow]
        pb = t["mbbox"].reshape(-1, C, 4)[prow, tc[prow]]
        l4 = (up[:, None] * _smooth_l1(f64(d["tbbox"]).reshape(-1, 4)[prow], pb)).sum() / (4.0 * npos)
        mh, mw = d["tmask"].shape[-2:]
        y = f64(d["tmask"]).reshape(-1, mh, mw)[prow]
        q = t["mmask"].reshape(-1, mh, mw, C)[prow, :, :, tc[prow]]
        uu = up[:, None, None]
        if dice:
            l5 = 1.0 - (2.0 * (uu * y * q).sum() + DICE_SMOOTH) / ((uu * y).sum() + (uu * q).sum() + DICE_SMOOTH)
        else:
            qc = torch.clamp(q, BCE_LO, BCE_HI)
            x = torch.log(qc / (1.0 - qc))
            bce = torch.relu(x) - x * y + torch.log1p(torch.exp(-torch.abs(x)))       # relu'(0) = 0 and sign(0) = 0, as in TF
            l5 = (uu * bce).sum() / (npos * mh * mw)
    ls = [l1, l2, l3, l4, l5]
    total = sum(w * l for w, l in zip(weights, ls))
    if total.requires_grad:
        total.backward()
    grads = {n: (np.zeros(d[n].shape, np.float64) if t[n].grad is None else t[n].grad.numpy()) for n in M.LOSS_GRADS}
    return np.array([float(l.detach()) for l in ls]), grads


def loss_cfg(dice, num_classes=4):
    from caesar_mrcnn_amd.config import run_py_config
    cfg = run_py_config(num_classes=num_classes)
    cfg.MASK_LOSS_FUNCTION = "dice_coef_loss" if dice else "binary_crossentropy"
    return cfg


class ToyDataset(object):
    """Duck-typed like mrcnn.utils.Dataset as the generator uses it: n in-memory 128 x 128 images with 2..4 bright boxes of the
    classes 1..3."""

    def __init__(self, n=4, size=128):
        self.image_ids = np.arange(n)
        self.image_info = [{"source": "toy", "id": i} for i in range(n)]
        self.num_classes = 4
        self.source_class_ids = {"toy": [0, 1, 2, 3]}
        self.size = size

    def _make(self, i):
        r = np.random.RandomState(700 + i)
        img = r.randint(0, 40, (self.size, self.size, 3)).astype(np.uint8)
        k = r.randint(2, 5)
        mask = np.zeros((self.size, self.size, k), bool)
        for g in range(k):
            y, x = r.randint(5, self.size - 40, 2)
            h, w = r.randint(8, 30, 2)
            mask[y:y + h, x:x + w, g] = True
            img[y:y + h, x:x + w] = 200
        return img, mask, (1 + (np.arange(k) + i) % 3).astype(np.int32)

    def load_image(self, i):
        return self._make(i)[0]

    def load_mask(self, i):
        return self._make(i)[1], self._make(i)[2]
