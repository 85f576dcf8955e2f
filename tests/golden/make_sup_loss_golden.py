"""Capture tests/golden/sup_losses.npz: the outputs of the reference's hdn/models/loss.py, executed in float64 on the CPU, on the inputs that
tests/sup_loss_cases.py regenerates by seed.  Outputs only: the five losses of every view of every case, and the gradients (autograd, upstream
UPSTREAM) of the cases with at most GOLDEN_GRAD_CELLS cells.  Nothing of the reference's text is copied: its module is imported and called.

    python tests/golden/make_sup_loss_golden.py [--reference DIR]

The import recipe (stub modules, .cuda() made the identity) is make_golden.install_stubs().  Form 0 is fed as the training forward feeds it:
x[sup_ids], F.softmax / F.log_softmax over the permuted maps, then the functions.  Where the reference raises (fewer negatives than k in its topk) the
entry is recorded as raised: the kernel's k_eff is a documented difference.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HDN_REFERENCE", "/root/reference"))
    args = ap.parse_args()
    import make_golden

    make_golden.install_stubs()
    sys.path.insert(0, args.reference)
    import hdn.models.loss as RL
    import sup_loss_cases as SC

    out = {}
    for name, view in SC.VIEWS.items():
        if not view.case.golden:
            continue
        t, sel = view.t, view.selected()
        leaves = {k: t[k].double().requires_grad_(True) for k in ("cls", "loc", "cls_lp", "loc_lp", "rows")}
        if view.form == 0:
            if len(sel) == 0:
                continue                                               # the reference computes nothing there
            g = lambda k: leaves[k][sel]
            lab = lambda k: t[k][sel]
            p, logp = F.softmax(g("cls").permute(0, 2, 3, 1).contiguous(), dim=3), F.log_softmax(g("cls_lp").permute(0, 2, 3, 1).contiguous(), dim=3)
        else:
            g = lambda k: leaves[k]
            lab = lambda k: t[k]
            p, logp = g("cls"), g("cls_lp")
        calls = (lambda: RL.select_xr_focal_fuse_smooth_l1_loss_top_k(p, lab("label_cls").double()),
                 lambda: RL.select_l1_loss_c(g("loc"), lab("label_loc_c").double(), lab("label_cls").double()),
                 lambda: RL.select_cross_entropy_loss(logp, lab("label_cls_lp")),
                 lambda: RL.select_l1_loss(g("loc_lp"), lab("label_loc_lp").double(), lab("label_cls_lp")),
                 lambda: RL.kalyo_l1_loss(leaves["rows"], t["rows_target"].double()))
        losses, raised, total = np.zeros(5), np.zeros(5, dtype=bool), 0
        for i, call in enumerate(calls):
            if i == 0 and view.topk != 100:
                raised[i] = True                                       # the reference's k is 100 n: other values exist in the ABI only
                continue
            try:
                v = call()
            except (RuntimeError, IndexError):
                raised[i] = True
                continue
            v = torch.as_tensor(v, dtype=torch.float64)
            losses[i] = float(v)
            if v.requires_grad:
                total = total + SC.UPSTREAM[i] * v
        out[name + "/losses"], out[name + "/raised"] = losses, raised
        if view.case.cells <= SC.GOLDEN_GRAD_CELLS and torch.is_tensor(total) and total.requires_grad:
            total.backward()
            for k, v in leaves.items():
                if SC.KEYS.index([q for q, w in SC.GRAD_OF.items() if w == k][0]) == 0 and raised[0]:
                    continue
                out[name + "/grad_" + k] = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()
    np.savez_compressed(SC.GOLDEN, **out)
    print("wrote", SC.GOLDEN, os.path.getsize(SC.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
