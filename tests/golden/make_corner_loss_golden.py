"""Capture tests/golden/corner_losses.npz: the outputs of the reference's DLT_solve (homo_estimator/Deep_homography/Oneline_DLTv1/utils.py, the one
model_builder_e2e_unconstrained_v2 imports) and kalyo_l1_loss (hdn/models/loss.py), executed on the CPU in float64 on the inputs that
tests/corner_loss_cases.py regenerates by seed (the cases of at most GOLDEN_MAX_B samples).  Outputs only.  Nothing of the reference's text is copied:
its modules are imported and called.

    python tests/golden/make_corner_loss_golden.py [--reference DIR]

Per case: H_gt [B,3,3] = DLT_solve(template_poly, pred_points_xy / pred_points_w - template_poly) for EVERY sample, as :502 calls it before its
gather; pos_loss = kalyo_l1_loss(x[sup_pos], delta) with delta the corners of the 127-square under the reference's own H_gt (:504-514 are statements
of the forward, formed here with numpy); neg_loss = kalyo_l1_loss(x[neg], 0) (:519-523).  An empty set stores 0.  The import recipe is
make_golden.install_stubs().
"""
import argparse
import os
import sys

import numpy as np
import torch

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
    from homo_estimator.Deep_homography.Oneline_DLTv1.utils import DLT_solve
    from hdn.models.loss import kalyo_l1_loss
    import corner_loss_cases as CC

    out = {}
    corners = np.concatenate([CC.SQUARE.T, np.ones((1, 4))])
    for name, c in CC.CASES.items():
        if c.B > CC.GOLDEN_MAX_B:
            continue
        pp, tp, x = (torch.from_numpy(a).double() for a in (c.pred_points, c.template_poly, c.x))
        homo = (pp.permute(0, 2, 1) / pp.permute(0, 2, 1)[:, :, 2].unsqueeze(2))[:, :, :-1]
        H = DLT_solve(tp.reshape(-1, 8), (homo - tp).reshape(-1, 8)).squeeze(1)
        out[f"{name}/H_gt"] = H.numpy()
        sp, ng = c.ids["sup_pos"], c.ids["neg"]
        pos = neg = 0.0
        if len(sp):
            Q = np.einsum("nrk,kj->nrj", H.numpy()[sp], corners)
            delta = ((Q[:, :2] / Q[:, 2:3]).transpose(0, 2, 1) - CC.SQUARE[None]).reshape(-1, 8)
            pos = float(kalyo_l1_loss(x[sp], torch.from_numpy(delta)))
        if len(ng):
            neg = float(kalyo_l1_loss(x[ng], torch.zeros(len(ng), 8, dtype=torch.float64)))
        out[f"{name}/pos_loss"], out[f"{name}/neg_loss"] = np.float64(pos), np.float64(neg)
    np.savez_compressed(CC.GOLDEN, **out)
    print("wrote", CC.GOLDEN, os.path.getsize(CC.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
