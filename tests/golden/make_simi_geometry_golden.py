"""Capture tests/golden/simi_geometry.npz: the outputs of the reference's Polar_Pick.get_polar_from_two_para_loc (hdn/models/logpolar.py), lp_pick
(hdn/utils/point.py) and combine_affine_c0_v2 / combine_affine_lt0 (hdn/utils/transform.py), executed on the CPU in fp32 and in float64 on the inputs
that tests/simi_geometry_cases.py regenerates by seed.  Outputs only, plus autograd gradients for the cases of at most GOLDEN_GRAD_CELLS cells.
Nothing of the reference's text is copied: its modules are imported and called.

    python tests/golden/make_simi_geometry_golden.py [--reference DIR]

The import recipe (stub modules, .cuda() made the identity) is make_golden.install_stubs().  The class maps stay fp32 in both runs (they only choose
the cell).  Two things the reference does to a float64 run are kept as they are: Polar_Pick writes into a fp32 buffer, so polar exists in fp32 only,
and both combine_affine functions end in .float(), so the float64 matrices arrive rounded to fp32.  The matrices are built, as in :401-404, from the
reference's own polar, scale and rot; the gradient scalar is sum(w scale) + sum(w rot) + sum(w affine_m) + sum(w affine_m_lt0) with the weights of the
case, taken to loc_lp and to polar (a float64 leaf holding the fp32 polar), and sum(w polar) taken to loc.
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
    import hdn.models.logpolar as RL
    import hdn.utils.point as RP
    import hdn.utils.transform as RT
    from hdn.core.config import cfg
    import simi_geometry_cases as SC

    cfg.BAN.KWARGS["cls_out_channels"] = 2
    cfg.POINT.STRIDE = SC.STRIDE
    half = SC.OUT_SZ / 2
    out = {}
    for name, c in SC.CASES.items():
        if not c.golden:
            continue
        cfg.TRAIN.OUTPUT_SIZE = c.S
        picker = RL.Polar_Pick()
        cls, cls_lp = torch.from_numpy(c.cls), torch.from_numpy(c.cls_lp)
        w = {k: torch.from_numpy(v).double() for k, v in c.w.items()}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            loc, loc_lp = (torch.from_numpy(a).to(dt).requires_grad_(True) for a in (c.loc, c.loc_lp))
            polar = picker.get_polar_from_two_para_loc(cls, loc * cfg.POINT.STRIDE)
            scale, rot = RP.lp_pick(cls_lp, loc_lp, 2, SC.STRIDE, SC.STRIDE_LP, c.S, SC.MAP_SIZE)
            pol = polar.detach().to(dt).requires_grad_(True)
            tcx, tcy = torch.from_numpy(c.temp_cx).to(dt), torch.from_numpy(c.temp_cy).to(dt)
            one, zero, zero2 = torch.ones(c.B, dtype=dt), torch.zeros(c.B, dtype=dt), torch.zeros(c.B, 2, dtype=dt)
            mats = (RT.combine_affine_c0_v2(half, half, pol, scale, rot, True, SC.IN_SZ, SC.OUT_SZ),
                    RT.combine_affine_lt0(half, half, pol, 1 / scale, -rot, SC.IN_SZ, SC.OUT_SZ),
                    RT.combine_affine_c0_v2(tcx, tcy, zero2, one, zero, True, SC.IN_SZ, SC.OUT_SZ),
                    RT.combine_affine_lt0(tcx, tcy, zero2, one, zero, SC.IN_SZ, SC.OUT_SZ))
            if tag == "f32":
                out[f"{name}/f32/polar"] = polar.detach().numpy()
                for mode, x in (("", cls), ("_lp", cls_lp)):                       # the indices the reference's own argmax lines give
                    score = x.view(c.B, 2, -1).permute(0, 2, 1)
                    out[f"{name}/best_idx{mode}"] = torch.argmax(score[:, :, 1] if mode == "" else score.softmax(2)[:, :, 1], 1).numpy()
            out[f"{name}/{tag}/scale"], out[f"{name}/{tag}/rot"] = scale.detach().numpy(), rot.detach().numpy()
            for k, m in zip(SC.MATS, mats):
                out[f"{name}/{tag}/{k}"] = m.detach().numpy()
            if tag == "f64" and c.B * c.n <= SC.GOLDEN_GRAD_CELLS:
                total = (w["scale"] * scale).sum() + (w["rot"] * rot).sum() + (w["affine_m"] * mats[0]).sum() + (w["affine_m_lt0"] * mats[1]).sum()
                g_lp, g_pol = torch.autograd.grad(total, (loc_lp, pol))
                g_loc, = torch.autograd.grad((w["polar"] * polar).sum(), loc)
                out[f"{name}/grad_loc_lp"], out[f"{name}/grad_polar"], out[f"{name}/pick_grad_loc"] = g_lp.numpy(), g_pol.numpy(), g_loc.numpy()
    np.savez_compressed(SC.GOLDEN, **out)
    print("wrote", SC.GOLDEN, os.path.getsize(SC.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
