"""Generates tests/golden/trunk_resnet50.npz from the reference's ResNet-50 homography trunk.

    python tests/golden/make_golden_trunk50.py [--reference DIR] [--out DIR]

The reference's resnet50(used_layers=[4]) (homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:97-133, 223-231: Bottleneck x
[3, 4, 6, 3], conv1 = Conv2d(2, 64, 7, 2, 3)) is filled with make_golden.seeded_trunk_state_ (tag 620, the ResNet-34 fixture's draw) and run on the
same seeded [2, 2, 127, 127] input (rng(621)).  Written like make_golden.gen_trunk writes trunk_resnet34.npz: the state_dict keys / shapes, the input,
the [2, 2048, 4, 4] output and the float64 sum of the parameters; the weights themselves are not stored.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def gen_trunk50(ref_resnet):
    m = mg.seeded_trunk_state_(ref_resnet.resnet50(used_layers=[4]).eval())
    x = mg.rng(621).standard_normal((2, 2, 127, 127)).astype(np.float32)
    with torch.no_grad():
        out = m(mg.t(x))
    sd = m.state_dict()
    mg.save("trunk_resnet50", keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]), x=x,
            out=out.numpy(), param_sum=np.float64(sum(float(v.double().sum()) for v in sd.values() if v.dtype == torch.float32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out:
        mg.OUT_DIR = os.path.abspath(args.out)
        os.makedirs(mg.OUT_DIR, exist_ok=True)
    if not os.path.isdir(args.reference):
        sys.exit(f"reference tree not found at {args.reference}")
    mg.install_stubs()
    sys.path.insert(0, args.reference)
    torch.set_num_threads(1)
    import homo_estimator.Deep_homography.Oneline_DLTv1.backbone.resnet as ref_resnet

    gen_trunk50(ref_resnet)


if __name__ == "__main__":
    main()
