"""CPU tests of hdn_amd.ops as the home of the BatchNorm fold and of the launch wrappers: the fold of both homography trunks and of the similarity
backbone's conv / BN pairs against the formula restated here, exactly, and hdn_amd.trunk's re-exports.  No kernel is launched here."""
import torch
import torch.nn as nn


def _seed_bn_(net, seed):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            n = m.num_features
            m.weight.data = torch.rand(n, generator=g) * 1.5 + 0.25
            m.bias.data = torch.randn(n, generator=g) * 0.3
            m.running_mean = torch.randn(n, generator=g) * 0.5
            m.running_var = torch.rand(n, generator=g) * 2.0 + 0.1
    return net.eval()


def _expected(conv, bn):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return (conv.weight.double() * s.view(-1, 1, 1, 1)).float(), (bn.bias.double() - bn.running_mean.double() * s).float()


def _pairs(net):
    """(name, conv, bn) of every conv / BN pair of a homography trunk, in the order of the folded convolutions of _folded()."""
    yield "conv1", net.conv1, net.bn1
    for ln in ("layer1", "layer2", "layer3", "layer4"):
        for i, blk in enumerate(getattr(net, ln)):
            for k in (1, 2, 3):
                if hasattr(blk, f"conv{k}"):
                    yield f"{ln}.{i}.conv{k}", getattr(blk, f"conv{k}"), getattr(blk, f"bn{k}")
            if blk.downsample is not None:
                yield f"{ln}.{i}.downsample", blk.downsample[0], blk.downsample[1]


def _folded(net):
    yield net.conv1
    for ln in ("layer1", "layer2", "layer3", "layer4"):
        for blk in getattr(net, ln):
            for k in (1, 2, 3):
                if hasattr(blk, f"conv{k}"):
                    yield getattr(blk, f"conv{k}")
            if blk.downsample is not None:
                yield blk.downsample


def test_fold_for_inference_is_the_float64_fold_rounded_once():
    from hdn_amd.trunk import fold_for_inference, resnet34_homo, resnet50_homo
    for seed, net in ((1, resnet34_homo()), (2, resnet50_homo(layers=(1, 1, 1, 1)))):
        net = _seed_bn_(net, seed)
        pairs, convs = list(_pairs(net)), list(_folded(fold_for_inference(net, channels_last=False)))
        assert len(pairs) == len(convs) == (36 if seed == 1 else 17)
        for (name, conv, bn), got in zip(pairs, convs):
            w, b = _expected(conv, bn)
            assert isinstance(got, nn.Conv2d) and (got.stride, got.padding) == (conv.stride, conv.padding), name
            assert torch.equal(got.weight, w), name
            assert torch.equal(got.bias, b), name


def test_fold_conv_bn_is_the_same_fold():
    from hdn_amd import backbone
    net = _seed_bn_(nn.Sequential(nn.Conv2d(32, 64, 3, 1, 2, 2, bias=False), nn.BatchNorm2d(64)), 3)
    w, b = _expected(net[0], net[1])
    got_w, got_b = backbone.fold_conv_bn(net[0], net[1])
    assert torch.equal(got_w, w) and torch.equal(got_b, b)


def test_trunk_re_exports_the_wrappers_of_ops():
    from hdn_amd import backbone, ops, trunk
    moved = ("_c_pack", "_host_f32", "pack_stem_mfma", "pack_conv3x3", "pack_conv3x3_v2", "pack_conv3x3s2_ds", "pack_conv3x3s2_ds_v2", "pack_conv1x1",
             "pack_conv3x3s2", "pack_conv3x3d", "pack_simi_stem", "bias_relu_", "conv3x3_bias_relu", "conv3x3s2_ds", "LazyAct", "chain_conv", "conv1x1",
             "conv3x3s2", "conv3x3d", "conv3x3v", "simi_stem", "ACT_SCALE_LOG2", "SPLIT_PIECES", "V2_MIN_BATCH", "MATRIX_CORE_CHANNELS", "_MC_SIDE",
             "S2_CHANNELS", "SIMI_STEM_MAX_SIDE")
    for name in moved:
        assert getattr(trunk, name) is getattr(ops, name), name
    assert backbone.fold_conv_bn is ops.fold_conv_bn


def test_packers_copy_weights_that_are_not_host_float32_contiguous():
    """A weight the packer has to convert (another dtype or layout: as a device tensor is) gives the stream of its float32 contiguous form."""
    from hdn_amd import ops
    g = torch.Generator().manual_seed(4)
    w, wd = torch.randn(128, 64, 3, 3, generator=g) * 0.05, torch.randn(128, 64, 1, 1, generator=g) * 0.05
    odd = lambda t: t.double().contiguous(memory_format=torch.channels_last)
    assert torch.equal(ops.pack_conv3x3d(odd(w)), ops.pack_conv3x3d(w))
    assert torch.equal(ops.pack_conv3x3s2_ds(odd(w), odd(wd)), ops.pack_conv3x3s2_ds(w, wd))
