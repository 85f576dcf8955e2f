"""Shared by tests/test_gpu_share_feature_train.py and tests/test_share_feature_train_host.py: the float64 truth, the fp32 CPU reference, the fixtures and
the device runners of PreShareFeature's training path (hdn_share_feature_train_fwd_f32 / hdn_share_feature_bwd_f32, hdn_amd.PreShareFeatureTrain).
Nothing here launches a kernel except the run_* functions.

Truth: restatement() - the chain in float64 with BatchNorm's forward and backward written out (mean, biased variance, invstd, x^, dz = g [z > 0],
S1 = sum dz, S2 = sum dz x^, dc = gamma invstd (dz - S1 / N - x^ S2 / N), the convolution's two adjoints, running = (1 - m) running + m stat with the
unbiased variance).  The host test pins it to float64 autograd through the stock nn.Sequential at 1e-12 relative.  With frozen statistics (eval mode)
the truth is that float64 autograd itself.

Reference: the stock fp32 nn.Sequential on the CPU on the same fixture; e_ref = its max error against the truth, per tensor.
Bound, per tensor: |got - truth| <= 4 e_ref + 1e-5 max|truth|.

ReLU margin: a ReLU's derivative jumps at zero, and one mask that differs between float64 and fp32 moves grad_gamma and the weight gradients by a whole
term.  Every bound fixture keeps each float64 pre-activation z away from zero: min|z| >= max(16 e_z, 2e-6 max|z|) per layer, e_z = the fp32 CPU
reference's own error on that layer's z (16: the geometry tests' "20 or more ulps" reasoning; a kernel as accurate as the reference on z then reads
the same masks).  Fixtures are seeded draws (image and grad_out standard normal, Kaiming weights, gamma in [0.5, 1.5], bias in [-0.5, 0.5]) from the
first seed offset >= 0 from SEED that satisfies the rule; the offsets are committed below and the host test re-derives them.  Beyond ~110k
pre-activations per layer the rule stops being satisfiable, so no BOUND fixture is larger than one 127 x 127 image; the exact fixtures of
tests/share_feature_train_exact_cases.py need no margin and go beyond it.

eps and momentum are one number for all three BatchNorms or one per layer (a 3-tuple); EPS3 / MOMENTA3 are the cases with three different ones.

Cases: the shapes of the issue, (1,2,3), and both sides of every boundary of the launch rule of csrc/share_feature_train.hip - a workgroup owns 1024
consecutive pixels of one image, a thread the pixels t, t + 256, ... of them (H W = 256 | 257 and 1024 | 1025), the weight finish adds 64 partials per
step (workgroups 64 | 65) and the statistics finish 256 (workgroups 256 | 257).  There is one launch form, hence no form query."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20261019
MAX_OFFSET = 64
LAYERS = ((0, 4), (4, 12), (12, 13))           # channel ranges of the three BatchNorms in gamma[13] / bias[13]
PX_PER_WORKGROUP = 1024
# (B, H, W) -> first seed offset that satisfies the margin rule in train mode (batch statistics)
TRAIN_CASES = {
    (2, 5, 7): 0, (3, 9, 11): 0, (5, 13, 33): 0, (2, 17, 130): 0, (3, 33, 65): 3, (1, 127, 127): 60, (1, 2, 3): 0,
    (1, 16, 16): 0, (1, 1, 257): 0, (1, 32, 32): 0, (1, 25, 41): 1, (64, 2, 3): 0, (65, 2, 3): 0, (256, 1, 2): 0, (257, 1, 2): 0,
}
# the same for frozen statistics (eval mode, random running mean / var) and for the three-call step
FROZEN_CASES = {(3, 9, 11): 0, (2, 17, 130): 0}
EPS3 = (1e-5, 1e-3, 1e-1)                      # three different eps: a permutation of them between the layers moves every tensor far beyond the bound
EPS3_CASES = {("train", (3, 9, 11)): 0, ("frozen", (3, 9, 11)): 0}             # (mode, shape) -> first seed offset under EPS3
MOMENTA3 = (0.1, None, 0.5)                    # not all equal: the per-layer loop of PreShareFeature._update_running
STEP_CASE = ((3, 9, 11), 0)
HINGE_MARGIN = 1e-4                            # the step's triplet hinge argument stays this far from zero (its fp32 error is ~1e-6)
OFFSETS = [(0, 0, 0, 0, 0), (1, 2, 3, 1, 2)]   # float offsets of out / grad_img, saved / grad_params, stats, img, grad_out in a 16-byte line
BYTE = 0xA5
FILL = float(np.frombuffer(bytes([BYTE] * 4), dtype=np.float32)[0])
PAD = 8
TENSORS = ("y", "rm1", "rm2", "rm3", "rv1", "rv2", "rv3", "gx", "gw1", "gw2", "gw3", "gg1", "gg2", "gg3", "gb1", "gb2", "gb3")


def workgroups(B, H, W):
    return B * ((H * W + PX_PER_WORKGROUP - 1) // PX_PER_WORKGROUP)


# ================================================================================================================= fixtures
def draw(B, H, W, seed):
    """The seeded draw: fp32 CPU tensors x, g [B,1,H,W], w1 [4,1,3,3], w2 [8,4,3,3], w3 [1,8,3,3], gamma[13], bias[13], running mean / var [13]
    (used by the frozen cases only), x2, x3 (the step's other two inputs)."""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    fix = {"x": f(rng.standard_normal((B, 1, H, W))), "g": f(rng.standard_normal((B, 1, H, W)))}
    for name, (co, ci) in (("w1", (4, 1)), ("w2", (8, 4)), ("w3", (1, 8))):
        fix[name] = f(rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (ci * 9)))     # nn.init.kaiming_normal_ (fan_in, relu gain)
    fix["gamma"] = f(rng.uniform(0.5, 1.5, 13))
    fix["bias"] = f(rng.uniform(-0.5, 0.5, 13))
    fix["rmean"] = f(rng.uniform(-0.5, 0.5, 13))
    fix["rvar"] = f(rng.uniform(0.5, 2.0, 13))
    fix["x2"] = f(rng.standard_normal((B, 1, H, W)))
    fix["x3"] = f(rng.standard_normal((B, 1, H, W)))
    return fix


def per_layer(v):
    """One value for all three BatchNorms, or one per layer."""
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def load_params(module, fix, running=None, momentum=0.1, eps=1e-5):
    """Copy the fixture's parameters (and, running = (mean, var), the buffers) into a PreShareFeature-like module; -> module."""
    seq = module.ShareFeature
    momentum, eps = per_layer(momentum), per_layer(eps)
    with torch.no_grad():
        for l, (c, b) in enumerate(((0, 1), (3, 4), (6, 7))):
            lo, hi = LAYERS[l]
            seq[c].weight.copy_(fix["w%d" % (l + 1)])
            seq[b].weight.copy_(fix["gamma"][lo:hi])
            seq[b].bias.copy_(fix["bias"][lo:hi])
            seq[b].momentum, seq[b].eps = momentum[l], eps[l]
            if running is not None:
                seq[b].running_mean.copy_(running[0][lo:hi])
                seq[b].running_var.copy_(running[1][lo:hi])
    return module


def collect(module, y, x, zs=None):
    """The result dict of a module after backward: y, buffers, gradients (those that exist), num_batches_tracked, and the pre-activations."""
    seq = module.ShareFeature
    out = {"y": y.detach().cpu()}
    if x.grad is not None:
        out["gx"] = x.grad.detach().cpu()
    for l, (c, b) in enumerate(((0, 1), (3, 4), (6, 7)), start=1):
        out["rm%d" % l], out["rv%d" % l] = seq[b].running_mean.detach().cpu().clone(), seq[b].running_var.detach().cpu().clone()
        out["nbt%d" % l] = int(seq[b].num_batches_tracked)
        for name, p in (("gw", seq[c].weight), ("gg", seq[b].weight), ("gb", seq[b].bias)):
            if p.grad is not None:
                out["%s%d" % (name, l)] = p.grad.detach().cpu()
    if zs is not None:
        out["z"] = zs
    return out


def stock(fix, dtype, train=True, running=None, momentum=0.1, calls=1, eps=1e-5):
    """The stock nn.Sequential on the CPU in `dtype`: `calls` forwards on fix['x'] (the last one with backward of fix['g']).  -> collect()'s dict with
    'z' = the three layers' pre-activations (BatchNorm outputs) and 'c' = the three convolutions' outputs of the last call."""
    from hdn_amd.share_feature import PreShareFeature
    m = load_params(PreShareFeature().to(dtype), fix, running, momentum, eps).train(train)
    zs, cs = [], []
    hooks = [m.ShareFeature[b].register_forward_hook(lambda mod, i, o: zs.append(o.detach().clone())) for b in (1, 4, 7)]
    hooks += [m.ShareFeature[c].register_forward_hook(lambda mod, i, o: cs.append(o.detach().clone())) for c in (0, 3, 6)]
    x = fix["x"].detach().clone().to(dtype).requires_grad_(True)
    for _ in range(calls):
        del zs[:], cs[:]
        y = m.ShareFeature(x)
    y.backward(fix["g"].to(dtype))
    for h in hooks:
        h.remove()
    out = collect(m, y, x, list(zs))
    out["c"] = list(cs)
    return out


def restatement(fix, momentum=0.1, calls=1, eps=1e-5):
    """The float64 truth with batch statistics, BatchNorm's forward and backward written out.  Buffers start at PyTorch's (0, 1) and are updated `calls`
    times with the same batch.  -> the dict of stock()."""
    momentum, eps = per_layer(momentum), per_layer(eps)
    d = lambda t: t.double()
    x, g = d(fix["x"]), d(fix["g"])
    ws = [d(fix["w1"]), d(fix["w2"]), d(fix["w3"])]
    N = x.shape[0] * x.shape[2] * x.shape[3]
    a, acts, keep, out = x, [], [], {}
    for l, (lo, hi) in enumerate(LAYERS):
        gamma, bias = d(fix["gamma"][lo:hi]).view(1, -1, 1, 1), d(fix["bias"][lo:hi]).view(1, -1, 1, 1)
        c = F.conv2d(a, ws[l], padding=1)
        mean = c.sum(dim=(0, 2, 3), keepdim=True) / N
        var = ((c - mean) ** 2).sum(dim=(0, 2, 3), keepdim=True) / N
        invstd = 1.0 / torch.sqrt(var + eps[l])
        xh = (c - mean) * invstd
        z = xh * gamma + bias
        acts.append(a)
        keep.append((gamma, invstd, xh, z))
        rm, rv = torch.zeros(hi - lo, dtype=torch.float64), torch.ones(hi - lo, dtype=torch.float64)
        for k in range(calls):
            m = 1.0 / (k + 1) if momentum[l] is None else momentum[l]
            rm = (1 - m) * rm + m * mean.reshape(-1)
            rv = (1 - m) * rv + m * (var.reshape(-1) * N / (N - 1))
        out["rm%d" % (l + 1)], out["rv%d" % (l + 1)], out["nbt%d" % (l + 1)] = rm, rv, calls
        a = torch.relu(z)
    out["y"], out["z"] = a, [k[3] for k in keep]
    grad = g
    for l in (2, 1, 0):
        gamma, invstd, xh, z = keep[l]
        dz = grad * (z > 0)
        S1, S2 = dz.sum(dim=(0, 2, 3), keepdim=True), (dz * xh).sum(dim=(0, 2, 3), keepdim=True)
        dc = gamma * invstd * (dz - S1 / N - xh * S2 / N)
        out["gb%d" % (l + 1)], out["gg%d" % (l + 1)] = S1.reshape(-1), S2.reshape(-1)
        out["gw%d" % (l + 1)] = torch.nn.grad.conv2d_weight(acts[l], ws[l].shape, dc, padding=1)
        grad = torch.nn.grad.conv2d_input(acts[l].shape, ws[l], dc, padding=1)
    out["gx"] = grad
    return out


def margin_ok(truth_z, ref_z):
    """The ReLU margin rule, per layer, and that no mask of the reference differs from the truth's."""
    for zt, zr in zip(truth_z, ref_z):
        e_z = float((zr.double() - zt).abs().max())
        if float(zt.abs().min()) < max(16.0 * e_z, 2e-6 * float(zt.abs().max())):
            return False
        if bool(((zr > 0) != (zt > 0)).any()):
            return False
    return True


def running_of(fix):
    return fix["rmean"], fix["rvar"]


@functools.lru_cache(maxsize=None)
def problem(shape, offset, mode="train", eps=1e-5):
    """(fixture, truth, reference) of one case at one seed offset; mode 'train' (batch statistics, momentum 0.1, one call) or 'frozen'."""
    fix = draw(*shape, SEED + offset)
    if mode == "train":
        return fix, restatement(fix, eps=eps), stock(fix, torch.float32, eps=eps)
    return (fix, stock(fix, torch.float64, train=False, running=running_of(fix), eps=eps),
            stock(fix, torch.float32, train=False, running=running_of(fix), eps=eps))


def first_offset(shape, mode="train", eps=1e-5):
    """The first seed offset in [0, MAX_OFFSET) whose draw satisfies the margin rule, or None."""
    for off in range(MAX_OFFSET):
        if mode == "step":
            if step_margin_ok(*step_problem(shape, off)[1:]):
                return off
            continue
        _, truth, ref = problem(shape, off, mode, eps)
        if margin_ok(truth["z"], ref["z"]):
            return off
    return None


def e_ref(truth, ref, name):
    return float((ref[name].double() - truth[name].double()).abs().max())


def excess(got, truth, ref, name):
    """(max |got - truth|, the bound 4 e_ref + 1e-5 max|truth|) of one tensor."""
    t = truth[name].double()
    err = float((got[name].double().reshape(t.shape) - t).abs().max())
    return err, 4.0 * e_ref(truth, ref, name) + 1e-5 * float(t.abs().max())


# ================================================================================================================= the step's pattern
def triplet_l1(anchor, positive, negative):
    """homo_model_builder.py:197-199: nn.TripletMarginLoss(margin=1.0, p=1, reduce=False) summed, over the batch and the 127 x 127 of the reference
    (here: the plane's own size)."""
    B, _, H, W = anchor.shape
    return F.triplet_margin_loss(anchor, positive, negative, margin=1.0, p=1, reduction="none").sum() / B / (H * W)


def step_run(module, fix, dtype, dev="cpu", zs=None):
    """One module called three times in one graph (train mode): on x, x2 (data) and x3 (requires grad), the triplet loss on top, backward.
    -> collect()'s dict, 'gx' = grad of x3, plus 'hinge' (the loss' hinge arguments)."""
    x1, x2 = fix["x"].to(dev, dtype), fix["x2"].to(dev, dtype)
    x3 = fix["x3"].detach().clone().to(dev, dtype).requires_grad_(True)
    p1, p2, p3 = module(x1), module(x2), module(x3)
    loss = triplet_l1(p2, p3, p1)
    loss.backward()
    out = collect(module, p3, x3, zs)
    with torch.no_grad():
        out["hinge"] = (F.pairwise_distance(p2, p3, p=1) - F.pairwise_distance(p2, p1, p=1) + 1.0).detach().cpu()
    out["loss"] = loss.detach().cpu()
    return out


def step_stock(fix, dtype):
    from hdn_amd.share_feature import PreShareFeature
    m = load_params(PreShareFeature().to(dtype), fix).train()      # the default module: the stock layers
    zs = []
    hooks = [m.ShareFeature[b].register_forward_hook(lambda mod, i, o: zs.append(o.detach().clone())) for b in (1, 4, 7)]
    out = step_run(m, fix, dtype, zs=zs)
    for h in hooks:
        h.remove()
    return out


@functools.lru_cache(maxsize=None)
def step_problem(shape, offset):
    fix = draw(*shape, SEED + offset)
    return fix, step_stock(fix, torch.float64), step_stock(fix, torch.float32)


def step_margin_ok(truth, ref):
    """The margin rule on the nine pre-activation tensors of the three calls, and the hinge argument away from its kink."""
    return margin_ok(truth["z"], ref["z"]) and float(truth["hinge"].abs().min()) >= HINGE_MARGIN and \
        not bool(((ref["hinge"] > 0) != (truth["hinge"] > 0)).any())


# ================================================================================================================= on the device
def run_module(fix, dev, train=True, running=None, momentum=0.1, calls=1, x_grad=True, p_grad=True, backward=True, eps=1e-5):
    """hdn_amd.PreShareFeatureTrain on `dev`: `calls` forwards on fix['x'], then backward of fix['g'].  -> collect()'s dict (+ 'grad_fn')."""
    import hdn_amd
    m = load_params(hdn_amd.PreShareFeatureTrain(), fix, running, momentum, eps).to(dev).train(train)
    for p in m.parameters():
        p.requires_grad_(p_grad)
    x = fix["x"].detach().clone().to(dev).requires_grad_(x_grad)
    for _ in range(calls):
        y = m(x)
    if backward and y.requires_grad:
        y.backward(fix["g"].to(dev))
    torch.cuda.synchronize(dev)
    out = collect(m, y, x)
    out["grad_fn"] = y.grad_fn is not None
    return out


def at_offset(t, off, dev, margin=0, fill=0.0):
    """(view, whole buffer): the values of t (an int: that many floats of NaN) at float offset margin + off of a fresh allocation that ends `margin`
    floats behind them; the rest holds `fill`."""
    n = t if isinstance(t, int) else t.numel()
    host = torch.full((margin + off + n + margin,), float(fill))
    host[margin + off:margin + off + n] = float("nan") if isinstance(t, int) else t.reshape(-1)
    buf = host.to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[margin + off:margin + off + n], buf


def untouched(buf, lo, hi):
    """Is every byte of the whole buffer (on the CPU) outside the floats [lo, hi) still 0xA5?"""
    raw = buf.numpy().view(np.uint8).reshape(-1, 4)
    return bool((raw[:lo] == BYTE).all()) and bool((raw[hi:] == BYTE).all())


def run_raw(fix, dev, offsets=(0, 0, 0, 0, 0), frozen=False, need_x=True, need_params=True, eps=1e-5):
    """One raw hdn_share_feature_train_fwd_f32 and one hdn_share_feature_bwd_f32: every output starts as NaN inside 0xA5 margins at the given float
    offsets; an output that is not asked for is NULL and its buffer 0xA5 everywhere.  -> (dict y, stats, gx | None, gp | None on the CPU, were all
    bytes outside the results left alone?)."""
    from hdn_amd import _lib
    lib = _lib.load()
    B, _, H, W = fix["x"].shape
    n = B * H * W
    P = _lib.ptr
    eps = per_layer(eps)
    xd, gd = at_offset(fix["x"], offsets[3], dev)[0], at_offset(fix["g"], offsets[4], dev)[0]
    par = {k: fix[k].to(dev) for k in ("w1", "w2", "w3", "gamma", "bias")}
    mv = torch.cat([fix["rmean"], fix["rvar"]]).to(dev) if frozen else None
    outs = {"y": at_offset(n, offsets[0], dev, PAD, FILL), "saved": at_offset(13 * n, offsets[1], dev, PAD, FILL),
            "stats": at_offset(39, offsets[2], dev, PAD, FILL), "gx": at_offset(n, offsets[0], dev, PAD, FILL),
            "gp": at_offset(422, offsets[1], dev, PAD, FILL)}
    off_of = {"y": offsets[0], "saved": offsets[1], "stats": offsets[2], "gx": offsets[0], "gp": offsets[1]}
    need = {"y": True, "saved": True, "stats": True, "gx": need_x, "gp": need_params}
    for k, wanted in need.items():
        if not wanted:
            outs[k][1].fill_(FILL)
    nbytes = lib.hdn_share_feature_train_workspace_bytes(B, H, W)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), device=dev)
    st = _lib.stream_ptr(dev)
    rc = lib.hdn_share_feature_train_fwd_f32(P(xd), P(par["w1"]), P(par["w2"]), P(par["w3"]), P(par["gamma"]), P(par["bias"]),
                                             P(mv) if frozen else None, eps[0], eps[1], eps[2], 1 if frozen else 0, P(outs["y"][0]), P(outs["saved"][0]),
                                             P(outs["stats"][0]), P(ws), nbytes, B, H, W, st)
    _lib.check(rc, "hdn_share_feature_train_fwd_f32")
    ws.fill_(float("nan"))
    rc = lib.hdn_share_feature_bwd_f32(P(xd), P(par["w1"]), P(par["w2"]), P(par["w3"]), P(par["gamma"]), P(par["bias"]), P(outs["saved"][0]),
                                       P(outs["stats"][0]), P(gd), P(outs["gx"][0]) if need_x else None, P(outs["gp"][0]) if need_params else None,
                                       P(ws), nbytes, 1 if frozen else 0, B, H, W, st)
    _lib.check(rc, "hdn_share_feature_bwd_f32")
    torch.cuda.synchronize(dev)
    res, clean = {}, True
    for k, (view, buf) in outs.items():
        cnt = view.numel()
        clean = clean and (untouched(buf.cpu(), PAD + off_of[k], PAD + off_of[k] + cnt) if need[k] else untouched(buf.cpu(), 0, 0))
        res[k] = view.cpu() if need[k] else None
    res["y"] = res["y"].view(B, 1, H, W)
    if need_x:
        res["gx"] = res["gx"].view(B, 1, H, W)
    return res, clean


def split_params(gp):
    """grad_params[422] -> the dict entries gw1..3, gg1..3, gb1..3."""
    out = {"gw1": gp[0:36].view(4, 1, 3, 3), "gw2": gp[36:324].view(8, 4, 3, 3), "gw3": gp[324:396].view(1, 8, 3, 3)}
    for l, (lo, hi) in enumerate(LAYERS, start=1):
        out["gg%d" % l], out["gb%d" % l] = gp[396 + lo:396 + hi], gp[409 + lo:409 + hi]
    return out
