"""A whole training iteration of the similarity model as one graph: hdn_amd.simi_training_forward -> total_loss.backward() ->
GatedAMSGrad.step(total_loss + bump), captured under the capture error mode "global" (a host read or an upload anywhere fails the capture) and
replayed for three batches refilled in place, the middle one with bump = inf.  The stand-in model and the batches are those of
tests/simi_train_cases.py.

  - the parameters after each replay are bit-equal to the same three iterations run eagerly;
  - the middle iteration leaves every parameter bit-unchanged, status 1;
  - after all three the parameters agree with the stock path on the device (the same forward, the host gate of train.py:277, clip_grad_norm_ and
    torch.optim.Adam(amsgrad=True)) within the bound.

Against the stock path there are two statements, because the two paths see the same gradients only in the first iteration:

  - after the first iteration (the gradients are bit-equal: same parameters, same batch, a reproducible backward) every parameter element is
    within max(4 d_ref, 1 ulp_fp32) of the stock path and of the float64 oracle of tests/opt_step_cases.py, d_ref the distance of stock fp32 Adam on
    the CPU from that oracle on the recorded gradients, per tensor (absolute: biases start at 0 and real gradients change sign);
  - after all three, the two paths have seen different gradients (from the second taken step on, by what a last-place difference of the
    parameters does to the forward and backward), so d_ref is the stock path's own answer to such a difference: a second stock path, identical
    but for every parameter nudged by one fp32 ulp (up at even positions, down at odd ones) after the first optimizer step - another honest fp32
    implementation - and its distance from the stock path, the largest over the tensors of a learning-rate group.  The bound is
    max(4 d_ref, 1 ulp_fp32(max |p|)) as everywhere; the recorded-gradient oracle check holds the optimizer itself for all three iterations.

Measured on an MI355X: at most one ulp from the stock path after all three iterations (d / bound <= 0.06), 0.50 of the bound after the first,
0.25 against the oracle.  (Before step() bumped the parameters' version counters this test failed by a factor 3.6: PreShareFeatureTrain kept
serving BatchNorm parameters packed before the first step.)"""
import pytest
import torch

import opt_step_cases as C
import simi_train_cases as ST
from hdn_amd import GatedAMSGrad, simi_training_forward  # noqa: F401  (the module is about them: without them nothing here is collected)

gpu = pytest.mark.gpu
BATCHES = (("mixed", 0), ("no_unsup_pos", 1), ("no_neg", 2))
BUMPS = (0.0, float("inf"), 0.0)
LRS = (C.LR_BASE, C.LR_HOMO)
MAX_NORM = 10.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pinned():
    """the stand-in's small convolutions are the library's, which picks an algorithm per process: pinned, as tests/test_gpu_simi_training_forward.py does"""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _groups(model):
    """build_opt_lr's split (tools/train.py:115-165): the homography estimator on its own learning rate"""
    hm = list(model.hm_net.parameters())
    ids = {id(p) for p in hm}
    return [{"params": [p for p in model.parameters() if id(p) not in ids], "lr": LRS[0]}, {"params": hm, "lr": LRS[1]}]


def _flat(groups):
    return [p for g in groups for p in g["params"]]


def _fill(static, k, dev):
    flags, seed = BATCHES[k]
    for key, v in ST.make_batch(flags, seed).items():
        static[key].copy_(v.to(dev))


def _bits(params):
    return [p.detach().clone().view(torch.int32) for p in params]


class _Recorded:
    """what opt_step_cases.stock_steps / reference_steps need of a case, for gradients recorded on the device"""

    def __init__(self, params0, grads, group_of, losses):
        self._p, self._g, self.group_of, self.lrs, self.max_norm, self._losses = params0, grads, group_of, LRS, MAX_NORM, losses

    def params0(self):
        return self._p

    def grads(self):
        return self._g

    def state0(self):
        return None

    def loss32(self, k):
        return self._losses[k]


@gpu
def test_a_whole_iteration_replays_as_one_graph(dev, pinned):
    import numpy as np
    import hdn_amd
    models = {k: ST.on_device(ST.make_model(), dev) for k in ("graph", "eager", "stock", "nudged")}
    groups = {k: _groups(m) for k, m in models.items()}
    flat = {k: _flat(g) for k, g in groups.items()}
    static = {k: v.to(dev).clone() for k, v in ST.make_batch(*BATCHES[0]).items()}
    bump = torch.zeros((), dtype=torch.float32, device=dev)
    kw = dict(betas=C.BETAS, eps=C.EPS, weight_decay=C.WEIGHT_DECAY)
    opts = {k: GatedAMSGrad(groups[k], max_norm=MAX_NORM, loss_limit=C.LOSS_LIMIT, **kw) for k in ("graph", "eager")}
    stock = {k: torch.optim.Adam(groups[k], amsgrad=True, **kw) for k in ("stock", "nudged")}
    params0 = [p.detach().cpu().numpy().copy() for p in flat["eager"]]

    # ---- capture: warm-up of forward and backward on a side stream (the constants of this batch size), no optimizer step
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            models["graph"].zero_grad(set_to_none=True)
            hdn_amd.simi_training_forward(models["graph"], static)["total_loss"].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    models["graph"].zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        out = hdn_amd.simi_training_forward(models["graph"], static)
        out["total_loss"].backward()
        opts["graph"].step(out["total_loss"] + bump)

    # ---- three iterations: replayed, eager, stock
    grads, losses, statuses = [], [], []
    for k in range(3):
        _fill(static, k, dev)
        bump.fill_(BUMPS[k])
        before = _bits(flat["graph"])
        graph.replay()
        torch.cuda.synchronize()
        statuses.append(int(opts["graph"].report.status))

        models["eager"].zero_grad(set_to_none=True)
        loss = hdn_amd.simi_training_forward(models["eager"], static)["total_loss"]
        loss.backward()
        grads.append([None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in flat["eager"]])
        losses.append(np.float32(float(loss.detach()) + BUMPS[k]))
        opts["eager"].step(loss + bump)
        torch.cuda.synchronize()
        assert int(opts["eager"].report.status) == statuses[-1]
        assert float(opts["eager"].report.grad_norm) == float(opts["graph"].report.grad_norm), k
        after = _bits(flat["graph"])
        assert all(torch.equal(a, b) for a, b in zip(after, _bits(flat["eager"]))), (k, "a replayed iteration differs from the eager one")
        if BUMPS[k] != 0.0:
            assert statuses[-1] == 1 and all(torch.equal(a, b) for a, b in zip(before, after)), "the gated iteration changed a parameter"
        else:
            assert statuses[-1] == 0 and any(not torch.equal(a, b) for a, b in zip(before, after))

        for name in ("stock", "nudged"):                                         # train.py:271-281
            models[name].zero_grad(set_to_none=True)
            loss = hdn_amd.simi_training_forward(models[name], static)["total_loss"] + bump
            if C.is_valid_number(loss.item()):
                loss.backward()
                torch.nn.utils.clip_grad_norm_(flat[name], MAX_NORM)
                stock[name].step()
        if k == 0:
            first = {name: [p.detach().double().cpu().numpy().reshape(-1) for p in flat[name]] for name in ("graph", "stock")}
            with torch.no_grad():
                for p in flat["nudged"]:
                    v = p.reshape(-1)
                    v[0::2] = torch.nextafter(v[0::2], torch.full_like(v[0::2], float("inf")))
                    v[1::2] = torch.nextafter(v[1::2], torch.full_like(v[1::2], float("-inf")))
    assert statuses == [0, 1, 0]
    assert opts["graph"].report.steps.tolist() == [0.0 if g is None else 2.0 for g in grads[0]]
    assert sum(g is not None for g in grads[0]) > len(grads[0]) // 2 and any(g is not None for g in grads[0][len(groups["eager"][0]["params"]):])

    # ---- the optimizer itself, on the recorded gradients: the float64 oracle and stock fp32 Adam on the CPU
    n0 = len(groups["eager"][0]["params"])
    group_of = [0] * n0 + [1] * len(groups["eager"][1]["params"])
    np64 = lambda t: t.detach().double().cpu().numpy().reshape(-1)

    def optimizer_bound(rows, gate, got, label, others=()):
        want = C.reference_steps(params0, rows, group_of, LRS, gate, max_norm=MAX_NORM)
        s32 = C.stock_steps(_Recorded(params0, rows, group_of, gate), torch.float32)
        assert want["status"] == s32["status"]
        worst = 0.0
        for i, ours in enumerate(got):
            o = want["param"][i].reshape(-1)
            d_ref = np.abs(s32["param"][i].reshape(-1) - o)
            bound = np.maximum(4.0 * d_ref.max(), C.ulp32(o))
            for x in (ours,) + tuple(other[i] for other in others):
                assert (np.abs(x - o) <= bound).all() and (np.abs(x - ours) <= bound).all(), (label, i, float(np.abs(x - o).max()), float(bound.max()))
                worst = max(worst, float((np.abs(x - o) / bound).max()), float((np.abs(x - ours) / bound).max()))
        print(f"TRAIN_STEP_GRAPH {label}: worst d / bound over {len(got)} parameter tensors {worst:.3f}")

    inf = np.float32(np.inf)
    optimizer_bound([grads[0]] * 3, [losses[0], inf, inf], first["graph"], "after the first iteration, against the oracle and the stock path",
                    others=(first["stock"],))
    optimizer_bound(grads, losses, [np64(p) for p in flat["graph"]], "after all three, against the oracle on the recorded gradients")

    # ---- all three iterations against the stock path: d_ref is the stock path's own answer to a one-ulp nudge, per learning-rate group
    dist = {name: [float(np.abs(np64(a) - np64(b)).max()) for a, b in zip(flat[name], flat["stock"])] for name in ("graph", "nudged")}
    for gi, (lo, hi) in enumerate(((0, n0), (n0, len(group_of)))):
        d_ref = max(dist["nudged"][lo:hi])
        for i in range(lo, hi):
            bound = max(4.0 * d_ref, float(C.ulp32(float(flat["stock"][i].detach().abs().max()))))
            print(f"TRAIN_STEP_GRAPH group {gi} tensor {i} {tuple(flat['stock'][i].shape)}: d {dist['graph'][i]:.3e}, the nudged stock path "
                  f"{dist['nudged'][i]:.3e}, bound {bound:.3e}, d / bound {dist['graph'][i] / bound:.3f}")
            assert dist["graph"][i] <= bound, (gi, i, dist["graph"][i], bound)
