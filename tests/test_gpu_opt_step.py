"""hdn_amd.optim.GatedAMSGrad and hdn_amd.grad_norm on the device against the float64 oracle of tests/opt_step_cases.py, K = 3 steps per case:
every parameter, the three moments, the counters, grad_norm and status - and the clipped gradients - within max(4 d_ref, 1 ulp) (counters and
status exactly); skipped steps leave parameters, moments and counters bit-identical; two runs are bit-identical; step() captured in a graph under
the capture error mode "global" and replayed after gradients, loss and learning rate were refilled in place is bit-equal to the eager steps; a
state_dict round-trips through stock Adam(amsgrad=True) and continues bit-equal; the device-side argument checks."""
import dataclasses
import warnings

import numpy as np
import pytest
import torch

import opt_step_cases as C
from hdn_amd import GatedAMSGrad, grad_norm  # noqa: F401  (the module is about them: without them nothing here is collected)
from hdn_amd._lib import HdnHipError

gpu = pytest.mark.gpu
STATE_KEYS = C.QUANTITIES[1:]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _placed(a, offset, dev):
    """the fp32 array on the device, `offset` floats off a 16-byte boundary (allocations are 16-byte aligned)"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    return view


def _off(offsets, i):
    return offsets[i] if offsets else 0


class Run:
    """The parameters of a case on the device (in the case's order), their static gradient buffers and a GatedAMSGrad over the case's groups."""

    def __init__(self, c, dev, clip_in_place=False):
        self.c, self.dev = c, dev
        self.params = [torch.nn.Parameter(_placed(a, _off(c.param_offset, i), dev)) for i, a in enumerate(c.params0())]
        for i, p in enumerate(self.params):
            assert p.data_ptr() % 16 == 4 * _off(c.param_offset, i)
        self.groups = [{"params": [p for i, p in enumerate(self.params) if c.group_of[i] == gi], "lr": lr} for gi, lr in enumerate(c.lrs)]
        self.opt = GatedAMSGrad(self.groups, betas=C.BETAS, eps=C.EPS, weight_decay=C.WEIGHT_DECAY, max_norm=c.max_norm, loss_limit=C.LOSS_LIMIT,
                                clip_grads_in_place=clip_in_place)
        st = c.state0()
        if st:
            for i, p in enumerate(self.params):
                self.opt.state[p]["step"].fill_(st["step"][i])
                for key in STATE_KEYS:
                    self.opt.state[p][key].copy_(torch.from_numpy(st[key][i]))
        self.grads = c.grads()
        self.gbuf = [_placed(np.zeros(n, np.float32), _off(c.grad_offset, i), dev) for i, n in enumerate(c.sizes)]
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.res = dict(status=[], grad_norm=[], clipped=[])

    def fill(self, k):
        """the gradients and the loss of step k, in place; an absent gradient is None"""
        for i, p in enumerate(self.params):
            g = self.grads[k][i]
            if g is None:
                p.grad = None
            else:
                self.gbuf[i].copy_(torch.from_numpy(g))
                p.grad = self.gbuf[i]
        loss = self.c.loss32(k)
        if loss is not None:
            self.loss.fill_(float(loss))
        return None if loss is None else self.loss

    def bits(self):
        """every parameter, moment and counter as int32 clones"""
        out = [p.detach().clone().view(torch.int32) for p in self.params]
        for p in self.params:
            out += [self.opt.state[p][key].clone().view(torch.int32) for key in STATE_KEYS + ("step",)]
        return out

    def record(self, before=None):
        """after a step (eager or replayed): status, grad_norm, the gradients as they are now; a skipped step changed no bit"""
        torch.cuda.synchronize()
        status = int(self.opt.report.status)
        self.res["status"].append(status)
        self.res["grad_norm"].append(float(self.opt.report.grad_norm))
        self.res["clipped"].append([None if p.grad is None else p.grad.detach().double().cpu().numpy() for p in self.params])
        if status != 0 and before is not None:
            assert all(torch.equal(a, b) for a, b in zip(before, self.bits())), (self.c.name, "a skipped step changed a bit")
        return status

    def finish(self):
        f64 = lambda t: t.detach().double().cpu().numpy()
        self.res["param"] = [f64(p) for p in self.params]
        for key in STATE_KEYS:
            self.res[key] = [f64(self.opt.state[p][key]) for p in self.params]
        self.res["steps"] = np.array([float(self.opt.state[p]["step"]) for p in self.params])
        flat = [p for g in self.groups for p in g["params"]]
        assert self.opt.report.steps.tolist() == [float(self.opt.state[p]["step"]) for p in flat]
        return self.res

    def eager(self):
        for k in range(C.K):
            loss = self.fill(k)
            before = self.bits()
            kept = [None if p.grad is None else p.grad.clone() for p in self.params]
            self.opt.step(loss)
            self.record(before)
            if not self.opt.clip_grads_in_place:
                assert all(a is None or torch.equal(a.view(torch.int32), p.grad.view(torch.int32)) for a, p in zip(kept, self.params))
        return self.finish()


CLIPPED_TOO = ("sizes", "below", "small_clip", "no_clip", "misaligned", "gate_nan", "gate_nan_grad")
RUNS = [(c.name, False) for c in C.all_cases()] + [(name, True) for name in CLIPPED_TOO]


@gpu
@pytest.mark.parametrize("name,clip_in_place", RUNS, ids=lambda v: str(v))
def test_three_steps_against_the_oracle(dev, name, clip_in_place):
    """Every case, clip_grads_in_place off; the cases of CLIPPED_TOO with it on as well, where the gradients left behind are compared too (off: they
    are bit-unchanged, checked in Run.eager).  Skipped steps are checked for bit-identity in Run.record."""
    c = C.case(name)
    res = Run(c, dev, clip_in_place).eager()
    C.check(res, c, clipped=clip_in_place, label=f"device clip_in_place={clip_in_place}")
    if name.startswith("gate_"):
        assert res["status"][1] == C.GATE_STATUS[name[5:]]


@gpu
def test_stock_pytorch_on_the_device_for_the_record(dev):
    """PyTorch-ROCm's own stock path (clip_grad_norm_ and Adam(amsgrad=True), foreach as it defaults) on the device, measured against the same
    bound for docs/PARITY.md: the figures are printed, status and counters are asserted (the quantities are somebody else's arithmetic)."""
    for name in ("sizes", "many", "warm"):
        c = C.case(name)
        C.check(C.stock_steps(c, torch.float32, device=dev, foreach=None), c, clipped=True, label="stock on the device", enforce=False)


@gpu
@pytest.mark.parametrize("name", ["sizes", "many"])
def test_two_runs_are_bit_identical(dev, name):
    c = C.case(name)
    a, b = Run(c, dev, True), Run(c, dev, True)
    a.eager(), b.eager()
    assert a.res["status"] == b.res["status"]
    assert np.array_equal(np.array(a.res["grad_norm"]).view(np.int64), np.array(b.res["grad_norm"]).view(np.int64))
    assert all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits()))
    assert all(torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)) for p, q in zip(a.params, b.params))


def _scheduled(run):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.optim.lr_scheduler.ExponentialLR(run.opt, gamma=0.8)


def _decay(sched):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # a replayed step is no call of optimizer.step(): the scheduler's order warning
        sched.step()


@gpu
@pytest.mark.parametrize("name,middle", [("sizes", float("nan")), ("many", 3.0)])
def test_a_captured_step_follows_gradients_loss_and_learning_rate_refilled_in_place(dev, name, middle):
    """One capture of step(loss) under the capture error mode "global" (a host read or an upload fails it), no warm-up step; three replays, the
    gradients and the loss refilled in place and the learning rates decayed by ExponentialLR(0.8) between them (it fills the 0-d views in place).
    Bit-equal to the same steps run eagerly with the same scheduler, and within the bound of the oracle with the learning rates that were set."""
    c = dataclasses.replace(C.case(name), name=name + "_graph", losses=(12.5, middle, 0.25), absent=frozenset())
    graphed, eager = Run(c, dev, True), Run(c, dev, True)
    runs = {"graph": graphed, "eager": eager}
    sched = {k: _scheduled(r) for k, r in runs.items()}
    for r in runs.values():
        r.fill(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="global"):
        graphed.opt.step(graphed.loss)
    lrs = []
    for k in range(C.K):
        lrs.append(tuple(float(g["lr"]) for g in graphed.opt.param_groups))
        assert lrs[-1] == tuple(float(g["lr"]) for g in eager.opt.param_groups)
        for r in runs.values():
            r.fill(k)
        before = graphed.bits()
        graph.replay()
        graphed.record(before)
        eager.opt.step(eager.loss)
        eager.record()
        assert all(torch.equal(a, b) for a, b in zip(graphed.bits(), eager.bits())), k
        assert all(torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32)) for p, q in zip(graphed.params, eager.params)), k
        for s in sched.values():
            _decay(s)
    assert lrs[1][0] == lrs[0][0] * 0.8 and lrs[2][1] < lrs[1][1] < lrs[0][1]
    assert graphed.res["status"] == eager.res["status"] == [0, 1 if middle != middle else 0, 0]
    res = graphed.finish()
    want = C.reference_steps(c.params0(), c.grads(), c.group_of, lrs, [c.loss32(k) for k in range(C.K)], max_norm=c.max_norm)
    stock = C.stock_steps(c, torch.float32, lrs_steps=lrs)       # d_ref of these very inputs and learning rates
    qs, qw = C.compared(stock, clipped=True), C.compared(want, clipped=True)
    d_ref = {key: C.distance(qs[key], qw[key]) for key in qw}
    assert res["status"] == want["status"] and np.array_equal(res["steps"], want["steps"])
    got, exp = C.compared(res, clipped=True), C.compared(want, clipped=True)
    for key in got:
        d, b = C.distance(got[key], exp[key]), C.bound(d_ref[key])
        print(f"OPT_STEP {c.name} replayed {key}: d {d:.3f} ulp, bound {b:.3f} ulp, d / bound {d / b:.3f}")
        assert d <= b, key


@gpu
def test_a_state_dict_round_trips_through_stock_adam_and_continues_bit_equal(dev):
    """One step, then state_dict() -> torch.optim.Adam(amsgrad=True).load_state_dict -> its state_dict() -> a fresh GatedAMSGrad on equal
    parameters; both then take the remaining steps.  The case has a tensor without a gradient in a step and three groups."""
    c = C.case("absent")
    a, b = Run(c, dev), Run(c, dev)
    a.opt.step(a.fill(0))
    sd = a.opt.state_dict()
    assert all(isinstance(g["lr"], float) for g in sd["param_groups"])
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "max_exp_avg_sq", "step"]
    stock = torch.optim.Adam([{"params": list(g["params"])} for g in a.groups], lr=1.0, betas=C.BETAS, eps=C.EPS, weight_decay=C.WEIGHT_DECAY, amsgrad=True)
    stock.load_state_dict(sd)
    assert [g["lr"] for g in stock.param_groups] == list(c.lrs)
    for p in a.params:
        for key in STATE_KEYS:
            assert torch.equal(stock.state[p][key], a.opt.state[p][key])
        assert float(stock.state[p]["step"]) == 1.0
    with torch.no_grad():
        for p, q in zip(a.params, b.params):
            q.copy_(p)
    b.opt.load_state_dict(stock.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits()))
    assert all(float(x["lr"]) == float(y["lr"]) and x["lr"].dtype == torch.float64 and x["lr"].dim() == 0
               for x, y in zip(b.opt.param_groups, a.opt.param_groups))
    for r in (a, b):
        r.record()
    for k in (1, 2):
        for r in (a, b):
            r.opt.step(r.fill(k))
            r.record()
        assert all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits())), k
    b.res["status"][0] = a.res["status"][0]                      # b never ran step 0: its record of that step is a's
    b.res["grad_norm"][0], b.res["clipped"][0] = a.res["grad_norm"][0], a.res["clipped"][0]
    C.check(b.finish(), c, label="after the round trip")


@gpu
def test_stock_adam_state_loads(dev):
    """A stock Adam(amsgrad=True) that has stepped on the device: its state_dict loads, moments and counters bit for bit."""
    c = C.case("warm")
    r = Run(c, dev)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in r.params]
    groups = [{"params": [p for i, p in enumerate(twins) if c.group_of[i] == gi], "lr": lr * 0.5} for gi, lr in enumerate(c.lrs)]
    stock = torch.optim.Adam(groups, lr=1.0, betas=C.BETAS, eps=C.EPS, weight_decay=C.WEIGHT_DECAY, amsgrad=True)
    for i, p in enumerate(twins):
        p.grad = torch.from_numpy(r.grads[0][i]).to(dev)
    stock.step()
    stock.step()
    r.opt.load_state_dict(stock.state_dict())
    for p, q in zip(r.params, twins):
        for key in STATE_KEYS:
            assert torch.equal(r.opt.state[p][key], stock.state[q][key])
        assert float(r.opt.state[p]["step"]) == 2.0
    assert [float(g["lr"]) for g in r.opt.param_groups] == [lr * 0.5 for lr in c.lrs]
    assert r.opt.report.steps.tolist() == [2.0] * len(twins)


@gpu
def test_grad_norm_alone(dev):
    """hdn_amd.grad_norm: the oracle's norm within one ulp (float64 sums, rounded once), the same bits twice, None entries skipped, views served"""
    c = C.case("sizes")
    grads = c.grads()[0]
    want = C.oracle(c)["grad_norm"][0]
    tensors = [_placed(g, i % 2, dev) for i, g in enumerate(grads)]
    a, b = grad_norm(tensors + [None]), grad_norm(tensors)
    assert a.dim() == 0 and a.dtype == torch.float32 and a.is_cuda
    assert float(a) == float(b) and abs(float(a) - want) <= C.ulp32(want)
    assert float(grad_norm([torch.full((5,), 2.0, device=dev)])) == float(np.float32(np.sqrt(20.0)))


@gpu
def test_argument_checks_on_the_device(dev, monkeypatch):
    p = torch.nn.Parameter(torch.ones(6, device=dev))
    with pytest.raises(TypeError, match="fp32"):
        GatedAMSGrad([torch.nn.Parameter(torch.ones(4, device=dev, dtype=torch.float16))])
    with pytest.raises(ValueError, match="contiguous"):
        GatedAMSGrad([torch.nn.Parameter(torch.ones(4, 4, device=dev).t())])
    opt = GatedAMSGrad([p], lr=2e-4, max_norm=10.0)
    before = p.detach().clone()
    p.grad = torch.ones(12, device=dev)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0, 2]], device=dev), torch.ones(2, device=dev), (6,))
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    p.grad = torch.ones(6, device=dev)
    with pytest.raises(HdnHipError, match="no CPU fallback"):
        opt.step(torch.tensor(1.0))
    with pytest.raises(ValueError, match="0-d"):
        opt.step(torch.ones(1, device=dev))
    with pytest.raises(TypeError, match="fp32"):
        opt.step(torch.tensor(1.0, device=dev, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="cannot be added"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(2, device=dev))]})
    assert torch.equal(p.detach(), before) and opt.report.steps.tolist() == [0.0]
    # anything that uploads refuses to run inside a capture
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the capture"):
        GatedAMSGrad([torch.nn.Parameter(torch.ones(4, device=dev))])
    opt.param_groups[0]["lr"] = 1e-3
    with pytest.raises(RuntimeError, match="in place"):
        opt.step()
    monkeypatch.undo()
    opt.step()                                                   # outside a capture the new number is written and bound again
    assert float(opt.param_groups[0]["lr"]) == 1e-3 and opt.param_groups[0]["lr"].dtype == torch.float64
    assert opt.report.steps.tolist() == [1.0] and int(opt.report.status) == 0
