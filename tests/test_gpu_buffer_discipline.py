"""The matrix-core kernels held to their buffers, in every launch form: each entry point is called through the raw C ABI on operands carved out of
ONE guarded arena per call (tests/buffer_guard.py: 64 KiB margins on both sides of every operand, NaN margins around inputs, 0xA5 margins around
outputs and workspaces, NaN where the kernel is to write, the workspace at exactly the queried size).  Data are the integer problems of the existing
case modules, the expectation their float64 / int64 truth, compared with torch.equal: there is no tolerance in this file.

Asserted for every case: return code 0; an empty verdict (no margin byte and no input byte changed, no NaN left in or computed into an output); the
output equal to the integer truth; with a workspace, bit-equal outputs from a NaN-filled and a 1e30-filled workspace.  Per entry point one variant
puts every pointer at another 16-byte offset that is no multiple of 64, and one runs in activation domain 1 where the entry point has one.

The cases, and the proof that they reach every launch form, are in tests/buffer_discipline_cases.py (checked without a GPU by
tests/test_buffer_guard_host.py).  One test per entry point walks all its cases, collects every finding and prints
    BUFFERS <entry point>: <n> cases, forms <set>, margins clean, workspace fills bit-equal"""
import ctypes
import functools

import pytest
import torch

import buffer_discipline_cases as BC
import buffer_guard as BG
import conv3x3_train_cases as TC
import head_batch_cases as HB
import head_tail_batch_cases as HT
import simi_full_cases as SC
import trunk34_forms as T
from test_gpu_trunk50_forms import _codes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _L():
    from hdn_amd import _lib
    return _lib


def _scale():
    from hdn_amd.trunk import ACT_SCALE_LOG2
    return 2.0 ** -ACT_SCALE_LOG2


@functools.lru_cache(maxsize=8)
def _packed(kind, *key):
    """The packed stream (CPU int16) of the one-hot weights a case uses, once per (packer, shape, code)."""
    from hdn_amd import ops
    if kind == "s1":
        C, k = key
        return ops.pack_conv3x3(T.onehot3x3(C, C, k)[0])
    if kind == "v2":
        return ops.pack_conv3x3_v2(T.onehot3x3(key[0], key[0])[0])
    if kind in ("s2ds", "s2v2"):
        CI, k = key
        w, wd = T.onehot3x3(2 * CI, CI, k)[0], T.onehot1x1(2 * CI, CI)[0]
        return (ops.pack_conv3x3s2_ds if kind == "s2ds" else ops.pack_conv3x3s2_ds_v2)(w, wd)
    if kind == "s2":
        return ops.pack_conv3x3s2(T.onehot3x3(key[0], key[0])[0])
    raise KeyError(kind)


class Tally:
    """The findings and the forms of one test, per entry point."""

    def __init__(self, *entries, workspace=True):
        self.n, self.forms, self.found, self.workspace = {e: 0 for e in entries}, {e: set() for e in entries}, [], workspace

    def add(self, entry, form, problems):
        self.n[entry] += 1
        self.forms[entry].add(form)
        self.found += problems

    def done(self):
        assert not self.found, f"{len(self.found)} findings:\n" + "\n".join(self.found)
        for e, n in self.n.items():
            forms = "{" + ", ".join(sorted(self.forms[e])) + "}"
            print(f"BUFFERS {e}: {n} cases, forms {forms}, margins clean, " + ("workspace fills bit-equal" if self.workspace else "no workspace"))


def guarded(dev, entry, case, form, ins, outs, ws, call, want, offsets=False, unscale=1.0, tag=""):
    """One guarded call.  ins: {name: CPU tensor or None (NULL)}; outs: {name: shape, or a CPU tensor for an in-place operand, or (shape, dtype)};
    ws: {name: bytes}; call(P, g) -> return code with P(name) the operand's pointer (None for an absent one); want: {output: CPU tensor in memory
    order}, compared with torch.equal after multiplying the result by `unscale` (a power of two).  Returns (findings, guard)."""
    g = BG.Guard(dev)
    names = [n for n, t in ins.items() if t is not None] + list(outs) + list(ws)
    offs = dict(zip(names, BG.offsets16(len(names)))) if offsets else {}
    for n, t in ins.items():
        if t is not None:
            g.input(n, t, offs.get(n, 0))
    for n, s in outs.items():
        if torch.is_tensor(s):
            g.inout(n, s, offs.get(n, 0))
        elif len(s) == 2 and isinstance(s[1], torch.dtype):
            g.output(n, s[0], offs.get(n, 0), dtype=s[1])
        else:
            g.output(n, s, offs.get(n, 0))
    for n, b in ws.items():
        g.workspace(n, b, offs.get(n, 0))
    P = lambda n: g.ptr(n) if n in g.ops else None
    rc = g.run(lambda g: call(P, g), {n: (w / unscale) for n, w in want.items()})
    found = [] if rc == 0 else [f"return code {rc}"]
    found += g.verdict()
    for n, w in want.items():
        got = g.result(n).cpu()
        d = BG.first_difference(got * unscale if unscale != 1.0 else got, w.reshape(got.shape), f"index in {n}")
        if d is not None:
            found.append(f"output {n!r}: {d}")
    where = f"{entry} case {case} form {form}" + (" 16-byte offsets " + str(offs) if offsets else "") + (f" {tag}" if tag else "")
    return [f"{where}: {f}" for f in found], g


def f32(t):
    return t.to(torch.float32)


# ----------------------------------------------------------------------------------------------------------------- the guard itself, on the device
def test_guard_reports_the_standin_faults_on_the_device(dev):
    """tests/test_buffer_guard_host.py's stand-in kernels (plain torch; every store stays inside the arena) on the GPU: the faultless one is clean and
    right, every fault is reported in the words the CPU run uses - the arena, the fills and the comparisons work on device memory."""
    import test_buffer_guard_host as H
    g, want = H._problem(device=dev)
    assert g.run(H._kernel()) == 0 and g.verdict() == [] and torch.equal(g.result("out").cpu(), want)
    assert g.view("out").is_cuda and g.ptr("ws").value == g.view("ws").data_ptr() and g.nbytes("ws") == 4 * g.view("ws").numel()
    for fault in H.FAULTS:
        g, want = H._problem(device=dev, offsets=BG.offsets16(4))
        g.run(H._kernel(fault), want={"out": want})
        assert any(H.MUST_SAY[fault] in s for s in g.verdict()), (fault, g.verdict())


# ----------------------------------------------------------------------------------------------------------------- the ResNet-34 trunk's 3x3 kernels
def _stride1(dev, tally, v2, S, C, B, variants):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_conv3x3_v2_f32" if v2 else "hdn_conv3x3_bias_relu_f32"
    fn = getattr(lib, entry)
    xi, ri, bi = _codes((B, S, S, C)), _codes((B, S, S, C), 40503, 2003, 1001), T.bias_int(C)
    _, src, tap = T.onehot3x3(C, C)
    raw = T.pick3x3(xi, src, tap)
    wp = _packed("v2", C) if v2 else _packed("s1", C, 0)
    nws = lib.hdn_conv3x3_v2_workspace_bytes(B, S, C) if v2 else lib.hdn_conv3x3_workspace_bytes(B, S, C, 1)
    form = BC.form_of(entry, (S, C, B))
    for residual, dom, offsets in variants:
        k = _scale() if dom else 1.0
        want = f32(torch.relu(raw + bi + (ri if residual else 0)))
        ins = dict(x=f32(xi) * k, wpacked=wp, bias=f32(bi) * k, residual=f32(ri) * k if residual else None)
        call = lambda P, g: fn(P("x"), P("wpacked"), P("bias"), P("residual"), P("out"), P("workspace"), g.nbytes("workspace"), B, S, C, dom, s)
        found, _ = guarded(dev, entry, (S, C, B), form, ins, dict(out=(B, S, S, C)), dict(workspace=nws), call, dict(out=want), offsets, 1.0 / k,
                           f"residual {residual} domain {dom}")
        tally.add(entry, form, found)


PLAIN = [(True, 0, False), (False, 0, False)]
EXTRA = [(True, 0, True), (True, 1, False)]                    # (residual, act_domain, 16-byte offsets): the two variants, at the smallest case


def test_conv3x3_bias_relu_buffers(dev):
    t = Tally("hdn_conv3x3_bias_relu_f32")
    for i, (S, C, B) in enumerate(sorted(BC.S1, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        _stride1(dev, t, False, S, C, B, PLAIN + (EXTRA if i == 0 else []))
    t.done()


def test_conv3x3_v2_buffers(dev):
    t = Tally("hdn_conv3x3_v2_f32")
    for i, (S, C, B) in enumerate(sorted(BC.V2, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        _stride1(dev, t, True, S, C, B, PLAIN + (EXTRA if i == 0 else []))
    # the variants at the S = 4 workspace form as well: the smallest case above has none
    S, C, B = next(c for c in BC.V2 if BC.form_of("hdn_conv3x3_v2_f32", c) != "z=1")
    _stride1(dev, t, True, S, C, B, EXTRA)
    t.done()


def _stride2(dev, tally, v2, S, CI, B, variants):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_conv3x3s2_v2_f32" if v2 else "hdn_conv3x3s2_ds_f32"
    CO = 2 * CI
    xi, bi = _codes((B, 2 * S, 2 * S, CI)), T.bias_int(CO)
    _, src, tap = T.onehot3x3(CO, CI)
    _, srcd = T.onehot1x1(CO, CI)
    want, want_ds = f32(torch.relu(T.pick3x3(xi, src, tap, 2) + bi)), f32(T.pick1x1s2(xi, srcd))
    wp = _packed("s2v2" if v2 else "s2ds", CI, 0)
    nws = 0 if v2 else lib.hdn_conv3x3_workspace_bytes(B, S, CI, 2)
    form = BC.form_of(entry, (S, CI, B))
    for dom, offsets in variants:
        k = _scale() if dom else 1.0
        ins = dict(x=f32(xi) * k, wpacked=wp, bias=f32(bi) * k)
        if v2:
            call = lambda P, g: lib.hdn_conv3x3s2_v2_f32(P("x"), P("wpacked"), P("bias"), P("out"), P("out_ds"), B, S, CI, dom, s)
        else:
            call = lambda P, g: lib.hdn_conv3x3s2_ds_f32(P("x"), P("wpacked"), P("bias"), P("out"), P("out_ds"), P("workspace"), g.nbytes("workspace"),
                                                         B, S, CI, dom, s)
        found, _ = guarded(dev, entry, (S, CI, B), form, ins, dict(out=(B, S, S, CO), out_ds=(B, S, S, CO)), {} if v2 else dict(workspace=nws), call,
                           dict(out=want, out_ds=want_ds), offsets, 1.0 / k, f"domain {dom}")
        tally.add(entry, form, found)


def test_conv3x3s2_ds_buffers(dev):
    t = Tally("hdn_conv3x3s2_ds_f32")
    for i, (S, CI, B) in enumerate(sorted(BC.S2DS, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        _stride2(dev, t, False, S, CI, B, [(0, False)] + ([(0, True), (1, False)] if i == 0 else []))
    t.done()


def test_conv3x3s2_v2_buffers(dev):
    t = Tally("hdn_conv3x3s2_v2_f32", workspace=False)
    for i, (S, CI, B) in enumerate(sorted(BC.S2V2, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        _stride2(dev, t, True, S, CI, B, [(0, False)] + ([(0, True), (1, False)] if i == 0 else []))
    t.done()


# ----------------------------------------------------------------------------------------------------------------- the chained form
def _chain(dev, tally, case, form, x, x_slices, x_bias, x_res, res_slices, want_x_out, wp, B, S, CI, stride, dom, want, offsets=False, tag=""):
    """One hdn_conv3x3_chain_f32 call; want: {"out_slices": the SUM over z expected, ...}: the slices are compared summed (exact: all but one slice
    of every element are exact zeros), x_out as it is.  Returns the guard (its results feed the next call)."""
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    z, CO, SI = T.z_chain(B, S, CI, stride), CI * stride, S * stride
    ins = dict(x=x, x_bias=x_bias, x_res=x_res, wpacked=wp)
    outs = dict(out_slices=(z, B, S, S, CO))
    if stride == 2:
        outs["out_ds_slices"] = (z, B, S, S, CO)
    if want_x_out is not None:
        outs["x_out"] = (B, SI, SI, CI)
    call = lambda P, g: lib.hdn_conv3x3_chain_f32(P("x"), x_slices, P("x_bias"), P("x_res"), res_slices, P("x_out"), P("wpacked"), P("out_slices"),
                                                  P("out_ds_slices"), B, S, CI, stride, dom, s)
    found, g = guarded(dev, "hdn_conv3x3_chain_f32", case, form, ins, outs, {}, call, {} if want_x_out is None else dict(x_out=want_x_out), offsets,
                       tag=tag + f" x_slices {x_slices} res_slices {res_slices} x_out {'given' if want_x_out is not None else 'NULL'} domain {dom}")
    for n, w in want.items():
        d = BG.first_difference(g.result(n).cpu().sum(0), w, f"(image, y, x, channel) of the sum of {n}")
        if d is not None:
            found.append(f"hdn_conv3x3_chain_f32 case {case} form {form} {tag}: {d}")
    tally.add("hdn_conv3x3_chain_f32", form, found)
    return g


def _finish(dev, tally, case, slices, bias, res, res_slices, B, S, C, want, offsets=False, tag=""):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    z = slices.shape[0]
    call = lambda P, g: lib.hdn_conv3x3_finish_f32(P("slices"), z, P("bias"), P("res"), res_slices, P("out"), B, S, C, s)
    found, _ = guarded(dev, "hdn_conv3x3_finish_f32", case, f"z={z}", dict(slices=slices, bias=bias, res=res), dict(out=(B, S, S, C)), {}, call,
                       dict(out=want), offsets, tag=tag + f" res_slices {res_slices}")
    tally.add("hdn_conv3x3_finish_f32", f"z={z}", found)


def test_conv3x3_chain_and_finish_buffers(dev):
    """conv -> lazy conv -> finish on chain1_case, the stride-2 block on chain2_case: x_slices 0 and > 0, res_slices 0 / 1 / > 1, x_out NULL and given;
    every slice tensor, x_out and the finished activation under guard.  The slices one call wrote are the next call's guarded input."""
    t = Tally("hdn_conv3x3_chain_f32", "hdn_conv3x3_finish_f32", workspace=False)
    sc = _scale()
    for i, (S, C, B) in enumerate(sorted(BC.CHAIN1, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        c = T.chain1_case(B, S, C)
        case, form = (S, C, B, 1), BC.form_of("hdn_conv3x3_chain_f32", (S, C, B, 1))
        for dom, offsets in [(0, False)] + ([(0, True), (1, False)] if i == 0 else []):
            k = sc if dom else 1.0
            b0, b1 = (f32(b) * k for b in c["b"])
            g0 = _chain(dev, t, case, form, f32(c["xi"]) * k, 0, None, None, 0, None, _packed("s1", C, 0), B, S, C, 1, dom,
                        dict(out_slices=f32(c["raw0"]) * k), offsets, "conv 0")
            g1 = _chain(dev, t, case, form, g0.result("out_slices").cpu(), g0.result("out_slices").shape[0], b0, f32(c["ri"]) * k, 1, f32(c["a"]) * k,
                        _packed("s1", C, 1), B, S, C, 1, dom, dict(out_slices=f32(c["raw1"]) * k), offsets, "conv 1")
            _finish(dev, t, case, g1.result("out_slices").cpu(), b1, g1.result("x_out").cpu(), 1, B, S, C, f32(c["out"]) * k, offsets, "finish")
            if not dom and not offsets:
                _finish(dev, t, case, g0.result("out_slices").cpu(), b0, None, 0, B, S, C, f32(torch.relu(c["raw0"] + c["b"][0])), False, "finish plain")
    for S, CI, B in BC.CHAIN2:
        c = T.chain2_case(B, S, CI)
        CO = 2 * CI
        case, form = (S, CI, B, 2), BC.form_of("hdn_conv3x3_chain_f32", (S, CI, B, 2))
        b0, b1, b2 = (f32(b) for b in c["b"])
        g0 = _chain(dev, t, case, "z=%d" % T.z_chain(B, 2 * S, CI, 1), f32(c["xi"]), 0, None, None, 0, None, _packed("s1", CI, 0), B, 2 * S, CI, 1, 0,
                    dict(out_slices=f32(c["raw0"])), False, "conv 0")
        s0 = g0.result("out_slices").cpu()
        g1 = _chain(dev, t, case, form, s0, s0.shape[0], b0, f32(c["ri"]), 1, f32(c["a"]), _packed("s2ds", CI, 1), B, S, CI, 2, 0,
                    dict(out_slices=f32(c["raw1"]), out_ds_slices=f32(c["d"])), False, "stride-2 conv")
        s1, sd = g1.result("out_slices").cpu(), g1.result("out_ds_slices").cpu()
        g2 = _chain(dev, t, case, "z=%d" % T.z_chain(B, S, CO, 1), s1, s1.shape[0], b1, None, 0, None, _packed("s1", CO, 2), B, S, CO, 1, 0,
                    dict(out_slices=f32(c["raw2"])), False, "conv 2")                    # x_slices > 0, res_slices 0, x_out NULL
        s2 = g2.result("out_slices").cpu()
        _finish(dev, t, case, s2, b2, sd, sd.shape[0], B, S, CO, f32(c["out"]), False, "finish with the downsample slices")      # res_slices > 1
        _chain(dev, t, case, "z=%d" % T.z_chain(B, S, CO, 1), s2, s2.shape[0], b2, sd, sd.shape[0], f32(c["out"]), _packed("s1", CO, 3), B, S, CO, 1, 0,
               dict(out_slices=f32(c["raw3"])), False, "next block")                     # res_slices > 1 into a convolution, x_out given
    t.done()


# ----------------------------------------------------------------------------------------------------------------- the ResNet-50 trunk's kernels
def test_conv1x1_buffers(dev):
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    t = Tally("hdn_conv1x1_f32", workspace=False)
    entry = "hdn_conv1x1_f32"
    for i, case in enumerate(sorted(BC.C1X1, key=lambda c: c[4] * c[2] * c[2] * c[0])):
        CI, CO, S, stride, B = case
        So = (S - 1) // stride + 1
        xi, ri, bi = _codes((B, S, S, CI)), _codes((B, So, So, CO), 40503, 2003, 1001), T.bias_int(CO)
        src = (5 * torch.arange(CO) + 3) % CI
        w = torch.zeros(CO, CI)
        w[torch.arange(CO), src] = 1.0
        wp = ops.pack_conv1x1(w)
        picked = xi[:, ::stride, ::stride, :][..., src] + bi
        form = BC.form_of(entry, case)
        for residual, relu, dom, offsets in [(True, 1, 0, False), (False, 0, 0, False)] + ([(True, 1, 0, True), (True, 1, 1, False)] if i == 0 else []):
            k = _scale() if dom else 1.0
            want = f32(torch.relu(picked + ri)) if residual else f32(picked)
            ins = dict(x=f32(xi) * k, wpacked=wp, bias=f32(bi) * k, residual=f32(ri) * k if residual else None)
            call = lambda P, g: lib.hdn_conv1x1_f32(P("x"), P("wpacked"), P("bias"), P("residual"), P("out"), B, S, CI, CO, stride, relu, dom, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(out=(B, So, So, CO)), {}, call, dict(out=want), offsets, 1.0 / k,
                               f"residual {residual} relu {relu} domain {dom}")
            t.add(entry, form, found)
    t.done()


def test_conv3x3s2_buffers(dev):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    t = Tally("hdn_conv3x3s2_f32")
    entry = "hdn_conv3x3s2_f32"
    for i, case in enumerate(sorted(BC.S2, key=lambda c: c[2] * c[0] * c[0] * c[1])):
        S, C, B = case
        xi, bi = _codes((B, 2 * S, 2 * S, C)), T.bias_int(C)
        _, src, tap = T.onehot3x3(C, C)
        want = f32(torch.relu(T.pick3x3(xi, src, tap, 2) + bi))
        nws = lib.hdn_conv3x3s2_workspace_bytes(B, S, C)
        form = BC.form_of(entry, case)
        for dom, offsets in [(0, False)] + ([(0, True), (1, False)] if i == 0 else []):
            k = _scale() if dom else 1.0
            ins = dict(x=f32(xi) * k, wpacked=_packed("s2", C), bias=f32(bi) * k)
            call = lambda P, g: lib.hdn_conv3x3s2_f32(P("x"), P("wpacked"), P("bias"), P("out"), P("workspace"), g.nbytes("workspace"), B, S, C, dom, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(out=(B, S, S, C)), dict(workspace=nws), call, dict(out=want), offsets, 1.0 / k, f"domain {dom}")
            t.add(entry, form, found)
    t.done()


# ----------------------------------------------------------------------------------------------------------------- dilated and valid 3x3, dgrad, wgrad
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _dilated_or_valid(dev, valid):
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_conv3x3v_f32" if valid else "hdn_conv3x3d_f32"
    fn, query = getattr(lib, entry), getattr(lib, entry.replace("_f32", "_workspace_bytes"))
    t = Tally(entry)
    cases = sorted(BC.VALID if valid else BC.DIL, key=lambda c: c[0] * c[1] * c[1] * c[2] * c[3])
    for i, case in enumerate(cases):
        B, S, CI, CO, step = case
        x, w, b, truth = (BC.valid_case if valid else BC.dilated_case)(*case)
        So = SC.v_out_side(S, step) if valid else S
        wp = ops.pack_conv3x3d(f32(w))
        nws = query(*case)
        form = BC.form_of(entry, case)
        # (bias, relu, act_domain, offsets): with a bias and raw (negative values survive); at the smallest case also bias NULL + ReLU and the variants
        for bias, relu, dom, offsets in [(True, 0, 0, False)] + ([(False, 1, 0, False), (True, 0, 0, True), (True, 0, 1, False)] if i == 0 else []):
            k = _scale() if dom else 1.0
            want = truth if bias else truth - b.double().view(1, CO, 1, 1)
            want = f32(nhwc(torch.relu(want) if relu else want))
            ins = dict(x=f32(nhwc(x)) * k, wpacked=wp, bias=f32(b) * k if bias else None)
            call = lambda P, g: fn(P("x"), P("wpacked"), P("bias"), P("out"), P("ws"), g.nbytes("ws"), B, S, CI, CO, step, relu, dom, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(out=(B, So, So, CO)), dict(ws=nws), call, dict(out=want), offsets, 1.0 / k,
                               f"bias {'given' if bias else 'NULL'} relu {relu} domain {dom}")
            t.add(entry, form, found)
    t.done()


def test_conv3x3d_buffers(dev):
    _dilated_or_valid(dev, False)


def test_conv3x3v_buffers(dev):
    _dilated_or_valid(dev, True)


def test_conv3x3v_dgrad_buffers(dev):
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_conv3x3v_dgrad_f32"
    t = Tally(entry)
    for i, case in enumerate(sorted(BC.DGRAD, key=lambda c: c[0] * c[1] * c[1] * c[2] * c[3])):
        B, S, CI, CO = case
        x, w, dy, gx, _ = BC.train_case(*case)
        wt = ops.pack_conv3x3d(TC.w_dgrad(f32(w)))                                  # the mode-1 stream: what the host packer writes for w'
        exp = torch.tensor([TC.grad_exponent(f32(dy))], dtype=torch.int32)
        nws = lib.hdn_conv3x3v_dgrad_workspace_bytes(*case)
        form = BC.form_of(entry, case)
        for offsets in [False] + ([True] if i == 0 else []):
            ins = dict(dy=f32(nhwc(dy)), wpacked_t=wt, exp=exp)
            call = lambda P, g: lib.hdn_conv3x3v_dgrad_f32(P("dy"), P("wpacked_t"), P("exp"), P("gx"), P("ws"), g.nbytes("ws"), B, S, CI, CO, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(gx=(B, S, S, CI)), dict(ws=nws), call, dict(gx=f32(nhwc(gx))), offsets)
            t.add(entry, form, found)
    t.done()


def test_conv3x3v_wgrad_and_grad_scale_buffers(dev):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry, scale = "hdn_conv3x3v_wgrad_f32", "hdn_grad_scale_f32"
    t, ts = Tally(entry), Tally(scale, workspace=False)
    for i, case in enumerate(sorted(BC.WGRAD, key=lambda c: c[0] * c[1] * c[1] * c[2] * c[3])):
        B, S, CI, CO = case
        x, w, dy, _, gw = BC.train_case(*case)
        e = TC.grad_exponent(f32(dy))
        exp = torch.tensor([e], dtype=torch.int32)
        nws = lib.hdn_conv3x3v_wgrad_workspace_bytes(*case)
        form = BC.form_of(entry, case)
        for offsets in [False] + ([True] if i == 0 else []):
            ins = dict(x=f32(nhwc(x)), dy=f32(nhwc(dy)), exp=exp)
            call = lambda P, g: lib.hdn_conv3x3v_wgrad_f32(P("x"), P("dy"), P("exp"), P("gw"), P("ws"), g.nbytes("ws"), B, S, CI, CO, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(gw=(CO, CI, 3, 3)), dict(ws=nws), call, dict(gw=f32(gw)), offsets)
            t.add(entry, form, found)
            n = dy.numel()
            call = lambda P, g: lib.hdn_grad_scale_f32(P("g"), n, P("exp_out"), s)
            found, _ = guarded(dev, scale, case, f"n={n}", dict(g=f32(nhwc(dy))), dict(exp_out=((1,), torch.int32)), {}, call,
                               dict(exp_out=torch.tensor([e], dtype=torch.int32)), offsets)
            ts.add(scale, "one", found)
    t.done()
    ts.done()


# ----------------------------------------------------------------------------------------------------------------- the two 7x7 first stages
def test_simi_stem_buffers(dev):
    """(No domain-1 variant: hdn_simi_stem_f32 answers HDN_E_SHAPE for act_domain != 0.)"""
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_simi_stem_f32"
    t = Tally(entry, workspace=False)
    for S in [7] + SC.STEM_TILING_SIZES:
        x3, w, b, want3 = BC.simi_stem_case(3, S)
        wp = ops.pack_simi_stem(f32(w))
        _, Sp = SC.stem_sides(S)
        for B in (1, 3):
            assert (B, S) in BC.SIMI_STEM
            for offsets in [False] + ([True] if (B, S) == (1, 7) else []):
                call = lambda P, g: lib.hdn_simi_stem_f32(P("x"), P("wpacked"), P("bias"), P("out"), B, S, 0, s)
                found, _ = guarded(dev, entry, (B, S), f"Sc={SC.stem_sides(S)[0]}", dict(x=f32(x3[:B]), wpacked=wp, bias=f32(b)), dict(out=(B, Sp, Sp, 64)), {},
                                   call, dict(out=f32(nhwc(want3[:B]))), offsets)
                t.add(entry, f"Sc={SC.stem_sides(S)[0]}", found)
    t.done()


def test_trunk_stem_mfma_buffers(dev):
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_trunk_stem_mfma_f32"
    t = Tally(entry, workspace=False)
    w, ci, ky, kx = T.stem_onehot()
    wp, bi = ops.pack_stem_mfma(w), T.bias_int(64)
    xi = _codes((max(BC.TRUNK_STEM), 2, 127, 127))
    want = T.stem_expected(xi, ci, ky, kx, bi)
    for B in BC.TRUNK_STEM:
        for dom, offsets in [(0, False)] + ([(0, True), (1, False)] if B == 1 else []):
            k = _scale() if dom else 1.0
            call = lambda P, g: lib.hdn_trunk_stem_mfma_f32(P("x"), P("wfrag"), P("bias"), P("out"), B, 127, 127, dom, s)
            found, _ = guarded(dev, entry, (B, 127), "127", dict(x=f32(xi[:B]), wfrag=wp, bias=f32(bi)), dict(out=(B, 32, 32, 64)), {}, call,
                               dict(out=f32(nhwc(want[:B]))), offsets, 1.0 / k, f"out_domain {dom}")
            t.add(entry, "127 px", found)
    t.done()


# ----------------------------------------------------------------------------------------------------------------- the heads
def _nan_gaps(x, stride):
    """x [B, image] -> [B, stride] with 0xFF bytes (NaN) behind every image."""
    B, image = x.shape
    buf = torch.full((B, stride), -1, dtype=torch.int32).view(torch.float32)
    buf[:, :image] = x
    return buf


def test_head_conv3x3_buffers(dev):
    """hdn_head_conv3x3_f32: every level's input and output an operand of its own (the pointer tables' targets), NCHW and channels-last."""
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_head_conv3x3_f32"
    t = Tally(entry, workspace=False)
    for i, case in enumerate(BC.HEAD_CONV):
        Hi, Wi, n, CO = case
        xs, ws, bs, want = T.head_conv_case(Hi, Wi, n, CO)
        wp = ops._pack_conv_search(ws)
        for nh, offsets in [(0, False), (1, False)] + ([(0, True), (1, True)] if i == 0 else []):
            ins = {f"x{l}": f32(nhwc(xs[l]) if nh else xs[l]) for l in range(n)}
            ins.update(w_packed=wp, bias=f32(bs))
            outs = {f"out{l}": (CO, Hi - 2, Wi - 2) for l in range(n)}

            def call(P, g):
                xp = (ctypes.c_void_p * n)(*[P(f"x{l}").value for l in range(n)])
                op = (ctypes.c_void_p * n)(*[P(f"out{l}").value for l in range(n)])
                return lib.hdn_head_conv3x3_f32(xp, P("w_packed"), P("bias"), op, n, CO, Hi, Wi, nh, s)
            found, _ = guarded(dev, entry, case, f"nhwc={nh}", ins, outs, {}, call, {f"out{l}": f32(want[l]) for l in range(n)}, offsets)
            t.add(entry, f"nhwc={nh}", found)
    t.done()


def test_head_conv3x3_batch_buffers(dev):
    """hdn_head_conv3x3_batch_f32: dense images, and images x_batch_stride > 256 Hi Wi apart with NaN in the gaps; the one output buffer under guard."""
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_head_conv3x3_batch_f32"
    t = Tally(entry, workspace=False)
    small = {}
    for case in BC.HEAD_CONV_BATCH:
        small.setdefault(bool(case[6]), case)                     # the first case of either layout gets the variants
    for case in BC.HEAD_CONV_BATCH:
        Hi, Wi, n, B, CO, groups, nh = case
        nh = int(nh)
        xs, ws, bs, want = HB.exact_case(Hi, Wi, n, B, CO)
        wp = ops._pack_conv_search(ws)
        image, Ho, Wo = 256 * Hi * Wi, Hi - 2, Wi - 2
        want = f32(want.view(n, B, groups, CO // groups, Ho, Wo).permute(0, 2, 1, 3, 4, 5).contiguous())      # [n][groups][B][CO / groups][P]
        for gap, offsets in [(0, False)] + ([(64, False), (0, True)] if small[bool(nh)] == case else []):
            stride = image + gap
            ins = {f"x{l}": _nan_gaps(f32(nhwc(xs[l]) if nh else xs[l]).reshape(B, image), stride) for l in range(n)}
            ins.update(w_packed=wp, bias=f32(bs))

            def call(P, g):
                xp = (ctypes.c_void_p * n)(*[P(f"x{l}").value for l in range(n)])
                return lib.hdn_head_conv3x3_batch_f32(xp, P("w_packed"), P("bias"), P("out"), n, B, groups, CO, Hi, Wi, nh, stride, s)
            form = f"nhwc={nh} groups={groups}"
            found, _ = guarded(dev, entry, case, form, ins, dict(out=tuple(want.shape)), {}, call, dict(out=want), offsets, tag=f"x_batch_stride {stride}")
            t.add(entry, form, found)
    t.done()


def test_head_tail_buffers(dev):
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_head_tail_f32"
    t = Tally(entry, workspace=False)
    for i, case in enumerate(BC.HEAD_TAIL):
        H, P_, n, om = case
        feats, w1, b1, wf, bf, want = T.head_tail_case(H, P_, n, om)
        ins = dict(feats=f32(feats), w1_packed=ops._pack_w1(w1), b1=f32(b1), wf=wf, bf=f32(bf))
        for offsets in [False] + ([True] if i == 0 else []):
            call = lambda P, g: lib.hdn_head_tail_f32(P("feats"), P("w1_packed"), P("b1"), P("wf"), P("bf"), P("out"), n, H, P_, om, s)
            found, _ = guarded(dev, entry, case, f"H={H}", ins, dict(out=(2, om, P_)), {}, call, dict(out=f32(want)), offsets)
            t.add(entry, f"H={H}", found)
    t.done()


def test_head_tail_batch_buffers(dev):
    """hdn_head_tail_batch_f32: the buffer is [B][oc][P] ++ [B][ol][P] and not a float more - rows o >= n_out[br] do not exist in it, so a write to
    one lands in the margin or in the other branch's rows."""
    from hdn_amd import ops
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_head_tail_batch_f32"
    t = Tally(entry, workspace=False)
    smallest = min(BC.HEAD_TAIL_BATCH, key=lambda c: c[0] * c[1] * c[2] * c[5])
    for case in BC.HEAD_TAIL_BATCH:
        H, P_, n, oc, ol, B = case
        feats, w1, b1, wf, bf, want = HT.exact_case(*case)
        ins = dict(feats=f32(feats), w1_packed=ops._pack_w1(w1), b1=f32(b1), wf=wf, bf=f32(bf))
        flat = torch.cat([f32(want[0]).reshape(-1), f32(want[1]).reshape(-1)])
        for offsets in [False] + ([True] if case == smallest else []):
            call = lambda P, g: lib.hdn_head_tail_batch_f32(P("feats"), P("w1_packed"), P("b1"), P("wf"), P("bf"), P("out"), n, B, H, P_, oc, ol, s)
            form = f"H={H} oc={oc} ol={ol}"
            found, _ = guarded(dev, entry, case, form, ins, dict(out=(B * (oc + ol) * P_,)), {}, call, dict(out=flat), offsets)
            t.add(entry, form, found)
    t.done()


# ----------------------------------------------------------------------------------------------------------------- the epilogue and the regressor's tail
def test_bias_relu_buffers(dev):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_bias_relu_f32"
    t = Tally(entry, workspace=False)
    for i, case in enumerate(BC.BIAS_RELU):
        B, C, HW, nh = case
        y, b, r, want_res, want = BC.bias_relu_case(*case)
        n = B * C * HW
        form = ("vector" if BC.bias_relu_vector(*case) else "scalar") + (" nhwc" if nh else " nchw") + (" loop" if n > BC.BIAS_RELU_GRID[BC.bias_relu_vector(*case)] else "")
        for residual, offsets in [(True, False), (False, False)] + ([(True, True)] if i < 4 else []):
            ins = dict(bias=f32(b), residual=f32(r) if residual else None)
            call = lambda P, g: lib.hdn_bias_relu_f32(P("y"), P("bias"), P("residual"), B, C, HW, nh, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(y=f32(y)), {}, call, dict(y=f32(want_res if residual else want)), offsets,
                               tag=f"residual {residual}")
            t.add(entry, form, found)
    t.done()


def test_avgpool_fc_buffers(dev):
    L = _L()
    lib, s = L.load(), L.stream_ptr(dev)
    entry = "hdn_avgpool_fc_f32"
    t = Tally(entry, workspace=False)
    smallest = min(BC.AVGPOOL_FC, key=lambda c: c[0] * c[1] * c[2])
    for case in BC.AVGPOOL_FC:
        B, C, HW, O, nh = case
        x, w, b, want = BC.avgpool_fc_case(*case)
        form = f"nhwc={nh} O={O}"
        for bias, dom, offsets in [(True, 0, False), (False, 0, False)] + ([(True, 0, True), (True, 1, False)] if case == smallest else []):
            k = _scale() if dom else 1.0
            ins = dict(x=f32(x) * k, w=f32(w), bias=f32(b) if bias else None)
            call = lambda P, g: lib.hdn_avgpool_fc_f32(P("x"), P("w"), P("bias"), P("out"), B, C, HW, O, nh, dom, s)
            found, _ = guarded(dev, entry, case, form, ins, dict(out=(B, O)), {}, call, dict(out=f32(want if bias else want - b.double())), offsets,
                               tag=f"bias {'given' if bias else 'NULL'} in_domain {dom}")
            t.add(entry, form, found)
    t.done()
