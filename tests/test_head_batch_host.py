"""CPU tests of the batched head convolution's host side (tests/test_gpu_head_batch.py runs the kernel): hdn_head_conv3x3_batch_f32 in the ABI, its
argument validation (every code, from host pointers: nothing is launched), the documented output offset against a float64 convolution, the
template-branch predicate of hdn_amd.heads and the HDN_HIP_HEADS switch being off by default."""
import copy
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_batch_cases as HB
from head_batch_cases import E_ALIAS, E_LIMIT, E_NULL, E_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hdn_head_conv3x3_batch_f32"


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_batch_entry_is_exported_declared_and_bound():
    from hdn_amd import _lib
    lib = _lib.load()
    assert lib.hdn_abi_version() == 10 == _lib.ABI_VERSION          # symbols are only added
    assert hasattr(lib, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 13 and args[11] is ctypes.c_longlong
    header = open(os.path.join(ROOT, "include", "hdn_hip.h")).read()
    assert f"int {NAME}(const float* const* xs, const void* w_packed, const float* bias, float* out, int n, int B, int groups, int CO" in header
    guard = header[header.index("Range guard of the two-fp16-piece kernels"):]
    assert NAME in guard[:guard.index("*/")]


# ----------------------------------------------------------------------------------------------------------------- validation
def _call(n=2, B=3, groups=2, CO=64, Hi=7, Wi=7, nhwc=0, xbs=None, xs="ok", w="ok", bias="ok", out="ok", w_off=0, out_alias=None, tiny=False):
    """hdn_head_conv3x3_batch_f32 on HOST memory.  Every call made here must be refused by the validation, which runs before the first HIP call and
    reads none of the buffers (tiny: they are not even allocated in full, for a case that is refused on its sizes)."""
    from hdn_amd import _lib
    lib = _lib.load()
    image = 256 * max(Hi, 1) * max(Wi, 1)
    xbs = image if xbs is None else xbs
    keep = [torch.zeros(8 if tiny else max(B, 1) * max(xbs, image) + 8) for _ in range(max(n, 1))]
    wbuf, bbuf = torch.zeros(1024), torch.zeros(max(n, 1) * max(CO, 1))
    obuf = torch.zeros(8 if tiny else max(n, 1) * max(B, 1) * max(CO, 1) * max(Hi - 2, 1) * max(Wi - 2, 1))
    ptrs = [t.data_ptr() for t in keep]
    if xs == "null_level":
        ptrs[-1] = None
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    o = obuf.data_ptr() if out_alias is None else keep[out_alias[0]].data_ptr() + 4 * out_alias[1]
    return lib.hdn_head_conv3x3_batch_f32(None if xs is None else arr, None if w is None else wbuf.data_ptr() + w_off, None if bias is None else bbuf.data_ptr(),
                                          None if out is None else o, n, B, groups, CO, Hi, Wi, nhwc, xbs, None)


def test_validation_null():
    for kw in ({"xs": None}, {"w": None}, {"bias": None}, {"out": None}, {"xs": "null_level"}):
        assert _call(**kw) == E_NULL, kw


def test_validation_shape():
    for kw in ({"n": 0}, {"n": -1}, {"B": 0}, {"B": -2}, {"CO": 0}, {"CO": -64}, {"Hi": 2}, {"Wi": 2}, {"groups": 3}, {"groups": 0}):
        assert _call(**kw) == E_SHAPE, kw


def test_validation_limit():
    cases = [{"n": 5}, {"CO": 96, "groups": 2}, {"CO": 48, "groups": 1}, {"CO": 33, "groups": 2},
             {"Hi": 5, "Wi": 75},                       # 64 output pixels touch 2 output rows: 4 patch rows of 75 pixels > 224
             {"Hi": 50, "Wi": 50},                      # ... 3 output rows of 48: 5 patch rows of 50
             {"Hi": 3, "Wi": 80},                       # even one output row: 3 x 80
             {"n": 4, "B": 16384, "Hi": 3, "Wi": 3, "tiny": True},    # n B = 65536 > the grid's 65535
             {"w_off": 4},                              # the stream must be 16-byte aligned
             {"xbs": 256 * 7 * 7 - 1}, {"xbs": 0}, {"xbs": -256 * 7 * 7}]
    for kw in cases:
        assert _call(**kw) == E_LIMIT, kw


def test_validation_alias():
    image = 256 * 7 * 7
    for al in ((0, 0), (1, 0), (1, 2 * image + 5), (0, 3 * image - 1)):          # out starting anywhere inside an input's [B images]
        assert _call(out_alias=al) == E_ALIAS, al
    # out ending inside an input: it starts before level 0's first element
    from hdn_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64 + 3 * image)
    x = buf[64:]
    arr = (ctypes.c_void_p * 1)(x.data_ptr())
    w, b = torch.zeros(1024), torch.zeros(64)
    assert lib.hdn_head_conv3x3_batch_f32(arr, w.data_ptr(), b.data_ptr(), buf.data_ptr(), 1, 3, 2, 64, 7, 7, 0, image, None) == E_ALIAS


# ----------------------------------------------------------------------------------------------------------------- the output layout
@pytest.mark.parametrize("groups", [1, 2])
def test_output_offset_formula_against_float64(groups):
    """The documented offset, written once (head_batch_cases.out_offset), against a float64 conv2d + ReLU reshaped to [n][groups][B][CO / groups][P];
    n = 2, B = 3, CO = 64.  With B = 1 it is the [n, CO, Ho, Wo] flattening hdn_head_conv3x3_f32 writes."""
    n, B, CO, Hi, Wi = 2, 3, 64, 7, 6
    xs, ws, bs = HB.random_case(Hi, Wi, n, B, CO, seed=11)
    ref = torch.stack([HB.conv_relu(xs[i].double(), ws[i].double(), bs[i].double()) for i in range(n)])          # [n, B, CO, Ho, Wo]
    P = (Hi - 2) * (Wi - 2)
    flat = HB.scatter_by_offset(ref.reshape(n, B, CO, P), groups)
    want = ref.reshape(n, B, groups, CO // groups, P).permute(0, 2, 1, 3, 4).contiguous().reshape(-1)
    assert not torch.isnan(flat).any()                                           # every element written once: the map is onto
    assert torch.equal(flat, want)
    one = ref[:, :1].reshape(n, 1, CO, P)
    assert torch.equal(HB.scatter_by_offset(one, groups), one.reshape(-1))       # B = 1: [n, CO, Ho, Wo]


def test_exact_case_expectation_is_the_convolution():
    """The integer-indexed expectation of the GPU addressing test against a float64 convolution with the same one-hot weights, independently of any kernel."""
    xs, ws, bs, want = HB.exact_case(7, 9, 2, 3, 64)
    for l in range(2):
        ref = HB.conv_relu(xs[l].double(), ws[l].double(), bs[l].double())
        assert torch.equal(ref, want[l].double())
    assert not torch.equal(want[0], want[1]) and int(want.max()) <= 25 and int((want == 0).sum()) > 0


# ----------------------------------------------------------------------------------------------------------------- the predicate
def _head(cls_name="MultiBAN", channels=256):
    from hdn_amd import heads
    torch.manual_seed(3)
    m = getattr(heads, cls_name)([channels] * 3, 2, weighted=True).eval()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.8, 1.2)
    return m


def _boxes(m):
    return [m.box2, m.box3, m.box4]


@pytest.mark.parametrize("cls_name,S", [("MultiBAN", 7), ("MultiCircBAN", 15)])
def test_template_packable_accepts_the_reference_layout(cls_name, S):
    from hdn_amd import heads
    m = _head(cls_name)
    for B in (1, 3):
        z = [torch.zeros(B, 256, S, S) for _ in range(3)]
        assert heads._template_packable(_boxes(m), z, need_gpu=False)
        assert not heads._template_packable(_boxes(m), z)                        # fp32 on a GPU: the kernel has no CPU form
    zm = [torch.empty(2, 256, S, S, device="meta") for _ in range(3)]
    assert heads._template_packable(_boxes(copy.deepcopy(m).to("meta")), zm, need_gpu=False)


def test_template_packable_refuses():
    from hdn_amd import heads
    z = [torch.zeros(1, 256, 7, 7) for _ in range(3)]
    ok = lambda m, zz=z: heads._template_packable(_boxes(m), zz, need_gpu=False)
    m = _head()
    assert ok(m)
    m.box3.loc.conv_kernel[1].train()                                            # a BatchNorm in training mode cannot be folded
    assert not ok(m)
    m = _head()
    m.box2.cls.conv_kernel[0] = nn.Conv2d(256, 256, 3, bias=True)                # a biased convolution
    assert not ok(m)
    m = _head()
    m.box4.cls.conv_kernel[0] = nn.Conv2d(256, 256, 3, padding=1, bias=False)
    assert not ok(m)
    m = _head()
    m.box2.loc.conv_kernel = nn.Sequential(m.box2.loc.conv_kernel[0], m.box2.loc.conv_kernel[1], nn.Identity())
    assert not ok(m)
    assert not ok(_head(channels=128), [torch.zeros(1, 128, 7, 7) for _ in range(3)])          # 128 input channels
    assert not ok(_head(), [torch.zeros(1, 256, 7, 7), torch.zeros(1, 256, 7, 7), torch.zeros(1, 256, 9, 9)])   # levels of different shape
    assert not ok(_head(), [t.double() for t in z])
    assert not ok(_head(), [torch.zeros(1, 256, 50, 50) for _ in range(3)])                    # beyond the 224-pixel patch
    m = _head()
    m.box2.cls.conv_kernel[0].weight.data[3, 5, 1, 1] = 7e4                                    # beyond fp16 after folding
    assert not ok(m)
    m = _head()
    m.box2.cls.conv_search[1].train()                                            # conv_search is not the template branch's business
    assert ok(m)


# What the parent of the heads' untangling answered, case by case (head_batch_cases.stage_case on conv_kernel, a [1, 256, 5, 5] template): the layout
# predicate is shared with conv_search since, and its truth table did not move.  (A 17 x 17 map is inside the patch limit: 8 rows of 17 <= 224 pixels.)
TEMPLATE_PACKABLE = {"reference": True, "hidden48": False, "cin128": False, "two_shapes": False, "five_levels": False, "side17": True, "side50": False,
                     "bias": False, "stride2": False, "padding1": False, "dilation2": False, "groups2": False, "bn_training": False, "bn_not_affine": False,
                     "bn_no_running_stats": False, "identity": False, "length4": False, "weight7e4": False}


def test_template_packable_truth_table():
    from hdn_amd import heads
    assert list(TEMPLATE_PACKABLE) == HB.STAGE_CASES
    got = {}
    for name in HB.STAGE_CASES:
        m, boxes, z = HB.stage_case(name, "conv_kernel")
        got[name] = heads._template_packable(boxes, z, need_gpu=False)
    assert got == TEMPLATE_PACKABLE


# ----------------------------------------------------------------------------------------------------------------- the switch
def _cpu_forward(monkeypatch, m, B=1):
    """fused_forward on CPU tensors with the correlation launch replaced by the oracle's (the only step of the module path without a CPU form)."""
    from hdn_amd import heads
    from oracle import hdn_oracle as O
    monkeypatch.setattr(heads, "xcorr_depthwise_multi", lambda srch, kern, circular=False, outs=None: [O.xcorr_depthwise(s, k) for s, k in zip(srch, kern)])
    g = torch.Generator().manual_seed(1)
    z = [torch.randn(B, 256, 5, 5, generator=g) for _ in range(3)]
    x = [torch.randn(B, 256, 7, 7, generator=g) for _ in range(3)]
    return m(z, x)


def test_switch_is_off_by_default_and_the_wrapper_is_never_reached(monkeypatch):
    from hdn_amd import heads

    def boom(*a, **k):
        raise AssertionError("head_conv_batch reached with the switch off")
    monkeypatch.delenv("HDN_HIP_HEADS", raising=False)
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
    monkeypatch.setattr(heads, "head_conv_batch", boom)
    monkeypatch.setattr(heads, "_template_packable", lambda *a, **k: True)       # even where the predicate would say yes
    assert heads.hip_heads() is False
    for B in (1, 2):
        m = _head()
        c, l = _cpu_forward(monkeypatch, m, B)
        assert c.shape == (B, 2, 3, 3) and l.shape == (B, 2, 3, 3)
        assert getattr(m, "_hdn_template_pack", None) is None and getattr(m, "_hdn_search_pack", None) is None
    m = _head()
    m._hdn_hip_heads = False                                                     # the attribute overrides the environment, both ways
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", True)
    _cpu_forward(monkeypatch, m)


def test_switch_on_reaches_the_wrapper_and_refuses_cpu_tensors(monkeypatch):
    """The same forward with the switch on: the template branch goes to head_conv_batch, which has no CPU fallback."""
    from hdn_amd import heads, _lib
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", False)
    monkeypatch.setattr(heads, "_template_packable", lambda *a, **k: True)
    monkeypatch.setattr(heads, "_pack_conv_search", lambda ws: torch.zeros(1))   # (the packer itself is host code; its stream is not looked at here)
    orig = heads._pack_convs

    def pack_as_if_on_gpu(boxes, name):
        pk = orig(boxes, name)
        pk.wsp, pk.bsp = torch.zeros(1), torch.stack(pk.bs)
        return pk
    monkeypatch.setattr(heads, "_pack_convs", pack_as_if_on_gpu)
    m = _head()
    m._hdn_hip_heads = True
    with pytest.raises(_lib.HdnHipError, match="no CPU fallback"):
        _cpu_forward(monkeypatch, m)
    monkeypatch.setenv("HDN_HIP_HEADS", "1")
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
    assert heads.hip_heads() is True
    monkeypatch.setenv("HDN_HIP_HEADS", "0")
    assert heads.hip_heads() is True                                             # read once
