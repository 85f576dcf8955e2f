"""CPU tests of the batched head tail's host side (tests/test_gpu_head_tail_batch.py runs the kernel): hdn_head_tail_batch_f32 in the ABI, its argument
validation (every code, from host pointers: nothing is launched), the LDS formula of hdn_amd.heads against the library's, the documented output offset
and the exact case's expectation against float64 products, the HDN_HIP_HEADS level and the tail-fits predicate."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import head_tail_batch_cases as HT
from head_tail_batch_cases import E_ALIAS, E_LIMIT, E_NULL, E_SHAPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hdn_head_tail_batch_f32"
ARGS = ("const float* feats, const void* w1_packed, const float* b1, const float* wf, const float* bf, float* out, "
        "int n_levels, int B, int hidden, int pixels, int n_out_cls, int n_out_loc, void* stream")


# ----------------------------------------------------------------------------------------------------------------- ABI
def test_batch_entry_is_exported_declared_and_bound():
    from hdn_amd import _lib
    lib = _lib.load()
    assert lib.hdn_abi_version() == 10 == _lib.ABI_VERSION          # symbols are only added
    assert hasattr(lib, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 13 and args[-1] is ctypes.c_void_p and all(a is ctypes.c_int for a in args[6:12])
    header = open(os.path.join(ROOT, "include", "hdn_hip.h")).read()
    assert f"int {NAME}({ARGS});" in re.sub(r"\s+", " ", header)
    guard = header[header.index("Range guard of the two-fp16-piece kernels"):]
    assert NAME in guard[:guard.index("*/")]
    for line in ("ban.py:60-66", "ban.py:113-127", "ban_lp.py:77-92"):   # the reference lines it replaces, in its own comment
        doc = header[:header.index(f"int {NAME}(")]
        assert line in doc[doc.rindex("/*"):]


# ----------------------------------------------------------------------------------------------------------------- validation
def _call(n=2, B=3, H=128, P=5, oc=2, ol=4, feats="ok", w="ok", b1="ok", wf="ok", bf="ok", out="ok", w_off=0, out_at=None, tiny=False):
    """hdn_head_tail_batch_f32 on HOST memory.  Every call made here must be refused by the validation, which runs before the first HIP call and
    reads none of the buffers (tiny: they are not even allocated in full, for a case that is refused on its sizes).  out_at: `out` that many floats
    from the start of feats (may be negative: the buffer has 128 floats in front)."""
    from hdn_amd import _lib
    lib = _lib.load()
    pos = lambda v: max(v, 1)
    buf = torch.zeros(136 if tiny else 128 + 2 * pos(n) * pos(B) * pos(H) * pos(P) + 8)
    fbuf = buf[128:]
    wbuf, small = torch.zeros(1024), torch.zeros(8 * 4 * 256 * 2)
    obuf = torch.zeros(8 if tiny else pos(B) * (pos(oc) + pos(ol)) * pos(P))
    o = obuf.data_ptr() if out_at is None else fbuf.data_ptr() + 4 * out_at
    arg = lambda what, p: None if what is None else p
    return lib.hdn_head_tail_batch_f32(arg(feats, fbuf.data_ptr()), arg(w, wbuf.data_ptr() + w_off), arg(b1, small.data_ptr()), arg(wf, small.data_ptr()),
                                       arg(bf, small.data_ptr()), arg(out, o), n, B, H, P, oc, ol, None)


def test_validation_null():
    for name in ("feats", "w", "b1", "wf", "bf", "out"):
        assert _call(**{name: None}) == E_NULL, name


def test_validation_shape():
    for name in ("n", "B", "H", "P", "oc", "ol"):
        for v in (0, -1):
            assert _call(**{name: v}) == E_SHAPE, (name, v)


def test_validation_limit():
    cases = [{"n": 5}, {"oc": 9}, {"ol": 9}, {"H": 192}, {"H": 64}, {"H": 512},
             {"B": 65536, "n": 1, "P": 1, "tiny": True},                      # grid z
             {"n": 4, "B": 4096, "H": 256, "P": 1024, "tiny": True},          # 2^33 elements of feats
             {"n": 1, "B": 65535, "H": 128, "P": 129, "tiny": True},          # 2^31 + 2^25 - ...: just above 2^31 - 1
             {"n": 4, "H": 256, "oc": 2, "ol": 8},                            # the staged operands: 176,128 bytes of LDS
             {"w_off": 4}, {"w_off": 8}]                                      # the stream must be 16-byte aligned
    assert 2 * 65535 * 128 * 129 > 2 ** 31 - 1 > 2 * 65535 * 128 * 127
    for kw in cases:
        assert _call(**kw) == E_LIMIT, kw


def test_validation_alias_and_the_order_of_the_checks():
    total = 2 * 2 * 3 * 128 * 5                                               # _call's default feats
    n_out = 3 * (2 + 4) * 5
    for at in (0, 1, total - 1, -1, -n_out + 1):                              # out starting inside feats, or ending inside it
        assert _call(out_at=at) == E_ALIAS, at
    # (n, H, om) = (4, 256, 2) passes every size check (151,552 bytes of LDS): it gets as far as the alias check, which is the last one before the
    # stream is touched; om = 8 is refused for its LDS before that
    assert _call(n=4, H=256, oc=2, ol=2, out_at=0) == E_ALIAS
    assert _call(n=4, H=256, oc=2, ol=8, out_at=0) == E_LIMIT
    assert _call(n=0, H=192, out_at=0) == E_SHAPE and _call(n=0, feats=None) == E_NULL


def test_lds_formula_is_the_librarys():
    from hdn_amd import _lib, heads
    lib = _lib.load()
    for H in (128, 256):
        for n in range(1, 5):
            for om in range(1, 9):
                assert lib.hdn_head_tail_lds_bytes(n, H, om) == heads._tail_lds_bytes(n, H, om), (n, H, om)
    assert heads._tail_lds_bytes(4, 256, 8) == 176128 > 160 * 1024 >= heads._tail_lds_bytes(4, 256, 2) == 151552
    assert lib.hdn_head_tail_lds_bytes(5, 256, 2) == E_LIMIT and lib.hdn_head_tail_lds_bytes(3, 192, 2) == E_LIMIT
    assert lib.hdn_head_tail_lds_bytes(3, 256, 9) == E_LIMIT and lib.hdn_head_tail_lds_bytes(0, 256, 2) == E_SHAPE


# ----------------------------------------------------------------------------------------------------------------- the output layout
def test_output_offset_formula_against_float64():
    """The documented offset, written once (head_tail_batch_cases.out_offset), against float64 baddbmm reshaped to [B][oc][P] ++ [B][ol][P], for
    oc != ol and B = 3; with B = 1 and oc == ol it is hdn_head_tail_f32's [2, n_out, P]."""
    H, P, n, oc, ol, B = 128, 7, 2, 2, 4, 3
    feats, w1, b1, wf, bf = (t.double() for t in HT.random_case(H, P, n, oc, ol, B, seed=13))
    ref = HT.tail(feats, w1, b1, wf, bf)                                      # [B, 2, om, P]
    flat = HT.scatter_by_offset(ref, oc, ol)
    assert not torch.isnan(flat).any()                                        # every element written once: the map is onto
    want = torch.cat([ref[:, 0, :oc].reshape(-1), ref[:, 1, :ol].reshape(-1)])
    assert torch.equal(flat, want)
    c, l = HT.split_views(flat, B, oc, ol, P)
    assert torch.equal(c, ref[:, 0, :oc]) and torch.equal(l, ref[:, 1, :ol])
    one = HT.tail(feats[:, :1], w1, b1, wf[:, :2], bf[:, :2])                 # B = 1, oc == ol == 2
    assert torch.equal(HT.scatter_by_offset(one, 2, 2), one[0].reshape(-1))


@pytest.mark.parametrize("case", [(128, 33, 4, 8, 1, 2), (256, 25, 3, 2, 4, 3)], ids=HT.case_id)
def test_exact_case_expectation_is_the_two_products(case):
    """The integer expectation of the GPU addressing test against float64 baddbmm on every image, independently of any kernel."""
    H, P, n, oc, ol, B = case
    feats, w1, b1, wf, bf, (wc, wl) = HT.exact_case(*case)
    ref = HT.tail(feats.double(), w1.double(), b1.double(), wf.double(), bf.double())
    assert torch.equal(ref[:, 0, :oc], wc.double()) and torch.equal(ref[:, 1, :ol], wl.double())
    assert not ref[:, 0, oc:].any() and not ref[:, 1, ol:].any()              # zero rows above n_out[br]
    assert all((wf[br, o] != 0).sum() == 8 for br, rows in enumerate((oc, ol)) for o in range(rows))
    assert not torch.equal(wc[0], wc[1]) and not torch.equal(feats[0, 0], feats[0, 1]) and not torch.equal(feats[0, 0], feats[1, 0])
    assert int(ref.abs().max()) < 1 << 24


# ----------------------------------------------------------------------------------------------------------------- the switch
def test_hip_heads_level_parses_the_environment_once(monkeypatch):
    from hdn_amd import heads
    for text, level in (("", 0), ("0", 0), ("1", 1), ("2", 2)):
        monkeypatch.setenv("HDN_HIP_HEADS", text)
        monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
        assert heads.hip_heads_level() == level, text
    monkeypatch.delenv("HDN_HIP_HEADS")
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
    assert heads.hip_heads_level() == 0                                       # default off
    monkeypatch.setenv("HDN_HIP_HEADS", "2")
    assert heads.hip_heads_level() == 0                                       # read once


def test_attribute_overrides_the_level_and_hip_heads_is_unchanged(monkeypatch):
    from hdn_amd import heads

    class Head:
        pass
    h = Head()
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", 2)
    assert heads._hip_heads_level_of(h) == 2
    for v, level in ((True, 1), (1, 1), (2, 2), (False, 0), (0, 0)):
        h._hdn_hip_heads = v
        assert heads._hip_heads_level_of(h) == level and heads._hip_heads_on(h) is bool(v), v
    monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", 0)
    h._hdn_hip_heads = None
    assert heads._hip_heads_level_of(h) == 0
    # hip_heads(): a bool, true for every level above 0, read once, independent of the level's cache
    for text, on in (("", False), ("0", False), ("1", True), ("2", True)):
        monkeypatch.setenv("HDN_HIP_HEADS", text)
        monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
        assert heads.hip_heads() is on, text
    monkeypatch.setenv("HDN_HIP_HEADS", "0")
    assert heads.hip_heads() is True


def test_one_switch_two_readings(monkeypatch):
    """HDN_HIP_HEADS and head._hdn_hip_heads, each as (on, level), written out; on is level >= 1 everywhere."""
    from hdn_amd import heads

    def env(text):
        monkeypatch.setenv("HDN_HIP_HEADS", text)
        monkeypatch.setattr(heads, "_HIP_HEADS_LEVEL", None)
        monkeypatch.setattr(heads, "_HIP_HEADS", None, raising=False)          # (a second cache, where a version of the module has one)
        return heads.hip_heads(), heads.hip_heads_level()
    for text, want in (("", (False, 0)), ("0", (False, 0)), ("1", (True, 1)), ("2", (True, 2)), (" 2 ", (True, 2)), ("yes", (True, 1)), ("3", (True, 1)),
                       (" 0", (False, 0))):                                     # " 0": "0" after strip(), off in both readings
        got = env(text)
        assert got == want and got[0] is (got[1] >= 1), (text, got)

    class Head:
        pass
    h = Head()
    for text, unset in (("0", (False, 0)), ("2", (True, 2))):
        env(text)
        for v, want in ((None, unset), (False, (False, 0)), (0, (False, 0)), (True, (True, 1)), (1, (True, 1)), (2, (True, 2)), (3, (True, 1))):
            h._hdn_hip_heads = v
            got = heads._hip_heads_on(h), heads._hip_heads_level_of(h)
            assert got == want and got[0] is (got[1] >= 1), (text, v, got)


# ----------------------------------------------------------------------------------------------------------------- the predicate
def _head(cls_name, channels):
    from hdn_amd import heads
    torch.manual_seed(3)
    m = getattr(heads, cls_name)([channels] * 3, 2, weighted=True).eval()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.2, 0.2)
            mod.running_var.uniform_(0.8, 1.2)
    return m


@pytest.mark.parametrize("cls_name,channels", [("MultiBAN", 256), ("MultiCircBAN", 256), ("MultiBAN", 128), ("MultiCircBAN", 128)])
def test_tail_fits_accepts_the_reference_heads(cls_name, channels):
    from hdn_amd import heads
    m = _head(cls_name, channels)
    with torch.no_grad():
        pk = heads._pack_head(m, [m.box2, m.box3, m.box4])
    assert pk.hidden == channels and (pk.oc, pk.ol) == (2, 4 if cls_name == "MultiCircBAN" else 2)
    assert heads._tail_fits(3, pk.hidden, max(pk.oc, pk.ol), pk.w1)
    assert pk.w1p is None                                                     # ... but the stream is only packed for a GPU


def test_tail_fits_refuses():
    from hdn_amd import heads
    w = torch.full((6, 4, 4), 0.5)
    assert heads._tail_fits(3, 256, 4, w) and heads._tail_fits(4, 256, 2, w) and heads._tail_fits(4, 128, 8, w)
    assert not heads._tail_fits(3, 192, 4, w)                                 # hidden
    assert not heads._tail_fits(3, 256, 9, w)                                 # out rows
    assert not heads._tail_fits(5, 256, 2, w)                                 # levels
    assert not heads._tail_fits(4, 256, 8, w)                                 # LDS
    big = w.clone()
    big[3, 1, 2] = -65504.0
    assert not heads._tail_fits(3, 256, 4, big)                               # beyond fp16 after folding
    big[3, 1, 2] = float("nan")
    assert not heads._tail_fits(3, 256, 4, big)
    m = _head("MultiBAN", 256)
    m.box3.loc.head[0].weight.data[7, 9, 0, 0] = 7e4
    with torch.no_grad():
        pk = heads._pack_head(m, [m.box2, m.box3, m.box4])
    assert not heads._tail_fits(3, pk.hidden, 2, pk.w1)


def test_level_two_on_cpu_tensors_is_the_module_path(monkeypatch):
    """Whatever the predicate refuses falls back silently: CPU tensors at level 2 give the module path's result, and the new wrapper is not reached."""
    from hdn_amd import heads
    from oracle import hdn_oracle as O

    def boom(*a, **k):
        raise AssertionError("head_tail_batch reached")
    monkeypatch.setattr(heads, "head_tail_batch", boom)
    monkeypatch.setattr(heads, "xcorr_depthwise_multi", lambda srch, kern, circular=False, outs=None: [O.xcorr_depthwise(s, k) for s, k in zip(srch, kern)])
    g = torch.Generator().manual_seed(1)
    z = [torch.randn(2, 256, 5, 5, generator=g) for _ in range(3)]
    x = [torch.randn(2, 256, 7, 7, generator=g) for _ in range(3)]
    m = _head("MultiBAN", 256)
    want = m(z, x)
    heads.invalidate_template_cache(m)
    m._hdn_hip_heads = 2
    got = m(z, x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
