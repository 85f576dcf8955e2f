"""Host side of tests/test_gpu_xcorr_bwd.py: the two entry points of csrc/xcorr_bwd.hip exist in the library, the header and the binding (ABI still 10),
every validation code of hdn_xcorr_depthwise_bwd_f32 is provoked with made-up addresses (nothing is launched), hdn_xcorr_bwd_form agrees with the
restated 60 KiB rule on both sides of it, the exact fixtures are exact in fp32 (computed), the position closed forms equal float64 autograd, and the
reference's own functions under fp32 CPU autograd give the helper's float64 gradients on the integer fixtures.  No GPU, no kernel."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

import xcorr_bwd_cases as BC
import xcorr_cases as XC

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
REFERENCE_XCORR = "/root/reference/hdn/core/xcorr.py"


def _lib():
    from hdn_amd import _lib as L
    return L


def test_symbols_in_the_library_the_header_and_the_binding():
    """hdn_xcorr_depthwise_bwd_f32 and hdn_xcorr_bwd_form: exported, declared, bound with the declared argument lists; the ABI is still 10; the header
    carries the formulas and the reference lines; the Python wrapper is exported."""
    L = _lib()
    lib = L.load()
    assert lib.hdn_abi_version() == L.ABI_VERSION == 10
    with open(os.path.join(XC.ROOT, "include", "hdn_hip.h")) as f:
        header = f.read()
    assert "#define HDN_ABI_VERSION 10" in header
    for name, nargs in (("hdn_xcorr_depthwise_bwd_f32", 13), ("hdn_xcorr_bwd_form", 5)):
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs
    assert [a is ctypes.c_void_p for a in L.SIGNATURES["hdn_xcorr_depthwise_bwd_f32"][1]] == [True] * 5 + [False] * 7 + [True]
    for text in ("hdn/core/xcorr.py:37-61", "gk[u][v]  = sum_{i,j} gout[i][j] xp[i+u][j+v]", "gxp[P][Q] = sum_{u,v} gout[P-u][Q-v] k[u][v]",
                 "{r + ph - Hx, r + ph, r + ph + Hx}"):
        assert text in header, text
    import hdn_amd
    assert hdn_amd.xcorr_depthwise_backward is hdn_amd.xcorr.xcorr_depthwise_backward
    import __graft_entry__ as G
    assert "xcorr_bwd.hip" in G.HIP_SOURCES


def test_every_validation_code_in_order():
    """Made-up host addresses: every call here is refused before a launch.  NULL first, then the forward's shape rules, then aliases, then the plane
    limits; gx or gk alone may be NULL."""
    f = _lib().load().hdn_xcorr_depthwise_bwd_f32
    x, k, g, gx, gk = (ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4, 5))
    ok = (0, 2, 3, 29, 29, 5, 5, None)                      # circular, B, C, Hx, Wx, Hk, Wk, stream
    bad = (0, 2, 3, 5, 5, 6, 5, None)                       # taps taller than the plane: HDN_E_SHAPE
    big = (0, 1 << 15, 1 << 15, 29, 29, 5, 5, None)         # 2^30 planes: HDN_E_LIMIT (plane count)
    # 1. NULL, also where the shape is wrong and an output aliases
    for args in ((None, k, g, gx, gk), (x, None, g, gx, gk), (x, k, None, gx, gk), (x, k, g, None, None)):
        assert f(*args, *ok) == E_NULL and f(*args, *bad) == E_NULL, args
    assert f(None, k, g, k, gk, *ok) == E_NULL
    # 2. the forward's rules, before the alias check
    shape_cases = [((0, 0, 3, 29, 29, 5, 5), E_SHAPE), ((0, 2, -1, 29, 29, 5, 5), E_SHAPE), ((0, 2, 3, 0, 29, 5, 5), E_SHAPE),
                   ((0, 2, 3, 29, 29, 5, 0), E_SHAPE), ((0, 2, 3, 5, 5, 6, 5), E_SHAPE), ((0, 2, 3, 5, 5, 5, 6), E_SHAPE),
                   ((1, 2, 3, 5, 5, 10, 9), E_SHAPE), ((1, 2, 3, 5, 5, 9, 10), E_SHAPE),       # circular: 5 x 5 pads to 9 x 9
                   ((0, 1, 1, 4097, 8, 3, 3), E_LIMIT), ((1, 1, 1, 8, 4097, 3, 3), E_LIMIT)]
    for dims, want in shape_cases:
        assert f(x, k, g, gx, gk, *dims, None) == want, dims
        assert f(x, k, g, x, gk, *dims, None) == want, dims                                     # ... although gx aliases x
        assert f(x, k, g, gx, None, *dims, None) == want and f(x, k, g, None, gk, *dims, None) == want
    # 3. aliases, before the plane limits
    for args in ((x, k, g, x, gk), (x, k, g, k, gk), (x, k, g, g, gk), (x, k, g, gx, x), (x, k, g, gx, k), (x, k, g, gx, g), (x, k, g, gx, gx),
                 (x, k, g, x, None), (x, k, g, None, g)):
        assert f(*args, *ok) == E_ALIAS and f(*args, *big) == E_ALIAS, args
    # 4. the plane limits: B C > (2^31 - 1) / 4, or B C HP WP > 2^31 - 1
    assert f(x, k, g, gx, gk, *big) == E_LIMIT
    assert f(x, k, g, gx, None, 0, 1 << 10, 1 << 10, 64, 64, 5, 5, None) == E_LIMIT             # 2^20 planes of 2^12 floats
    assert f(x, k, g, None, gk, 1, 1 << 10, 1 << 10, 32, 32, 5, 5, None) == E_LIMIT             # circular: 32 x 32 pads to 64 x 64
    assert (1 << 10) * 511 * 64 * 64 < 2 ** 31                                                   # (one plane row fewer would have been launched)


def test_form_query_on_both_sides_of_the_switch():
    """hdn_xcorr_bwd_form = the restated rule on every shape of the tables; the four switch shapes sit at exactly 60 KiB and one float above it, plain
    and circular; bad shapes answer like the entry point."""
    q = _lib().load().hdn_xcorr_bwd_form
    for S in BC.SHAPES.values():
        assert q(int(S.circular), S.Hx, S.Wx, S.Hk, S.Wk) == BC.form(S), S
    floats = {}
    for S in BC.SWITCH:
        _, _, HP, WP, Ho, Wo = BC.geometry(S)
        floats[S.name] = HP * WP + S.Hk * S.Wk + Ho * Wo
    limit = BC.LDS_LIMIT_BYTES // 4
    assert [floats[n] for n in BC.SWITCH_KINDS] == [limit, limit + 1, limit, limit + 1]
    assert {(BC.form(S), S.circular) for S in BC.SWITCH} == {(0, False), (1, False), (0, True), (1, True)}
    assert all(BC.form(BC.SHAPES[n]) == BC.FORM_LDS for n in BC.EXACT_KINDS)
    # the production training shapes: 6.0 KB and 3.9 KB of LDS
    assert 4 * (29 * 29 + 25 + 25 * 25) == 5964 and 4 * (25 * 25 + 169 + 169) == 3852
    # the forward's generic kinds around ITS switch (two arrays) are all beyond this one's (three arrays) or not, by the rule
    for name in ("gen_123x124_12x9", "genc_61x62_89x4", "gen_123x124_109x1", "genc_62x62_5x1"):
        K = XC.KINDS[name]
        assert q(int(K.circular), K.Hx, K.Wx, K.Hk, K.Wk) == BC.form(BC.Shape(name, K.circular, K.Hx, K.Wx, K.Hk, K.Wk)) == BC.FORM_GLOBAL
    assert q(0, 5, 5, 6, 5) == E_SHAPE and q(1, 5, 5, 10, 9) == E_SHAPE and q(0, 0, 5, 1, 1) == E_SHAPE and q(0, 4097, 8, 3, 3) == E_LIMIT
    assert q(1, 5, 5, 9, 9) == 0 and q(0, 4096, 4096, 1, 1) == 1


def test_exact_fixtures_are_exact_in_fp32():
    """Every (kind, planes) of the exact GPU test: integers in [-3, 3] with all three values of sign present, float64 gradients that are integers, and the
    largest possible partial sum of either gradient (the backward on |x|, |k|, |g|) below 2^24 - computed per fixture, and its largest printed."""
    worst = {}
    for kind, P in BC.exact_table():
        S = BC.SHAPES[kind]
        x, k, g, gx, gk = BC.exact_problem(kind, P)
        _, _, _, _, Ho, Wo = BC.geometry(S)
        assert x.shape == gx.shape == (P, S.Hx, S.Wx) and k.shape == gk.shape == (P, S.Hk, S.Wk) and g.shape == (P, Ho, Wo)
        assert gx.dtype == gk.dtype == torch.float64
        for t in (x, k, g):
            assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) <= 3
        assert torch.equal(gx, gx.round()) and torch.equal(gk, gk.round())
        head = BC.exactness_headroom(x, k, g, S.circular)
        assert head < 2.0 ** -4, (kind, P, head)
        worst[kind] = max(worst.get(kind, 0.0), head)
    for kind, head in worst.items():
        print(f"XCORR-BWD exact fixture {kind}: largest possible |partial sum| = {head:.3e} of 2^24")


@pytest.mark.parametrize("kind", BC.POSITION_KINDS)
def test_position_closed_forms_equal_float64_autograd(kind):
    """One plane per output position: the index arithmetic of position_problem (no convolution) equals float64 autograd through direct_sum, every
    position is there once, and every expectation is exact in fp32."""
    S = BC.SHAPES[kind]
    x, k, g, want_gx, want_gk = BC.position_problem(kind)
    _, _, _, _, Ho, Wo = BC.geometry(S)
    P = Ho * Wo
    assert g.shape == (P, Ho, Wo) and torch.equal(g.reshape(P, P), torch.eye(P))
    gx, gk = BC.backward_ref(x, k, g, S.circular)
    assert torch.equal(want_gx, gx) and torch.equal(want_gk, gk)
    assert torch.equal(want_gx.float().double(), want_gx) and torch.equal(want_gk.float().double(), want_gk)
    assert float(want_gk.amin()) > 0 and float(want_gx.amax(dim=(1, 2)).min()) > 0
    # exact in any order: multiples of 2^-s that add up to far less than 2^24 of them
    s = 2.0 ** 8
    assert torch.equal(want_gx * s, (want_gx * s).round()) and float(want_gx.max()) * s < 2 ** 24


def test_reference_degenerate_rules_on_a_tiny_case():
    """(3, 1) circular with (2, 1) taps by hand: ph = 1, pw = 0, xp rows = x[2], x[0], x[1], x[2], x[0]; out[i] = xp[i] k0 + xp[i + 1] k1, i = 0..3."""
    x = torch.tensor([[[1.0], [2.0], [4.0]]])
    k = torch.tensor([[[3.0], [5.0]]])
    g = torch.tensor([[[1.0], [10.0], [100.0], [1000.0]]])
    gx, gk = BC.backward_ref(x, k, g, True)
    # gk0 = sum g[i] xp[i] = 4 + 10 + 200 + 4000; gk1 = sum g[i] xp[i + 1] = 1 + 20 + 400 + 1000
    assert gk.flatten().tolist() == [4214.0, 1421.0]
    # gxp[P] = g[P] k0 + g[P - 1] k1: [3, 35, 350, 3500, 5000]; x[0] <- P = 1, 4; x[1] <- P = 2; x[2] <- P = 0, 3
    assert gx.flatten().tolist() == [5035.0, 350.0, 3503.0]


@pytest.mark.skipif(not os.path.isfile(REFERENCE_XCORR), reason="reference tree only exists in the build container")
def test_reference_functions_under_fp32_autograd_give_the_same_integers():
    """The reference's own xcorr_depthwise / xcorr_depthwise_circular (hdn/core/xcorr.py:37-61) under fp32 CPU autograd on the integer fixtures:
    torch.equal to the helper's float64 gradients."""
    spec = importlib.util.spec_from_file_location("_reference_xcorr", REFERENCE_XCORR)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    seen = 0
    for kind in BC.EXACT_KINDS + BC.SWITCH_KINDS:
        S = BC.SHAPES[kind]
        P = 2 if kind in BC.SWITCH_KINDS else 3
        x, k, g, gx, gk = BC.exact_problem(kind, P)
        xr, kr = x.clone().unsqueeze(0).requires_grad_(True), k.clone().unsqueeze(0).requires_grad_(True)
        out = (ref.xcorr_depthwise_circular if S.circular else ref.xcorr_depthwise)(xr, kr)
        assert out.dtype == torch.float32 and out.shape[2:] == g.shape[1:]
        out.backward(g.unsqueeze(0))
        assert torch.equal(xr.grad[0].double(), gx) and torch.equal(kr.grad[0].double(), gk), kind
        seen += 1
    assert seen == len(BC.EXACT_KINDS) + 4


def test_stn_polar_drop_in_refuses_a_grad_carrying_input():
    """The reference's training forward (model_builder_e2e_unconstrained_v2.py:377-379) passes a polar that carries the first head's graph through
    STN_Polar, which is differentiable there.  The drop-in's kernel has no backward: with autograd recording it raises for an x or a polar that
    requires grad instead of detaching it - before any device check, so this runs on the CPU.  Under no_grad, and for plain inputs (the inference
    loops: a zero polar, an image crop), it goes on to the device check as before."""
    import hdn_amd
    from hdn_amd import _lib
    m = hdn_amd.STN_Polar(31)
    x, polar = torch.zeros(2, 3, 31, 31), torch.zeros(2, 2)
    w = torch.ones(2, 2, requires_grad=True)
    for args in ((x, polar * w), (x.clone().requires_grad_(True), polar)):
        with pytest.raises(RuntimeError, match="inference-only.*uninstall"):
            m(*args)
        with torch.no_grad(), pytest.raises(_lib.HdnHipError):             # not refused: reaches "runs on the GPU only"
            m(*args)
    with pytest.raises(_lib.HdnHipError):
        m(x, polar)
