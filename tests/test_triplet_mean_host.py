"""Host side of tests/test_gpu_triplet_mean.py: the fp32 restatement of tests/triplet_mean_cases.py lies inside the bound on every case, each
mutation leaves it on at least one, the division order shows in the bits of its fixtures, the seeds leave no row out of the gradient comparison; the
two entry points exist in the library, the header and the binding (ABI still 10) and refuse in the documented order (made-up addresses: nothing is
launched); hdn_amd.triplet_l1_mean and HomoModelBuilder.training_forward(host_free=True) refuse as documented.  No GPU, no kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import triplet_cases as TC
import triplet_mean_cases as MC
from hdn_amd import triplet_l1_mean, triplet_l1_mean_backward  # noqa: F401  (the module is about them: without them nothing here is collected)

E_NULL, E_SHAPE, E_LIMIT, E_ALIAS = -1, -2, -3, -4
NEW = {"hdn_triplet_l1_mean_f32": 16, "hdn_triplet_l1_mean_bwd_f32": 17}


@pytest.mark.parametrize("name", MC.NAMES)
def test_restatement_is_inside_the_bound(name):
    c = MC.CASES[name]
    t = c.truth()
    got = MC.restate32(c)
    assert got.dtype == np.float32
    ratio = MC.check_value(c, got, (t["n_sel"], t["n_neg"]), "fp32 restatement")
    print(f"TRIPLET_MEAN {name}: n_sel {t['n_sel']} n_neg {t['n_neg']} used rows {t['rows']} value64 {t['value']:.9g} bound {t['bound']:.3g} "
          f"fp32 |err| / bound {ratio:.3f} rows left out {t['excluded']}")
    assert t["excluded"] == 0                                                # these seeds leave no row out of the gradient comparison ...
    assert t["excluded"] <= MC.EXCLUDED_CAP * max(t["rows"], 1)              # ... and the cap holds in any case
    assert np.isfinite(float(got))                                           # the NaN-filled samples are unused ones


def test_the_cases_cover_what_they_claim():
    seen = {(c.N, c.R) for c in MC.CASES.values()} , {c.D for c in MC.CASES.values()}
    assert set(MC.SHAPES) <= seen[0] and set(MC.DS) <= seen[1]
    by = lambda pred: [c for c in MC.CASES.values() if pred(c, c.truth())]
    assert by(lambda c, t: t["n_sel"] == c.N and c.N > 1)                                            # all selected
    assert by(lambda c, t: t["n_sel"] == 0 and t["n_neg"] > 0) and by(lambda c, t: t["n_sel"] == 0 and t["n_neg"] == 0)
    assert by(lambda c, t: t["n_sel"] == 1 and c.N > 2 and bool(t["used"][0]) and t["used"].sum() == 1)    # only the first
    assert by(lambda c, t: t["n_sel"] == 1 and c.N > 2 and bool(t["used"][-1]) and t["used"].sum() == 1)   # only the last
    assert by(lambda c, t: bool((c.if_pos == 0.5).any()) and 0 < t["n_sel"] < c.N)
    quirk = by(lambda c, t: c.rule == 1 and t["n_neg"] == 0 and 0 < t["n_sel"] < c.N)
    assert quirk and all(t["used"].all() for t in (c.truth() for c in quirk))                        # every sample summed, n_sel the divisor
    nan = by(lambda c, t: bool(torch.isnan(c.a).any()))
    assert nan and all(not torch.isnan(c.a[torch.from_numpy(c.truth()["used"])]).any() for c in nan)
    for rule in (0, 1):
        assert by(lambda c, t: c.rule == rule and 0 < t["n_sel"] < c.N and t["n_neg"] > 0)


@pytest.mark.parametrize("variant", MC.MUTATIONS)
def test_mutations_leave_the_bound(variant):
    outside = []
    for c in MC.CASES.values():
        t = c.truth()
        bad = float(MC.restate32(c, variant))
        if abs(bad - t["value"]) > t["bound"]:
            outside.append(c.name)
    print(f"TRIPLET_MEAN mutation {variant}: outside the bound on {len(outside)} of {len(MC.CASES)} cases")
    assert outside, variant


def test_the_division_order_shows_in_the_bits_of_its_fixtures():
    vals = {}
    for name in MC.ORDER_CASES:
        c = MC.CASES[name]
        good, bad = MC.restate32(c), MC.restate32(c, "div_order")
        assert good.tobytes() != bad.tobytes(), name                           # ... while both are inside the bound: only the bits tell
        t = c.truth()
        assert abs(float(bad) - t["value"]) <= t["bound"] and abs(float(good) - t["value"]) <= t["bound"]
        assert c.exact and t["n_sel"] == 3
        vals[c.rule] = good
    assert vals[0].tobytes() != vals[1].tobytes()                              # rule 0 divides by denom first, rule 1 by n_sel


# ------------------------------------------------------------------------------------------------------------------------------------ ABI surface
def test_symbols_in_the_library_the_header_and_the_binding():
    from hdn_amd import _lib as L
    lib = L.load()
    assert lib.hdn_abi_version() == L.ABI_VERSION == 10                        # symbols are only added
    with open(os.path.join(TC.ROOT, "include", "hdn_hip.h")) as f:
        header = f.read()
    assert "#define HDN_ABI_VERSION 10" in header
    for name, nargs in NEW.items():
        assert hasattr(lib, name) and name in L.SIGNATURES
        res, args = L.SIGNATURES[name]
        assert len(args) == nargs and res is ctypes.c_int
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs
        assert args[-1] is ctypes.c_void_p and "void* stream" in decl.group(1).split(",")[-1]
        assert [a is ctypes.c_float for a in args[-4:-1]] == [True] * 3
        assert all(s in decl.group(1) for s in ("int rule", "float denom", "float margin", "float eps", "const float* if_pos", "const float* if_unsup"))
    for name in ("hdn_triplet_l1_f32", "hdn_triplet_l1_bwd_f32"):               # the row kernels' entry points are what they were
        assert hasattr(lib, name) and len(L.SIGNATURES[name][1]) == {"hdn_triplet_l1_f32": 12, "hdn_triplet_l1_bwd_f32": 15}[name]
    for text in ("sel: fp32(if_pos[b] if_unsup[b]) == 1", "neg: if_pos[b] == 0", "out = (S / denom) / n_sel", "out = (S / n_sel) / denom",
                 "its own quirk", "n_sel == 0 gives out = 0", "divides by zero under rule 1", "is not read", "no float atomics",
                 "c = (grad_out / denom) / n_sel", "c = (grad_out / n_sel) / denom", "N > 65536", "rule outside {0, 1}"):
        assert text in header, text
    import hdn_amd
    assert hdn_amd.triplet_l1_mean is hdn_amd.triplet.triplet_l1_mean and hdn_amd.triplet_l1_mean_backward is hdn_amd.triplet.triplet_l1_mean_backward
    import __graft_entry__ as G
    assert G.HIP_SOURCES.count("triplet_loss.hip") == 1                        # the build list is what it was: the kernels live in the same source


def test_validation_codes_in_order():
    """Made-up host addresses: every call here is refused before a launch.  NULL -> -1, shape -> -2, limits -> -3, aliases -> -4."""
    from hdn_amd import _lib as L
    lib = L.load()
    a = [ctypes.c_void_p(v << 34) for v in range(1, 14)]
    tail = (16129.0, 1.0, 1e-6, None)
    ok = (3, 5, 7, 0)
    # ---- forward: anchor, positive, negative, if_pos, if_unsup, partial, out, counts | N R D rule | denom margin eps
    f = lib.hdn_triplet_l1_mean_f32
    ptrs = a[:8]
    for i in range(8):
        q = list(ptrs)
        q[i] = None
        assert f(*q, *ok, *tail) == E_NULL and f(*q, 0, 5, 7, 0, *tail) == E_NULL, i                  # NULL before shape
    for k in range(3):
        dims = list(ok)
        dims[k] = 0
        assert f(*ptrs, *dims, *tail) == E_SHAPE, dims
        assert f(*ptrs[:5], a[0], a[6], a[7], *dims, *tail) == E_SHAPE                                # shape before alias
    for rule in (-1, 2):
        assert f(*ptrs, 3, 5, 7, rule, *tail) == E_SHAPE and f(*ptrs, 65537, 5, 7, rule, *tail) == E_SHAPE   # shape before limit
    for denom in (0.0, -1.0, float("nan")):
        assert f(*ptrs, *ok, denom, 1.0, 1e-6, None) == E_SHAPE
    assert f(*ptrs, 65537, 1, 7, 0, *tail) == E_LIMIT and f(*ptrs, 65537, 1, 7, 1, *tail) == E_LIMIT
    assert f(*ptrs, 65536, 1 << 15, 7, 0, *tail) == E_LIMIT                                           # N R > 2^30
    assert f(*ptrs, 3, 5, (1 << 20) + 1, 0, *tail) == E_LIMIT
    assert f(*ptrs[:5], a[0], a[6], a[7], 3, 5, (1 << 20) + 1, 0, *tail) == E_LIMIT                   # limit before alias
    for i in range(5):                                                                               # an output on an input
        for o in range(3):
            q = list(ptrs)
            q[5 + o] = a[i]
            assert f(*q, *ok, *tail) == E_ALIAS, (i, o)
    assert f(*ptrs[:5], a[5], a[5], a[7], *ok, *tail) == E_ALIAS and f(*ptrs[:5], a[5], a[6], a[6], *ok, *tail) == E_ALIAS   # outputs on each other
    assert f(*ptrs[:5], a[5], a[6], ctypes.c_void_p((6 << 34) + 3 * 5 * 4 - 4), *ok, *tail) == E_ALIAS  # counts on the last float of partial
    assert f(a[0], a[0], a[0], *ptrs[3:], 3, 5, 7, 2, *tail) == E_SHAPE                               # the inputs may alias each other
    # ---- backward: anchor, positive, negative, if_pos, if_unsup, grad_out | ga gp gn | N R D rule | denom margin eps
    f = lib.hdn_triplet_l1_mean_bwd_f32
    ins = a[:6]
    for i in range(6):
        q = list(ins)
        q[i] = None
        assert f(*q, a[6], a[7], a[8], *ok, *tail) == E_NULL and f(*q, None, None, None, 0, 5, 7, 0, *tail) == E_NULL, i
    assert f(*ins, None, None, None, *ok, *tail) == E_SHAPE                                           # no gradient asked for
    for k in range(3):
        dims = list(ok)
        dims[k] = 0
        assert f(*ins, a[0], a[7], a[8], *dims, *tail) == E_SHAPE, dims
    assert f(*ins, a[6], a[7], a[8], 3, 5, 7, 2, *tail) == E_SHAPE
    assert f(*ins, a[6], a[7], a[8], 65537, 1, 7, 1, *tail) == E_LIMIT
    assert f(*ins, a[0], a[7], a[8], 3, 5, (1 << 20) + 1, 0, *tail) == E_LIMIT
    for ga, gp, gn in ((a[0], a[7], a[8]), (a[6], a[1], a[8]), (a[6], a[7], a[2]), (a[3], None, None), (None, a[4], None), (None, None, a[5]),
                       (a[6], a[6], None), (a[6], None, a[6]), (None, a[7], a[7])):
        assert f(*ins, ga, gp, gn, *ok, *tail) == E_ALIAS, (ga, gp, gn)


# ------------------------------------------------------------------------------------------------------------------------------------ Python layer
def test_python_refusals():
    import hdn_amd
    from hdn_amd import _lib
    a, p, n = torch.zeros(2, 3, 7), torch.zeros(2, 3, 7), torch.zeros(2, 3, 7)
    fp, fu = torch.ones(2), torch.ones(2)
    with pytest.raises(_lib.HdnHipError):                                                             # CPU tensors: no fallback
        hdn_amd.triplet_l1_mean(a, p, n, fp, fu, 0)
    with pytest.raises(_lib.HdnHipError):
        hdn_amd.triplet_l1_mean(a.clone().requires_grad_(True), p, n, fp, fu, 1)
    with pytest.raises(_lib.HdnHipError):
        hdn_amd.triplet_l1_mean_backward(a, p, n, fp, fu, torch.ones(1), 0)
    for bad in ((fp.clone().requires_grad_(True), fu), (fp, fu.clone().requires_grad_(True))):
        with pytest.raises(ValueError, match="no gradient"):                                          # before any device check
            hdn_amd.triplet_l1_mean(a, p, n, *bad, 0)
    for rule in (2, -1, None, 0.5):
        with pytest.raises(ValueError, match="rule"):
            hdn_amd.triplet_l1_mean(a, p, n, fp, fu, rule)
    for flags in ((torch.ones(3), fu), (fp, torch.ones(2, 1)), (fp, torch.ones(()))):
        with pytest.raises(ValueError):
            hdn_amd.triplet_l1_mean(a, p, n, *flags, 0)
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1_mean(a, torch.zeros(2, 3, 8), n, fp, fu, 0)                                # no broadcasting
    with pytest.raises(ValueError, match="denom"):
        hdn_amd.triplet_l1_mean(a, p, n, fp, fu, 0, denom=0)
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1_mean_backward(a, p, n, fp, fu, torch.ones(1), 0, need_anchor=False, need_positive=False, need_negative=False)
    with pytest.raises(ValueError):
        hdn_amd.triplet_l1_mean_backward(a, p, n, fp, fu, torch.ones(2), 0)


def test_training_forward_host_free_needs_device_flags():
    import inspect

    import hdn_amd
    from hdn_amd import _lib
    net = hdn_amd.HomoModelBuilder().train()
    sig = inspect.signature(net.training_forward)
    assert sig.parameters["host_free"].default is False                                               # today's path is the default
    B = 2
    data = {"org_imgs": torch.zeros(B, 2, 127, 127), "input_tensors": torch.zeros(B, 2, 127, 127), "h4p": torch.zeros(B, 8),
            "patch_indices": torch.zeros(B, 127 * 127)}
    with pytest.raises(KeyError, match="if_pos"):
        net.training_forward(data, host_free=True)
    data["if_pos"] = torch.ones(B)
    with pytest.raises(KeyError, match="if_unsup"):
        net.training_forward(data, host_free=True)
    data["if_unsup"] = torch.ones(B, 1, 127, 127)
    with pytest.raises(ValueError, match="if_unsup"):
        net.training_forward(data, host_free=True)
    data["if_unsup"] = torch.ones(B)
    with pytest.raises(_lib.HdnHipError):                                                             # flags and images on the host: no upload, no fallback
        net.training_forward(data, host_free=True)
    net.eval()
    with pytest.raises(RuntimeError, match="ShareFeature.*eval.*hip_train"):                          # the refusal of the default path holds here too
        net.training_forward(data, host_free=True)
