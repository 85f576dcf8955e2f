"""tests/buffer_guard.py tested with no device: stand-in "kernels" (plain torch on the CPU, writing into the arena's views) of a K-split product,
one faultless and one per fault that tests/test_gpu_buffer_discipline.py is there to find.  The faultless one must give an empty verdict, every
faulty one a non-empty verdict, no two the same.  Then the helper's own arithmetic, the exact builders that the GPU file adds (against float64) and
the coverage of every launch form by the cases the GPU file runs (host queries of the library; nothing is launched)."""

import pytest
import torch

import buffer_guard as BG
from buffer_guard import Guard

M, C, S, T = 21, 8, 3, 8                      # rows, channels, K slices, rows per tile: the last tile has 5 rows


def _problem(margin=BG.DEFAULT_MARGIN, offsets=(0, 0, 0, 0), device="cpu"):
    """out[m][c] = sum_s ws[s][m][c] in slice order, ws[s][m][c] = x[m][c] * w[4 s] (a "weight stream" of S 16-byte words)."""
    x = ((torch.arange(M * C, dtype=torch.int64) * 7919) % 201 - 100).float().view(M, C)
    w = torch.arange(1, 4 * S + 1, dtype=torch.float32)
    g = Guard(device, margin)
    g.input("x", x, offsets[0])
    g.input("w", w, offsets[1])
    g.output("out", (M, C), offsets[2])
    g.workspace("ws", S * M * C * 4, offsets[3])
    want = (x.double() * w[::4].double().sum()).float()
    return g, want


def _kernel(fault=None):
    def call(g):
        x, w, out, ws = g.view("x"), g.view("w"), g.view("out"), g.view("ws").view(S, M, C)
        n_written = S - 1 if fault == "unwritten_slice" else S
        for s in range(n_written):
            ws[s] = x * w[4 * s]
        rows = M // T * T if fault == "partial_tile" else M
        acc = torch.zeros(M, C, device=x.device)
        for s in range(S):
            acc = acc + ws[s]
        if fault == "x_row_beyond":
            acc[M - 1] += g.window("x", after=C)[M * C:]
        if fault == "w_word_beyond":
            acc = acc + g.window("w", after=4)[4 * S:].sum()
        out[:rows] = acc[:rows]
        if fault == "row_past_end":
            g.window("out", after=C)[M * C:] = acc[0]
        if fault == "row_before_start":
            g.window("out", before=C)[:C] = acc[0]
        if fault == "slice_too_many":
            g.window("ws", after=M * C)[S * M * C:] = x.reshape(-1)
        if fault == "clobber_input":
            x[3, 1] = 0.0
        return 0
    return call


FAULTS = ("row_past_end", "row_before_start", "partial_tile", "slice_too_many", "unwritten_slice", "x_row_beyond", "w_word_beyond", "clobber_input")
# a word every verdict of that fault must carry: the fault is named for what it is, not merely noticed
MUST_SAY = {"row_past_end": "margin AFTER output 'out'", "row_before_start": "margin BEFORE output 'out'", "partial_tile": "left unwritten",
            "slice_too_many": "margin AFTER workspace 'ws'", "unwritten_slice": "read before", "x_row_beyond": "reads beyond that input",
            "w_word_beyond": "reads beyond that input", "clobber_input": "input 'x' changed"}


def test_faultless_standin_is_clean_and_right():
    g, want = _problem()
    assert g.run(_kernel()) == 0
    assert g.verdict() == []
    assert torch.equal(g.result("out"), want)
    assert len(g.rcs) == 2                                   # a NaN and a 1e30 workspace, nothing else when clean


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_is_reported(fault):
    g, want = _problem()
    g.run(_kernel(fault), want={"out": want})
    v = g.verdict()
    print(f"BUFFER GUARD {fault}: " + " | ".join(v))
    assert v, fault
    assert any(MUST_SAY[fault] in s for s in v), (fault, v)


def test_no_two_faults_are_reported_alike():
    texts = {}
    for fault in FAULTS:
        g, want = _problem()
        g.run(_kernel(fault), want={"out": want})
        texts[fault] = "\n".join(g.verdict())
    assert len(set(texts.values())) == len(FAULTS), texts
    # the reads beyond an input name the input
    assert "'x'" in texts["x_row_beyond"] and "'w'" not in texts["x_row_beyond"].split("margins of input")[1]
    assert "'w'" in texts["w_word_beyond"] and "'x'" not in texts["w_word_beyond"].split("margins of input")[1]
    # unwritten and computed NaN are told apart
    assert "kernel computed" not in texts["partial_tile"] and "left unwritten" not in texts["x_row_beyond"]
    # first offsets: the row past the end starts at byte 0 past the end, the row in front ends 1 byte in front
    assert "first at byte 0 past its end" in texts["row_past_end"]
    assert "the nearest 1 bytes in front" in texts["row_before_start"] and f"the farthest {4 * C}" in texts["row_before_start"]
    assert f"first flat index {M // T * T * C} = ({M // T * T}, 0)" in texts["partial_tile"]
    assert f"of {4 * M * C} (element {3 * C + 1})" in texts["clobber_input"]


def test_faults_are_found_at_loose_alignment_too():
    offs = BG.offsets16(4)
    for fault in (None,) + FAULTS:
        g, want = _problem(offsets=offs)
        g.run(_kernel(fault), want={"out": want})
        assert bool(g.verdict()) == (fault is not None), (fault, g.verdict())
        if fault is None:
            assert torch.equal(g.result("out"), want)


def test_layout_arithmetic():
    offs = BG.offsets16(4)
    assert len(set(offs)) == 4 and all(o % 16 == 0 and o % 64 != 0 and 0 < o < BG.LINE for o in offs)
    assert len(set(BG.offsets16(12))) == 12
    for margin in (BG.DEFAULT_MARGIN, 4096, 3 * 65536 + 16):
        g, _ = _problem(margin, offs)
        g.ptr("x")                                           # allocates
        g.check_layout()
        base = g.mem.data_ptr()
        assert base % BG.LINE == 0
        spans = []
        for (name, op), off in zip(g.ops.items(), offs):
            assert g.ptr(name).value == base + op.start and g.ptr(name).value % BG.LINE == off
            assert op.start - op.lo >= margin and op.hi - op.end >= margin
            assert op.end - op.start == g.nbytes(name)
            spans.append((op.lo, op.hi))
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[0][0] == 0 and spans[-1][1] == g.mem.numel()   # no shared margin
        assert g.mem.numel() >= 8 * margin                   # one allocation: 4 operands, 2 margins each
    assert BG.DEFAULT_MARGIN == 128 * 128 * 4                # one 128-pixel x 128-channel fp32 tile


def test_fill_patterns():
    g, _ = _problem()
    g._fill(None, BG.UNWRITTEN)
    for name, op in g.ops.items():
        edge = BG.IN_MARGIN if op.kind == "in" else BG.OUT_MARGIN
        assert bool((g.mem[op.lo:op.start] == edge).all()) and bool((g.mem[op.end:op.hi] == edge).all()), name
    assert bool(torch.isnan(g.view("out")).all()) and bool(torch.isnan(g.view("ws")).all())
    assert bool(torch.isnan(g.window("x", before=4)[:4]).all())                                      # 0xFF is NaN as fp32 ...
    assert bool(torch.isnan(g.mem[g.ops["x"].lo:g.ops["x"].lo + 8].view(torch.float16)).all())        # ... and as fp16
    g._fill(BG.WS_FINITE, BG.ALT_UNWRITTEN)
    assert bool((g.view("ws") == 1e30).all()) and bool(torch.isfinite(g.view("out")).all())


def test_workspace_is_handed_over_at_exactly_the_queried_size():
    for nbytes in (0, 4, 20, 4 * S * M * C, 65536 + 4):
        g = Guard("cpu")
        g.input("x", torch.zeros(4))
        g.workspace("ws", nbytes, 48)
        g.ptr("x")
        op = g.ops["ws"]
        assert g.nbytes("ws") == nbytes == op.end - op.start
        assert (g.ptr("ws") is None) == (nbytes == 0)        # no workspace: NULL
        g._fill(None, BG.UNWRITTEN)
        assert int(g.mem[op.end]) == BG.OUT_MARGIN and int(g.mem[op.start - 1]) == BG.OUT_MARGIN      # the margin starts at the next byte
        if nbytes:
            assert int(g.mem[op.end - 1]) == BG.UNWRITTEN
    # one byte (here: one float) beyond the queried size is a finding
    g = Guard("cpu")
    g.workspace("ws", 20)
    g.output("out", (1,))

    def call(g):
        g.window("ws", after=1)[:] = 1.0
        g.view("out")[0] = 1.0
        return 0
    g.run(call)
    assert any("margin AFTER workspace 'ws'" in s and "first at byte 0 past its end (its size: 20 bytes)" in s for s in g.verdict()), g.verdict()


def test_alignment_and_declaration_asserts():
    g = Guard("cpu")
    for bad in (8, 17, 256, -16, 16.0):
        with pytest.raises(AssertionError):
            g.input("x", torch.zeros(4), bad)
    g.input("x", torch.zeros(4), 240)
    with pytest.raises(AssertionError):
        g.input("x", torch.zeros(4))                         # twice
    with pytest.raises(AssertionError):
        g.workspace("ws", -2)                                # an error code is no size
    with pytest.raises(AssertionError):
        g.workspace("ws", 6)
    for bad in (0, -16, 1000, 65536.0):
        with pytest.raises(AssertionError):
            Guard("cpu", bad)
    g.ptr("x")
    with pytest.raises(AssertionError):
        g.output("late", (4,))                               # after the arena exists


def test_inplace_and_other_dtypes():
    g = Guard("cpu", 4096)
    g.inout("y", torch.arange(12, dtype=torch.float32).view(3, 4), 16)
    g.input("e", torch.tensor([7], dtype=torch.int32), 48)
    g.input("p", torch.arange(32, dtype=torch.uint8), 80)

    def call(g):
        assert int(g.view("e")[0]) == 7 and g.view("p").dtype == torch.uint8
        g.view("y").add_(1.0)
        return 0
    assert g.run(call) == 0 and g.verdict() == []
    assert torch.equal(g.result("y"), torch.arange(12, dtype=torch.float32).view(3, 4) + 1)

    def bad(g):
        g.window("y", before=1)[0] = 2.0
        g.view("e")[0] = 8
        return 0
    g.run(bad)
    v = g.verdict()
    assert any("margin BEFORE in-place operand 'y'" in s for s in v) and any("input 'e' changed" in s for s in v), v


def test_return_codes_are_kept():
    g, _ = _problem()
    assert g.run(lambda g: -3) == -3 and set(g.rcs) == {-3}
    assert any("left unwritten" in s for s in g.verdict())   # nothing ran: the whole output is still NaN, and says so


# ----------------------------------------------------------------------------------------------------------------- the GPU file's cases and builders
def test_buffer_cases_reach_every_form():
    """The cases tests/test_gpu_buffer_discipline.py runs reach every launch form of every entry point that has a query (host queries only)."""
    import buffer_discipline_cases as BC
    for entry, forms in BC.check_coverage().items():
        print(f"BUFFERS coverage {entry}: forms {forms}")


@pytest.mark.parametrize("case", [(3, 8, 20, 1), (3, 5, 20, 0), (3, 6, 15, 1), (3, 5, 15, 0)])
def test_bias_relu_builder_against_float64(case):
    import buffer_discipline_cases as BC
    B, C, HW, nhwc = case
    y, b, r, want_res, want = BC.bias_relu_case(*case)
    nchw = (lambda t: t.permute(0, 2, 1)) if nhwc else (lambda t: t)
    ref = nchw(y).double() + b.double().view(1, C, 1)
    assert torch.equal(nchw(want).double(), ref.clamp_min(0)) and torch.equal(nchw(want_res).double(), (ref + nchw(r).double()).clamp_min(0))
    assert int(max(want_res.max(), y.abs().max() + r.abs().max() + 100)) < 1 << 24
    assert int((want == 0).sum()) and int((want > 0).sum()) and int((want_res != want).sum())       # the ReLU and the residual both matter


def test_avgpool_fc_builder_against_float64():
    import buffer_discipline_cases as BC
    for case in BC.AVGPOOL_FC:
        B, C, HW, O, nhwc = case
        x, w, b, want = BC.avgpool_fc_case(*case)
        xn = x.permute(0, 2, 1) if nhwc else x                                  # [B, C, HW]
        ref = torch.nn.functional.linear(xn.double().mean(2), w.double(), b.double())
        assert torch.equal(want, ref), case
        assert torch.equal(want.float().double(), want) and float(want.abs().max()) * HW < 1 << 24, case
        assert len(want.unique()) > 1


def test_fast_integer_truths_equal_the_case_modules_own():
    """The float64 convolutions buffer_discipline_cases uses at the large cases give what the case modules' integer indexing gives, on the same data."""
    import buffer_discipline_cases as BC
    import conv3x3_train_cases as TC
    import simi_full_cases as SC
    for case in SC.V_EXACT[:2] + [(2, 3, 32, 32, 2), (3, 7, 96, 32, 1)]:
        x, w, b, want = SC.v_integer_problem(*case)
        x2, w2, b2, want2 = BC.valid_case(*case)
        assert torch.equal(x, x2) and torch.equal(w, w2) and torch.equal(b, b2) and torch.equal(want.double(), want2), case
        assert float(want2.abs().max()) < 1 << 24
    for case in TC.EXACT_CASES[:4]:
        x, w, dy, _, gx, gw = TC.integer_problem(*case)
        x2, w2, dy2, gx2, gw2 = BC.train_case(*case)
        assert torch.equal(x, x2) and torch.equal(w, w2) and torch.equal(dy, dy2), case
        assert torch.equal(gx.double(), gx2) and torch.equal(gw.double(), gw2), case
    for case in BC.DGRAD + BC.WGRAD:
        assert TC.integer_sum_limit(*case) < 1 << 24, case
    for B, S, CI, CO, d in BC.DIL + BC.VALID:
        assert 9 * CI * 4 * 2 + 9 < 1 << 24
    x, w, b, want = BC.dilated_case(2, 5, 32, 96, 2)
    g = torch.Generator().manual_seed(5 + 5)                                       # test_gpu_conv3x3d.py::test_conv3x3d_addressing_is_exact's draws
    assert torch.equal(x.float(), torch.randint(-4, 5, (2, 32, 5, 5), generator=g).float())
    for got, want in zip(BC.simi_stem_case_f64(2, 11), SC.stem_integer_problem(2, 11)):
        assert torch.equal(got, want)
    assert tuple(BC.simi_stem_case(3, 7)[3].shape) == (3, 64, 1, 1) and int(BC.simi_stem_case(3, 7)[3].max()) > 0
