"""Host side of tests/test_gpu_share_feature_forms.py: the exact PreShareFeature fixture is exact and clips at every ReLU, and the case tables of
tests/share_feature_cases.py reach every strip height, every end of a strip and every tile edge.  No GPU, no kernel."""
import pytest
import torch

import share_feature_cases as SC


@pytest.mark.parametrize("shape", [(SC.SWEEP_B, 26, 128), (2, 9, 257), (2, 127, 127)])
def test_fixture_is_exact_in_fp32(shape):
    """The fp32 and the float64 chain agree bit for bit, every partial sum in ANY order fits fp32 (headroom), the parameter block holds the fixture's
    scales and shifts where include/hdn_hip.h puts them, and all of it is what the docstring says: small integers and powers of two."""
    ws, alpha, beta, folded = SC.exact_params()
    x = SC.exact_image(*shape)
    assert x.shape == (shape[0], 1, shape[1], shape[2]) and x.dtype == torch.float32
    assert torch.equal(x, x.round()) and float(x.min()) == -3 and float(x.max()) == 3
    for w in ws:
        assert torch.equal(w, w.round()) and float(w.min()) == -2 and float(w.max()) == 2
    assert set(SC.SCALE_EXPS) <= {2, 3, 4, 5} and all(isinstance(s, int) for s in SC.SHIFTS)
    assert torch.equal(folded[SC.SF_ALPHA:SC.SF_ALPHA + 13].double(), alpha) and torch.equal(folded[SC.SF_BETA:].double(), beta)
    assert torch.equal(folded[:SC.SF_ALPHA], folded[:SC.SF_ALPHA].round()) and float(folded[:SC.SF_ALPHA].abs().max()) == 2
    r64 = SC.reference64(x, (ws, alpha, beta, folded))
    r32 = SC.chain(x, ws, alpha, beta, dtype=torch.float32)
    assert r32.dtype == torch.float32 and torch.equal(r32, r64.float()) and torch.equal(r32.double(), r64)
    head = SC.exactness_headroom(x, (ws, alpha, beta, folded))
    print(f"SHARE_FEATURE exact fixture {shape}: largest partial-sum bound = {head:.3e} of fp32's 2^24 quanta, output max {float(r64.max()):.4f}")
    assert head < 1.0 / 16
    assert float(r64.max()) > 1.0                     # outputs of order 1, as the real module's


@pytest.mark.parametrize("shape", [(SC.SWEEP_B, 26, 33), (SC.SWEEP_B, 5, 3), (2, 9, 257), (2, 127, 127)])
def test_every_relu_clips_a_share_of_the_fixture(shape):
    """A condition on the fixture: between 10 % and 90 % of the values in front of each ReLU are negative (a ReLU that never or always clips would
    hide a wrong sign or a wrong shift), at a small, a tiny, a wide and the production size."""
    shares = SC.clip_shares(SC.exact_image(*shape), SC.exact_params())
    print(f"SHARE_FEATURE clip shares {shape}: " + ", ".join(f"{s:.3f}" for s in shares))
    lo, hi = SC.CLIP_SHARE
    assert (lo, hi) == (0.10, 0.90) and len(shares) == 3 and all(lo <= s <= hi for s in shares), shares


def test_ones_fixture_counts_paths():
    """All-ones weights: the output counts the paths from the one bright pixel, 4 x 8 channel routes for each of the 3-step walks of a king that may
    stand still: 9^3 walks in all, 49 of them back at the centre, the 7 x 7 box reached."""
    ws, alpha, beta, folded = SC.ones_params()
    x = torch.zeros(1, 1, 9, 9)
    x[0, 0, 4, 4] = 1
    y = SC.reference64(x, (ws, alpha, beta, folded))
    assert float(y.sum()) == 9 ** 3 * 32 and int((y != 0).sum()) == 49 and float(y[0, 0, 4, 4]) == 32 * 49
    assert torch.equal(folded[:SC.SF_ALPHA + 13], torch.ones(SC.SF_ALPHA + 13)) and not folded[SC.SF_BETA:].any()


def test_strip_rows_restates_the_launch_rule():
    """strip_rows against the sentences of the launch rule (csrc/share_feature.hip, launch_sf_rows), and PROD + N16 reach every strip height."""
    assert SC.strip_rows(1, 1024) == 1 and SC.strip_rows(1, 1025) == 2 and SC.strip_rows(8, 128) == 1 and SC.strip_rows(1025, 1) == 2
    assert SC.strip_rows(48, 127) == 2 and SC.strip_rows(49, 127) == 4        # 48 x 64 = 3072 waves fit, 49 x 64 do not
    assert SC.strip_rows(96, 127) == 4 and SC.strip_rows(97, 127) == 8
    assert SC.strip_rows(65535, 3) == 4 and SC.strip_rows(65535, 127) == 128  # stops once a strip holds the image
    got = [SC.strip_rows(B, H) for B, H, _ in SC.PROD + SC.N16]
    assert got == SC.PROD_N + SC.N16_N, got
    assert set(got) == {1, 2, 4, 8, 16}
    assert [B for B, _, _ in SC.PROD] == [1, 8, 9, 47, 64, 128] and all((H, W) == (127, 127) for _, H, W in SC.PROD)
    B, H, W = SC.N16[1]
    assert SC.strip_rows(B, H) >= H and B * -(-H // (SC.strip_rows(B, H) // 2)) > 3072   # the loop ended on n >= H, not on the wave count
    assert all(W <= SC.ROWS_MAX_W and 1 <= B <= 65535 for B, _, W in SC.PROD + SC.N16)


@pytest.mark.parametrize("n", SC.FORCED_N)
def test_sweep_reaches_every_strip_end(n):
    """For a forced strip height n the sweep's heights hold every (H mod 3, length of the last strip) with the length in 1 .. min(n, 3), a strip whose
    condition-free rounds are cut by the image's last row (rb + 2 > H - 1) and one cut by the strip's own end (rb + 2 <= H - 1); over all heights every
    strip length 1 .. n occurs, and so every residue mod 3 of it that n allows (the exit round3 leaves a strip by)."""
    hs = SC.SWEEP_H + SC.SWEEP_H_TALL
    assert SC.SWEEP_H == tuple(range(1, 27))
    seen = {(H % 3, SC.strips(n, H)[-1][1] - SC.strips(n, H)[-1][0]) for H in hs}
    want = {(m, l) for m in range(3) for l in range(1, min(n, 3) + 1)}
    assert want <= seen, sorted(want - seen)
    all_strips = [(ra, rb, H) for H in hs for ra, rb in SC.strips(n, H)]
    assert any(rb + 2 > H - 1 for _, rb, H in all_strips) and any(rb + 2 <= H - 1 for _, rb, H in all_strips)
    assert {rb - ra for ra, rb, _ in all_strips} == set(range(1, n + 1))
    assert any(ra > 0 and rb < H for ra, rb, H in all_strips) or n >= 16      # a strip with a neighbour on both sides (16 rows: 35 < 3 x 16)
    for H in hs:                                                              # strips() tiles the image
        s = SC.strips(n, H)
        assert s[0][0] == 0 and s[-1][1] == H and all(a[1] == b[0] for a, b in zip(s, s[1:])) and all(0 < rb - ra <= n for ra, rb in s)


def test_sweep_widths_sit_on_the_lane_boundaries():
    """A lane holds two columns, a DPP row 16 lanes, a wave 64: widths on both sides of 32, 64 and 128 columns, both parities, and the smallest."""
    assert SC.SWEEP_W == (1, 2, 3, 31, 32, 33, 63, 64, 65, 126, 127, 128) and max(SC.SWEEP_W) == SC.ROWS_MAX_W
    assert len(SC.sweep_sizes()) == len(set(SC.sweep_sizes())) == (26 + len(SC.SWEEP_H_TALL)) * 12


def test_tile_cases_sit_on_the_tile_edges():
    """The W > 128 kernel works on 4 x 128 tiles: a width on each side of every 128-column edge the list reaches, a height on each side of a 4-row edge,
    an image lower than one tile, B = 2."""
    ws = sorted({W for _, _, W in SC.TILE})
    hs = sorted({H for _, H, _ in SC.TILE})
    assert ws == [129, 130, 255, 256, 257, 384, 385] and hs == [1, 3, 4, 5, 8, 9] and len(SC.TILE) == 42
    assert all(B == 2 and W > SC.ROWS_MAX_W for B, _, W in SC.TILE)
    for edge in range(SC.TILE_COLS, max(ws), SC.TILE_COLS):                    # 128 (only wider images come here: 129 is its far side), 256, 384
        assert any(W == edge + 1 for W in ws) and (edge == SC.TILE_COLS or any(W in (edge - 1, edge) for W in ws)), edge
    for edge in range(SC.TILE_ROWS, max(hs), SC.TILE_ROWS):                    # 4, 8
        assert edge - 1 in hs or edge in hs, edge
        assert edge in hs and edge + 1 in hs, edge
    assert 3 in hs and 5 in hs


def test_bright_pixels_lie_in_the_image():
    for H, W in SC.BRIGHT_SIZES:
        pts = SC.bright_pixels(H, W)
        assert all(0 <= r < H and 0 <= c < W for r, c in pts) and {(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0)} <= set(pts)
        assert any(c in (63, 64) for _, c in pts) and any(r in (7, 8) for r, _ in pts)
    assert SC.BRIGHT_SIZES == [(13, 127), (26, 128), (9, 257)]
