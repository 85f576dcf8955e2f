"""CPU tests beside tests/test_gpu_trunk50_forms.py: the hdn_pack_conv3x3s2_f32 stream decoded from its documented layout, and hdn_conv1x1_form
(the launch form of hdn_conv1x1_f32 for a problem) at hand-computed cases and on bad arguments.  No kernel is launched here."""
import numpy as np
import pytest
import torch

E_SHAPE, E_LIMIT = -2, -3


def cfg(NT, WM, WN, KW):
    """The value hdn_conv1x1_form gives for Cfg<NT, WM, WN, KW> (include/hdn_hip.h)."""
    return NT | WM << 8 | WN << 16 | KW << 24


@pytest.mark.parametrize("C", [128, 256, 512])
def test_pack_conv3x3s2_stream_decoded_by_its_documented_layout(C):
    """include/hdn_hip.h / csrc/pack.hip: [C/64][C/32 chunks][9 taps][2 n tiles][2 k steps][piece][k half g][32 n][8] fp16, element e of lane (g, n) =
    piece of w[64 nb + 32 nt + n][32 chunk + 16 k step + 8 g + e][tap].  Indexed so with numpy, piece 0 is fp16(w) and piece 1 is
    fp16((w - piece 0) 2^11) bit for bit at every (co, ci, tap), and p0 + 2^-11 p1 gives w back to 2^-21 relative (two pieces of 11 significand bits)
    wherever both pieces are normal fp16 numbers, |w| >= 2^-14.  Below that piece 0 is an fp16 subnormal and so may piece 1 be: a multiple of 2^-24
    each, so the rebuilt value is within 2^-25 x 2^-11 = 2^-36 ABSOLUTE of w (relative 2^-21 cannot hold for |w| < 2^-15: the format, not the
    packer).  He-scaled weights of this size have members of both classes; every element is under one of the two bounds."""
    from hdn_amd import trunk as T
    w = torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(C + 21)) * (2.0 / (9 * C)) ** 0.5
    stream = T.pack_conv3x3s2(w).numpy().view(np.float16)
    assert stream.size == 2 * 9 * C * C
    p = stream.reshape(C // 64, C // 32, 9, 2, 2, 2, 2, 32, 8)                 # (nb, chunk, tap, nt, ks, piece, g, n, e)
    p = p.transpose(0, 3, 7, 1, 4, 6, 8, 2, 5).reshape(C, C, 9, 2)            # (nb, nt, n | chunk, ks, g, e | tap | piece) = (co, ci, tap, piece)
    w9 = w.reshape(C, C, 9)
    p0 = w9.half()
    p1 = ((w9 - p0.float()) * 2048.0).half()
    got0, got1 = torch.from_numpy(p[..., 0].copy()), torch.from_numpy(p[..., 1].copy())
    for name, got, want in (("piece 0", got0, p0), ("piece 1", got1, p1)):
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
        if bad.shape[0]:
            raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements are not where the layout says; first (co, ci, tap) = {bad[0].tolist()}")
    back = got0.double() + got1.double() * 2.0 ** -11
    err, mag = (back - w9.double()).abs(), w9.double().abs()
    normal = mag >= 2.0 ** -14
    assert normal.any() and (~normal).any()
    worst = int(torch.argmax(torch.where(normal, err / mag.clamp_min(1e-300), torch.zeros_like(err))))
    co, ci, tap = np.unravel_index(worst, (C, C, 9))
    assert bool((err[normal] <= 2.0 ** -21 * mag[normal]).all()), ("worst (co, ci, tap):", (co, ci, tap), float(err[co, ci, tap]), float(mag[co, ci, tap]))
    assert float(err[~normal].max()) <= 2.0 ** -36, float(err[~normal].max())


def test_conv1x1_form_hand_computed():
    """hdn_conv1x1_form against the rule documented at the top of csrc/conv1x1.hip, worked out by hand (FILL = 512 workgroups):
    CO % 64 -> <1,4,1,1>; else WN = 4 / 2 / 1 by CO / 64 % 4 / % 2, workgroups = ceil(M / (32 (4 / WN))) (CO / 64 / WN); fewer than FILL and CI / 32 a
    multiple of 4 -> the small-M form <1,1,1,4>; else <2,1,4,1> / <2,2,2,1> / <2,4,1,1>."""
    from hdn_amd import _lib
    f = _lib.load().hdn_conv1x1_form
    # (B, S, CI, CO, stride)
    assert f(64, 32, 64, 64, 1) == cfg(2, 4, 1, 1)          # M = 65,536: 512 workgroups of 128 pixels, not below FILL (and 2 chunks: never small-M)
    assert f(1, 4, 2048, 512, 1) == cfg(1, 1, 1, 4)         # M = 16: 2 workgroups, 64 chunks
    assert f(3, 7, 64, 96, 1) == cfg(1, 4, 1, 1)            # CO = 96
    assert f(1, 3, 128, 96, 1) == cfg(1, 4, 1, 1)           # ... also where CI / 32 is a multiple of 4 and M = 9
    assert f(64, 32, 256, 128, 1) == cfg(2, 2, 2, 1)        # WN = 2: 65,536 / 64 = 1024 workgroups
    assert f(64, 32, 64, 256, 1) == cfg(2, 1, 4, 1)         # WN = 4: 2048 workgroups
    assert f(1, 32, 256, 64, 1) == cfg(1, 1, 1, 4)          # M = 1024: 8 workgroups, 8 chunks
    assert f(3, 7, 64, 64, 1) == cfg(2, 4, 1, 1)            # M = 147: 2 workgroups but 2 chunks
    assert f(3, 7, 64, 128, 2) == cfg(2, 2, 2, 1)           # stride 2 on an odd side: So = 4, M = 48
    assert f(5, 9, 64, 256, 2) == cfg(2, 1, 4, 1)           # So = 5, M = 125
    # the small-M -> large switch of (256 -> 128 @ 32): WN = 2, workgroups = ceil(1024 B / 64) = 16 B: 512 at B = 32
    assert f(31, 32, 256, 128, 1) == cfg(1, 1, 1, 4) and f(32, 32, 256, 128, 1) == cfg(2, 2, 2, 1)
    # (2048 -> 512 @ 4): WN = 4, workgroups = ceil(16 B / 32) 2 = B (B even): 512 at B = 511 (ceil(8176 / 32) = 256)
    assert f(510, 4, 2048, 512, 1) == cfg(1, 1, 1, 4) and f(511, 4, 2048, 512, 1) == cfg(2, 1, 4, 1)


def test_conv1x1_form_argument_errors():
    """It validates like hdn_conv1x1_f32: HDN_E_SHAPE / HDN_E_LIMIT for the same arguments, and the entry point (whose pointer checks come first
    only for NULL) answers the same for them."""
    import ctypes
    from hdn_amd import _lib
    lib = _lib.load()
    f = lib.hdn_conv1x1_form
    x, w, b, o = (ctypes.c_void_p(v << 34) for v in (1, 2, 3, 4))
    cases = [((0, 32, 64, 64, 1), E_SHAPE), ((-1, 32, 64, 64, 1), E_SHAPE), ((2, 0, 64, 64, 1), E_SHAPE), ((2, 32, 48, 64, 1), E_SHAPE),
             ((2, 32, 64, 80, 1), E_SHAPE), ((2, 32, 0, 64, 1), E_SHAPE), ((2, 32, 64, 0, 1), E_SHAPE), ((2, 32, 64, 64, 3), E_SHAPE),
             ((2, 32, 64, 64, 0), E_SHAPE), ((1 << 14, 32, 256, 64, 1), E_LIMIT),           # 2^32 input elements
             ((1 << 12, 32, 32, 1024, 1), E_LIMIT),                                          # 2^32 output elements
             ((1, 4, 64, 65536 + 64, 1), E_LIMIT)]                                           # CO > 65,536
    for args, want in cases:
        assert f(*args) == want, args
        B, S, CI, CO, stride = args
        assert lib.hdn_conv1x1_f32(x, w, b, None, o, B, S, CI, CO, stride, 1, 0, None) == want, args
    assert f(1, 4, 64, 65536, 1) > 0
    assert lib.hdn_abi_version() == 10
