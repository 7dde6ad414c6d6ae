"""The lane -> LDS address maps of the persistent 3x3 kernel's consumers (csrc/cn_conv3x3p.hip, lane_consts / step /
epilogue) in both MFMA shapes, and the swizzle the loaders apply through their source addresses, restated in plain
Python (CPU).

A halo row is one pixel's 32-channel chunk: 128 bytes = eight 16-byte slots, slot L = channels 8 (L & 3) .. + 7 of
the high (L < 4) or low part.  The loaders put slot L of halo row r at physical slot L ^ key(halo column of r), of
weight row n at L ^ ((n >> 1) & 7).  A ds_read_b128 is served in four groups of 16 lanes, one LDS cycle per group
when its 16 addresses fall into 16 distinct 16-byte units of the 256-byte bank row.

(a) every lane group of every fragment read -- form, tap offset, operand, high / low part, wave -- is conflict-free;
(b) the slot a consumer lane reads is the slot the MFMA layout wants there: physical = logical ^ the loader's key;
(c) the epilogue's accumulator -> (pixel, channel) map is the MFMA's D layout, a bijection onto the 64 x 32 wave
    tile, and the strip bytes it writes are exactly the bytes the row-layout pass reads back.
"""
import itertools
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_HW = 18
# lane groups of ds_read_b128 (one LDS cycle each when conflict-free)
_G0 = list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))
_G1 = list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))
GROUPS = [_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1]]
KEY16 = [0, 0, 1, 1, 2, 2, 4, 4, 5, 5, 6, 6, 2, 2, 6, 6, 0, 0]
# kx a form's steps take: nine taps 0 .. 2; stride 2 (parity planes) 0 .. 1; transposed t % 2 + parity 0 .. 2
FORM_KX = {"s1": (0, 1, 2), "s2": (0, 1), "deconv": (0, 1, 2)}


def halo_key(s16, hx):
    """p3_halo_key"""
    return (0x062654210 >> (4 * (hx >> 1))) & 7 if s16 else (hx >> 1) & 7


def weight_key(n):
    return (n >> 1) & 7


def halo_reads(s16, wm, ky, kx, key=None):
    """[(tag, [(byte address, logical slot, halo column)] per lane)] of one step's pixel fragments."""
    key = key or (lambda hx: halo_key(s16, hx))
    out = []
    if s16:
        for pb, part in itertools.product(range(4), range(2)):
            lanes = []
            for ln in range(64):
                px, sl = ln & 15, ln >> 4
                row = (4 * wm + pb + ky) * P_HW + px + kx
                lanes.append((row * 128 + ((((sl ^ key(px + kx)) & 7) << 4) ^ (part << 6)), sl + 4 * part, px + kx))
            out.append((("x", pb, part), lanes))
    else:
        for i, kh, part in itertools.product(range(2), range(2), range(2)):
            lanes = []
            for ln in range(64):
                l31, lh, px = ln & 31, ln >> 5, ln & 15
                row = (4 * wm + 2 * i + (l31 >> 4) + ky) * P_HW + px + kx
                lanes.append((row * 128 + ((((lh ^ key(px + kx)) & 7) << 4) ^ (kh << 5) ^ (part << 6)),
                              lh + 2 * kh + 4 * part, px + kx))
            out.append((("x", i, kh, part), lanes))
    return out


def weight_reads(s16, wn):
    out = []
    if s16:
        for cb, part in itertools.product(range(2), range(2)):
            lanes = []
            for ln in range(64):
                px, sl = ln & 15, ln >> 4
                n = 32 * wn + 16 * cb + px
                lanes.append(((32 * wn + px) * 128 + (((sl ^ ((px >> 1) & 7)) & 7) << 4) + cb * 2048 ^ (part << 6), sl + 4 * part, n))
            out.append((("w", cb, part), lanes))
    else:
        for kh, part in itertools.product(range(2), range(2)):
            lanes = []
            for ln in range(64):
                l31, lh = ln & 31, ln >> 5
                n = 32 * wn + l31
                lanes.append((n * 128 + ((((lh ^ ((l31 >> 1) & 7)) & 7) << 4) ^ (kh << 5) ^ (part << 6)), lh + 2 * kh + 4 * part, n))
            out.append((("w", kh, part), lanes))
    return out


def worst_conflict(lanes):
    """largest number of distinct addresses on one 16-byte unit within a lane group"""
    worst = 1
    for grp in GROUPS:
        units = {}
        for ln in grp:
            units.setdefault((lanes[ln][0] >> 4) & 15, set()).add(lanes[ln][0])
        worst = max(worst, max(len(v) for v in units.values()))
    return worst


def test_the_key_table_is_the_kernel_s():
    src = open(os.path.join(ROOT, "centernet_amd", "csrc", "cn_conv3x3p.hip")).read()
    assert "0x062654210ull >> (4 * (hx >> 1))" in src and "((hx >> 1) & 7)" in src
    assert [halo_key(True, hx) for hx in range(P_HW)] == KEY16
    assert [halo_key(False, hx) for hx in range(P_HW)] == [(hx >> 1) & 7 for hx in range(P_HW)]


@pytest.mark.parametrize("s16", [False, True])
def test_every_fragment_read_is_conflict_free(s16):
    seen = 0
    for form, kxs in FORM_KX.items():
        for wm, ky, kx in itertools.product(range(2), range(3), kxs):
            for tag, lanes in halo_reads(s16, wm, ky, kx):
                assert worst_conflict(lanes) == 1, (form, wm, ky, kx, tag)
                seen += 1
    for wn in range(2):
        for tag, lanes in weight_reads(s16, wn):
            assert worst_conflict(lanes) == 1, (wn, tag)
            seen += 1
    assert seen == (2 * 3 * 3 * 2 + 2 * 3 * 2) * 8 + 2 * 4


def test_the_check_sees_a_conflict():
    """the 16-row mapping under the 32-row key: free at kx = 0, two-way at kx = 1 and 2 -- why the key changed"""
    old = lambda hx: (hx >> 1) & 7
    worst = {kx: max(worst_conflict(l) for _, l in halo_reads(True, 0, 0, kx, key=old)) for kx in range(3)}
    assert worst == {0: 1, 1: 2, 2: 2}


@pytest.mark.parametrize("s16", [False, True])
def test_a_lane_reads_the_slot_the_loader_put_there(s16):
    """Loader: physical slot ps of halo row r receives source slot ps ^ key(column) (weights: ps ^ ((n >> 1) & 7)).
    So the logical slot a lane's address holds is (physical ^ key) -- and it is the one the MFMA layout assigns to
    the lane: K index 8 (lane >> 4) + j = channels of slot (lane >> 4) for 16x16x32; 8 (lane >> 5) + j of K half kh =
    slot 2 kh + (lane >> 5) for 32x32x16; + 4 for the low part."""
    for wm, ky, kx in itertools.product(range(2), range(3), range(3)):
        for tag, lanes in halo_reads(s16, wm, ky, kx):
            for addr, logical, hx in lanes:
                assert addr % 128 % 16 == 0 and ((addr % 128) >> 4) ^ halo_key(s16, hx) == logical, (tag, addr)
                assert addr // 128 % P_HW == hx and addr // 128 < 10 * P_HW
    for wn in range(2):
        for tag, lanes in weight_reads(s16, wn):
            for addr, logical, n in lanes:
                assert addr // 128 == n and ((addr % 128) >> 4) ^ weight_key(n) == logical, (tag, addr)


def _epilogue_pieces(s16, i):
    """[(lane, piece g, strip row, first channel c0, [(accumulator, register)] of its four values)] of half i"""
    out = []
    for ln, g in itertools.product(range(64), range(4)):
        if s16:
            out.append((ln, g, 16 * (g & 1) + (ln & 15), 16 * (g >> 1) + 4 * (ln >> 4),
                        [(4 * (g >> 1) + 2 * i + (g & 1), e) for e in range(4)]))
        else:
            out.append((ln, g, ln & 31, 8 * g + 4 * (ln >> 5), [(i, 4 * g + e) for e in range(4)]))
    return out


def _mfma_d(s16, ln, acc, reg):
    """(pixel of the wave tile, channel of the wave's group) of accumulator `acc`, register `reg`, lane ln: D =
    [channel][pixel], 16x16x32: row 4 (lane >> 4) + reg, column lane & 15; 32x32x16: row (reg & 3) + 8 (reg >> 2) +
    4 (lane >> 5), column lane & 31"""
    if s16:
        cb, pb = acc >> 2, acc & 3
        return 16 * pb + (ln & 15), 16 * cb + 4 * (ln >> 4) + reg
    return 32 * acc + (ln & 31), (reg & 3) + 8 * (reg >> 2) + 4 * (ln >> 5)


@pytest.mark.parametrize("out_plain", [False, True])
@pytest.mark.parametrize("s16", [False, True])
def test_the_epilogue_map_is_the_mfma_layout_and_a_bijection(s16, out_plain):
    tile = set()
    for i in range(2):
        written = {}
        for ln, g, row, c0, regs in _epilogue_pieces(s16, i):
            for e, (acc, reg) in enumerate(regs):
                pix, ch = _mfma_d(s16, ln, acc, reg)
                assert (pix, ch) == (32 * i + row, c0 + e), (ln, g, e)      # strip row r = pixel 32 i + r of the wave
                assert (pix, ch) not in tile
                tile.add((pix, ch))
            # bytes of the piece in the strip row: plain 16 at 4 c0; f32s 8 at 2 c0 (high) and 8 at 64 + 2 c0 (low)
            spans = [(4 * c0, 16)] if out_plain else [(2 * c0, 8), (64 + 2 * c0, 8)]
            for off, n in spans:
                for b in range(off, off + n):
                    assert (row, b) not in written
                    written[(row, b)] = ln
        # the row-layout pass: lane reads 16 bytes at rcol * 16 of rows 8 k + (lane >> 3), k = 0 .. 3
        read = {(8 * k + (ln >> 3), (ln & 7) * 16 + b) for ln in range(64) for k in range(4) for b in range(16)}
        assert read == set(written)
    assert tile == {(p, c) for p in range(64) for c in range(32)}
