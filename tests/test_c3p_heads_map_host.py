"""The lane maps of the fused heads of the persistent 3x3 kernel on v_mfma_f32_16x16x32_f16 (csrc/cn_conv3x3p.hip,
`HEADS && S16`), restated in plain Python (CPU).

A consumer wave owns tile rows 2 w, 2 w + 1 (pixel blocks pb = 0, 1 of 16 pixels) and the 64 hidden channels of
the item's head as four blocks cb of 16 MFMA rows.  Lane = (r = lane & 15, s = lane >> 4): r is the row of an A
fragment and the column of a B / D fragment, s the 16-byte K slot (K = 8 s .. 8 s + 7) of an A / B fragment and
the row group (rows 4 s .. 4 s + 3) of D.

* Row r of weight block cb = 2 j + u is read from LDS row n = 32 j + 8 u + (r & 7) + 16 (r >> 3): a row <-> lane
  map is only an LDS address.  The weight loader keys row n with p3_weight_key(true, n) -- bits 1, 2 and 4 of n, in
  terms of r the (r >> 1) & 7 of the other forms -- and the halo loader with p3_halo_key(true, .).
  (a) every lane group of every ds_read_b128 (tests/test_c3p_fragment_map_host.py: four groups of 16 lanes, one LDS
      cycle each when their addresses fall into 16 distinct 16-byte units of the 256-byte bank row) of the weight
      and pixel fragments is conflict-free at kx = 0, 1, 2, and reads the slot the loader put there.
* D row 4 s + e of block 2 j + u is therefore hidden channel 32 j + 16 (s >> 1) + 4 (s & 1) + e + 8 u, and the eight
  values (u, e) a lane holds of blocks 2 j, 2 j + 1 are its B fragment of K step j of the 1x1 GEMM.
  (b) they are the K set, in order, of the packed piece (row >> 5, j, s >> 1, part, (row & 31) + 32 (s & 1)) of
      cn_pack_head_w2_f32s that the lane reads as its A fragment: the buffer the 32x32x16 form reads.
* The 1x1 output runs in cdiv(cout, 16) blocks of 16 rows, lane (r, s) holding rows 16 ob + 4 s + e of pixel r.
  (c) every (row < cout, pixel of the tile) is written exactly once, for cout = 1, 2, 17, 80 and 96, no row >= cout is
      written and no packed piece beyond cn_packed_head_w2_bytes is read.
"""
import itertools
import os

import pytest

from test_c3p_fragment_map_host import GROUPS, KEY16, P_HW, halo_key, worst_conflict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUTS = (1, 2, 17, 80, 96)


def weight_key16h(n):
    """p3_weight_key(true, n)"""
    return ((n >> 1) & 3) | (((n >> 4) & 1) << 2)


def weight_row(cb, r):
    """LDS row of MFMA row r of weight block cb: wblk(cb) / 128 + the row part of b0"""
    return 32 * (cb >> 1) + 8 * (cb & 1) + (r & 7) + 16 * (r >> 3)


def weight_reads():
    """[(tag, [(byte address, logical slot, row)] per lane)]: wh / wl of the four channel blocks (reads1, reads 2)"""
    out = []
    for cb, part in itertools.product(range(4), range(2)):
        lanes = []
        for ln in range(64):
            r, sl = ln & 15, ln >> 4
            b0 = ((r & 7) + 16 * (r >> 3)) * 128 + (((sl ^ ((r >> 1) & 7)) & 7) << 4)
            lanes.append(((32 * (cb >> 1) + 8 * (cb & 1)) * 128 + (b0 ^ (part << 6)), sl + 4 * part, weight_row(cb, r)))
        out.append((("w", cb, part), lanes))
    return out


def halo_reads(wave, ky, kx):
    """xh / xl of the two pixel blocks: tile row 2 wave + pb, column lane & 15, tap (ky, kx)"""
    out = []
    for pb, part in itertools.product(range(2), range(2)):
        lanes = []
        for ln in range(64):
            px, sl = ln & 15, ln >> 4
            arow = (2 * wave * P_HW + px) * 128
            swz = ((sl ^ halo_key(True, px + kx)) & 7) << 4
            addr = (ky * P_HW + kx) * 128 + pb * P_HW * 128 + ((arow + swz) ^ (part << 6))
            lanes.append((addr, sl + 4 * part, px + kx))
        out.append((("x", pb, part), lanes))
    return out


def test_the_maps_are_the_kernel_s():
    src = open(os.path.join(ROOT, "centernet_amd", "csrc", "cn_conv3x3p.hip")).read()
    for text in ("hs16 ? (((n >> 1) & 3) | (((n >> 4) & 1) << 2)) : ((n >> 1) & 7)",
                 "p3_weight_key(HEADS && S16, n)",
                 "b0 = ((px & 7) + 16 * (px >> 3)) * 128 + (((sl ^ ((px >> 1) & 7)) & 7) << 4);",
                 "arow = (2 * wv * P_HW + px) * 128;",
                 "return (32 * (cb >> 1) + 8 * (cb & 1)) * 128;",
                 "const int n = 32 * j + 8 * u + 16 * (s >> 1) + 4 * (s & 1);",
                 "const int piece = (((row >> 5) * 2 + j) * 2 + (s >> 1)) * 2, l2 = (row & 31) + 32 * (s & 1);",
                 "const int row = 16 * ob + (ln & 15), s = ln >> 4;",
                 "const int co0 = 16 * ob + 4 * s;",
                 "const int nob = (cout2 + 15) >> 4;"):
        assert text in src, text
    assert [halo_key(True, hx) for hx in range(P_HW)] == KEY16
    assert len(GROUPS) == 4 and sorted(l for g in GROUPS for l in g) == list(range(64))


def test_every_fragment_read_is_conflict_free_and_reads_the_loader_s_slot():
    seen = 0
    for wave, ky, kx in itertools.product(range(4), range(3), range(3)):
        for tag, lanes in halo_reads(wave, ky, kx):
            assert worst_conflict(lanes) == 1, (wave, ky, kx, tag)
            for addr, logical, hx in lanes:
                assert addr % 16 == 0 and ((addr % 128) >> 4) ^ halo_key(True, hx) == logical, (tag, addr)
                assert addr // 128 % P_HW == hx and addr // 128 < 10 * P_HW
            seen += 1
    rows = []
    for tag, lanes in weight_reads():
        assert worst_conflict(lanes) == 1, tag
        for addr, logical, n in lanes:
            assert addr // 128 == n and ((addr % 128) >> 4) ^ weight_key16h(n) == logical, (tag, addr)
        rows += [n for _, _, n in lanes[:16]] if tag[2] == 0 else []
        seen += 1
    assert sorted(rows) == list(range(64))          # the four blocks take every row of the 64-row tile once
    assert seen == 4 * 3 * 3 * 4 + 8


def test_the_check_sees_a_conflict():
    """the same reads under the key of the other forms, (n >> 1) & 7: two lanes per unit -- why this form has its own"""
    worst = 1
    for (_, cb, part), lanes in weight_reads():
        rekeyed = [((a & ~127) | (((((a % 128) >> 4) ^ weight_key16h(n) ^ ((n >> 1) & 7)) & 7) << 4), l, n) for a, l, n in lanes]
        worst = max(worst, worst_conflict(rekeyed))
    assert worst == 2


def _hidden_of_d(cb, ln, e):
    """hidden channel of D row 4 s + e of block cb on lane ln: the weight row that A row fed"""
    return weight_row(cb, 4 * (ln >> 4) + e)


def _packed_k(j, s2, lh, q):
    """pack_head_w2_kernel: K index of element q of the piece (., j, s2, ., lane with lane >> 5 = lh)"""
    return 32 * j + 16 * s2 + 8 * (q >> 2) + 4 * lh + (q & 3)


def test_the_hidden_layout_and_the_packed_pieces_name_the_same_k():
    for ln in range(64):
        s = ln >> 4
        for j in range(2):
            # B fragment of K step j: elements 0 .. 3 from block 2 j, 4 .. 7 from block 2 j + 1 (the shufflevector)
            b_k = [_hidden_of_d(2 * j + (q >> 2), ln, q & 3) for q in range(8)]
            assert b_k == [32 * j + 16 * (s >> 1) + 4 * (s & 1) + (q & 3) + 8 * (q >> 2) for q in range(8)]
            # the stash index the epilogue reads scale / bias1 at: n + e of block 2 j + u
            for u, e in itertools.product(range(2), range(4)):
                assert 32 * j + 8 * u + 16 * (s >> 1) + 4 * (s & 1) + e == _hidden_of_d(2 * j + u, ln, e)
            # A fragment: for every 16-row output block the piece the lane reads holds row 16 ob + (lane & 15) and
            # the same K, element by element; a lane's MFMA partner (same s) holds the same K slot
            for ob in range(6):
                row = 16 * ob + (ln & 15)
                l2 = (row & 31) + 32 * (s & 1)
                jb, s2 = row >> 5, s >> 1
                assert jb * 32 + (l2 & 31) == row                      # the piece's row (pack: row = jb * 32 + l31)
                assert [_packed_k(j, s2, l2 >> 5, q) for q in range(8)] == b_k
    # every hidden channel is the K of exactly one (j, s, q)
    ks = sorted(_hidden_of_d(2 * j + (q >> 2), 16 * s, q & 3) for j in range(2) for s in range(4) for q in range(8))
    assert ks == list(range(64))


@pytest.mark.parametrize("cout", COUTS)
def test_the_epilogue_writes_every_output_once(cout):
    nob = (cout + 15) >> 4
    packed_bytes = (cout + 31) // 32 * 8192                            # cn_packed_head_w2_bytes
    written = {}
    for wave, ob, ln, pb, e in itertools.product(range(4), range(nob), range(64), range(2), range(4)):
        s, px = ln >> 4, ln & 15
        co = 16 * ob + 4 * s + e
        assert co < 96                                                 # the output scale / bias stash holds 96 rows
        if co < cout:
            key = (co, 2 * wave + pb, px)
            assert key not in written, key
            written[key] = (wave, ob, ln)
    assert set(written) == {(co, y, x) for co in range(cout) for y in range(8) for x in range(16)}
    for ob, ln, j, part in itertools.product(range(nob), range(64), range(2), range(2)):
        row, s = 16 * ob + (ln & 15), ln >> 4
        piece = (((row >> 5) * 2 + j) * 2 + (s >> 1)) * 2 + part
        off = (piece * 64 + (row & 31) + 32 * (s & 1)) * 16
        assert 0 <= off and off + 16 <= packed_bytes, (cout, ob, ln)
