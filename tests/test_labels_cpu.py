"""Text labels on the CPU (-m "not gpu"): arrows.draw_labels_host / format_labels_host -- the host twins of mcg_draw_labels and
mcg_format_labels -- against pixels written out by hand, a scalar restatement in Python integers (tests/labels_cases.py), and str(); the font
table; the argument checks of the three entries (MCG_ERR_ARG before any launch, so no GPU is needed).  tests/test_gpu_labels.py holds the
kernels to these twins bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mcgaze_amd import arrows as R
from mcgaze_amd import attention as A
from mcgaze_amd import lib as L
from mcgaze_amd.nv12 import bgr_to_yuv
from tests import draw_cases as D
from tests import labels_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCG_ERR_ARG = 1                                                   # enum of include/mcgaze_hip.h

# '#7' at advance 6, written out from the font rows of '#' and '7' (the eighth row of the cell is empty)
HASH_SEVEN = ['.#.#..#####.',
              '.#.#......#.',
              '#####....#..',
              '.#.#....#...',
              '#####..#....',
              '.#.#...#....',
              '.#.#...#....',
              '............']


def art(lines):
    return np.array([[c == '#' for c in line] for line in lines])


# ---------------------------------------------------------------- the font
def test_label_font_is_a_5x7_table_of_95_distinct_glyphs():
    f = R.LABEL_FONT
    assert f.dtype == np.uint8 and f.shape == (96, 8)
    assert not (f & 0xE0).any() and not f[:, 7].any()             # bits only in columns 0 .. 4 and rows 0 .. 6
    assert not f[0].any() and not f[95].any()                     # space, and the spare entry
    assert all(f[g].any() for g in range(1, 95))
    assert len({f[g].tobytes() for g in range(95)}) == 95
    with pytest.raises(ValueError):
        f[0, 0] = 1                                               # the table is data, stated once
    assert R.glyph_sheet().splitlines()[0].split()[ord('#') - 32] == '.#.#.'
    # bit c, from the least significant, is column c from the left
    assert [int(v) for v in f[ord('7') - 32]] == [0b11111, 0b10000, 0b01000, 0b00100, 0b00010, 0b00010, 0b00010, 0]
    assert np.array_equal(art(HASH_SEVEN)[:, :6], (f[ord('#') - 32][:, None] >> np.arange(6)) & 1)


# ---------------------------------------------------------------- the twin against hand-worked cases
def test_one_label_at_scale_1_pixel_by_pixel_and_at_scale_2_as_its_kron():
    frame = np.full((40, 48, 3), 200, np.uint8)
    kw = dict(color=(1, 2, 3), background=(9, 8, 7), advance=6, pad=1)
    out, flags = R.draw_labels_host(frame, [LC.ROWS[0][2]], None, R.encode_labels(['#7']), scale=1, **kw)
    assert flags.tolist() == [0] and (frame == 200).all()
    # box (5.5, 14.2, ..): X = 5, PH = 8 + 2 = 10, Y = 14 - 10 = 4: the plate [5, 19) x [4, 14), the text origin (6, 5)
    want = np.full((40, 48, 3), 200, np.uint8)
    want[4:14, 5:19] = (9, 8, 7)
    want[5:13, 6:18][art(HASH_SEVEN)] = (1, 2, 3)
    assert np.array_equal(out, want)
    # scale 2: every font bit is a 2 x 2 block.  PH = 20: no room above y = 14 -> below the box, Y = 31, clamped to 40 - 20 = 20
    out2, _ = R.draw_labels_host(frame, [LC.ROWS[0][2]], None, R.encode_labels(['#7']), scale=2, **kw)
    want2 = np.full((40, 48, 3), 200, np.uint8)
    want2[20:40, 5:33] = (9, 8, 7)
    want2[22:38, 7:31][np.kron(art(HASH_SEVEN), np.ones((2, 2), bool))] = (1, 2, 3)
    assert np.array_equal(out2, want2)
    # without a background only the glyph pixels are written
    out3, _ = R.draw_labels_host(frame, [LC.ROWS[0][2]], None, R.encode_labels(['#7']), scale=1, color=(1, 2, 3), background=None)
    want3 = np.full((40, 48, 3), 200, np.uint8)
    want3[5:13, 6:18][art(HASH_SEVEN)] = (1, 2, 3)
    assert np.array_equal(out3, want3)


def test_placement_above_below_clamped_wider_than_the_frame_and_place_1():
    sizes = D.SHAPES
    p = R.label_plan(LC.BOXES, LC.IMAGE_OF, LC.TEXT, sizes, LC.PLACE, scale=1, advance=6, pad=1)
    assert p['flag'].tolist() == LC.FLAGS
    box = lambda k: tuple(int(p[f][k]) for f in ('x0', 'y0', 'x1', 'y1'))
    origin = lambda k: (int(p['x'][k]), int(p['y'][k]))
    assert box(0) == (5, 4, 19, 14) and origin(0) == (6, 5)                 # above: 14 - 10
    assert box(1) == (0, 21, 48, 31) and origin(1) == (1, 22)               # 3 - 10 < 0: below, by2 + 1 = 21; PW = 50 > 48: X = 0, clipped
    assert box(2) == (34, 20, 48, 30)                                       # PW = 14: X = min(40, 48 - 14)
    assert box(3) == (4, 22, 48, 32) and origin(3) == (5, 23)               # place 1: (bx1, by1) = (10, 22), PW = 44: X = min(10, 4)
    assert box(4) == (3, 2, 11, 12) and box(4)[3] <= 12                     # the 12 x 16 frame: 9 - 10 < 0 -> below: 12, clamped to 12 - 10
    assert box(5) == (0, 2, 22, 12) and origin(5) == (1, 3)                 # 19 characters: PW = 116 in a 22-wide frame; place 7 is "above": 12 - 10
    assert box(6) == (0, 0, 2, 2) and origin(6) == (1, 1)                   # the 2 x 2 frame
    assert box(7) == (0, 0, 0, 0) and p['image'][7] == -1                   # the empty label
    assert box(9) == (34, 30, 48, 40) and box(10) == (0, 0, 8, 10)          # boxes wholly outside: moved inside


def test_a_later_plate_hides_earlier_text_and_the_nv12_chroma_rule():
    frame = np.zeros((40, 48, 3), np.uint8)
    rows = [0, 8]                                                 # row 8's plate [6, 20) x [5, 15) lies over most of row 0's text
    kw = dict(scale=1, colors=LC.COLORS[rows], background=(9, 8, 7))
    out, _ = R.draw_labels_host(frame, LC.BOXES[rows], None, LC.TEXT[rows], **kw)
    alone, _ = R.draw_labels_host(frame, LC.BOXES[rows[1:]], None, LC.TEXT[rows[1:]], scale=1, colors=LC.COLORS[rows[1:]], background=(9, 8, 7))
    assert np.array_equal(out[5:15, 6:20], alone[5:15, 6:20])    # under the later plate nothing of row 0 is left
    assert (out[5:13, 6] == (9, 8, 7)).all() and (out[4, 5:19] == (9, 8, 7)).all()
    # row 0's text [6, 18) x [5, 13) lies wholly under it: its colour is gone, only the rim of its plate (row 4, column 5) is left
    assert not (out == LC.COLORS[0]).all(axis=2).any() and (out == LC.COLORS[8]).all(axis=2).any()
    swapped, _ = R.draw_labels_host(frame, LC.BOXES[rows[::-1]], None, LC.TEXT[rows[::-1]], scale=1, colors=LC.COLORS[rows[::-1]], background=(9, 8, 7))
    assert (swapped[7, 6] == LC.COLORS[0]).all()                  # the other order: the highest row wins, '#' row 2 starts at (6, 7)
    # NV12: one label without a plate; a chroma pair is written iff one of its four luma pixels is a glyph pixel
    y, uv = np.full((40, 48), 50, np.uint8), np.full((20, 48), 60, np.uint8)
    (oy, ouv), _ = R.draw_labels_host((y, uv), [LC.ROWS[0][2]], None, R.encode_labels(['#7']), scale=1, color=(10, 200, 90), background=None,
                                      pixel_format='nv12', matrix='bt709')
    yuv = bgr_to_yuv(np.array((10, 200, 90), np.uint8), 'bt709')
    glyph = np.zeros((40, 48), bool)
    glyph[5:13, 6:18] = art(HASH_SEVEN)
    assert np.array_equal(oy, np.where(glyph, yuv[0], 50))
    pairs = glyph.reshape(20, 2, 24, 2).any(axis=(1, 3))
    # the pair at chroma (2, 3) covers luma rows 4 .. 5, columns 6 .. 7: only (5, 7) is a glyph pixel -- the pair straddles the glyph's edge
    assert glyph[5, 7] and not glyph[4, 6] and not glyph[4, 7] and not glyph[5, 6] and pairs[2, 3]
    assert np.array_equal(ouv.reshape(20, 24, 2), np.where(pairs[:, :, None], np.array(yuv[1:], np.uint8), 60))
    # with a plate, the pair takes the (U, V) of the highest stroke among its four: the glyph's
    (oy, ouv), _ = R.draw_labels_host((y, uv), [LC.ROWS[0][2]], None, R.encode_labels(['#7']), scale=1, color=(10, 200, 90), background=(0, 0, 0),
                                      pixel_format='nv12', matrix='bt709')
    black = bgr_to_yuv(np.array((0, 0, 0), np.uint8), 'bt709')
    assert oy[4, 6] == black[0] and oy[5, 7] == yuv[0] and tuple(ouv.reshape(20, 24, 2)[2, 3]) == tuple(yuv[1:])
    assert tuple(ouv.reshape(20, 24, 2)[2, 2]) == tuple(black[1:])          # luma (4 .. 5, 4 .. 5): plate at (4, 5), (5, 5) only


def test_text_codes_and_lengths():
    n = len(LC.CODE_TEXT)
    boxes = np.tile(np.array([(0, 20, 5, 30)], np.float32), (n, 1))
    sizes = [(40, 200)]
    p = R.label_plan(boxes, np.zeros(n, np.int32), LC.CODE_TEXT, sizes, scale=1, advance=6, pad=0)
    assert p['len'].tolist() == LC.CODE_LENGTHS and p['flag'].tolist() == [0, 0, 1, 0, 0, 0]
    assert p['x1'].tolist() == [6 * l for l in LC.CODE_LENGTHS]
    _, _, cover = R.label_coverage(p, 0, LC.CODE_TEXT, scale=1, advance=6)
    cell = lambda i: cover[:, 6 * i:6 * i + 6]
    glyph = lambda ch: (R.LABEL_FONT[ord(ch) - 32][:, None] >> np.arange(6)) & 1
    for i, ch in enumerate('A? ~??'):                             # 31, 127 and 255 are drawn as '?'; 32 is the space, 126 the tilde
        assert np.array_equal(cell(i), glyph(ch)), i
    _, _, cover = R.label_coverage(p, 1, LC.CODE_TEXT, scale=1, advance=6)
    assert cover.shape == (8, 12) and np.array_equal(cover[:, 6:], glyph('C'))       # the code behind the zero is not drawn
    _, _, cover = R.label_coverage(p, 5, LC.CODE_TEXT, scale=1, advance=6)
    assert cover.shape == (8, 144) and np.array_equal(cover[:, 138:], glyph('x'))    # 24 codes and no terminator


@pytest.mark.parametrize('nv12', [False, True], ids=['bgr', 'nv12'])
@pytest.mark.parametrize('scale,advance,pad,background', [(1, 6, 1, True), (2, 6, 1, True), (3, 1, 0, False), (1, 8, 8, True), (16, 5, 2, False)])
def test_the_twin_equals_the_scalar_restatement_on_random_tables(scale, advance, pad, background, nv12):
    frames = D.NV12_FRAMES if nv12 else D.BGR_FRAMES
    font = np.random.RandomState(3).randint(0, 256, (96, 8)).astype(np.uint8) if advance == 8 else R.LABEL_FONT     # advance 8 reads columns 5 .. 7
    boxes, image_of, text, place = LC.random_tables(11 + scale, 40, D.SHAPES)
    colors = np.random.RandomState(5).randint(0, 256, (40, 3)).astype(np.uint8)
    bg = (9, 8, 7) if background else None
    got, flags = R.draw_labels_host(frames, boxes, image_of, text, colors=colors, background=bg, scale=scale, advance=advance, pad=pad, place=place,
                                    font=font, pixel_format='nv12' if nv12 else 'bgr', matrix='bt601')
    winner, want_flags = LC.scalar_labels(D.SHAPES, boxes, image_of, text, place, scale, advance, pad, font, nv12, background)
    assert flags.tolist() == want_flags and {0, 1, 2} <= set(want_flags)
    fg = [bgr_to_yuv(c, 'bt601') for c in colors] if nv12 else colors
    bgc = bgr_to_yuv(np.array((9, 8, 7), np.uint8), 'bt601') if nv12 else (9, 8, 7)
    LC.same('nv12' if nv12 else 'bgr', got, LC.paint(frames, winner, fg, bgc, nv12), (scale, advance, pad))
    if nv12:
        assert all(f == 2 for f, io in zip(want_flags, image_of) if 0 <= io < len(D.SHAPES) and (D.SHAPES[io][0] | D.SHAPES[io][1]) & 1)


def test_strict_and_argument_errors_of_the_twin():
    frame = np.zeros((20, 30, 3), np.uint8)
    text = R.encode_labels(['a'])
    with pytest.raises(ValueError):
        R.draw_labels_host(frame, [(0, 0, 9000, 4)], None, text, strict=True)
    assert R.draw_labels_host(frame, [(0, 0, 9000, 4)], None, text)[1].tolist() == [2]
    for bad in (dict(scale=0), dict(scale=17), dict(advance=0), dict(advance=9), dict(pad=-1), dict(pad=9), dict(scale=1.5), dict(background=(1, 2)),
                dict(colors=(1, 2, 3)), dict(font=np.zeros((95, 8), np.uint8))):
        with pytest.raises(ValueError):
            R.draw_labels_host(frame, [(0, 0, 5, 4)], None, text, **bad)
    with pytest.raises(ValueError):
        R.draw_labels_host(frame, [(0, 0, 5, 4)], None, np.zeros((1, 23), np.uint8))
    with pytest.raises(TypeError):
        R.draw_labels_host(frame, [(0, 0, 5, 4)], [0.5], text)
    assert np.array_equal(R.encode_labels(['#7', '', 'é'])[:, :3], [[35, 55, 0], [0, 0, 0], [233, 0, 0]])
    assert R.encode_labels(['x' * 24])[0].all()
    with pytest.raises(ValueError):
        R.encode_labels(['x' * 25])
    with pytest.raises(ValueError):
        R.encode_labels(['€'])


# ---------------------------------------------------------------- format_labels_host
@pytest.mark.parametrize('rate', [(1, 1), (30, 1), (30000, 1001), (1 << 20, 1)])
def test_format_labels_host_equals_python_integers_and_str(rate):
    num, den = rate
    ids = [0, -1, 1, 9, 10, 2147483647]
    values = [None, 0, 1, 299, 2147483647]
    cut = 0
    for v in values:
        table = R.format_labels_host(ids, None if v is None else [v] * len(ids), rate)
        assert table.dtype == np.uint8 and table.shape == (len(ids), 24)
        for k, i in enumerate(ids):
            want = ''
            if i > 0:
                want = '#' + str(i)
                if v is not None and v > 0:
                    q = v * 10 * den // num
                    want += ' ' + str(q // 10) + '.' + str(q % 10) + 's'
            # every text of at most 24 characters is written whole; the one text of 25 (ten digits on both sides) loses its 's'
            assert len(want) <= 24 or (len(want) == 25 and i == 2147483647 and v == 2147483647 and rate == (1, 1)), (i, v, rate)
            cut += len(want) > 24
            assert bytes(table[k]) == want.encode()[:24].ljust(24, b'\0'), (i, v, rate)
    assert cut == (rate == (1, 1))
    assert bytes(R.format_labels_host([12], [102], (30, 1))[0]).rstrip(b'\0') == b'#12 3.4s'
    assert bytes(R.format_labels_host([12], [299], (30000, 1001))[0]).rstrip(b'\0') == b'#12 9.9s'      # 299 * 1001 / 30000 = 9.976..: floored


def test_format_labels_host_refuses_bad_rates_and_tables():
    for rate in ((0, 1), (1, 2), ((1 << 20) + 1, 1), (30, 0), (30.0, 1), 30, (True, 1)):
        with pytest.raises(ValueError):
            R.format_labels_host([1], None, rate)
    with pytest.raises(TypeError):
        R.format_labels_host([1.5])
    with pytest.raises(ValueError):
        R.format_labels_host([1, 2], [3])


# ---------------------------------------------------------------- region names
def test_region_label_rows_follow_the_pictures_draw_attention_draws_into():
    regions = [[2, 3, 20, 30], [[5, 5], [30, 8], [12, 40]], [1, 1, 2, 2], [9, 9, 3, 3]]
    boxes, image_of, text, place = A.region_label_rows(regions, [-1, 1, 0, -1], ['AISLE', 'SHELF A', None, 'inverted'], 4, region_period=2)
    assert image_of.tolist() == [0, 1, 1, 2, 3, 3] and place.tolist() == [1] * 6       # the unnamed and the unusable region get no row
    assert [bytes(t).rstrip(b'\0') for t in text] == [b'AISLE', b'AISLE', b'SHELF A', b'AISLE', b'AISLE', b'SHELF A']
    assert boxes[0].tolist() == [2, 3, 20, 30] and boxes[2].tolist() == [5, 5, 30, 40] and boxes.dtype == np.float32
    assert A.region_label_rows(None, None, [], 3)[0].shape == (0, 4)
    with pytest.raises(ValueError):
        A.region_label_rows(regions, None, ['a'], 1)
    with pytest.raises(ValueError):
        A.region_label_rows(regions, None, ['x' * 25, '', '', ''], 1)


# ---------------------------------------------------------------- the library entries
def test_header_exports_and_abi():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION == 20
    assert int(re.search(r'#define MCG_LABEL_CHARS (\d+)', hdr).group(1)) == L.LABEL_CHARS == R.LABEL_CHARS == 24
    lib = L.load()
    for name in ('mcg_format_labels', 'mcg_draw_labels', 'mcg_draw_labels_nv12'):
        assert name in L.EXPORTS and re.search(r'\bint %s\(' % name, hdr) and hasattr(lib, name)
    assert C.sizeof(L.LabelDesc) == 64 and 'text labels' in hdr


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """Every call here fails the host-side checks and returns MCG_ERR_ARG: nothing is launched, so no GPU is needed and no pointer is read."""
    lib = L.load()
    vp, p = C.c_void_p, 0x1000                                    # a non-null address that is never read
    color = (C.c_ubyte * 3)(1, 2, 3)

    def fmt(ids=p, n=4, num=30, den=1, out=p):
        return lib.mcg_format_labels(None, vp(ids), None, n, num, den, vp(out))

    for bad in (dict(ids=None), dict(out=None), dict(n=-1), dict(n=65536), dict(den=0), dict(num=1, den=2), dict(num=(1 << 20) + 1), dict(num=0, den=0)):
        assert fmt(**bad) == MCG_ERR_ARG, bad
    assert fmt(n=0) == L.MCG_OK

    for entry in (lib.mcg_draw_labels, lib.mcg_draw_labels_nv12):
        def draw(images=p, num_images=1, max_h=40, max_w=48, boxes=p, image_of=p, text=p, n=4, font=p, scale=2, advance=6, pad=1, color_=color, colors=None,
                 plan=p):
            return entry(None, vp(images), num_images, max_h, max_w, vp(boxes), vp(image_of), vp(text), None, n, vp(font), scale, advance, pad, color_,
                         vp(colors), None, vp(plan), None)

        for bad in (dict(images=None), dict(boxes=None), dict(image_of=None), dict(text=None), dict(font=None), dict(plan=None), dict(color_=None),
                    dict(num_images=0), dict(num_images=65536), dict(n=-1), dict(n=65536), dict(max_h=0), dict(max_w=8193), dict(scale=0), dict(scale=17),
                    dict(advance=0), dict(advance=9), dict(pad=-1), dict(pad=9)):
            assert draw(**bad) == MCG_ERR_ARG, bad
        assert entry.__name__.encode() in lib.mcg_last_error()
        assert draw(n=0) == L.MCG_OK
        assert draw(n=0, color_=None, colors=p) == L.MCG_OK      # per-row colours stand in for the one colour


def test_the_document_shows_the_glyph_sheet_of_the_table():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    sheet = '\n'.join('    ' + line if line else '' for line in R.glyph_sheet().splitlines())
    assert sheet in doc and len(R.glyph_sheet().splitlines()) == 6 * 8 - 1


def test_the_labels_option_of_livegaze_and_run_head_video():
    assert R._label_options('x', None, True) is None and R._label_options('x', False, False) is None
    assert R._label_options('x', True, True) == dict(scale=2, advance=6, pad=1, background=(0, 0, 0), fps=(30, 1), region_names=None)
    assert R._label_options('x', dict(scale=4, fps=(30000, 1001)), True)['fps'] == (30000, 1001)
    for labels, draw in ((True, False), (dict(), None), (3, True), (dict(size=2), True), (dict(scale=17), True), (dict(fps=(1, 2)), True), (dict(fps=30), True),
                         (dict(background=(1, 2)), True), (dict(pad=9), True)):
        with pytest.raises(ValueError):
            R._label_options('x', labels, draw)
