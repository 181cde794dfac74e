"""The frame renderer's host side without a GPU: the numpy checker of tests/util_render.py pinned by hand cases, the Gall row table, the
colour table, the PNG writer and reader, and the drivers' flags."""
import struct
import zlib

import numpy as np
import pytest

from mlperf_deepcam_amd import nn as dnn
from mlperf_deepcam_amd import png
import util_render as ur


# ------------------------------------------------------------------------------------------------------------------ 1. the checker
def _seam_block():
    m = np.zeros((5, 8), np.uint8)
    m[1:4, [6, 7, 0]] = 1                                  # a 3 x 3 block across the seam
    return m


def test_checker_width_1_is_the_blocks_border():
    out = ur.outline(_seam_block(), 1, 1)
    want = np.zeros((5, 8), bool)
    want[1:4, [6, 7, 0]] = True
    want[2, 7] = False                                     # the centre has four neighbours of its class
    assert np.array_equal(out, want) and int(out.sum()) == 8
    assert not ur.outline(_seam_block(), 2, 1).any()       # no class 2 anywhere


def test_checker_width_3_is_the_5x5_block_with_its_centre():
    out = ur.outline(_seam_block(), 1, 3)
    want = np.zeros((5, 8), bool)
    want[0:5, [5, 6, 7, 0, 1]] = True
    assert np.array_equal(out, want) and out[2, 7]


def test_checker_rows_that_do_not_exist_are_no_neighbours():
    m = np.zeros((6, 16), np.uint8)
    m[0:3, 4:10] = 2                                       # touches row 0
    e = ur.edges(m, 2)
    assert not e[0, 5:9].any()                             # left, right and below are class 2, above is nothing: no edge along row 0
    assert e[0, 4] and e[0, 9] and e[2, 4:10].all() and e[1, 4] and not e[1, 5:9].any()
    m[3:6, 4:10] = 2                                       # ... and the last row: only the two sides are left
    e = ur.edges(m, 2)
    assert np.array_equal(np.argwhere(e)[:, 1], np.tile([4, 9], 6)) and not ur.edges(m, 1).any()
    full = np.full((4, 8), 1, np.uint8)                    # a class that fills the periodic field has no edge at all
    assert not ur.edges(full, 1).any() and not ur.outline(full, 1, 7).any()


def test_checker_colour_index_and_blend():
    lo, scale = np.float32(0.0), np.float32(1.0) / np.float32(4.0)
    v = np.asarray([-1.0, -0.0, 0.0, 0.999, 1.0, 1.5, 3.999, 4.0, 9.0, np.nan, np.inf, -np.inf], np.float32)
    idx, finite = ur.colour_index(v, lo, scale, 4)
    assert idx.tolist()[:9] == [0, 0, 0, 0, 1, 1, 3, 3, 3] and finite.tolist() == [True] * 9 + [False] * 3
    assert ur.colour_index(np.asarray([0.5], np.float32), 0.0, 1.0, 1)[0].tolist() == [0]
    rgb = np.asarray([[10, 20, 30], [10, 20, 30]], np.int64)
    out = ur.blend(rgb, np.asarray([True, False]), 0x80FF0000)
    assert out.tolist() == [[(255 * 128 + 10 * 127 + 127) // 255, (20 * 127 + 127) // 255, (30 * 127 + 127) // 255], [10, 20, 30]]
    assert ur.blend(rgb, np.asarray([True, True]), 0xFF010203).tolist() == [[1, 2, 3]] * 2          # opaque: the foreground
    assert ur.blend(rgb, np.asarray([True, True]), 0x00FFFFFF).tolist() == rgb.tolist()             # transparent: unchanged


def test_checker_render_small_frame_by_hand():
    """2 x 8 field, identity rows flipped, shift 3, one panel: every output pixel from the rule, one at a time"""
    H, W, shift = 2, 8, 3
    f = np.arange(H * W, dtype=np.float32).reshape(1, H, W, 1)
    f[0, 1, 2, 0] = np.nan
    lut = np.asarray([[i, 2 * i, 3 * i] for i in range(16)], np.uint8)
    m = np.zeros((1, H, W), np.int64)
    m[0, 0, 0] = 1
    m[0, 1, 5] = 2
    m[0, 1, 7] = -1
    rows, row_line, col_line = [1, 0, 7], [0, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0]
    out = ur.render(f, 0, 0.0, np.float32(1) / np.float32(16), lut, [m], rows, shift, row_line, col_line, 1)
    assert out.shape == (1, 1, 3, W, 3)
    for y, r in enumerate([1, 0, 1]):                      # 7 clamps to H - 1
        for x in range(W):
            c = (x + shift) % W
            v = f[0, r, c, 0]
            px = [0x40, 0x40, 0x40] if np.isnan(v) else [int(v), 2 * int(v), 3 * int(v)]
            if row_line[y] or col_line[x]:
                px = [(255 * 0x50 + old * (255 - 0x50) + 127) // 255 for old in px]
            if m[0, r, c] == 1:
                px = [0xFF, 0x40, 0x30]
            if m[0, r, c] == 2:
                px = [0xFF, 0xE0, 0x40]
            assert out[0, 0, y, x].tolist() == px, (y, x)


# ------------------------------------------------------------------------------------------------------------------ 2. tables
def test_gall_rows_at_the_benchmark_shape():
    t = dnn.gall_rows(768, 1152)
    ho = len(t)
    assert t.dtype == np.int32 and ho == 885 and t[0] == 767 and t[-1] == 0
    assert (np.diff(t.astype(np.int64)) <= 0).all()
    y = np.arange(ho)
    # 885 rows are odd and 768 even: the middle output row shows the equator, half way between source rows 383 and 384, and is its own
    # mirror image, so t[y] + t[Ho - 1 - y] = 767 cannot hold there; it holds for every other row
    mirrored = y != ho - 1 - y
    assert int(mirrored.sum()) == ho - 1
    assert ((t + t[::-1])[mirrored] == 767).all() and t[ho // 2] in (383, 384)
    small = dnn.gall_rows(64, 96)
    assert len(small) == 74 and small[0] == 63 and small[-1] == 0 and ((small + small[::-1]) == 63).all()
    assert np.array_equal(dnn.plate_rows(5), [4, 3, 2, 1, 0])


def test_graticule_tables():
    t = dnn.gall_rows(768, 1152)
    rl, cl = dnn.graticule(t, 1152, 576, height=768)
    assert rl.dtype == np.uint8 and cl.dtype == np.uint8 and rl.shape == (885,) and cl.shape == (1152,)
    assert int(rl.sum()) == 5 and int(cl.sum()) == 6       # parallels at 0, +-30, +-60; meridians every 60 degrees
    assert np.array_equal(rl, rl[::-1]) and rl[442] == 1   # symmetric about the equator
    assert np.array_equal(np.nonzero(cl)[0], np.arange(6) * 192)      # longitude 0 = source column 0 sits at column W / 2 after the roll
    rl, cl = dnn.graticule(t, 1152, 0, parallels=0, meridians=0, height=768)
    assert not rl.any() and not cl.any()


def test_render_palette():
    p = dnn.render_palette()
    assert p.shape == (64, 3) and p.dtype == np.uint8
    assert tuple(p[0]) == dnn.RENDER_BACKGROUND            # the lowest value is fully transparent: the background itself
    assert (np.diff(p.astype(int).sum(axis=1)) >= 0).all() and p[-1].sum() > 3 * 200        # brightness grows with the value
    for n in (1, 50, 256):
        q = dnn.render_palette(n)
        assert q.shape == (n, 3) and q.dtype == np.uint8
    with pytest.raises(Exception):
        dnn.render_palette(257)


# ------------------------------------------------------------------------------------------------------------------ 3. PNG
def _images():
    rs = np.random.RandomState(5)
    return {"rgb3x5": rs.randint(0, 256, (3, 5, 3)).astype(np.uint8), "grey3x5": rs.randint(0, 256, (3, 5)).astype(np.uint8),
            "rgb1x1": np.asarray([[[1, 2, 3]]], np.uint8), "rgb17x9": rs.randint(0, 4, (17, 9, 3)).astype(np.uint8),
            "grey7x13": np.zeros((7, 13), np.uint8)}


@pytest.mark.parametrize("level", [0, 1, 6])
@pytest.mark.parametrize("name", list(_images()))
def test_png_round_trip(tmp_path, name, level):
    img = _images()[name]
    path = str(tmp_path / f"{name}.png")
    png.write_png(path, img, level=level)
    back = png.read_png(path)
    assert back.dtype == np.uint8 and back.shape == img.shape and np.array_equal(back, img)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, kinds = 8, []
    while pos < len(data):                                 # every chunk's CRC, checked here and not through the reader
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        kinds.append(kind)
        pos += 12 + n
    assert kinds == [b"IHDR", b"IDAT", b"IEND"] and pos == len(data)          # one IDAT chunk
    h, w = img.shape[:2]
    assert struct.unpack(">IIBBBBB", data[16:29]) == (w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)
    raw = zlib.decompress(data[41:41 + struct.unpack(">I", data[33:37])[0]])
    assert len(raw) == h * (1 + img[0].size) and set(raw[::1 + img[0].size]) == {0}           # filter type 0 on every scanline


@pytest.mark.parametrize("name", ["rgb3x5", "grey3x5", "rgb17x9"])
def test_png_is_what_pil_reads(tmp_path, name):
    Image = pytest.importorskip("PIL.Image")
    img = _images()[name]
    path = str(tmp_path / "a.png")
    png.write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == ("RGB" if img.ndim == 3 else "L") and np.array_equal(np.asarray(im), img)


def _filtered(img, ftypes):
    """a PNG of img whose scanline y uses filter type ftypes[y], two IDAT chunks"""
    h, w = img.shape[:2]
    bpp = 3 if img.ndim == 3 else 1
    rows = img.reshape(h, -1).astype(int)
    raw = bytearray()
    for y in range(h):
        cur, up = rows[y], rows[y - 1] if y else np.zeros_like(rows[0])
        left = np.concatenate([np.zeros(bpp, int), cur[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, int), up[:-bpp]])
        ft = ftypes[y]
        if ft == 0:
            line = cur
        elif ft == 1:
            line = cur - left
        elif ft == 2:
            line = cur - up
        elif ft == 3:
            line = cur - (left + up) // 2
        else:
            p = left + up - upleft
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - upleft)
            line = cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        raw += bytes([ft]) + bytes((line % 256).astype(np.uint8))
    z = zlib.compress(bytes(raw), 6)
    head = struct.pack(">IIBBBBB", w, h, 8, 2 if bpp == 3 else 0, 0, 0, 0)
    return png.SIGNATURE + png._chunk(b"IHDR", head) + png._chunk(b"IDAT", z[:7]) + png._chunk(b"tEXt", b"k\0v") + png._chunk(b"IDAT", z[7:]) \
        + png._chunk(b"IEND", b"")


@pytest.mark.parametrize("name", ["rgb17x9", "grey3x5", "rgb3x5"])
def test_png_reader_takes_filters_0_to_4(name):
    img = _images()[name]
    if name == "rgb17x9":
        img = np.random.RandomState(9).randint(0, 256, img.shape).astype(np.uint8)
    data = _filtered(img, [y % 5 for y in range(img.shape[0])])
    assert np.array_equal(png.decode_png(data), img)
    assert np.array_equal(png.decode_png(_filtered(img, [4, 3, 4] + [3] * (img.shape[0] - 3))), img)


def test_png_reader_refuses_damage():
    data = bytearray(png.encode_png(_images()["rgb3x5"]))
    data[45] ^= 1                                          # a byte of the image data: the chunk's CRC no longer verifies
    with pytest.raises(ValueError, match="CRC"):
        png.decode_png(bytes(data))
    with pytest.raises(ValueError):
        png.decode_png(b"not a png")
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((3, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        png.encode_png(np.zeros((3, 5), np.float32))
    interlaced = png.SIGNATURE + png._chunk(b"IHDR", struct.pack(">IIBBBBB", 1, 1, 8, 2, 0, 0, 1)) + png._chunk(b"IEND", b"")
    with pytest.raises(ValueError, match="interlace"):
        png.decode_png(interlaced)


# ------------------------------------------------------------------------------------------------------------------ 4. drivers
def test_predict_parser_has_the_plot_flags():
    from mlperf_deepcam_amd import predict
    base = ["--checkpoint", "m", "--data_dir", "d", "--stats_file", "s", "--output_dir", "o"]
    a = predict.build_parser().parse_args(base)
    assert a.plots is False and a.plot_every == 1 and a.plot_channel == 0 and a.events is False and a.verify is False
    a = predict.build_parser().parse_args(base + ["--plots", "--plot_every", "4", "--plot_channel", "2", "--verify"])
    assert a.plots is True and a.plot_every == 4 and a.plot_channel == 2 and a.verify is True and a.events is True
    assert predict.plot_name("data-2000-01-01.h5") == "data-2000-01-01.png"


def test_train_parser_has_plots_and_keeps_its_defaults():
    from mlperf_deepcam_amd import train
    with_plots = vars(train.build_parser().parse_args(["--plots"]))
    plain = vars(train.build_parser().parse_args([]))
    assert plain["plots"] is False and with_plots["plots"] is True
    assert {k: v for k, v in with_plots.items() if k != "plots"} == {k: v for k, v in plain.items() if k != "plots"}
    assert plain["training_visualization_frequency"] == 50 and plain["validation_visualization_frequency"] == 50
    assert plain["local_batch_size"] == 1 and plain["optimizer"] == "Adam" and plain["amp_opt_level"] == "O0" and plain["virtual_ranks"] == 1
    assert plain["validation_batch_size"] == 1 and plain["save_frequency"] == 100 and plain["max_epochs"] == 30
    a = train.build_parser().parse_args(["--training_visualization_frequency", "0", "--validation_visualization_frequency", "0"])
    assert a.training_visualization_frequency == 0 and a.validation_visualization_frequency == 0 and a.plots is False
