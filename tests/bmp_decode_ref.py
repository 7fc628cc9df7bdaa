"""The device BMP decoder (csrc/bmp_parse.h, csrc/bmpdec.hip) restated in numpy: the plan -- ``BmpImagePlugin._bitmap`` as restated, with
its refusal reasons -- and both planes, and a writer for files Pillow never writes: every header size, depth, mask layout and direction.
Pillow's rules as restated (each checked against Pillow in tests/test_bmp_decode_cpu.py):
  * headers of 12, 40, 52, 56, 64, 108 and 124 bytes; a height whose top byte is FF is top-down (height 2^32 - value), else bottom-up;
  * rows ((w * bits + 31) >> 3) & ~3 bytes apart, from the file header's offset -- offset 0: behind the header, the masks of a 40-byte
    header and the table; an offset that points AT the table of a 1-, 4- or 8-bit file is moved behind it;
  * 1, 4 and 8 bits: a table of ``colors`` (0: 1 << bits) entries B G R (3 bytes in a 12-byte header's file, else 4); mode 1 when it has
    two entries, black then white; L when entry i is (i & 255, i & 255, i & 255) for every i (a 2-entry table excepted), whatever the
    table's length; P otherwise, an index without an entry black -- a table of more than 256 entries that is no such ramp makes Pillow
    raise "invalid palette size" on load, and the plan refuses it (PALETTE);
  * 16 bits: 5-5-5 uncompressed, bit fields 5-6-5 or 5-5-5, a channel v expanded as v * 255 // 31 (// 63 for six bits); 24 bits B G R;
    32 bits B G R X uncompressed and the eight mask layouts, alpha dropped.
Refused although Pillow may read them (they take the host path): a table that makes Pillow's mode 1 or L on samples of another depth
(Pillow raises or reads the rows at the wrong depth: GRAY_TABLE), a table the file ends inside, RLE."""
import io
import struct

import numpy as np

REASONS = ("OK", "NOT_BMP", "TRUNCATED", "HEADER", "DIMENSIONS", "PIXELS", "DEPTH", "RLE", "COMPRESSION", "MASKS", "PALETTE", "GRAY_TABLE")
(OK, NOT_BMP, TRUNCATED, HEADER, DIMENSIONS, PIXELS, DEPTH, RLE, COMPRESSION, MASKS, PALETTE, GRAY_TABLE) = range(12)
MAX_PIXELS = 2 * 89478485
MODE_P, MODE_1, MODE_L, MODE_RGB = range(4)
PLAN_FIELDS = ("width", "height", "bits", "compression", "header_size", "top_down", "colors", "mode", "r_at", "g_at", "b_at", "six_bit_green",
               "table_offset", "table_entry", "row_stride", "data_offset", "supported", "reason")
# (r, g, b, a) masks of a 32-bit file -> the byte of a pixel that holds R, G, B
MASKS32 = {(0xFF0000, 0xFF00, 0xFF, 0): (2, 1, 0), (0xFF000000, 0xFF0000, 0xFF00, 0): (3, 2, 1), (0xFF000000, 0xFF00, 0xFF, 0): (3, 1, 0),
           (0xFF000000, 0xFF0000, 0xFF00, 0xFF): (3, 2, 1), (0xFF, 0xFF00, 0xFF0000, 0xFF000000): (0, 1, 2),
           (0xFF0000, 0xFF00, 0xFF, 0xFF000000): (2, 1, 0), (0xFF000000, 0xFF00, 0xFF, 0xFF0000): (3, 1, 0), (0, 0, 0, 0): (2, 1, 0)}


def plan(f):
    pl = {k: 0 for k in PLAN_FIELDS}

    def refuse(r):
        pl["reason"] = r
        return pl

    n = len(f)
    if n < 2 or f[:2] != b"BM":
        return refuse(NOT_BMP)
    if n < 18:
        return refuse(TRUNCATED)
    u16 = lambda at: struct.unpack_from("<H", f, at)[0]
    u32 = lambda at: struct.unpack_from("<I", f, at)[0]
    offset, hs = u32(10), u32(14)
    pl["header_size"] = hs
    if hs not in (12, 40, 52, 56, 64, 108, 124):
        return refuse(HEADER)
    if n < 14 + hs:
        return refuse(TRUNCATED)
    at = 14 + hs                                                         # Pillow's read position from here on
    if hs == 12:
        w, h, bits, comp, colors, entry = u16(18), u16(20), u16(24), 0, 0, 3
    else:
        w, h, bits, comp, colors, entry = u32(18), u32(22), u16(28), u32(30), u32(46), 4
        if f[25] == 0xFF:
            h, pl["top_down"] = 2 ** 32 - h, 1
    pl["bits"], pl["compression"] = bits, comp
    if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
        return refuse(DIMENSIONS)
    pl["width"], pl["height"] = w, h
    if w * h > MAX_PIXELS:
        return refuse(PIXELS)
    if not colors:
        colors = 1 << min(bits, 31)
    if offset == 14 + hs and bits <= 8:
        offset += entry * colors
    if bits not in (1, 4, 8, 16, 24, 32):
        return refuse(DEPTH)
    pl["mode"], pl["r_at"], pl["g_at"], pl["b_at"] = MODE_RGB, 2, 1, 0
    if comp == 3:
        if hs >= 52:
            masks = (u32(54), u32(58), u32(62), u32(66) if hs >= 56 else 0)
        else:
            if n < at + 12:
                return refuse(TRUNCATED)
            masks = (u32(at), u32(at + 4), u32(at + 8), 0)
            at += 12
        if bits == 32 and masks in MASKS32:
            pl["r_at"], pl["g_at"], pl["b_at"] = MASKS32[masks]
        elif bits == 24 and masks[:3] == (0xFF0000, 0xFF00, 0xFF):
            pass
        elif bits == 16 and masks[:3] in ((0xF800, 0x7E0, 0x1F), (0x7C00, 0x3E0, 0x1F)):
            pl["six_bit_green"] = int(masks[1] == 0x7E0)
        else:
            return refuse(MASKS)
    elif comp in (1, 2):
        return refuse(RLE)
    elif comp != 0:
        return refuse(COMPRESSION)
    if bits <= 8:
        if not 0 < colors <= 65536:
            return refuse(PALETTE)
        pl["colors"], pl["table_offset"], pl["table_entry"] = colors, at, entry
        if n < at + entry * colors:
            return refuse(TRUNCATED)
        table = [f[at + entry * i:at + entry * i + 3] for i in range(colors)]
        at += entry * colors
        want = (0, 255) if colors == 2 else range(colors)
        if all(t == bytes([v & 255]) * 3 for t, v in zip(table, want)):
            if bits == 1 and colors == 2:
                pl["mode"] = MODE_1
            elif bits == 8 and colors != 2:
                pl["mode"] = MODE_L
            else:
                return refuse(GRAY_TABLE)
        elif colors > 256:
            return refuse(PALETTE)                                       # Pillow opens such a file and raises "invalid palette size" on load
        else:
            pl["mode"] = MODE_P
    pl["row_stride"] = ((w * bits + 31) >> 3) & ~3
    pl["data_offset"] = offset or at
    if n < pl["data_offset"] + pl["row_stride"] * h:
        return refuse(TRUNCATED)
    pl["supported"] = 1
    return pl


def decode(f):
    """-> dict(plan, rgb, gray)"""
    pl = plan(f)
    assert pl["supported"], pl["reason"]
    w, h, bits, stride = pl["width"], pl["height"], pl["bits"], pl["row_stride"]
    rows = np.frombuffer(f, np.uint8, stride * h, pl["data_offset"]).reshape(h, stride)
    if not pl["top_down"]:
        rows = rows[::-1]
    luma = lambda rgb: ((rgb[..., 0].astype(np.int32) * 9797 + rgb[..., 1].astype(np.int32) * 19234 + rgb[..., 2].astype(np.int32) * 3737) >> 15).astype(np.uint8)
    if bits <= 8:
        x = np.arange(w)
        if bits == 1:
            v = (rows[:, x >> 3] >> (7 - (x & 7))) & 1
        elif bits == 4:
            v = (rows[:, x >> 1] >> np.where(x & 1, 0, 4)) & 15
        else:
            v = rows[:, :w]
        if pl["mode"] in (MODE_1, MODE_L):
            gray = (v * 255).astype(np.uint8) if pl["mode"] == MODE_1 else v.astype(np.uint8)
            return dict(plan=pl, rgb=np.repeat(gray[:, :, None], 3, axis=2), gray=np.ascontiguousarray(gray))
        table = np.zeros((max(256, pl["colors"]), 3), np.uint8)
        e = pl["table_entry"]
        raw = np.frombuffer(f, np.uint8, e * pl["colors"], pl["table_offset"]).reshape(-1, e)
        table[:pl["colors"]] = raw[:, 2::-1]
        rgb = table[v]
    elif bits == 16:
        px = rows[:, 0:2 * w:2].astype(np.int32) | (rows[:, 1:2 * w:2].astype(np.int32) << 8)
        if pl["six_bit_green"]:
            r, g, b = (px >> 11) & 31, ((px >> 5) & 63) * 255 // 63, px & 31
        else:
            r, g, b = (px >> 10) & 31, ((px >> 5) & 31) * 255 // 31, px & 31
        rgb = np.stack([r * 255 // 31, g, b * 255 // 31], axis=2).astype(np.uint8)
    else:
        k = bits // 8
        px = rows[:, :k * w].reshape(h, w, k)
        rgb = np.ascontiguousarray(px[..., [pl["r_at"], pl["g_at"], pl["b_at"]]])
    return dict(plan=pl, rgb=np.ascontiguousarray(rgb), gray=luma(rgb))


# ------------------------------------------------------------------------------------------------ writers
def bmp_file(w, h, bits, pixels=None, header=40, top_down=False, compression=0, masks=None, table=None, colors=None, offset=None, seed=0, cut=0,
             height_field=None):
    """a BMP file: ``pixels``: the rows top to bottom as stored bytes (stride each), None: noise; ``table``: entries as (b, g, r) triples;
    ``masks``: (r, g, b[, a]); ``offset``: the file header's offset field (None: where the rows are); ``cut``: bytes dropped from the end"""
    stride = ((w * bits + 31) >> 3) & ~3
    if pixels is None:
        pixels = np.random.default_rng(seed).integers(0, 256, stride * h, dtype=np.uint8).tobytes()
    rows = [pixels[i * stride:(i + 1) * stride] for i in range(h)]
    body = b"".join(rows if top_down else rows[::-1])
    entry = 3 if header == 12 else 4
    n_table = len(table) if table is not None else 0
    if header == 12:
        hd = struct.pack("<IHHHH", 12, w, h, 1, bits)
    else:
        hf = height_field if height_field is not None else ((2 ** 32 - h) if top_down else h)
        hd = struct.pack("<IIIHHIIIIII", header, w, hf, 1, bits, compression, len(body), 2835, 2835, n_table if colors is None else colors, 0)
        m = tuple(masks or ()) + (0,) * (4 - len(masks or ()))
        if header >= 52:
            hd += struct.pack("<III", *m[:3])
        if header >= 56:
            hd += struct.pack("<I", m[3])
        hd += bytes(header - len(hd))
        if header == 40 and compression == 3:
            hd += struct.pack("<III", *m[:3])
    tb = b"".join(bytes(t[:3]) + bytes(entry - 3) for t in (table or ()))
    where = 14 + len(hd) + len(tb)
    f = b"BM" + struct.pack("<IHHI", where + len(body), 0, 0, where if offset is None else offset) + hd + tb + body
    return f[:len(f) - cut] if cut else f


def rle8_file(gray, table):
    """a valid RLE8 file of a gray array [H,W] (the plan refuses it, Pillow reads it): one encoded run per pixel, end of line, end of bitmap"""
    h, w = gray.shape
    rows = b"".join(b"".join(bytes([1, int(v)]) for v in gray[y]) + b"\0\0" for y in range(h - 1, -1, -1)) + b"\0\1"
    head = bmp_file(w, 1, 8, pixels=bytes((w + 3) & ~3), compression=1, table=table, height_field=h)[:54 + 4 * len(table)]
    return head + rows


def grays(n):
    return [(i, i, i) for i in range(n)]


def colour_table(n, seed=0):
    return [tuple(int(v) for v in t) for t in np.random.default_rng(seed).integers(0, 256, (n, 3))]


def pillow_file(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="BMP", **kw)
    return buf.getvalue()


def matrix():
    """Pillow-written files: modes 1, L, P, RGB and RGBA, odd and even shapes"""
    from PIL import Image

    rng = np.random.default_rng(6)
    out = []
    for name, (h, w) in (("23x37", (23, 37)), ("1x1", (1, 1)), ("41x1", (41, 1)), ("1x41", (1, 41)), ("64x96", (64, 96))):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        out.append((f"mode1_{name}", pillow_file(Image.fromarray(a[..., 0] > 127))))
        out.append((f"modeL_{name}", pillow_file(Image.fromarray(a[..., 0]))))
        out.append((f"modeP_{name}", pillow_file(Image.fromarray(a[..., :3]).quantize(200))))
        out.append((f"modeP16_{name}", pillow_file(Image.fromarray(a[..., :3]).quantize(16))))
        out.append((f"modeRGB_{name}", pillow_file(Image.fromarray(a[..., :3]))))
        out.append((f"modeRGBA_{name}", pillow_file(Image.fromarray(a))))
    return out


def handbuilt():
    """every header size, depth, mask layout and direction; widths 1, 7, 8, 9, 31, 32 and 33 for the sub-byte rows"""
    out = []
    k = 0
    for header in (12, 40, 52, 56, 64, 108, 124):
        for top in (False, True):
            if header == 12 and top:
                continue
            for bits in (1, 4, 8, 16, 24, 32):
                k += 1
                table = colour_table(1 << bits, k) if bits <= 8 else None
                out.append((f"h{header}_{'top' if top else 'bottom'}_{bits}", bmp_file(13, 7, bits, header=header, top_down=top, table=table, seed=k)))
    for w in (1, 7, 8, 9, 31, 32, 33):
        for bits in (1, 4):
            out.append((f"w{w}_{bits}bit", bmp_file(w, 5, bits, table=colour_table(1 << bits, w), seed=w)))
        out.append((f"w{w}_1bit_bw", bmp_file(w, 5, 1, table=[(0, 0, 0), (255, 255, 255)], seed=w, top_down=bool(w & 1))))
    for i, m in enumerate(MASKS32):
        for header in (56, 124) if m[3] else (40, 52, 108):
            out.append((f"masks32_{i}_h{header}", bmp_file(11, 6, 32, header=header, compression=3, masks=m, seed=30 + i)))
    for header in (40, 52, 124):
        out.append((f"masks24_h{header}", bmp_file(11, 6, 24, header=header, compression=3, masks=(0xFF0000, 0xFF00, 0xFF), seed=40)))
        out.append((f"masks565_h{header}", bmp_file(11, 6, 16, header=header, compression=3, masks=(0xF800, 0x7E0, 0x1F), seed=41, top_down=True)))
        out.append((f"masks555_h{header}", bmp_file(11, 6, 16, header=header, compression=3, masks=(0x7C00, 0x3E0, 0x1F), seed=42)))
    all16 = np.arange(65536, dtype="<u2").tobytes()                          # every 16-bit pixel value, in all three layouts
    out.append(("all_555", bmp_file(256, 256, 16, pixels=all16)))
    out.append(("all_565", bmp_file(256, 256, 16, pixels=all16, compression=3, masks=(0xF800, 0x7E0, 0x1F))))
    out.append(("gray_ramp_8bit", bmp_file(13, 7, 8, table=grays(256), seed=50)))
    out.append(("gray_ramp_8bit_16_entries", bmp_file(13, 7, 8, table=grays(16), seed=51)))          # mode L whatever the samples
    out.append(("gray_ramp_8bit_300_entries", bmp_file(13, 7, 8, table=[(i & 255,) * 3 for i in range(300)], seed=62)))   # mode L: Pillow reads it
    out.append(("short_table_8bit", bmp_file(13, 7, 8, table=colour_table(16, 52), seed=52)))       # indices without an entry
    out.append(("short_table_4bit", bmp_file(13, 7, 4, table=colour_table(5, 53), seed=53)))
    out.append(("one_colour_1bit", bmp_file(13, 7, 1, table=colour_table(1, 54), seed=54)))
    out.append(("white_then_black", bmp_file(13, 7, 1, table=[(255, 255, 255), (0, 0, 0)], seed=55)))  # not black then white: mode P
    out.append(("colors_field_0", bmp_file(13, 7, 4, table=colour_table(16, 56), colors=0, seed=56)))
    out.append(("offset_at_the_table", bmp_file(13, 7, 8, table=colour_table(256, 57), offset=54, seed=57)))
    out.append(("offset_0", bmp_file(13, 7, 24, offset=0, seed=58)))
    out.append(("offset_0_with_table", bmp_file(13, 7, 4, table=colour_table(16, 59), offset=0, seed=59)))
    out.append(("gap_before_rows", bmp_file(13, 7, 24, seed=60)[:54] + bytes(10) + bmp_file(13, 7, 24, seed=60)[54:]))
    out[-1] = (out[-1][0], out[-1][1][:10] + struct.pack("<I", 64) + out[-1][1][14:])
    out.append(("bytes_behind_the_rows", bmp_file(13, 7, 24, seed=61) + b"trailing"))
    return out


def refusals():
    """[(name, file, reason)]"""
    g = bmp_file(13, 7, 24, seed=1)
    t16 = colour_table(16, 2)
    return [("not_bmp", b"BA" + g[2:], NOT_BMP), ("empty", b"", NOT_BMP), ("gif", b"GIF89a" + bytes(40), NOT_BMP),
            ("file_header_cut", g[:17], TRUNCATED), ("header_cut", g[:40], TRUNCATED), ("rows_cut", bmp_file(13, 7, 24, seed=1, cut=1), TRUNCATED),
            ("table_cut", bmp_file(13, 7, 8, table=colour_table(256, 3), seed=3)[:500], TRUNCATED),
            ("masks_cut", bmp_file(11, 6, 32, compression=3, masks=(0xFF0000, 0xFF00, 0xFF), seed=4)[:60], TRUNCATED),
            ("header_16", g[:14] + struct.pack("<I", 16) + g[18:], HEADER), ("header_0", g[:14] + bytes(4) + g[18:], HEADER),
            ("zero_width", bmp_file(0, 7, 24), DIMENSIONS), ("zero_height", bmp_file(13, 0, 24), DIMENSIONS),
            ("negative_width", g[:18] + struct.pack("<i", -13) + g[22:], DIMENSIONS),
            ("too_many_pixels", g[:18] + struct.pack("<II", 60000, 60000) + g[26:], PIXELS),
            ("depth_2", bmp_file(13, 7, 2, table=colour_table(4, 5)), DEPTH), ("depth_48", bmp_file(13, 7, 48), DEPTH), ("depth_0", bmp_file(13, 7, 0), DEPTH),
            ("rle8", bmp_file(13, 7, 8, compression=1, table=colour_table(256, 6)), RLE), ("rle4", bmp_file(13, 7, 4, compression=2, table=t16), RLE),
            ("jpeg", bmp_file(13, 7, 24, compression=4), COMPRESSION), ("png", bmp_file(13, 7, 24, compression=5), COMPRESSION),
            ("alpha_bitfields", bmp_file(13, 7, 32, compression=6), COMPRESSION),
            ("masks_other_32", bmp_file(11, 6, 32, compression=3, masks=(0xFF00, 0xFF0000, 0xFF000000)), MASKS),
            ("masks_other_16", bmp_file(11, 6, 16, compression=3, masks=(0xF00, 0xF0, 0xF)), MASKS),
            ("masks_alpha_in_h40", bmp_file(11, 6, 32, header=52, compression=3, masks=(0xFF, 0xFF00, 0xFF0000)), MASKS),
            ("masks_8bit", bmp_file(11, 6, 8, compression=3, masks=(0xFF0000, 0xFF00, 0xFF), table=colour_table(256, 7)), MASKS),
            ("table_of_70000", bmp_file(13, 7, 8, table=colour_table(16, 8), colors=70000), PALETTE),
            ("table_of_257_8bit", bmp_file(13, 7, 8, table=colour_table(257, 13), seed=13), PALETTE),
            ("table_of_300_8bit", bmp_file(13, 7, 8, table=colour_table(300, 14), seed=14), PALETTE),
            ("table_of_300_4bit", bmp_file(13, 7, 4, table=colour_table(300, 15), seed=15), PALETTE),
            ("table_of_300_1bit", bmp_file(13, 7, 1, table=colour_table(300, 16), seed=16), PALETTE),
            ("table_of_65536_8bit", bmp_file(13, 7, 8, table=colour_table(65536, 17), seed=17), PALETTE),
            ("gray_ramp_4bit", bmp_file(13, 7, 4, table=grays(16), seed=9), GRAY_TABLE),
            ("black_white_8bit", bmp_file(13, 7, 8, table=[(0, 0, 0), (255, 255, 255)], seed=10), GRAY_TABLE),
            ("black_white_4bit", bmp_file(13, 7, 4, table=[(0, 0, 0), (255, 255, 255)], seed=11), GRAY_TABLE),
            ("one_black_entry_1bit", bmp_file(13, 7, 1, table=[(0, 0, 0)], seed=12), GRAY_TABLE)]
