"""The device TIFF decoder (csrc/tiffdec.hip, csrc/tiff_parse.h, csrc/tiff_codecs.h) restated in numpy / plain python: the IFD walk with
its refusal reasons, the four strip codecs (none, PackBits, LZW, Deflate), predictor 2 and the output rules -- and the writers of the
files the tests need: Pillow's own over a matrix, hand-built files Pillow never writes, hand-written code streams, damaged strips and one
file per refusal reason.  What the restatement gives for a sound file is checked against ``reader.decode_file`` (Pillow + the stated gray
rule) in tests/test_tiff_decode_cpu.py; the library is then checked against the restatement stage by stage.

Rules pinned here:
  * ColorMap: a colour is the HIGH byte of its SHORT (``value >> 8``), Pillow's rule (TiffImagePlugin: ``b // 256``).
  * LZW: MSB-first codes, the early change (a code has 9 bits while the next free entry is below 511, 10 below 1023, 11 below 2047,
    else 12); an entry is added from the second code behind a Clear on; a strip starts with a Clear (stricter than libtiff).
  * A strip is damaged when it ends before ``rows * row_bytes`` bytes, when a run or a string would cross that count (libtiff cuts such a
    run and goes on: the device reports the file and the host path decides), when an LZW code is above the next free entry or the code
    behind a Clear is no literal, and when a Deflate strip fails zlib's header, stream or Adler-32 checks.  Bytes behind the point where
    the count is reached are never read.
  * "A strip count that does not fit" has two readings and both are here: a strip TABLE whose length is not ceil(height / rows) is a
    refusal of the plan (``STRIPS``); a strip whose BYTE count is short of its rows is damage (``raw_short_count``).
"""
import io
import struct
import zlib

import numpy as np

REASONS = ("OK", "NOT_TIFF", "BIGTIFF", "TRUNCATED", "HEADER", "DIMENSIONS", "TILES", "PLANAR", "FILL_ORDER", "DEPTH", "SUBBYTE", "GRAY_ALPHA",
           "ASSOC_ALPHA", "PHOTOMETRIC", "SAMPLES", "JPEG", "CCITT", "COMPRESSION", "PREDICTOR", "OLD_LZW", "STRIPS", "PALETTE")
globals().update({name: i for i, name in enumerate(REASONS)})                # bbocr.h BBOCR_TIFF_*
MAX_PIXELS = 2 * 89478485
STREAM_MAX = 0x7FFFFFFF
PLAN_FIELDS = ("width", "height", "bits", "samples", "photometric", "compression", "predictor", "big_endian", "rows_per_strip", "strips",
               "extra_sample", "row_bytes", "strip_bytes", "supported", "reason")


class Damaged(Exception):
    """a strip the decoder must answer with a status"""


# ------------------------------------------------------------------------------------------------ the walk
def walk(f):
    """-> (plan dict with PLAN_FIELDS, [(offset, stored bytes)] of the strips, palette uint8 [256,3] or None); the order of the checks is
    csrc/tiff_parse.h's"""
    pl = dict.fromkeys(PLAN_FIELDS, 0)
    pl["extra_sample"] = -1
    strips = []

    def refuse(reason):
        pl["supported"], pl["reason"] = 0, reason
        return pl, strips, None

    n = len(f)
    if n < 8 or f[:2] not in (b"II", b"MM"):
        return refuse(NOT_TIFF)
    E = ">" if f[:2] == b"MM" else "<"
    pl["big_endian"] = int(E == ">")
    magic = struct.unpack_from(E + "H", f, 2)[0]
    if magic == 43:
        return refuse(BIGTIFF)
    if magic != 42:
        return refuse(NOT_TIFF)
    ifd = struct.unpack_from(E + "I", f, 4)[0]
    if ifd > n or n - ifd < 2:
        return refuse(TRUNCATED)
    entries = struct.unpack_from(E + "H", f, ifd)[0]
    if (n - ifd - 2) // 12 < entries:
        return refuse(TRUNCATED)
    tags = {}
    for e in range(entries):
        at = ifd + 2 + 12 * e
        tag, typ, count = struct.unpack_from(E + "HHI", f, at)
        tags[tag] = (typ, count, at + 8)

    def values(tag):
        """-> (present, reason or 0, list)"""
        if tag not in tags:
            return False, 0, []
        typ, count, at = tags[tag]
        size = {1: 1, 3: 2, 4: 4}.get(typ, 0)
        if not size or count == 0:
            return True, HEADER, []
        if count * size > 4:
            at = struct.unpack_from(E + "I", f, at)[0]
            if at > n or (n - at) // size < count:
                return True, TRUNCATED, []
        return True, 0, list(struct.unpack_from(E + str(count) + {1: "B", 2: "H", 4: "I"}[size], f, at))

    def scalar(tag, default, required=False):
        has, r, v = values(tag)
        if r:
            return r, 0
        if not has and required:
            return HEADER, 0
        return 0, (v[0] if has else default)

    if any(t in tags for t in (322, 323, 324, 325)):
        return refuse(TILES)
    r, w = scalar(256, 0, True)
    if r:
        return refuse(r)
    r, h = scalar(257, 0, True)
    if r:
        return refuse(r)
    if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
        return refuse(DIMENSIONS)
    pl["width"], pl["height"] = w, h
    if w * h > MAX_PIXELS:
        return refuse(DIMENSIONS)
    r, comp = scalar(259, 1)
    if r:
        return refuse(r)
    pl["compression"] = comp
    if comp in (6, 7):
        return refuse(JPEG)
    if comp in (2, 3, 4):
        return refuse(CCITT)
    if comp not in (1, 5, 8, 32946, 32773):
        return refuse(COMPRESSION)
    r, planar = scalar(284, 1)
    if r:
        return refuse(r)
    if planar != 1:
        return refuse(PLANAR)
    r, fill = scalar(266, 1)
    if r:
        return refuse(r)
    if fill != 1:
        return refuse(FILL_ORDER)
    r, samples = scalar(277, 1)
    if r:
        return refuse(r)
    if samples == 0 or samples > 64:
        return refuse(SAMPLES)
    pl["samples"] = samples
    has, r, bits = values(258)
    if r:
        return refuse(r)
    if not has:
        bits = [1]
    if len(bits) != samples:
        return refuse(HEADER)
    pl["bits"] = bits[0]
    if any(b != bits[0] for b in bits):
        return refuse(DEPTH)
    has, r, fmt = values(339)
    if r:
        return refuse(r)
    if has and any(s != 1 for s in fmt):
        return refuse(DEPTH)
    if bits[0] in (2, 4):
        return refuse(SUBBYTE)
    if bits[0] not in (1, 8):
        return refuse(DEPTH)
    r, phot = scalar(262, 0, True)
    if r:
        return refuse(r)
    pl["photometric"] = phot
    if phot > 3:
        return refuse(PHOTOMETRIC)
    has, r, extra = values(338)
    if r:
        return refuse(r)
    palette = None
    if phot <= 1:
        if samples == 2:
            return refuse(GRAY_ALPHA)
        if samples != 1:
            return refuse(SAMPLES)
    elif phot == 2:
        if bits[0] != 8:
            return refuse(DEPTH)
        if samples == 4:
            if len(extra) != 1:
                return refuse(SAMPLES)
            if extra[0] == 1:
                return refuse(ASSOC_ALPHA)
            if extra[0] not in (0, 2):
                return refuse(SAMPLES)
            pl["extra_sample"] = extra[0]
        elif samples != 3:
            return refuse(SAMPLES)
    else:
        if bits[0] != 8:
            return refuse(DEPTH)
        if samples != 1:
            return refuse(SAMPLES)
        has, r, cmap = values(320)
        if r == TRUNCATED:
            return refuse(r)
        if not has or r or tags[320][0] != 3 or len(cmap) != 768:
            return refuse(PALETTE)
        palette = (np.array(cmap, np.uint32).reshape(3, 256).T >> 8).astype(np.uint8)          # the high byte: Pillow's rule
    pl["row_bytes"] = (w * samples * bits[0] + 7) // 8
    if pl["row_bytes"] > STREAM_MAX // h:
        return refuse(DIMENSIONS)
    r, pred = scalar(317, 1)
    if r:
        return refuse(r)
    pl["predictor"] = pred
    if pred != 1 and not (pred == 2 and bits[0] == 8 and comp in (5, 8, 32946)):
        return refuse(PREDICTOR)
    r, rows = scalar(278, 0xFFFFFFFF)
    if r:
        return refuse(r)
    if rows == 0:
        return refuse(STRIPS)
    rows = min(rows, h)
    pl["rows_per_strip"] = rows
    nstrips = -(-h // rows)
    pl["strips"] = nstrips
    has_o, r_o, offs = values(273)
    if r_o == TRUNCATED:
        return refuse(r_o)
    has_c, r_c, counts = values(279)
    if r_c == TRUNCATED:
        return refuse(r_c)
    if r_o or r_c:
        return refuse(HEADER)
    if not has_o or not has_c or len(offs) != nstrips or len(counts) != nstrips:
        return refuse(STRIPS)
    for o, c in zip(offs, counts):
        if o > n or c > n - o:
            return refuse(TRUNCATED)
        strips.append((o, c))
        pl["strip_bytes"] += c
    if comp == 5 and counts[0] >= 2 and f[offs[0]] == 0 and f[offs[0] + 1] & 1:
        return refuse(OLD_LZW)
    pl["supported"], pl["reason"] = 1, OK
    return pl, strips, palette


def plan(f):
    return walk(f)[0]


# ------------------------------------------------------------------------------------------------ the codecs
def unpackbits(data, need):
    out, at = bytearray(), 0
    while len(out) < need:
        if at >= len(data):
            raise Damaged("packbits: input")
        hdr = data[at] - 256 if data[at] > 127 else data[at]
        at += 1
        if hdr == -128:
            continue
        if hdr < 0:
            if at >= len(data):
                raise Damaged("packbits: input")
            if 1 - hdr > need - len(out):
                raise Damaged("packbits: overrun")
            out += bytes([data[at]]) * (1 - hdr)
            at += 1
        else:
            if hdr + 1 > len(data) - at:
                raise Damaged("packbits: input")
            if hdr + 1 > need - len(out):
                raise Damaged("packbits: overrun")
            out += data[at:at + hdr + 1]
            at += hdr + 1
    return bytes(out)


def lzw_width(next_free):
    return 9 if next_free < 511 else (10 if next_free < 1023 else (11 if next_free < 2047 else 12))


def unlzw(data, need, codes_out=None):
    """the match copy of csrc/tiff_codecs.h: an entry is (offset in the output, length).  ``need`` None: everything up to the EOI code"""
    until_eoi, need = need is None, (1 << 62 if need is None else need)
    out = bytearray()
    bitpos, nbits = 0, 8 * len(data)
    table = {}
    next_free, prev, first = 258, None, True
    while len(out) < need:
        w = lzw_width(next_free)
        if bitpos + w > nbits:
            raise Damaged("lzw: input")
        byte, shift = divmod(bitpos, 8)
        code = (int.from_bytes(data[byte:byte + 3], "big") >> (24 - shift - w)) & ((1 << w) - 1) if byte + 3 <= len(data) else \
            (int.from_bytes(data[byte:].ljust(3, b"\0"), "big") >> (24 - shift - w)) & ((1 << w) - 1)
        bitpos += w
        if codes_out is not None:
            codes_out.append((code, w))
        if first and code != 256:
            raise Damaged("lzw: no clear at the start")
        first = False
        if code == 256:
            next_free, prev = 258, None
            continue
        if code == 257:
            if until_eoi:
                return bytes(out)
            raise Damaged("lzw: eoi before the count")
        o = len(out)
        if prev is None:
            if code > 255:
                raise Damaged("lzw: no literal behind a clear")
            out.append(code)
            prev = (o, 1)
            continue
        if code > next_free or (code == next_free and next_free >= 4096):
            raise Damaged("lzw: code above the next free entry")
        if code < 256:
            src, ln = None, 1
        elif code == next_free:
            src, ln = prev[0], prev[1] + 1
        else:
            src, ln = table[code]
        if ln > need - o:
            raise Damaged("lzw: overrun")
        if next_free < 4096:
            table[next_free] = (prev[0], prev[1] + 1)
            next_free += 1
        if src is None:
            out.append(code)
        else:
            for i in range(ln):                                   # in order: the KwKwK byte is there when it is read
                out.append(out[src + i])
        prev = (o, ln)
    return bytes(out)


def inflate_strip(data, need):
    if len(data) < 2 or data[0] & 15 != 8 or data[0] >> 4 > 7 or data[1] & 0x20 or ((data[0] << 8) | data[1]) % 31:
        raise Damaged("deflate: zlib header")
    o = zlib.decompressobj()
    try:
        out = o.decompress(data)
    except zlib.error as e:
        raise Damaged("deflate: %s" % e)
    if not o.eof or len(out) != need:
        raise Damaged("deflate: %d bytes for %d, eof %s" % (len(out), need, o.eof))
    return out


def decode_strip(comp, data, need):
    if comp == 1:
        if len(data) < need:
            raise Damaged("raw: short strip")
        return bytes(data[:need])
    return {32773: unpackbits, 5: unlzw}.get(comp, inflate_strip)(data, need)


def decode(f):
    """-> dict(plan, stage0: the strips' stream, stage1: after the predictor (bytes), rgb [H,W,3], gray [H,W]); Damaged for a damaged strip"""
    pl, strips, palette = walk(f)
    assert pl["supported"], REASONS[pl["reason"]]
    H, W, S, rb, rows = pl["height"], pl["width"], pl["samples"], pl["row_bytes"], pl["rows_per_strip"]
    stage0 = b"".join(decode_strip(pl["compression"], f[o:o + c], min(rows, H - s * rows) * rb) for s, (o, c) in enumerate(strips))
    a = np.frombuffer(stage0, np.uint8).reshape(H, rb)
    if pl["predictor"] == 2:
        a = np.cumsum(a.reshape(H, W, S), axis=1, dtype=np.uint32).astype(np.uint8).reshape(H, rb)
    stage1 = a.tobytes()
    if pl["bits"] == 1:
        v = np.unpackbits(a, axis=1)[:, :W] * np.uint8(255)
    else:
        v = a.reshape(H, W, S)
    phot = pl["photometric"]
    if phot <= 1:
        g = v.reshape(H, W)
        g = 255 - g if phot == 0 else g
        rgb, gray = np.repeat(g[..., None], 3, axis=2), g
    else:
        rgb = palette[v.reshape(H, W)] if phot == 3 else v[..., :3]
        q = rgb.astype(np.int32)
        gray = ((q[..., 0] * 9797 + q[..., 1] * 19234 + q[..., 2] * 3737) >> 15).astype(np.uint8)
    return dict(plan=pl, stage0=stage0, stage1=stage1, rgb=np.ascontiguousarray(rgb), gray=np.ascontiguousarray(gray))


# ------------------------------------------------------------------------------------------------ encoders
def packbits_encode(data):
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j + 1 < n and data[j + 1] == data[i] and j - i < 127:
            j += 1
        if j > i:
            out += bytes([257 - (j - i + 1), data[i]])
            i = j + 1
            continue
        j = i
        while j + 1 < n and j - i < 127 and not (j + 2 < n and data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([j - i]) + bytes(data[i:j + 1])
        i = j + 1
    return bytes(out)


def lzw_pack(codes):
    """codes (Clear and EOI included) -> bytes; every code written with the width the DECODER reads it with"""
    acc, nacc, out = 0, 0, bytearray()
    next_free, behind_clear = 258, True
    for c in codes:
        w = lzw_width(next_free)
        acc, nacc = (acc << w) | c, nacc + w
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 255)
            nacc -= 8
        acc &= (1 << nacc) - 1
        if c == 256:
            next_free, behind_clear = 258, True
        elif c != 257:
            if not behind_clear and next_free < 4096:
                next_free += 1
            behind_clear = False
    if nacc:
        out.append((acc << (8 - nacc)) & 255)
    return bytes(out)


def lzw_codes(data, eoi=True):
    """the greedy encoder: Clear first, a Clear when the table holds entry 4093 (libtiff's rule), EOI last -> the code list"""
    codes, table, next_enc = [256], {}, 258
    w = b""
    for b in data:
        wc = w + bytes([b])
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        codes.append(w[0] if len(w) == 1 else table[w])
        table[wc] = next_enc
        next_enc += 1
        if next_enc == 4094:
            codes.append(256)
            table, next_enc = {}, 258
        w = bytes([b])
    if w:
        codes.append(w[0] if len(w) == 1 else table[w])
    return codes + ([257] if eoi else [])


def lzw_encode(data):
    return lzw_pack(lzw_codes(data))


def encode_strip(comp, data, level=6):
    return {1: bytes, 32773: packbits_encode, 5: lzw_encode}.get(comp, lambda d: zlib.compress(d, level))(data)


# ------------------------------------------------------------------------------------------------ the hand-built file
def tiff_file(stream, width, height, bits=8, samples=1, photometric=1, compression=1, predictor=None, rows_per_strip=None, order="II",
              strip_order="forward", gap=0, short_tables=False, extra_samples=None, colormap=None, extra_tags=(), strips=None, drop_tags=(),
              magic=42, table_strips=None, planar=None, fill_order=None, sample_format=None, bits_list=None):
    """A classic TIFF of the decoded stream ``stream`` (height * row_bytes bytes, the predictor NOT yet applied: it is applied here).
    ``rows_per_strip`` None: the tag is absent (one strip).  ``strips``: the stored strips themselves instead of encoding ``stream``.
    ``strip_order`` "reverse": the last strip stands first in the file; ``gap``: that many filler bytes between strips; ``short_tables``:
    SHORT strip tables; ``table_strips``: the table's length when it shall differ; ``extra_tags``: [(tag, type, values)]."""
    E = ">" if order == "MM" else "<"
    rb = (width * samples * bits + 7) // 8
    rows = min(rows_per_strip if rows_per_strip is not None else height, height) or height
    nstrips = -(-height // rows)
    if strips is None:
        a = np.frombuffer(bytes(stream), np.uint8).reshape(height, rb)
        if predictor == 2:
            p = a.reshape(height, width, samples).astype(np.int16)
            p[:, 1:] -= p[:, :-1].copy()
            a = p.astype(np.uint8).reshape(height, rb)
        strips = [encode_strip(compression, a[s * rows:(s + 1) * rows].tobytes()) for s in range(nstrips)]
    body = bytearray(b"\0" * 8)
    offs = [0] * len(strips)
    for s in (range(len(strips) - 1, -1, -1) if strip_order == "reverse" else range(len(strips))):
        body += b"\xAA" * gap
        offs[s] = len(body)
        body += strips[s]
    if len(body) & 1:
        body += b"\0"
    counts = [len(s) for s in strips]
    if table_strips is not None:
        offs, counts = (offs * table_strips)[:table_strips], (counts * table_strips)[:table_strips]
    tt = 3 if short_tables else 4
    tags = [(256, 4, [width]), (257, 4, [height]), (258, 3, bits_list or [bits] * samples), (259, 3, [compression]), (262, 3, [photometric]),
            (273, tt, offs), (277, 3, [samples]), (279, tt, counts)]
    if rows_per_strip is not None:
        tags.append((278, 4, [rows_per_strip]))
    for tag, val in ((317, predictor), (284, planar), (266, fill_order)):
        if val is not None:
            tags.append((tag, 3, [val]))
    if extra_samples is not None:
        tags.append((338, 3, list(extra_samples)))
    if sample_format is not None:
        tags.append((339, 3, [sample_format] * samples))
    if colormap is not None:
        tags.append((320, 3, list(colormap)))
    tags += list(extra_tags)
    tags = sorted((t for t in tags if t[0] not in drop_tags), key=lambda t: t[0])
    ifd_at = len(body)
    data_at = ifd_at + 2 + 12 * len(tags) + 4
    ifd, data = struct.pack(E + "H", len(tags)), bytearray()
    for tag, typ, vals in tags:
        raw = struct.pack(E + str(len(vals)) + {1: "B", 3: "H", 4: "I"}[typ], *vals)
        if len(raw) <= 4:
            ifd += struct.pack(E + "HHI", tag, typ, len(vals)) + raw.ljust(4, b"\0")
        else:
            ifd += struct.pack(E + "HHII", tag, typ, len(vals), data_at + len(data))
            data += raw + (b"\0" if len(raw) & 1 else b"")
    body += ifd + struct.pack(E + "I", 0) + data
    body[:8] = (b"MM" if order == "MM" else b"II") + struct.pack(E + "HI", magic, ifd_at)
    return bytes(body)


def wrap_strip(comp, strip, width, height, **kw):
    """one stored strip as the only strip of a photometric-1, 8-bit file of width x height"""
    return tiff_file(None, width, height, compression=comp, strips=[strip], **kw)


# ------------------------------------------------------------------------------------------------ pictures
def picture(mode, w, h, seed):
    """a PIL image with flat runs, a gradient and noise, so that every codec meets runs, literals and matches"""
    from PIL import Image

    rng = np.random.default_rng(seed)
    ch = {"1": 1, "L": 1, "P": 1, "RGB": 3, "RGBA": 4}[mode]
    a = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    a[: h // 3] = (np.arange(w)[None, :, None] * 3 + np.arange(ch)[None, None] * 40) & 255
    a[h // 3: h // 2, : max(1, w // 2)] = 200
    if mode == "1":
        return Image.fromarray(a[..., 0] > 100)
    if mode in ("L", "P"):
        img = Image.fromarray(a[..., 0], "L")
        if mode == "P":
            img = Image.fromarray(a[..., 0], "P")
            img.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
        return img
    return Image.fromarray(a, mode)


MODES = ("1", "L", "P", "RGB", "RGBA")
COMPRESSIONS = ("raw", "packbits", "tiff_lzw", "tiff_adobe_deflate")
SHAPES = ((1, 7), (37, 23), (65, 50), (200, 131))             # (width, height): one pixel wide, no multiple of 8, one past a wave, the largest
STRIPPINGS = ("one", "few", "many")


def pillow_file(img, compression, predictor=1, stripping="one"):
    """Pillow's own writer with ``TiffImagePlugin.STRIP_SIZE`` set for one, about three, or one-row strips"""
    from PIL import TiffImagePlugin

    w, h = img.size
    stride = (w * {"1": 1, "L": 8, "P": 8, "RGB": 24, "RGBA": 32}[img.mode] + 7) // 8
    old = TiffImagePlugin.STRIP_SIZE
    TiffImagePlugin.STRIP_SIZE = {"one": 1 << 30, "few": stride * -(-h // 3), "many": 1}[stripping]
    try:
        b = io.BytesIO()
        img.save(b, "TIFF", compression=compression, **({"tiffinfo": {317: 2}} if predictor == 2 else {}))
    finally:
        TiffImagePlugin.STRIP_SIZE = old
    return b.getvalue()


def combos():
    for mode in MODES:
        for comp in COMPRESSIONS:
            for pred in (1, 2):
                if pred == 2 and (mode == "1" or comp in ("raw", "packbits")):
                    continue
                yield mode, comp, pred


def matrix(shapes=SHAPES):
    """[(name, file)]: every (mode, compression, predictor) with every shape; the stripping rotates so that every combination meets all
    three.  Computed once per process."""
    key = tuple(shapes)
    if key not in _MATRIX:
        out = []
        for ci, (mode, comp, pred) in enumerate(combos()):
            for si, (w, h) in enumerate(shapes):
                strip = STRIPPINGS[(ci + si) % 3]
                name = "%s-%s-p%d-%dx%d-%s" % (mode, comp, pred, w, h, strip)
                out.append((name, pillow_file(picture(mode, w, h, 100 * ci + si), comp, pred, strip)))
        _MATRIX[key] = out
    return _MATRIX[key]


_MATRIX = {}


def _noise(n, seed, levels=256):
    return np.random.default_rng(seed).integers(0, levels, n, dtype=np.uint8).tobytes()


def handbuilt():
    """[(name, file)]: files Pillow never writes, all within the plan's scope"""
    w, h = 37, 23
    L = _noise(w * h, 1, 7)
    bits1 = np.packbits(np.frombuffer(_noise(w * h, 2, 2), np.uint8).reshape(h, w), axis=1).tobytes()
    rgb = _noise(w * h * 3, 3, 5)
    rgbx = _noise(65 * 9 * 4, 4, 9)
    cmap = [int(v) for v in np.random.default_rng(5).integers(0, 65536, 768)]
    out = [
        ("mm_L_lzw", tiff_file(L, w, h, compression=5, rows_per_strip=5, order="MM")),
        ("mm_rgb_deflate_p2_short_tables", tiff_file(rgb, w, h, samples=3, photometric=2, compression=8, predictor=2, rows_per_strip=4, order="MM",
                                                     short_tables=True)),
        ("mm_palette_packbits", tiff_file(L, w, h, photometric=3, compression=32773, rows_per_strip=6, order="MM", colormap=cmap)),
        ("phot0_8bit", tiff_file(L, w, h, photometric=0, compression=32773, rows_per_strip=7)),
        ("phot0_1bit", tiff_file(bits1, w, h, bits=1, photometric=0, compression=5, rows_per_strip=8)),
        ("phot1_1bit_raw", tiff_file(bits1, w, h, bits=1, photometric=1, rows_per_strip=3)),
        ("reverse_gaps_lzw", tiff_file(rgb, w, h, samples=3, photometric=2, compression=5, rows_per_strip=4, strip_order="reverse", gap=5)),
        ("reverse_gaps_raw_short", tiff_file(L, w, h, rows_per_strip=2, strip_order="reverse", gap=3, short_tables=True)),
        ("rows_absent", tiff_file(L, w, h, compression=8)),
        ("rows_max", tiff_file(L, w, h, compression=5, rows_per_strip=0xFFFFFFFF)),
        ("one_row_strips_deflate_32946", tiff_file(rgb, w, h, samples=3, photometric=2, compression=32946, rows_per_strip=1)),
        ("one_row_strips_packbits", tiff_file(L, w, h, compression=32773, rows_per_strip=1)),
        ("rgbx_extra0_lzw_p2", tiff_file(rgbx, 65, 9, samples=4, photometric=2, compression=5, predictor=2, rows_per_strip=2, extra_samples=[0])),
        ("rgba_extra2_raw", tiff_file(rgbx, 65, 9, samples=4, photometric=2, rows_per_strip=4, extra_samples=[2])),
        ("rgb_raw_one_row_strips", tiff_file(rgb, w, h, samples=3, photometric=2, rows_per_strip=1)),
        ("palette_raw_few_strips", tiff_file(L, w, h, photometric=3, rows_per_strip=9, colormap=cmap)),
        ("width1_lzw",tiff_file(_noise(11, 6), 1, 11, compression=5, rows_per_strip=4)),
    ]
    return out


def _edge_codes(edge, seed):
    """literals until the decoder's next free entry is edge - 1, then the newest entry (read with the old width; it defines entry edge - 1
    and the width grows), that entry (the first code of the new width), KwKwK of the new width, a literal, EOI"""
    rng = np.random.default_rng(seed)
    codes = [256] + [int(v) for v in rng.integers(0, 256, edge - 1 - 258 + 1)]
    return codes + [edge - 2, edge - 1, edge + 1, 65, 257]


def handwritten():
    """[(name, compression, the stored strip, (width, height))]: code streams written by hand; what they decode to is the restatement's
    answer, which tests/test_tiff_decode_cpu.py holds against Pillow wherever Pillow accepts the file"""
    out = [
        ("lzw_kwkwk_first_entry", 5, lzw_pack([256, 65, 258, 66, 257]), (4, 1)),
        ("lzw_clear_mid_strip", 5, lzw_pack([256, 65, 66, 258, 256, 67, 68, 258, 259, 257]), (5, 2)),
        ("lzw_double_clear", 5, lzw_pack([256, 256, 65, 66, 258, 257]), (4, 1)),
        ("lzw_no_eoi", 5, lzw_pack([256, 65, 66, 258, 260, 67]), (4, 2)),
    ]
    for edge in (511, 1023, 2047):
        strip = lzw_pack(_edge_codes(edge, edge))
        n = len(unlzw_all(strip))
        out.append(("lzw_width_edge_%d" % edge, 5, strip, (n, 1)))
    noisy = _noise(100 * 70, 9)
    codes = lzw_codes(noisy)
    assert codes.count(256) >= 2                                                   # the table filled to 4093 entries and was cleared
    out.append(("lzw_table_fills_and_clears", 5, lzw_pack(codes), (100, 70)))
    lit128, rep128 = _noise(128, 10), b"\x07"
    out += [
        ("packbits_noop_header", 32773, bytes([0x80, 2, 1, 2, 3, 0x80, 0x80, 0xFE, 9]), (6, 1)),
        ("packbits_runs_of_128", 32773, bytes([127]) + lit128 + bytes([0x81]) + rep128, (64, 4)),
        ("packbits_run_crosses_rows", 32773, bytes([257 - 25, 5, 4]) + b"abcde", (10, 3)),
        ("packbits_bytes_behind", 32773, bytes([257 - 6, 1]) + b"\x03junk", (3, 2)),
    ]
    return out


def unlzw_all(strip):
    """the bytes a sound hand-written LZW strip holds up to its EOI (to size its file)"""
    return unlzw(strip, None)


def handwritten_files():
    return [(name, wrap_strip(comp, strip, w, h)) for name, comp, strip, (w, h) in handwritten()]


def damaged():
    """[(name, file)]: every file passes the plan and holds a damaged strip; none is built to do anything but end in a status.  Most
    have three strips of which the MIDDLE one is damaged."""
    w, h, rows = 37, 12, 4
    data = _noise(w * h, 11, 6)
    parts = [data[s * rows * w:(s + 1) * rows * w] for s in range(3)]

    def three(comp, middle):
        s = [encode_strip(comp, p) for p in parts]
        s[1] = middle(s[1])
        return tiff_file(None, w, h, compression=comp, rows_per_strip=rows, strips=s)

    half = lambda s: s[: len(s) // 2]
    out = [("%s_truncated" % n, three(c, half)) for n, c in (("raw", 1), ("packbits", 32773), ("lzw", 5), ("deflate", 8))]
    out.append(("raw_short_count", three(1, lambda s: s[:-1])))
    out.append(("lzw_code_above_next_free", three(5, lambda s: lzw_pack([256, 65, 66, 300] + [65] * 200))))
    out.append(("lzw_eoi_early", three(5, lambda s: lzw_pack([256, 65, 66, 257]))))
    out.append(("lzw_no_clear_at_start", three(5, lambda s: lzw_pack(lzw_codes(parts[1])[1:]))))
    out.append(("lzw_no_literal_behind_clear", three(5, lambda s: lzw_pack([256, 65, 256, 258] + [65] * 200))))
    # strips that over-produce: the last run / string / match crosses the strip's count
    out.append(("lzw_overproduces", three(5, lambda s: lzw_pack(lzw_codes(parts[1][:-1], eoi=False) + [258, 257]))))   # two bytes where one is left
    out.append(("packbits_overproduces", three(32773, lambda s: packbits_encode(parts[1][:-3]) + bytes([257 - 9, 1]))))
    out.append(("deflate_overproduces", three(8, lambda s: zlib.compress(parts[1] + b"tail"))))
    out.append(("deflate_adler", three(8, lambda s: s[:-1] + bytes([s[-1] ^ 1]))))
    out.append(("deflate_zlib_header", three(8, lambda s: bytes([s[0] ^ 0x0F]) + s[1:])))
    return out


def refusals():
    """[(name, file, reason)]: one file per reason (some reasons on more than one)"""
    w, h = 8, 4
    L = _noise(w * h, 12)
    ok = tiff_file(L, w, h, rows_per_strip=2)
    ifd = struct.unpack_from("<I", ok, 4)[0]
    cmap = [0] * 768
    out = [
        ("not_tiff", b"\x89PNG\r\n\x1a\n" + b"\0" * 16, NOT_TIFF),
        ("short_file", b"II*\0", NOT_TIFF),
        ("magic_41", tiff_file(L, w, h, magic=41), NOT_TIFF),
        ("bigtiff", tiff_file(L, w, h, magic=43), BIGTIFF),
        ("ifd_past_end", ok[:4] + struct.pack("<I", len(ok) + 4) + ok[8:], TRUNCATED),
        ("ifd_cut", ok[: ifd + 2 + 12 * 3], TRUNCATED),
        ("value_past_end", tiff_file(L, w, h, rows_per_strip=1)[:-6], TRUNCATED),
        ("strip_past_end", _retag(ok, 279, [2 * w + 4000, 2 * w]), TRUNCATED),
        ("no_width", tiff_file(L, w, h, drop_tags=(256,)), HEADER),
        ("no_photometric", tiff_file(L, w, h, drop_tags=(262,)), HEADER),
        ("bits_count", tiff_file(L * 3, w, h, samples=3, photometric=2, bits_list=[8]), HEADER),
        ("width_0", tiff_file(b"", 0, 1, strips=[b""]), DIMENSIONS),
        ("height_0", _retag(ok, 257, [0]), DIMENSIONS),
        ("too_many_pixels", tiff_file(None, 20000, 9000, strips=[b""]), DIMENSIONS),
        ("tiles", tiff_file(L, w, h, extra_tags=[(322, 3, [16]), (323, 3, [16])]), TILES),
        ("planar_2", tiff_file(L * 3, w, h, samples=3, photometric=2, planar=2), PLANAR),
        ("fill_order_2", tiff_file(L, w, h, fill_order=2), FILL_ORDER),
        ("16_bit", tiff_file(L * 2, w, h, bits=16), DEPTH),
        ("float", tiff_file(L * 4, w, h, bits=32, sample_format=3), DEPTH),
        ("signed", tiff_file(L, w, h, sample_format=2), DEPTH),
        ("4_bit", tiff_file(L[: w * h // 2], w, h, bits=4), SUBBYTE),
        ("2_bit", tiff_file(L[: w * h // 4], w, h, bits=2), SUBBYTE),
        ("gray_alpha", tiff_file(L * 2, w, h, samples=2, extra_samples=[2]), GRAY_ALPHA),
        ("associated_alpha", tiff_file(L * 4, w, h, samples=4, photometric=2, extra_samples=[1]), ASSOC_ALPHA),
        ("four_samples_no_extra", tiff_file(L * 4, w, h, samples=4, photometric=2), SAMPLES),
        ("cmyk", tiff_file(L * 4, w, h, samples=4, photometric=5), PHOTOMETRIC),
        ("ycbcr", tiff_file(L * 3, w, h, samples=3, photometric=6), PHOTOMETRIC),
        ("cielab", tiff_file(L * 3, w, h, samples=3, photometric=8), PHOTOMETRIC),
        ("jpeg", tiff_file(L, w, h, compression=7, strips=[L]), JPEG),
        ("old_jpeg", tiff_file(L, w, h, compression=6, strips=[L]), JPEG),
        ("ccitt_g3", tiff_file(L[:4], w, h, bits=1, compression=3, strips=[L]), CCITT),
        ("ccitt_g4", tiff_file(L[:4], w, h, bits=1, compression=4, strips=[L]), CCITT),
        ("zstd", tiff_file(L, w, h, compression=50000, strips=[L]), COMPRESSION),
        ("predictor_3", tiff_file(L, w, h, compression=5, strips=[lzw_encode(L)], extra_tags=[(317, 3, [3])]), PREDICTOR),
        ("predictor_2_raw", tiff_file(L, w, h, extra_tags=[(317, 3, [2])]), PREDICTOR),
        ("predictor_2_1bit", tiff_file(L[:4], w, h, bits=1, compression=5, strips=[lzw_encode(L[:4])], extra_tags=[(317, 3, [2])]), PREDICTOR),
        ("old_lzw", tiff_file(L, w, h, compression=5, strips=[b"\x00\x01" + L]), OLD_LZW),
        ("strip_table_length", tiff_file(L, w, h, rows_per_strip=2, table_strips=3), STRIPS),
        ("rows_per_strip_0", tiff_file(L, w, h, strips=[L], extra_tags=[(278, 4, [0])]), STRIPS),
        ("no_strip_table", tiff_file(L, w, h, drop_tags=(273,)), STRIPS),
        ("no_colormap", tiff_file(L, w, h, photometric=3), PALETTE),
        ("colormap_length", tiff_file(L, w, h, photometric=3, colormap=cmap[:48]), PALETTE),
        ("palette_1bit", tiff_file(L[:4], w, h, bits=1, photometric=3, colormap=cmap[:6]), DEPTH),
    ]
    return out


def _retag(f, tag, vals):
    """little-endian file ``f`` with the inline LONG / SHORT values of ``tag`` rewritten"""
    f = bytearray(f)
    ifd = struct.unpack_from("<I", f, 4)[0]
    for e in range(struct.unpack_from("<H", f, ifd)[0]):
        at = ifd + 2 + 12 * e
        t, typ, count = struct.unpack_from("<HHI", f, at)
        if t == tag:
            size = 2 if typ == 3 else 4
            where = at + 8 if count * size <= 4 else struct.unpack_from("<I", f, at + 8)[0]
            struct.pack_into("<%d%s" % (len(vals), "H" if typ == 3 else "I"), f, where, *vals)
    return bytes(f)
