"""The CCITT side of the device TIFF decoder (csrc/tiff_fax.h, the lenient walk of csrc/tiff_parse.h) restated in plain python: the code
tables of T.4 / T.6, an encoder for the three TIFF schemes, the STRICT decoder the device runs, the plan walk with the reasons of
``bbocr_host_tiff_fax_plan``, designed pages and a damage list.  What the restatement gives for a sound file is checked against
``reader.decode_file`` (Pillow with libtiff) in tests/test_tiff_fax_cpu.py; the library is then checked against the restatement.

Rules pinned here:
  * A white run decodes to 0 bits, a black run to 1 bits; the photometric tag is the output pass's business.
  * Compression 2: a row is a sequence of runs, white first, and starts on a byte boundary; no EOL.  Compression 3: every row is preceded by
    an EOL (any number of 0 bits, at least eleven, then a 1), with T4Options bit 0 followed by a tag bit (1: a 1-D row, 0: a 2-D row).
    Compression 4: 2-D rows back to back.  The reference line of a strip's first row is white.
  * A run is any number of make-up codes and one terminating code.  A row ends when its runs reach the width -- exactly.
  * The changing elements of a row are kept as DECODED (a zero-length run leaves two equal elements), and b1 is the first element of the
    reference line right of a0 whose index has the parity of the colour being coded: what libtiff does with its run arrays.
  * FillOrder 2: the bits of every stored byte are reversed on read.
  * Strict: a pattern that is no code, an extension code, runs beyond the width, a vertical mode that does not move a0 forwards or moves
    it past the width, a pass mode whose b2 is the end of the line, a missing EOL, input that ends early: ``Damaged``.  Bytes behind the
    strip's last row (RTC, EOFB, padding) are never read.
"""
import struct

import numpy as np

import tiff_decode_ref as R
from tiff_decode_ref import Damaged, tiff_file

# ------------------------------------------------------------------------------------------------ the tables (T.4 tables 2 and 3)
WHITE_TERM = """00110101 000111 0111 1000 1011 1100 1110 1111 10011 10100 00111 01000 001000 000011 110100 110101
101010 101011 0100111 0001100 0001000 0010111 0000011 0000100 0101000 0101011 0010011 0100100 0011000 00000010 00000011 00011010
00011011 00010010 00010011 00010100 00010101 00010110 00010111 00101000 00101001 00101010 00101011 00101100 00101101 00000100 00000101 00001010
00001011 01010010 01010011 01010100 01010101 00100100 00100101 01011000 01011001 01011010 01011011 01001010 01001011 00110010 00110011 00110100""".split()
WHITE_MAKE = """11011 10010 010111 0110111 00110110 00110111 01100100 01100101 01101000 01100111 011001100 011001101 011010010 011010011
011010100 011010101 011010110 011010111 011011000 011011001 011011010 011011011 010011000 010011001 010011010 011000 010011011""".split()
BLACK_TERM = """0000110111 010 11 10 011 0011 0010 00011 000101 000100 0000100 0000101 0000111 00000100 00000111 000011000
0000010111 0000011000 0000001000 00001100111 00001101000 00001101100 00000110111 00000101000 00000010111 00000011000 000011001010 000011001011
000011001100 000011001101 000001101000 000001101001 000001101010 000001101011 000011010010 000011010011 000011010100 000011010101 000011010110
000011010111 000001101100 000001101101 000011011010 000011011011 000001010100 000001010101 000001010110 000001010111 000001100100 000001100101
000001010010 000001010011 000000100100 000000110111 000000111000 000000100111 000000101000 000001011000 000001011001 000000101011 000000101100
000001011010 000001100110 000001100111""".split()
BLACK_MAKE = """0000001111 000011001000 000011001001 000001011011 000000110011 000000110100 000000110101 0000001101100 0000001101101 0000001001010
0000001001011 0000001001100 0000001001101 0000001110010 0000001110011 0000001110100 0000001110101 0000001110110 0000001110111 0000001010010
0000001010011 0000001010100 0000001010101 0000001011010 0000001011011 0000001100100 0000001100101""".split()
EXT_MAKE = """00000001000 00000001100 00000001101 000000010010 000000010011 000000010100 000000010101 000000010110 000000010111 000000011100
000000011101 000000011110 000000011111""".split()                             # 1792 .. 2560, both colours
EOL = "000000000001"
MODES = {"P": "0001", "H": "001", "V0": "1", "VR1": "011", "VR2": "000011", "VR3": "0000011", "VL1": "010", "VL2": "000010", "VL3": "0000010"}
MODE_OF = {bits: name for name, bits in MODES.items()}
EXT_2D, EXT_1D = "0000001", "000000001"                                        # the prefixes of the extension (uncompressed mode) codes


def code_set(colour):
    """the 104 code words of a colour in the table's order -> [(bits, run)]: index i < 64 is the terminating code of run i, index 63 + k the
    make-up code of 64 k"""
    term, make = (WHITE_TERM, WHITE_MAKE) if colour == 0 else (BLACK_TERM, BLACK_MAKE)
    words = term + make + EXT_MAKE
    assert len(words) == 104
    return [(b, i if i < 64 else 64 * (i - 63)) for i, b in enumerate(words)]


RUN_OF = [{b: r for b, r in code_set(c)} for c in (0, 1)]
BITS_OF = [{r: b for b, r in code_set(c)} for c in (0, 1)]

MAX_WIDTH = 10240                                                              # bbocr.h BBOCR_FAX_MAX_WIDTH
FAX_REASONS = ("OK", "PLAIN", "FILL_ORDER", "DEPTH", "OPTIONS", "WIDTH")
FAX_OK, FAX_PLAIN, FAX_FILL_ORDER, FAX_DEPTH, FAX_OPTIONS, FAX_WIDTH = range(6)                        # bbocr.h BBOCR_FAX_*
FAX_FIELDS = ("scheme", "t4_options", "fill_order", "reason")
REV = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


# ------------------------------------------------------------------------------------------------ rows as changing elements
def changes(row):
    """a row of 0 / 1 pixels -> the positions at which the colour changes, the row starting white (a black first pixel: position 0)"""
    row = np.asarray(row, np.uint8)
    prev = np.concatenate([[0], row[:-1]])
    return [int(x) for x in np.flatnonzero(row != prev)]


def render(ch, W):
    """changing elements as decoded -> the row's W pixels"""
    t = np.zeros(W + 1, np.uint8)
    for c in ch:
        t[min(c, W)] ^= 1
    return (np.cumsum(t[:W]) & 1).astype(np.uint8)


def pack_rows(rows):
    return np.packbits(np.asarray(rows, np.uint8), axis=1).tobytes()


# ------------------------------------------------------------------------------------------------ the encoder
def run_bits(colour, n):
    out = ""
    while n > 2623:
        out += BITS_OF[colour][2560]
        n -= 2560
    if n >= 64:
        out += BITS_OF[colour][n - n % 64]
    return out + BITS_OF[colour][n % 64]


def row_1d(ch, W):
    out, x, colour = "", 0, 0
    for c in list(ch) + [W]:
        out += run_bits(colour, c - x)
        x, colour = c, colour ^ 1
    return out


def row_2d(cur, ref, W):
    """the coding procedure of T.4 4.2.1.3 over the canonical changing elements of both lines"""
    def after(lst, a0, parity=None):
        for i, c in enumerate(lst):
            if c > a0 and (parity is None or i % 2 == parity):
                return i, c
        return len(lst), W
    out, a0, colour = "", -1, 0
    while a0 < W:
        i, a1 = after(cur, a0)
        a2 = cur[i + 1] if i + 1 < len(cur) else W
        j, b1 = after(ref, a0, colour)
        b2 = ref[j + 1] if j + 1 < len(ref) else W
        if b2 < a1:
            out, a0 = out + MODES["P"], b2
        elif abs(a1 - b1) <= 3:
            out += MODES["V0" if a1 == b1 else ("VR%d" % (a1 - b1) if a1 > b1 else "VL%d" % (b1 - a1))]
            a0, colour = a1, colour ^ 1
        else:
            out += MODES["H"] + run_bits(colour, a1 - max(a0, 0)) + run_bits(colour ^ 1, a2 - a1)
            a0 = a2
    return out


def to_bytes(bits, fill_order=1):
    bits += "0" * (-len(bits) % 8)
    data = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return data.translate(REV) if fill_order == 2 else data


def encode_strip(rows, scheme, t4_options=0, k=None, tail=False, fill_order=1):
    """rows [n][W] of 0 / 1 -> the stored strip.  scheme 2: 1-D rows, each from a byte boundary; 3: EOL before every row, with T4Options
    bit 2 filled so that it ENDS on a byte boundary, with bit 0 a tag bit and every ``k``-th row 1-D (None: only the first); 4: T.6.
    ``tail``: RTC (scheme 3) or EOFB (scheme 4) behind the last row."""
    rows = np.asarray(rows, np.uint8)
    W = rows.shape[1]
    two_d = scheme == 4 or (scheme == 3 and t4_options & 1)
    out, ref = "", []
    for y, row in enumerate(rows):
        cur = changes(row)
        if scheme == 2:
            out += row_1d(cur, W)
            out += "0" * (-len(out) % 8)
        elif scheme == 3:
            if t4_options & 4:
                out += "0" * ((-(len(out) + 12)) % 8)
            out += EOL
            one_d = not two_d or (y == 0 if k is None else y % k == 0)
            if two_d:
                out += "1" if one_d else "0"
            out += row_1d(cur, W) if one_d else row_2d(cur, ref, W)
        else:
            out += row_2d(cur, ref, W)
        ref = cur
    if tail:
        out += (EOL + ("1" if two_d else "")) * 6 if scheme == 3 else (EOL * 2 if scheme == 4 else "")
    return to_bytes(out, fill_order)


def fax_file(rows, scheme, t4_options=0, k=None, tail=False, fill_order=None, photometric=0, rows_per_strip=None, order="II", strips=None,
             options_tag=True, **kw):
    """a 1-bit TIFF of the pixel rows (0 white / 1 black as coded) in the scheme; ``strips``: the stored strips themselves"""
    rows = np.asarray(rows, np.uint8)
    H, W = rows.shape
    per = min(rows_per_strip or H, H)
    if strips is None:
        strips = [encode_strip(rows[s:s + per], scheme, t4_options, k, tail, fill_order or 1) for s in range(0, H, per)]
    extra = list(kw.pop("extra_tags", ()))
    if options_tag and scheme in (3, 4):
        extra.append((292 if scheme == 3 else 293, 4, [t4_options]))
    return tiff_file(None, W, H, bits=1, photometric=photometric, compression=scheme, rows_per_strip=rows_per_strip, order=order,
                     strips=strips, fill_order=fill_order, extra_tags=extra, **kw)


# ------------------------------------------------------------------------------------------------ the strict decoder
class Bits:
    def __init__(self, data, fill_order=1):
        data = bytes(data).translate(REV) if fill_order == 2 else bytes(data)
        self.s = "".join("{:08b}".format(b) for b in data)
        self.at = 0

    def peek(self, n):
        return self.s[self.at:self.at + n]

    def left(self):
        return len(self.s) - self.at


def read_run(b, colour, W, codes=None):
    run = 0
    while True:
        for n in range(2, 14):
            r = RUN_OF[colour].get(b.peek(n)) if b.left() >= n else None
            if r is not None:
                break
        else:
            if b.left() < 13:
                raise Damaged("fax: input")
            raise Damaged("fax: extension code" if b.peek(9) == EXT_1D else "fax: no code")
        b.at += n
        run += r
        if codes is not None:
            codes.append((colour, r))
        if run > W:
            raise Damaged("fax: a run beyond the width")
        if r < 64:
            return run


def decode_1d(b, W, codes=None):
    cur, x, colour = [], 0, 0
    while x < W:
        x += read_run(b, colour, W, codes)
        if x > W:
            raise Damaged("fax: runs beyond the width")
        if len(cur) >= W + 4:
            raise Damaged("fax: more changing elements than the line holds")
        cur.append(x)
        colour ^= 1
    return cur


def decode_2d(b, ref, W, codes=None):
    ref = list(ref) + [W, W, W]
    cur, a0, colour, pb = [], -1, 0, 0
    while a0 < W:
        while ref[pb] <= a0 and ref[pb] < W:
            pb += 2
        for n in range(1, 8):
            mode = MODE_OF.get(b.peek(n)) if b.left() >= n else None
            if mode:
                break
        else:
            if b.left() < 7:
                raise Damaged("fax: input")
            raise Damaged("fax: extension code" if b.peek(7) == EXT_2D else "fax: no mode code")
        b.at += n
        if codes is not None:
            codes.append(mode)
        if len(cur) + 2 > W + 4:
            raise Damaged("fax: more changing elements than the line holds")
        if mode == "P":
            if ref[pb + 1] >= W:
                raise Damaged("fax: pass mode at the end of the line")
            a0 = ref[pb + 1]
            pb += 2
        elif mode == "H":
            a1 = max(a0, 0) + read_run(b, colour, W, codes)
            a2 = a1 + read_run(b, colour ^ 1, W, codes)
            if a2 > W:
                raise Damaged("fax: runs beyond the width")
            cur += [a1, a2]
            a0 = a2
        else:
            d = 0 if mode == "V0" else int(mode[2]) * (1 if mode[1] == "R" else -1)
            a1 = ref[pb] + d
            if a1 <= a0 or a1 > W:
                raise Damaged("fax: a vertical mode moves a0 backwards or past the width")
            cur.append(a1)
            a0, colour = a1, colour ^ 1
            pb = pb - 1 if d < 0 and pb > 0 else pb + 1
    return cur


def skip_eol(b):
    zeros = 0
    while True:
        if b.left() < 1:
            raise Damaged("fax: input")
        bit = b.peek(1)
        b.at += 1
        if bit == "1":
            if zeros < 11:
                raise Damaged("fax: no EOL before the row")
            return
        zeros += 1


def decode_strip(data, W, rows, scheme, t4_options=0, fill_order=1, codes=None):
    """the stored strip -> rows * ceil(W / 8) bytes; ``codes``: a list that receives every code read"""
    b = Bits(data, fill_order)
    out, ref = [], []
    for _ in range(rows):
        if scheme == 2:
            b.at += -b.at % 8
            cur = decode_1d(b, W, codes)
        elif scheme == 3:
            skip_eol(b)
            one_d = True
            if t4_options & 1:
                if b.left() < 1:
                    raise Damaged("fax: input")
                one_d = b.peek(1) == "1"
                b.at += 1
            cur = decode_1d(b, W, codes) if one_d else decode_2d(b, ref, W, codes)
        else:
            cur = decode_2d(b, ref, W, codes)
        out.append(render(cur, W))
        ref = cur
    return pack_rows(out)


# ------------------------------------------------------------------------------------------------ the plan
def _entry(f, tag):
    """-> (E, at, typ, count) of the LAST entry of ``tag`` in the first IFD (the walk has found the IFD sound), or None"""
    E = ">" if f[:2] == b"MM" else "<"
    ifd = struct.unpack_from(E + "I", f, 4)[0]
    found = None
    for e in range(struct.unpack_from(E + "H", f, ifd)[0]):
        at = ifd + 2 + 12 * e
        t, typ, count = struct.unpack_from(E + "HHI", f, at)
        if t == tag:
            found = (E, at, typ, count)
    return found


def _first_value(f, tag, default):
    ent = _entry(f, tag)
    if ent is None:
        return default
    E, at, typ, count = ent
    size = {1: 1, 3: 2, 4: 4}[typ]
    where = at + 8 if count * size <= 4 else struct.unpack_from(E + "I", f, at + 8)[0]
    return struct.unpack_from(E + {1: "B", 2: "H", 4: "I"}[size], f, where)[0]


def _with_first_value(f, tag, value):
    E, at, typ, count = _entry(f, tag)
    size = {1: 1, 3: 2, 4: 4}[typ]
    where = at + 8 if count * size <= 4 else struct.unpack_from(E + "I", f, at + 8)[0]
    g = bytearray(f)
    struct.pack_into(E + {1: "B", 2: "H", 4: "I"}[size], g, where, value)
    return bytes(g)


def fax_walk(f):
    """-> (plan dict with R.PLAN_FIELDS, fax dict with FAX_FIELDS, strips): csrc/tiff_parse.h's walk in the mode that goes on behind a CCITT
    compression and a fill order other than 1 and finishes its checks (restated by walking a copy of the file in which the two values
    read 1), then the checks of the fax plan in their order"""
    f = bytes(f)
    fax = dict(scheme=0, t4_options=0, fill_order=1, reason=FAX_OK)
    pl, strips, _ = R.walk(f)
    if pl["reason"] not in (R.CCITT, R.FILL_ORDER):
        fax["reason"] = FAX_OK if pl["supported"] else FAX_PLAIN
        return pl, fax, strips
    first = pl["reason"]
    comp, g = pl["compression"], f
    if first == R.CCITT:
        g = _with_first_value(g, 259, 1)
        pl, strips, _ = R.walk(g)
    if pl["reason"] == R.FILL_ORDER:
        fax["fill_order"] = _first_value(g, 266, 1)
        g = _with_first_value(g, 266, 1)
        pl, strips, _ = R.walk(g)
    pl["compression"] = comp
    if not pl["supported"]:
        fax["reason"] = FAX_PLAIN
        return pl, fax, strips
    ccitt = comp in (2, 3, 4)
    fax["scheme"] = comp if ccitt else 0
    if comp in (3, 4):
        fax["t4_options"] = _first_value(f, 292 if comp == 3 else 293, 0) if _sound(f, 292 if comp == 3 else 293) else -1

    def refuse(reason):
        pl["supported"], pl["reason"], fax["reason"] = 0, first, reason
        return pl, fax, strips

    if fax["t4_options"] < 0:
        fax["t4_options"] = 0
        return refuse(FAX_OPTIONS)
    if fax["fill_order"] not in (1, 2) or not ccitt:
        return refuse(FAX_FILL_ORDER)
    if pl["bits"] != 1 or pl["samples"] != 1:
        return refuse(FAX_DEPTH)
    assert pl["photometric"] <= 1                                             # (on one 1-bit sample the walk has refused anything above)
    if fax["t4_options"] & (~5 if comp == 3 else ~0):
        return refuse(FAX_OPTIONS)
    if pl["width"] > MAX_WIDTH:
        return refuse(FAX_WIDTH)
    return pl, fax, strips


def _sound(f, tag):
    """the options tag is absent, or BYTE / SHORT / LONG with a value that lies in the file"""
    ent = _entry(f, tag)
    if ent is None:
        return True
    E, at, typ, count = ent
    size = {1: 1, 3: 2, 4: 4}.get(typ, 0)
    if not size or count == 0:
        return False
    if count * size > 4:
        where = struct.unpack_from(E + "I", f, at + 8)[0]
        return where <= len(f) and (len(f) - where) // size >= count
    return True


def fax_plan(f):
    pl, fax, _ = fax_walk(f)
    return pl, fax


def decode(f):
    """-> dict(plan, fax, stage0: the strips' stream, rgb, gray); Damaged for a damaged strip.  A file of the plain plan goes to
    tiff_decode_ref.decode."""
    pl, fax, strips = fax_walk(f)
    assert pl["supported"], (R.REASONS[pl["reason"]], FAX_REASONS[fax["reason"]])
    if not fax["scheme"]:
        return R.decode(f)
    H, W, rows = pl["height"], pl["width"], pl["rows_per_strip"]
    stage0 = b"".join(decode_strip(f[o:o + c], W, min(rows, H - s * rows), fax["scheme"], fax["t4_options"], fax["fill_order"])
                      for s, (o, c) in enumerate(strips))
    v = np.unpackbits(np.frombuffer(stage0, np.uint8).reshape(H, pl["row_bytes"]), axis=1)[:, :W] * np.uint8(255)
    g = 255 - v if pl["photometric"] == 0 else v
    return dict(plan=pl, fax=fax, stage0=stage0, stage1=stage0, rgb=np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2)),
                gray=np.ascontiguousarray(g))


# ------------------------------------------------------------------------------------------------ pages
def runs_row(runs, W):
    """alternating run lengths, white first -> a row of W pixels (the last run is cut or extended to the width)"""
    row, x, colour = np.zeros(W, np.uint8), 0, 0
    for r in runs:
        row[x:x + r] = colour
        x, colour = x + r, colour ^ 1
    row[x:] = colour ^ 1 if x < W and runs else 0
    return row


def every_length_rows():
    """rows of width 2561 + 5120 that hold every terminating length 0 .. 63 and every make-up multiple 64 .. 2560 in both colours:
    [W] pixel rows, to be coded 1-D (a 2-D coder meets them in horizontal mode where the lines differ enough)"""
    W = 7681
    rows = []
    lengths = list(range(1, 64)) + [64 * k for k in range(1, 41)] + [64 * k + 1 for k in (1, 27, 28, 40)]
    at = 0
    while at < len(lengths):                                                  # pack lengths into rows: white L, black L, white L', ...
        runs, x = [], 0
        while at < len(lengths) and x + 2 * lengths[at] <= W - 2:
            runs += [lengths[at], lengths[at]]
            x += 2 * lengths[at]
            at += 1
        rows.append(runs_row(runs + [W - x], W))
    rows.append(np.ones(W, np.uint8))                                         # white 0, black 2560 2560 2560 + 1
    rows.append(np.zeros(W, np.uint8))
    rows.append(runs_row([0, 5121, 2560], W))
    return np.array(rows, np.uint8)


def text_page(W, H, seed):
    """a text-like page: lines of short black runs with white gaps and blank lines between them"""
    rng = np.random.default_rng(seed)
    a = np.zeros((H, W), np.uint8)
    y = 4
    while y + 10 < H:
        x = 8
        while x + 12 < W - 8:
            w = int(rng.integers(3, 10))
            glyph = rng.integers(0, 2, (8, w), dtype=np.uint8)
            glyph[:, 0] |= glyph[:, -1]
            a[y:y + 8, x:x + w] = glyph
            x += w + int(rng.integers(1, 4)) + (6 if rng.integers(0, 5) == 0 else 0)
        y += 14
    return a


def mode_rows(W=65):
    """rows (against the row above; the first against white) whose 2-D coding meets V0, VR1-3, VL1-3, pass and horizontal mode, b1 at the
    first pixel with a0 before the row, a change at the last pixel, all-white and all-black rows and a row that begins black"""
    r = [runs_row([10, 5, 20, 6, W], W)]                                     # against white: horizontal modes
    r.append(runs_row([10, 5, 20, 6, W], W))                                 # V0 everywhere
    r.append(runs_row([11, 6, 17, 9, W], W))                                 # VR1 VR2 (16+1=17->35+...): shifts to the right
    r.append(runs_row([8, 8, 17, 6, W], W))                                  # VL3 VL1 ...
    r.append(runs_row([W], W))                                               # all white: passes over the runs above
    r.append(runs_row([0, W], W))                                            # all black: b1 none, a row that begins black
    r.append(runs_row([0, 3, 5, W], W))                                      # begins black against black: b1 at the first pixel
    r.append(runs_row([2, 3, 3, 30, 26, 1], W))                              # a change at the last pixel
    r.append(runs_row([2, 3, 3, 30, 26, 1], W))
    r.append(runs_row([5, 1, 1, 31, 24, 3], W))                              # VR3 / VL2 / VL3 mixtures
    r.append(runs_row([W - 1, 1], W))
    r.append(runs_row([W], W))
    return np.array(r, np.uint8)


def designed():
    """[(name, rows)]: the small pages of the GPU tests"""
    out = []
    for W in (1, 7, 8, 9, 63, 64, 65, 1728, 2561):
        rng = np.random.default_rng(W)
        H = 3 + W % 10
        a = np.zeros((H, W), np.uint8)
        for y in range(H):
            x, colour = int(rng.integers(0, 3)) * int(rng.integers(0, 2)), 1
            while x < W:
                n = int(rng.integers(1, max(2, min(W, 70))))
                a[y, x:x + n] = colour
                x, colour = x + n, colour ^ 1
            if y and rng.integers(0, 3) == 0:
                a[y] = a[y - 1]
                a[y, int(rng.integers(0, W))] ^= 1
        a[-1, -1] ^= 1
        out.append(("w%d" % W, a))
    out.append(("every_length", every_length_rows()))
    out.append(("modes", mode_rows()))
    out.append(("dots_64x16", np.random.default_rng(64).integers(0, 2, (16, 64), dtype=np.uint8)))
    out.append(("text_640x96", text_page(640, 96, 5)))
    return out


def variants(name, a):
    """the files of one designed page: all three schemes (T.4 with options 0, 1, 4, 5 and K = 1, 2, none), both fill orders, both
    photometrics, one / two / three strips, both byte orders, tails -> [(name, file)]"""
    H = a.shape[0]
    out = []
    k = 0
    for scheme, opt, kk in ((2, 0, None), (3, 0, None), (3, 4, None), (3, 1, 1), (3, 1, 2), (3, 5, None), (4, 0, None)):
        for rps in (None, -(-H // 2), -(-H // 3)):
            fo = (None, 2, 1)[k % 3]
            ph = k % 2
            order = "MM" if k % 4 == 3 else "II"
            out.append(("%s-c%d-o%d-k%s-rps%s-fo%s-ph%d-%s" % (name, scheme, opt, kk, rps, fo, ph, order),
                        fax_file(a, scheme, opt, kk, tail=k % 2 == 1, fill_order=fo, photometric=ph, rows_per_strip=rps, order=order)))
            k += 1
    return out


_FILES = []


def designed_files():
    """[(name, file)] over designed(): every variant of the small pages, every fourth of the wide ones.  Computed once per process."""
    if not _FILES:
        for name, a in designed():
            v = variants(name, a)
            _FILES.extend(v[::4] if a.shape[1] > 1000 else v)
    return list(_FILES)


def handbuilt():
    """[(name, file)]: files Pillow never writes and Pillow reads"""
    a = dict(designed())["modes"]
    b = dict(designed())["w63"]
    return [
        ("phot0_g4", fax_file(a, 4, photometric=0)),
        ("phot1_g4", fax_file(a, 4, photometric=1)),
        ("mm_g4", fax_file(a, 4, order="MM", rows_per_strip=5)),
        ("mm_g3_2d_fill2", fax_file(a, 3, 5, order="MM", fill_order=2, rows_per_strip=4)),
        ("one_strip_mh", fax_file(b, 2)),
        ("rows_per_strip_1_g4", fax_file(a, 4, rows_per_strip=1)),
        ("rows_per_strip_1_g3", fax_file(a, 3, 1, rows_per_strip=1)),
        ("short_last_strip_g3", fax_file(a, 3, 0, rows_per_strip=5)),
        ("short_last_strip_mh_fill2", fax_file(a, 2, fill_order=2, rows_per_strip=7)),
        ("k1", fax_file(a, 3, 1, k=1)),
        ("k2", fax_file(a, 3, 1, k=2, tail=True)),
        ("k_inf", fax_file(a, 3, 1, k=None)),
        ("k_inf_aligned", fax_file(a, 3, 5, k=None, tail=True)),
        ("g4_eofb", fax_file(a, 4, tail=True, rows_per_strip=6)),
        ("g3_no_options_tag", fax_file(a, 3, 0, options_tag=False)),
        ("g4_no_options_tag", fax_file(a, 4, options_tag=False)),
    ]


def handwritten():
    """[(name, scheme, t4_options, bits of the strip, (W, H), the rows expected)]: streams no encoder here writes"""
    W = 2600
    long_white = BITS_OF[0][2560] * 2 + BITS_OF[0][0]                         # 2560 twice and a terminating 0: 5120
    out = [
        ("makeups_repeated", 2, 0, BITS_OF[0][64] + BITS_OF[0][64] + BITS_OF[0][1792] + BITS_OF[0][40] + BITS_OF[1][640] + BITS_OF[1][0], (2600, 1),
         [runs_row([1960, 640], 2600)]),
        ("long_run_5120", 2, 0, long_white + BITS_OF[1][1], (5121, 1), [runs_row([5120, 1], 5121)]),
        ("fill_before_eol", 3, 0, "0" * 21 + EOL + row_1d([3], 8) + "0" * 5 + EOL + row_1d([], 8), (8, 2), [runs_row([3, 5], 8), runs_row([8], 8)]),
        ("zero_white_run_first", 4, 0, MODES["H"] + BITS_OF[0][0] + BITS_OF[1][4] + MODES["V0"], (9, 1), [runs_row([0, 4, 5], 9)]),
    ]
    return out


def handwritten_files():
    return [(name, fax_file(np.zeros((h, w), np.uint8), scheme, opt, strips=[to_bytes(bits)])) for name, scheme, opt, bits, (w, h), _ in handwritten()]


def damaged():
    """[(name, file)]: every file passes the fax plan and holds a strip the decoder must answer with a status.  Most have three strips of
    which the MIDDLE one is damaged; every one is an ordinary data error."""
    a = dict(designed())["modes"][:9]
    W = a.shape[1]
    parts = [a[0:3], a[3:6], a[6:9]]

    def three(scheme, opt, middle, fill_order=None):
        s = [encode_strip(p, scheme, opt, fill_order=fill_order or 1) for p in parts]
        s[1] = middle(s[1]) if callable(middle) else to_bytes(middle, fill_order or 1)
        return fax_file(a, scheme, opt, rows_per_strip=3, strips=s, fill_order=fill_order)

    half = lambda s: s[: len(s) // 2]
    white = row_1d([], W)
    out = [("%s_truncated" % n, three(c, o, half)) for n, c, o in (("mh", 2, 0), ("g3", 3, 0), ("g3_2d", 3, 5), ("g4", 4, 0))]
    out += [
        ("mh_no_code", three(2, 0, "0000000001" + "1" * 40)),                                # nine 0 bits and a 1: no word, no extension, no EOL
        ("mh_no_code_black", three(2, 0, run_bits(0, 3) + "0000000001" + "1" * 40)),
        ("mh_extension", three(2, 0, "000000001111" + "1" * 30)),
        ("mh_runs_beyond_width", three(2, 0, run_bits(0, 60) + run_bits(1, 6) + "0" * 7 + white * 2)),
        ("mh_row_ends_early", three(2, 0, run_bits(0, 60) + run_bits(1, 4))),
        ("g3_missing_eol", three(3, 0, EOL + white + white + EOL + white)),
        ("g3_short_eol", three(3, 0, "0" * 10 + "1" + white + EOL + white + EOL + white)),
        ("g3_tag_bit_missing", three(3, 1, "0" * 11 + "1")),
        ("g3_fill2_no_code", three(3, 0, EOL + "0000000001" + "1" * 30, fill_order=2)),
        ("g4_no_mode", three(4, 0, "00000001" + "1" * 30)),
        ("g4_eofb_early", three(4, 0, MODES["V0"] + EOL * 2)),
        ("g4_extension", three(4, 0, "0000001111" + "1" * 30)),
        ("g4_vertical_left_of_a0", three(4, 0, MODES["H"] + run_bits(0, 4) + run_bits(1, 2) + MODES["V0"] + MODES["V0"] + MODES["VL2"] + "1" * 20)),
        ("g4_vertical_past_width", three(4, 0, MODES["VR1"] + "1" * 20)),
        ("g4_pass_at_line_end", three(4, 0, MODES["H"] + run_bits(0, 4) + run_bits(1, W - 4) + MODES["P"] + "1" * 20)),
        ("g4_horizontal_beyond_width", three(4, 0, MODES["H"] + run_bits(0, 60) + run_bits(1, 6) + "1" * 20)),
        ("g4_zero_runs_without_end", three(4, 0, (MODES["H"] + BITS_OF[0][0] + BITS_OF[1][0]) * 60)),
    ]
    return out


def fax_refusals():
    """[(name, file, plain reason, fax reason)]: one file per reason of the fax plan"""
    a = dict(designed())["w9"]
    H, W = a.shape
    g4 = encode_strip(a, 4)
    wide = np.zeros((1, MAX_WIDTH + 1), np.uint8)
    byte_rows = bytes(range(W * H))
    return [
        ("lzw_16_bit", tiff_file(bytes(2 * W * H), W, H, bits=16, compression=5), R.DEPTH, FAX_PLAIN),
        ("g4_tiles", fax_file(a, 4, extra_tags=[(322, 3, [16]), (323, 3, [16])]), R.TILES, FAX_PLAIN),
        ("g4_planar_2", fax_file(a, 4, planar=2), R.PLANAR, FAX_PLAIN),
        ("g4_strip_past_end", R._retag(fax_file(a, 4), 279, [len(g4) + 4000]), R.TRUNCATED, FAX_PLAIN),
        ("g4_strip_table", fax_file(a, 4, rows_per_strip=2, table_strips=1), R.STRIPS, FAX_PLAIN),
        ("g4_fill_order_count_0", fax_file(a, 4, extra_tags=[(266, 3, [])]), R.HEADER, FAX_PLAIN),
        ("g4_4_bit", tiff_file(None, W, H, bits=4, compression=4, strips=[g4]), R.SUBBYTE, FAX_PLAIN),
        ("g4_fill_order_3", fax_file(a, 4, fill_order=3), R.CCITT, FAX_FILL_ORDER),
        ("lzw_fill_order_2", tiff_file(byte_rows, W, H, compression=5, fill_order=2), R.FILL_ORDER, FAX_FILL_ORDER),
        ("raw_fill_order_2", tiff_file(byte_rows, W, H, fill_order=2), R.FILL_ORDER, FAX_FILL_ORDER),
        ("g4_8_bit", tiff_file(None, W, H, bits=8, compression=4, strips=[g4]), R.CCITT, FAX_DEPTH),
        ("g4_palette", fax_file(a, 4, photometric=3, colormap=[0] * 6), R.DEPTH, FAX_PLAIN),
        ("g4_rgb", fax_file(a, 4, photometric=2), R.DEPTH, FAX_PLAIN),
        ("g4_cmyk", fax_file(a, 4, photometric=5), R.PHOTOMETRIC, FAX_PLAIN),
        ("g3_uncompressed_bit", fax_file(a, 3, 2), R.CCITT, FAX_OPTIONS),
        ("g3_unknown_bit", fax_file(a, 3, 8), R.CCITT, FAX_OPTIONS),
        ("g4_uncompressed_bit", fax_file(a, 4, 2), R.CCITT, FAX_OPTIONS),
        ("g4_unknown_bit", fax_file(a, 4, 1), R.CCITT, FAX_OPTIONS),
        ("g3_options_count_0", fax_file(a, 3, 0, options_tag=False, extra_tags=[(292, 3, [])]), R.CCITT, FAX_OPTIONS),
        ("g4_too_wide", fax_file(wide, 4), R.CCITT, FAX_WIDTH),
        ("mh_too_wide_fill_2", fax_file(wide, 2, fill_order=2), R.CCITT, FAX_WIDTH),
    ]
