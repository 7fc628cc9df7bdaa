"""The device GIF decoder (csrc/gif_parse.h, csrc/gif_lzw.h, csrc/gifdec.hip) restated in numpy and plain Python: the plan walk with its
refusal reasons, the LZW rule, the split of a code stream at its clear codes (piece table, lengths, offsets), the index stream and both
planes -- and writers for files no encoder writes: frames inside, at the edge of and past the screen, local over global tables, hand-written
code streams.  Pillow's rules as restated here (each checked against Pillow in tests/test_gif_decode_cpu.py):
  * frame 0 only; the canvas is max(screen, x0 + w) by max(screen, y0 + h); pixels outside the frame hold the transparency index of the
    last graphic control extension before the image that sets one, else 0;
  * the table in force is the local one over the global one; mode L when every entry i of it is (i, i, i), whatever its length, and when
    the file has no table at all (Pillow then reads the indices as gray levels); P otherwise;
  * an index at or above the table's length reads black (0, 0, 0) in mode P -- a function of the file alone, restated, not flagged;
  * a local table that is a ramp over a global one that is none: Pillow's mode is L (the gray plane is the index) but its convert("RGB")
    looks the index up in the GLOBAL table; restated as it is, through the plan's ``table`` (the RGB plane's lookup);
  * decoding stops once w * h indices exist, whatever follows; a stream that ends sooner (end code, end of the payload) is damage.
Stricter than Pillow (such files take the host path): a data block chain without its terminator although the frame is full, an unknown
block introducer before the image (Pillow skips the byte), a graphic control block shorter than four bytes, a piece table beyond
``piece_cap`` (a stream that clears more often than once in 128 payload bits over more than 4096 pieces)."""
import io

import numpy as np

REASONS = ("OK", "NOT_GIF", "TRUNCATED", "NO_IMAGE", "EMPTY", "PIXELS", "CODE_SIZE")         # bbocr.h BBOCR_GIF_*
(OK, NOT_GIF, TRUNCATED, NO_IMAGE, EMPTY, PIXELS, CODE_SIZE) = range(7)
PLAN_FIELDS = ("screen_w", "screen_h", "x0", "y0", "width", "height", "canvas_w", "canvas_h", "interlace", "table_len", "local_table",
               "transparency", "min_code", "mode_l", "payload_bytes", "supported", "reason")
MAX_PIXELS = 2 * 89478485
END_CLEAR, END_EOI, END_INPUT = 0, 1, 2            # how a piece ends: a clear code, the end code, the end of the payload
ERR_FIRST, ERR_CODE, ERR_SHORT, ERR_PIECES = 1, 2, 4, 8
STEP = 64                                          # codes per scan step (one wavefront)


class Damaged(Exception):
    pass


# ------------------------------------------------------------------------------------------------ the plan
def plan(f):
    """bbocr_host_gif_plan: -> dict (fields the walk did not reach stay 0 / -1), with "table" (768 bytes) and "payload" (bytes)"""
    pl = dict(screen_w=0, screen_h=0, x0=0, y0=0, width=0, height=0, canvas_w=0, canvas_h=0, interlace=0, table_len=0, local_table=0,
              transparency=-1, min_code=0, mode_l=0, payload_bytes=0, supported=0, reason=OK, table=bytes(768), payload=b"")

    def refuse(r):
        pl["reason"] = r
        return pl

    n = len(f)
    if n < 6 or f[:6] not in (b"GIF87a", b"GIF89a"):
        return refuse(NOT_GIF)
    if n < 13:
        return refuse(TRUNCATED)
    u16 = lambda at: f[at] | (f[at + 1] << 8)
    pl["screen_w"], pl["screen_h"] = u16(6), u16(8)
    at = 13
    table, tlen, gtable = None, 0, None
    if f[10] & 128:
        tlen = 2 << (f[10] & 7)
        if n - at < 3 * tlen:
            return refuse(TRUNCATED)
        table = gtable = f[at:at + 3 * tlen]
        at += 3 * tlen
    while True:
        if at >= n:
            return refuse(TRUNCATED)
        tag = f[at]
        at += 1
        if tag == 0x3B:
            return refuse(NO_IMAGE)
        if tag == 0x2C:
            break
        if tag != 0x21:
            return refuse(TRUNCATED)
        if at >= n:
            return refuse(TRUNCATED)
        label = f[at]
        at += 1
        first = True
        while True:
            if at >= n:
                return refuse(TRUNCATED)
            size = f[at]
            at += 1
            if size == 0:
                break
            if n - at < size:
                return refuse(TRUNCATED)
            if first and label == 0xF9:
                if size < 4:
                    return refuse(TRUNCATED)
                if f[at] & 1:
                    pl["transparency"] = f[at + 3]
            first = False
            at += size
    if n - at < 9:
        return refuse(TRUNCATED)
    pl["x0"], pl["y0"], pl["width"], pl["height"] = u16(at), u16(at + 2), u16(at + 4), u16(at + 6)
    flags = f[at + 8]
    at += 9
    pl["interlace"] = 1 if flags & 64 else 0
    if flags & 128:
        tlen = 2 << (flags & 7)
        if n - at < 3 * tlen:
            return refuse(TRUNCATED)
        table = f[at:at + 3 * tlen]
        at += 3 * tlen
        pl["local_table"] = 1
    pl["table_len"] = tlen if table is not None else 0
    pl["canvas_w"], pl["canvas_h"] = max(pl["screen_w"], pl["x0"] + pl["width"]), max(pl["screen_h"], pl["y0"] + pl["height"])
    if pl["width"] == 0 or pl["height"] == 0:
        return refuse(EMPTY)
    if pl["canvas_w"] * pl["canvas_h"] > MAX_PIXELS:
        return refuse(PIXELS)
    is_ramp = lambda t: all(t[3 * i:3 * i + 3] == bytes([i]) * 3 for i in range(len(t) // 3))
    pl["mode_l"] = 1 if table is None or is_ramp(table) else 0
    # the RGB plane's lookup: the table in force, entries it does not have black; mode L: the ramp -- but behind a LOCAL ramp Pillow keeps
    # a global table that is none for convert("RGB"), while the gray plane stays the index
    lookup = table if not pl["mode_l"] else (gtable if pl["local_table"] and gtable is not None and not is_ramp(gtable) else ramp(256))
    pl["table"] = bytes(lookup) + bytes(768 - len(lookup))
    if at >= n:
        return refuse(TRUNCATED)
    pl["min_code"] = f[at]
    at += 1
    if not 2 <= pl["min_code"] <= 8:
        return refuse(CODE_SIZE)
    payload = bytearray()
    while True:
        if at >= n:
            return refuse(TRUNCATED)
        size = f[at]
        at += 1
        if size == 0:
            break
        if n - at < size:
            return refuse(TRUNCATED)
        payload += f[at:at + size]
        at += size
    pl["payload"], pl["payload_bytes"] = bytes(payload), len(payload)
    pl["supported"] = 1
    return pl


# ------------------------------------------------------------------------------------------------ the LZW rule
def code_width(m, k):
    """the width of code k (0-based) behind a clear: the next free entry is clear + 2 + max(0, k - 1) when it is read"""
    return min(12, (((1 << m) + 1 + k).bit_length()))


def code_pos(m, k):
    """the bit offset of code k behind a clear, in closed form: per width, the count of codes read with it"""
    c1, bits = (1 << m) + 1, 0
    for w in range(m + 1, 13):
        lo, hi = max(c1, 1 << (w - 1)), c1 + k if w == 12 else min(c1 + k, 1 << w)
        if hi > lo:
            bits += (hi - lo) * w
    return bits


def read_code(payload, bit, width):
    """the code at a bit position, LSB first; None when it reaches past the payload"""
    if bit + width > 8 * len(payload):
        return None
    v = int.from_bytes(payload[bit >> 3:(bit >> 3) + 3], "little")
    return (v >> (bit & 7)) & ((1 << width) - 1)


def piece_cap(payload_bytes, m):
    """the piece table's room: the bound payload_bits / (m + 1) + 1, at most max(4096, payload_bytes / 16)"""
    return min(8 * payload_bytes // (m + 1) + 1, max(4096, payload_bytes // 16))


def scan(payload, m):
    """the piece table: [(first bit, data codes, how it ends)] and the scan's error bits (ERR_PIECES: more pieces than piece_cap).  In
    steps of STEP codes from the last clear, as the wavefront walks it."""
    clear, pieces, bit, k0 = 1 << m, [], 0, 0
    cap = piece_cap(len(payload), m)
    while True:
        stop = None
        for lane in range(STEP):
            k = k0 + lane
            code = read_code(payload, bit + code_pos(m, k), code_width(m, k))
            if code is None or code == clear or code == clear + 1:
                stop = (k, END_INPUT if code is None else (END_CLEAR if code == clear else END_EOI))
                break
        if stop is None:
            k0 += STEP
            continue
        if len(pieces) >= cap:
            return pieces, ERR_PIECES
        pieces.append((bit, stop[0], stop[1]))
        if stop[1] != END_CLEAR:
            return pieces, 0
        bit, k0 = bit + code_pos(m, stop[0]) + code_width(m, stop[0]), 0


def piece_walk(payload, m, first_bit, codes, room):
    """one piece decoded on its own: -> (its bytes, clipped at room, error bits).  An error ends the piece where it is met."""
    clear = 1 << m
    out = bytearray()
    entries = {}                                    # code -> (offset into out, length)
    nxt, prev = clear + 2, None
    for k in range(codes):
        if len(out) >= room:
            break
        code = read_code(payload, first_bit + code_pos(m, k), code_width(m, k))
        if prev is None:
            if code >= clear:
                return bytes(out[:room]), ERR_FIRST
            off, ln = len(out), 1
            out.append(code)
        else:
            if code > nxt or (code == nxt and nxt >= 4096):
                return bytes(out[:room]), ERR_CODE
            off = len(out)
            if code < clear:
                out.append(code)
                ln = 1
            elif code == nxt:
                out += out[prev[0]:prev[0] + prev[1]]
                out.append(out[prev[0]])
                ln = prev[1] + 1
            else:
                o, ln = entries[code]
                out += out[o:o + ln]
            if nxt < 4096:
                entries[nxt] = (prev[0], prev[1] + 1)
                nxt += 1
        prev = (off, ln)
    return bytes(out[:room]), 0


def stages(payload, m, need):
    """-> dict(pieces, lengths, errors, offsets, total, status, stream): the lengths pass (each piece alone, clipped at ``need``), the
    exclusive prefix sum saturated at ``need``, the file's status and the index stream (``need`` bytes, zero where nothing was written)"""
    pieces, err = scan(payload, m)
    walked = [piece_walk(payload, m, b, c, need) for b, c, _ in pieces]
    lengths, errors = [len(w[0]) for w in walked], [w[1] for w in walked]
    offsets, cum, status, done = [], 0, err, False
    for (b, c, end), ln, e in zip(pieces, lengths, errors):
        offsets.append(min(cum, need))
        if not done and not status:
            if cum + ln >= need:
                done = True
            elif e:
                status |= e
            elif end != END_CLEAR:
                status |= ERR_SHORT
        cum += ln
    if not done and not status:
        status |= ERR_SHORT                        # (cannot happen: the last piece ends in the end code or the payload's end)
    stream = bytearray(need)
    for off, (data, _) in zip(offsets, walked):
        stream[off:off + len(data)] = data[:need - off]
    return dict(scan_error=err, pieces=pieces, lengths=lengths, errors=errors, offsets=offsets, total=min(cum, need), status=status, stream=bytes(stream))


def serial_indices(payload, m, need):
    """Pillow's decoder restated in one serial walk (no pieces): the first ``need`` indices, or Damaged"""
    clear, out, bit = 1 << m, bytearray(), 0
    nxt, width, prev, strings = clear + 2, m + 1, None, {}
    while len(out) < need:
        code = read_code(payload, bit, width)
        if code is None or code == clear + 1:
            raise Damaged("short stream")
        bit += width
        if code == clear:
            nxt, width, prev, strings = clear + 2, m + 1, None, {}
            continue
        if prev is None:
            if code > clear:
                raise Damaged("bad first code")
            s = bytes([code])
        else:
            if code > nxt or (code == nxt and nxt >= 4096):
                raise Damaged("code above the table")
            s = bytes([code]) if code < clear else (prev + prev[:1] if code == nxt else strings[code])
            if nxt < 4096:
                strings[nxt] = prev + s[:1]
                nxt += 1
                if nxt == 1 << width and width < 12:
                    width += 1
        out += s
        prev = s
    return bytes(out[:need])


def stored_row(y, h, interlace):
    """the stored row that holds frame row y"""
    if not interlace:
        return y
    n0, n1, n2 = (h + 7) // 8, (h + 3) // 8, (h + 1) // 4
    if y % 8 == 0:
        return y // 8
    if y % 8 == 4:
        return n0 + y // 8
    if y % 4 == 2:
        return n0 + n1 + y // 4
    return n0 + n1 + n2 + y // 2


def decode(f):
    """-> dict(plan, stage0 .. stage2 as the stage entry point returns them, status, rgb, gray); the planes are None for a damaged file"""
    pl = plan(f)
    assert pl["supported"], pl["reason"]
    w, h, m = pl["width"], pl["height"], pl["min_code"]
    st = stages(pl["payload"], m, w * h)
    d = dict(plan=pl, status=st["status"], stages=st, rgb=None, gray=None)
    head = np.array([len(st["pieces"]), st["scan_error"], 0, 0], np.uint32).tobytes()
    d["stage0"] = head + b"".join(np.array([b & 0xFFFFFFFF, b >> 32, c, e], np.uint32).tobytes() for b, c, e in st["pieces"])
    d["stage1"] = np.array(st["offsets"] + [st["total"]], np.uint32).tobytes()
    d["stage2"] = st["stream"]
    if st["status"]:
        return d
    idx = np.frombuffer(st["stream"], np.uint8).reshape(h, w)
    rows = [stored_row(y, h, pl["interlace"]) for y in range(h)]
    canvas = np.full((pl["canvas_h"], pl["canvas_w"]), max(pl["transparency"], 0), np.uint8)
    canvas[pl["y0"]:pl["y0"] + h, pl["x0"]:pl["x0"] + w] = idx[rows]
    table = np.frombuffer(pl["table"], np.uint8).reshape(256, 3)
    rgb = table[canvas]
    a = rgb.astype(np.int32)
    d["rgb"], d["gray"] = rgb, canvas if pl["mode_l"] else ((a[..., 0] * 9797 + a[..., 1] * 19234 + a[..., 2] * 3737) >> 15).astype(np.uint8)
    return d


# ------------------------------------------------------------------------------------------------ writers
def lzw_codes(data, m, clear_every=None, start_clear=True, end=True):
    """a plain LZW encoder -> the code list; ``clear_every``: a clear code after every that many data codes"""
    clear, codes = 1 << m, []
    table, nxt, cur, count = {}, clear + 2, None, 0
    if start_clear:
        codes.append(clear)
    for b in data:
        if cur is None:
            cur = b
            continue
        if (cur, b) in table:
            cur = table[(cur, b)]
            continue
        codes.append(cur)
        count += 1
        if nxt < 4096:
            table[(cur, b)] = nxt
            nxt += 1
        cur = b
        if clear_every and count >= clear_every:
            codes.append(clear)
            table, nxt, count = {}, clear + 2, 0
    if cur is not None:
        codes.append(cur)
    if end:
        codes.append(clear + 1)
    return codes


def pack_codes(codes, m):
    """the code list -> payload bytes, each code at the width the rule gives its position"""
    clear, acc, nbits, k = 1 << m, 0, 0, 0
    for c in codes:
        acc |= c << nbits
        nbits += code_width(m, k)
        k = 0 if c == clear else k + 1
    return acc.to_bytes((nbits + 7) // 8, "little")


def gif_file(w, h, m, payload, screen=None, x0=0, y0=0, gct=None, lct=None, transparency=None, interlace=False, terminator=True,
             extensions=(), gce_flags=1, version=b"GIF89a", block=255, trailer=True):
    """a GIF file around a payload: ``gct`` / ``lct``: tables as bytes (length 3 * 2^k) or None; ``extensions``: raw bytes before the image"""
    sw, sh = screen if screen is not None else (w, h)
    le = lambda v: bytes([v & 255, v >> 8])
    size_bits = lambda t: (len(t) // 3).bit_length() - 2
    out = bytearray(version + le(sw) + le(sh))
    out += bytes([(0x80 | size_bits(gct)) if gct is not None else 0, 0, 0])
    if gct is not None:
        out += gct
    if transparency is not None:
        out += b"\x21\xf9\x04" + bytes([gce_flags, 0, 0, transparency]) + b"\x00"
    for e in extensions:
        out += e
    out += b"\x2c" + le(x0) + le(y0) + le(w) + le(h)
    out += bytes([(0x40 if interlace else 0) | ((0x80 | size_bits(lct)) if lct is not None else 0)])
    if lct is not None:
        out += lct
    out.append(m)
    for at in range(0, len(payload), block):
        out.append(len(payload[at:at + block]))
        out += payload[at:at + block]
    if terminator:
        out.append(0)
    if trailer:
        out.append(0x3B)
    return bytes(out)


def ramp(n):
    return bytes(v for i in range(n) for v in (i, i, i))


def colours(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, 3 * n, dtype=np.uint8).tobytes()


def noisy(w, h, m, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << m, w * h, dtype=np.uint8).tobytes()


def pillow_file(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="GIF", **kw)
    return buf.getvalue()


def matrix():
    """Pillow-written files: modes 1, L, P, RGB and RGBA, interlaced or not, table sizes 2 .. 256, and the sizes the device tests name"""
    from PIL import Image

    rng = np.random.default_rng(5)
    out = []
    for name, (w, h) in (("96x64", (96, 64)), ("128x96", (128, 96))):       # noisy L pages: 3 and 5 pieces
        out.append(("noisy_L_" + name, pillow_file(Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8)))))
    a = rng.integers(0, 256, (23, 37, 4), dtype=np.uint8)
    for inter in (0, 1):
        out.append((f"mode1_i{inter}", pillow_file(Image.fromarray(a[..., 0] > 127), interlace=inter)))
        out.append((f"modeL_i{inter}", pillow_file(Image.fromarray(a[..., 0]), interlace=inter)))
        out.append((f"modeRGB_i{inter}", pillow_file(Image.fromarray(a[..., :3]), interlace=inter)))
        out.append((f"modeRGBA_i{inter}", pillow_file(Image.fromarray(a), interlace=inter)))
    for colors in (2, 3, 4, 7, 16, 33, 64, 128, 200, 256):
        p = Image.fromarray(a[..., :3]).quantize(colors)
        out.append((f"modeP_{colors}", pillow_file(p, interlace=colors % 2)))
    text = np.full((192, 256), 255, np.uint8)
    text[20:24, 10:200] = 0
    text[60:90:3, 30:220:2] = 40
    out.append(("text_256x192", pillow_file(Image.fromarray(text))))
    out.append(("one_pixel", pillow_file(Image.fromarray(np.array([[77]], np.uint8)))))
    out.append(("one_by_n", pillow_file(Image.fromarray(rng.integers(0, 256, (41, 1), dtype=np.uint8)))))
    out.append(("n_by_one", pillow_file(Image.fromarray(rng.integers(0, 256, (1, 41), dtype=np.uint8)))))
    return out


def handbuilt():
    """files Pillow does not write: the frame against the screen, transparency, tables"""
    out = []
    for name, screen, (x0, y0), (w, h) in (("inside", (12, 10), (3, 2), (6, 5)), ("edge", (9, 7), (3, 2), (6, 5)), ("past", (4, 4), (3, 2), (6, 5)),
                                           ("past_x", (20, 3), (18, 0), (5, 3)), ("past_y", (3, 20), (0, 18), (3, 5))):
        data = noisy(w, h, 3, seed=w + x0)
        for tr in (None, 5):
            for inter in (False, True):
                out.append((f"frame_{name}_t{tr}_i{int(inter)}", gif_file(w, h, 3, pack_codes(lzw_codes(data, 3), 3), screen=screen, x0=x0, y0=y0,
                                                                       gct=colours(8, 1), transparency=tr, interlace=inter)))
    data = noisy(11, 9, 4, seed=2)
    pay = pack_codes(lzw_codes(data, 4), 4)
    out.append(("local_over_global", gif_file(11, 9, 4, pay, gct=colours(16, 2), lct=colours(16, 3))))
    out.append(("local_only", gif_file(11, 9, 4, pay, lct=colours(16, 4))))
    out.append(("ramp_global", gif_file(11, 9, 4, pay, gct=ramp(16))))
    out.append(("ramp_local_over_colours", gif_file(11, 9, 4, pay, gct=colours(16, 5), lct=ramp(16))))
    out.append(("ramp_local_over_short_colours", gif_file(11, 9, 4, pay, gct=colours(4, 5), lct=ramp(16))))
    out.append(("ramp_local_over_ramp", gif_file(11, 9, 4, pay, gct=ramp(4), lct=ramp(16))))
    out.append(("colours_local_over_ramp", gif_file(11, 9, 4, pay, gct=ramp(16), lct=colours(16, 6))))
    out.append(("ramp_256", gif_file(11, 9, 4, pay, gct=ramp(256))))
    out.append(("ramp_short_table", gif_file(11, 9, 4, pay, gct=ramp(4))))                     # indices above the ramp's length: still L
    out.append(("short_table", gif_file(11, 9, 4, pay, gct=colours(4, 7))))                    # mode P, indices without an entry
    out.append(("no_table", gif_file(11, 9, 4, pay)))
    for rows in (1, 2, 3, 5, 9, 17):                                         # (Pillow's writer does not interlace below 16 rows)
        out.append((f"interlaced_{rows}_rows", gif_file(19, rows, 6, pack_codes(lzw_codes(noisy(19, rows, 6, seed=rows), 6), 6), gct=colours(64, rows),
                                                        interlace=True)))
    out.append(("table_of_2", gif_file(11, 9, 2, pack_codes(lzw_codes(bytes(np.frombuffer(data, np.uint8) & 1), 2), 2), gct=colours(2, 13))))
    out.append(("table_of_32", gif_file(11, 9, 5, pack_codes(lzw_codes(noisy(11, 9, 5, seed=3), 5), 5), lct=colours(32, 14))))
    out.append(("transparency_no_flag", gif_file(11, 9, 4, pay, screen=(14, 12), gct=colours(16, 8), transparency=9, gce_flags=0)))
    out.append(("transparency_ramp", gif_file(11, 9, 4, pay, screen=(14, 12), gct=ramp(16), transparency=200)))
    out.append(("transparency_beyond_table", gif_file(11, 9, 4, pay, screen=(14, 12), gct=colours(16, 9), transparency=99)))
    ext = (b"\x21\xfe\x05hello\x03abc\x00", b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00", b"\x21\xf9\x04\x01\x00\x00\x03\x00", b"\x21\xf9\x04\x00\x00\x00\x07\x00")
    out.append(("extensions", gif_file(11, 9, 4, pay, screen=(14, 12), gct=colours(16, 10), extensions=ext)))
    out.append(("gif87a_small_blocks", gif_file(11, 9, 4, pay, gct=colours(16, 11), version=b"GIF87a", block=7)))
    second = b"\x2c" + bytes(9) + b"\x02\x00"                                                  # a later frame, damaged: never read
    out.append(("later_frames", gif_file(11, 9, 4, pay, gct=colours(16, 12), trailer=False) + second))
    return out


def handwritten():
    """hand-written code streams: [(name, w, h, m, payload)], each at a place where the scan or a piece can go wrong"""
    out = []
    for m in range(2, 9):                                                    # every minimum code size, clears at odd distances
        data = noisy(29, 13, m, seed=m)
        out.append((f"m{m}", 29, 13, m, pack_codes(lzw_codes(data, m, clear_every=50 + 13 * m), m)))
    data = noisy(13, 7, 3, seed=20)
    clear, eoi = 8, 9
    out.append(("clear_before_every_code", 13, 7, 3, pack_codes([c for b in data for c in (clear, b)] + [eoi], 3)))
    out.append(("two_clears_in_a_row", 13, 7, 3, pack_codes([clear, clear] + lzw_codes(data[:40], 3, start_clear=False, end=False) + [clear, clear, clear]
                                                          + lzw_codes(data[40:], 3, start_clear=False), 3)))
    out.append(("no_leading_clear", 13, 7, 3, pack_codes(lzw_codes(data, 3, start_clear=False), 3)))
    big = noisy(160, 120, 8, seed=21)
    out.append(("never_clears", 160, 120, 8, pack_codes(lzw_codes(big, 8), 8)))                # ~19,000 codes: the table fills, 12 bits go on
    for at in (63, 64, 65, 127, 128):                                        # a clear as the last code of a scan step, the first of the next
        out.append((f"clear_at_{at}", 31, 11, 5, pack_codes(lzw_codes(noisy(31, 11, 5, seed=at), 5, clear_every=at), 5)))
    # width changes on the LAST lane of a scan step: the first code of a new width is code k = 2^w - 2^m - 1 -- with m = 6 codes 63, 191,
    # 447, ..., each lane 63 of its step, so the step's last code is wider than the 63 before it.  (k is odd: a change never falls on a
    # step's first lane, and for m < 6 it falls inside a step, which the m2 .. m5 streams cover.)
    out.append(("width_change_at_step_end", 40, 30, 6, pack_codes(lzw_codes(noisy(40, 30, 6, seed=22), 6), 6)))
    # the code equal to the next free entry: a run (every code behind the first is one), also as the second code behind a clear
    run = bytes([3]) * 200 + bytes([1, 1, 1, 1, 2, 2, 2])
    out.append(("kwkwk_run", 23, 9, 2, pack_codes(lzw_codes(run, 2), 2)))
    out.append(("kwkwk_second_code", 23, 9, 2, pack_codes(lzw_codes(run, 2, clear_every=2), 2)))
    codes = lzw_codes(data, 3, end=False)
    out.append(("data_after_full_frame", 13, 7, 3, pack_codes(codes + [clear, 7, 15, 15, 3, clear, 12, eoi], 3) + b"\xff\x13\x77"))
    out.append(("no_end_code", 13, 7, 3, pack_codes(codes, 3)))
    out.append(("string_across_the_frame_end", 23, 9, 2, pack_codes(lzw_codes(noisy(10, 10, 2, seed=23) + bytes([3]) * 300, 2, end=False), 2)))
    return out


def handwritten_files():
    return [(n, gif_file(w, h, m, pay, gct=colours(1 << m, m), interlace=(k % 3 == 1))) for k, (n, w, h, m, pay) in enumerate(handwritten())]


def damaged():
    """[(name, file)]: the plan supports each, the stream is damaged; Pillow raises on every one"""
    data = noisy(13, 7, 3, seed=30)
    clear, eoi = 8, 9
    codes = lzw_codes(data, 3, end=False)
    g = lambda pay, **kw: gif_file(13, 7, 3, pay, gct=colours(8, 3), **kw)
    out = [("bad_first_code", g(pack_codes([clear, 10] + codes[2:] + [eoi], 3))),
           ("bad_first_code_behind_second_clear", g(pack_codes(codes[:20] + [clear, 11] + codes[20:], 3))),
           ("code_above_the_table", g(pack_codes(codes[:5] + [15] + codes[5:], 3))),
           ("end_code_early", g(pack_codes(codes[:30] + [eoi], 3))),
           ("payload_ends_early", g(pack_codes(codes[:30], 3))),
           ("empty_payload", g(b"")),
           ("only_clears", g(pack_codes([clear] * 9, 3)))]
    big = noisy(160, 120, 8, seed=21)
    pay = pack_codes(lzw_codes(big, 8), 8)
    out.append(("long_stream_cut", gif_file(160, 120, 8, pay[:len(pay) // 2], gct=colours(256, 1))))
    return out


def refusals():
    """[(name, file, reason)]"""
    pay = pack_codes(lzw_codes(noisy(11, 9, 4, seed=2), 4), 4)
    good = gif_file(11, 9, 4, pay, gct=colours(16, 1))
    return [("not_gif", b"GIF88a" + good[6:], NOT_GIF), ("short_signature", b"GIF8", NOT_GIF), ("png", b"\x89PNG\r\n\x1a\n" + bytes(30), NOT_GIF),
            ("screen_cut", good[:11], TRUNCATED), ("table_cut", good[:30], TRUNCATED), ("descriptor_cut", good[:13 + 48 + 5], TRUNCATED),
            ("data_cut", good[:-20], TRUNCATED), ("no_terminator", gif_file(11, 9, 4, pay, gct=colours(16, 1), terminator=False, trailer=False), TRUNCATED),
            ("unknown_block", gif_file(11, 9, 4, pay, gct=colours(16, 1), extensions=(b"\x55",)), TRUNCATED),
            ("short_gce", gif_file(11, 9, 4, pay, gct=colours(16, 1), extensions=(b"\x21\xf9\x02\x01\x00\x00",)), TRUNCATED),
            ("extension_cut", good[:13 + 48] + b"\x21\xfe\x09abc", TRUNCATED),
            ("no_image", good[:13 + 48] + b"\x21\xfe\x03abc\x00\x3b", NO_IMAGE),
            ("zero_width", gif_file(0, 9, 4, pay, screen=(5, 5), gct=colours(16, 1)), EMPTY),
            ("zero_height", gif_file(11, 0, 4, pay, gct=colours(16, 1)), EMPTY),
            ("too_many_pixels", gif_file(60000, 60000, 4, pay, gct=colours(16, 1)), PIXELS),
            ("code_size_1", gif_file(11, 9, 1, pay, gct=colours(16, 1)), CODE_SIZE), ("code_size_9", gif_file(11, 9, 9, pay, gct=colours(16, 1)), CODE_SIZE),
            ("code_size_0", gif_file(11, 9, 0, pay, gct=colours(16, 1)), CODE_SIZE)]
