"""The device PNG decoder (csrc/pngdec.cpp + csrc/pngdec.hip + csrc/png_inflate.h) restated in numpy / Python: what the device is held to,
byte for byte, and the files its tests run on.

``plan``     the chunk walk of ``bbocr_host_png_plan``: the same fields, the same ``BBOCR_PNG_*`` reason.
stage 0      ``zlib.decompress`` of the IDAT payloads: the filtered scanlines, ``H * (1 + row_bytes)`` bytes.
stage 1      ``unfilter``: the five filters reversed at byte distance ``bpp``, the row above the first row zero.
stage 2      ``planes``: RGB as Pillow's ``convert("RGB")`` (gray replicated, depths 1 / 2 / 4 scaled by 255 / 85 / 17, alpha dropped, palette
             looked up); gray the stored (scaled) sample for colour types 0 and 4, else ``(9797 R + 19234 G + 3737 B) >> 15``.
The files: ``matrix`` (every supported (depth, colour type) pair against every width, height, row-filter plan, compressor setting and IDAT
split), ``handwritten`` (deflate streams written token by token: what zlib's compressor never emits) and ``damaged``.
"""
import struct
import zlib

import numpy as np

from png_ref import CL_EXTRA_BITS, CL_ORDER, LEN_BASE, LEN_EXTRA, LEN_SYM, _pack, canonical_codes

SIG = b"\x89PNG\r\n\x1a\n"
MAX_PIXELS = 2 * 89478485            # above it Pillow raises DecompressionBombError (twice Image.MAX_IMAGE_PIXELS): the plan refuses the file
(OK, NOT_PNG, TRUNCATED, CRC, DIMENSIONS, DEPTH, INTERLACE, PALETTE, IDAT_ORDER, APNG, ZLIB, HEADER) = range(12)      # bbocr.h BBOCR_PNG_*
PAIRS = [(1, 0), (2, 0), (4, 0), (8, 0), (1, 3), (2, 3), (4, 3), (8, 3), (8, 2), (8, 4), (8, 6)]                       # (depth, colour type)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
WIDTHS, HEIGHTS = (1, 2, 7, 8, 9, 63, 64, 65), (1, 2, 63, 64, 65, 129)
GPU_WIDTHS, GPU_HEIGHTS = (1, 8, 63, 64, 65), (1, 63, 64, 65, 129)
FILTER_PLANS = [("all", k) for k in range(5)] + [("first", k) for k in range(5)] + [("random", 0)]
COMPRESSORS = ("level0", "fixed", "default", "huffman", "rle", "fullflush", "wbits9")
SPLITS = ("one", "bytes", "zero")


class Refused(ValueError):
    """the restatement gives up on the file: ``args[0]`` says where"""


# ------------------------------------------------------------------------------------------------ the plan
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def walk(data):
    """-> (plan dict, [IDAT payloads], palette bytes).  plan["reason"] as bbocr_host_png_plan's."""
    pl = dict(width=0, height=0, bit_depth=0, color_type=0, channels=0, bpp=0, row_bytes=0, palette_entries=0, idat_chunks=0, idat_bytes=0,
              supported=0, reason=OK)
    idat, palette = [], b""

    def refuse(reason):
        pl["supported"], pl["reason"] = 0, reason
        return pl, idat, palette

    if data[:8] != SIG:
        return refuse(NOT_PNG)
    at, first, seen_idat, last_idat, seen_plte = 8, True, False, False, False
    while True:
        if len(data) - at < 12:
            return refuse(TRUNCATED)
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if n > 0x7FFFFFFF or n > len(data) - at - 12:
            return refuse(TRUNCATED)
        body = data[at + 8:at + 8 + n]
        if zlib.crc32(kind + body) != struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]:       # every chunk, as Pillow checks every chunk
            return refuse(CRC)
        if first:
            if kind != b"IHDR" or n != 13:
                return refuse(HEADER)
            first = False
            w, h, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", body)
            pl["bit_depth"], pl["color_type"] = depth, ct
            if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
                return refuse(DIMENSIONS)
            pl["width"], pl["height"] = w, h
            if ct not in CHANNELS:
                return refuse(HEADER)
            legal = depth in (1, 2, 4, 8, 16) and (ct == 0 or (ct == 3 and depth <= 8) or (ct in (2, 4, 6) and depth >= 8))
            if not legal or depth == 16:
                return refuse(DEPTH)
            pl["channels"] = CHANNELS[ct]
            pl["bpp"] = pl["channels"] if depth == 8 else 1
            pl["row_bytes"] = (w * pl["channels"] * depth + 7) // 8
            if comp or flt or lace > 1:
                return refuse(HEADER)
            if lace == 1:
                return refuse(INTERLACE)
            if h * (1 + pl["row_bytes"]) > 2 ** 31 - 1 or w * h > MAX_PIXELS:
                return refuse(DIMENSIONS)
        elif kind == b"IHDR":
            return refuse(HEADER)
        elif kind == b"PLTE":
            if seen_idat or seen_plte or n == 0 or n > 768 or n % 3:
                return refuse(PALETTE)
            seen_plte, palette = True, body
            pl["palette_entries"] = n // 3
        elif kind == b"acTL":
            return refuse(APNG)
        elif kind == b"IDAT":
            if seen_idat and not last_idat:
                return refuse(IDAT_ORDER)
            if pl["color_type"] == 3 and not seen_plte:
                return refuse(PALETTE)
            seen_idat = True
            idat.append(body)
            pl["idat_chunks"] += 1
            pl["idat_bytes"] += n
        last_idat = kind == b"IDAT"
        at += 12 + n
        if kind == b"IEND":
            break
    if not seen_idat:
        return refuse(HEADER)
    z = b"".join(idat)[:2]
    if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or (z[1] & 0x20) or ((z[0] << 8) | z[1]) % 31:
        return refuse(ZLIB)
    pl["supported"] = 1
    return pl, idat, palette


def plan(data):
    return walk(data)[0]


# ------------------------------------------------------------------------------------------------ stages 1 and 2
def unfilter(stream, h, row_bytes, bpp):
    """The filtered stream -> the scanlines uint8 [h, 1 + row_bytes] (filter bytes kept, as the device keeps them).  Anti-diagonals of
    pixels: everything a pixel needs lies on the two diagonals before its own."""
    s = np.frombuffer(bytes(stream), np.uint8).reshape(h, 1 + row_bytes)
    f = s[:, 0].astype(np.int64)
    if (f > 4).any():
        raise Refused("filter byte above 4")
    npx = row_bytes // bpp
    px = s[:, 1:].reshape(h, npx, bpp).astype(np.int64)
    out = np.zeros((h + 1, npx + 1, bpp), np.int64)                       # row 0 and column 0: the zeros outside the image
    for d in range(h + npx - 1):
        ys = np.arange(max(0, d - npx + 1), min(h - 1, d) + 1)
        xs = d - ys
        a, b, c = out[ys + 1, xs], out[ys, xs + 1], out[ys, xs]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        pred = np.stack([np.zeros_like(a), a, b, (a + b) >> 1, paeth])[f[ys], np.arange(len(ys))]
        out[ys + 1, xs + 1] = (px[ys, xs] + pred) & 255
    return np.hstack([s[:, :1], out[1:, 1:].reshape(h, row_bytes).astype(np.uint8)])


def samples(scan, pl):
    """the unfiltered scanlines -> the samples int64 [H, W, channels]"""
    h, w, depth, ch = pl["height"], pl["width"], pl["bit_depth"], pl["channels"]
    rows = scan[:, 1:]
    if depth == 8:
        return rows.reshape(h, w, ch).astype(np.int64)
    bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth).astype(np.int64)
    return (bits << np.arange(depth - 1, -1, -1)).sum(axis=2)[:, :, None]


def planes(scan, pl, palette):
    """-> (rgb uint8 [H,W,3], gray uint8 [H,W])"""
    v, depth, ct = samples(scan, pl), pl["bit_depth"], pl["color_type"]
    if ct in (0, 4):
        g = (v[:, :, 0] * {1: 255, 2: 85, 4: 17, 8: 1}[depth]).astype(np.uint8)
        return np.repeat(g[:, :, None], 3, axis=2), g
    if ct == 3:
        if (v >= pl["palette_entries"]).any():
            raise Refused("palette index at or above palette_entries")
        rgb = np.frombuffer(palette, np.uint8).reshape(-1, 3)[v[:, :, 0]]
    else:
        rgb = v[:, :, :3].astype(np.uint8)
    a = rgb.astype(np.int64)
    return np.ascontiguousarray(rgb), ((a[..., 0] * 9797 + a[..., 1] * 19234 + a[..., 2] * 3737) >> 15).astype(np.uint8)


def decode(data):
    """-> dict(plan, stage0 bytes, stage1 uint8 [H, 1 + row_bytes], rgb, gray); ``Refused`` where the device must answer with a status
    (or, for the plan, where it refuses the file)"""
    pl, idat, palette = walk(data)
    if not pl["supported"]:
        raise Refused("plan reason %d" % pl["reason"])
    want = pl["height"] * (1 + pl["row_bytes"])
    try:
        d = zlib.decompressobj()
        s0 = d.decompress(b"".join(idat))
    except zlib.error as e:
        raise Refused("zlib: %s" % e)
    if not d.eof or len(s0) != want:
        raise Refused("the stream inflates to %d bytes, not %d" % (len(s0), want))
    s1 = unfilter(s0, pl["height"], pl["row_bytes"], pl["bpp"])
    rgb, gray = planes(s1, pl, palette)
    return dict(plan=pl, stage0=s0, stage1=s1, rgb=rgb, gray=gray)


# ------------------------------------------------------------------------------------------------ writing files
def pack_rows(v, depth):
    """samples int [H, W, channels] -> the scanlines' bytes uint8 [H, row_bytes]"""
    h = v.shape[0]
    if depth == 8:
        return v.reshape(h, -1).astype(np.uint8)
    bits = ((v.reshape(h, -1, 1) >> np.arange(depth - 1, -1, -1)) & 1).astype(np.uint8).reshape(h, -1)
    return np.packbits(bits, axis=1)


def apply_filters(rows, filters, bpp):
    """scanlines uint8 [H, row_bytes] + a filter number per row -> the filtered stream's bytes"""
    h = rows.shape[0]
    raw = rows.astype(np.int64)
    up = np.vstack([np.zeros((1, raw.shape[1]), np.int64), raw[:-1]])
    left = np.hstack([np.zeros((h, bpp), np.int64), raw[:, :-bpp]])[:, :raw.shape[1]]
    upleft = np.hstack([np.zeros((h, bpp), np.int64), up[:, :-bpp]])[:, :raw.shape[1]]
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    cand = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - paeth]) & 255
    filters = np.asarray(filters, np.int64)
    out = cand[np.minimum(filters, 4), np.arange(h)].astype(np.uint8)
    return np.hstack([filters.astype(np.uint8)[:, None], out]).tobytes()


def compress(stream, how):
    kw = dict(level0=dict(level=0), fixed=dict(strategy=zlib.Z_FIXED), default={}, huffman=dict(strategy=zlib.Z_HUFFMAN_ONLY),
              rle=dict(strategy=zlib.Z_RLE), fullflush={}, wbits9=dict(wbits=9))[how]
    c = zlib.compressobj(kw.get("level", 6), zlib.DEFLATED, kw.get("wbits", 15), 8, kw.get("strategy", zlib.Z_DEFAULT_STRATEGY))
    if how == "fullflush":
        return c.compress(stream[:len(stream) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(stream[len(stream) // 2:]) + c.flush()
    return c.compress(stream) + c.flush()


def split_idat(z, how):
    if how == "one":
        return [z]
    if how == "bytes":
        return [z[i:i + 1] for i in range(len(z))]
    return [z[:len(z) // 2], b"", z[len(z) // 2:]]


def ihdr(w, h, depth, ct, lace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ct, 0, 0, lace))


def png_bytes(w, h, depth, ct, idat, palette=None, before_plte=b"", after_plte=b"", lace=0):
    """the file around IDAT payloads (a list) -- ``palette``: the PLTE payload; before_plte / after_plte: further chunks"""
    out = SIG + ihdr(w, h, depth, ct, lace) + before_plte
    if palette is not None:
        out += chunk(b"PLTE", palette)
    return out + after_plte + b"".join(chunk(b"IDAT", p) for p in idat) + chunk(b"IEND", b"")


def palette_of(depth, seed):
    return np.random.default_rng(1000 + seed).integers(0, 256, 3 << depth, dtype=np.uint8).tobytes()


def content(w, h, depth, ct, seed):
    """samples [H, W, channels]: flat runs, a ramp and noise, so that every compressor setting finds literals and matches"""
    rng = np.random.default_rng(seed)
    ch = CHANNELS[ct]
    y, x = np.mgrid[0:h, 0:w]
    base = (x * 3 + y * 5)[:, :, None] + np.arange(ch) * 40
    noise = rng.integers(0, 256, (h, w, ch))
    mask = rng.random((h, w, 1)) < 0.35
    v = np.where(mask, noise, base)
    v[h // 3:h // 3 + 2] = 200                                          # (equal rows: matches at the row distance, filters that give zeros)
    return (v >> (8 - depth)) & ((1 << depth) - 1)


def filters_of(fplan, h, seed):
    kind, k = fplan
    if kind == "all":
        return np.full(h, k)
    if kind == "first":
        return np.concatenate([[k], (np.arange(1, h) + k) % 5])
    return np.random.default_rng(77 + seed).integers(0, 5, h)


def case(pair, w, h, fplan, comp, split, seed):
    depth, ct = pair
    rows = pack_rows(content(w, h, depth, ct, seed), depth)
    bpp = CHANNELS[ct] if depth == 8 else 1
    z = compress(apply_filters(rows, filters_of(fplan, h, seed), bpp), comp)
    pal = palette_of(depth, seed) if ct == 3 else None                      # (ancillary chunks: skipped, as convert("RGB") ignores them)
    return png_bytes(w, h, depth, ct, split_idat(z, split), pal, chunk(b"gAMA", struct.pack(">I", 45455)),
                     chunk(b"tRNS", b"\x00\x01") if ct == 0 else b"")


def matrix(widths=WIDTHS, heights=HEIGHTS):
    """[(name, file)]: per (depth, colour type) pair every width against every height; along those files the filter plans, the compressor
    settings and the IDAT splits rotate at coprime steps, so that each pair meets every value of every axis (the full product of all six
    axes is 121,968 files)."""
    out = []
    for pi, pair in enumerate(PAIRS):
        i = pi
        for w in widths:
            for h in heights:
                fplan, comp, split = FILTER_PLANS[i % 11], COMPRESSORS[(i // 2 + pi) % 7], SPLITS[(i + i // 3) % 3]
                name = "d%dt%d_%dx%d_%s%d_%s_%s" % (pair + (w, h) + fplan + (comp, split))
                out.append((name, case(pair, w, h, fplan, comp, split, len(out))))
                i += 1
    return out


def axis_values(names):
    """the (pair, axis value) combinations a list of matrix names holds: the tests assert that none is missing"""
    seen = set()
    for n in names:
        pair, size, fplan, comp, split = n.split("_")
        w, h = size.split("x")
        seen |= {(pair, "w" + w), (pair, "h" + h), (pair, fplan), (pair, comp), (pair, split)}
    return seen


# ------------------------------------------------------------------------------------------------ deflate, token by token
class Bits:
    """values of n bits each, least significant bit first, back to back"""

    def __init__(self):
        self.vals, self.bits = [], []

    def put(self, v, n):
        if n:
            self.vals.append(int(v))
            self.bits.append(int(n))

    def count(self):
        return sum(self.bits)

    def align(self):
        self.put(0, -self.count() % 8)

    def raw(self, data):
        assert self.count() % 8 == 0
        for b in data:
            self.put(b, 8)

    def bytes(self):
        return _pack(self.vals, self.bits) if self.vals else b""


DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def dist_sym(d):
    return max(s for s in range(30) if DIST_BASE[s] <= d)


def stored(w, data, final=0):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF, 16)
    w.raw(data)


def put_tokens(w, tokens, lit_lens, dist_lens):
    """tokens: an int is a literal, (length, distance) a match; then the end of block"""
    lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            s = int(LEN_SYM[n])
            assert lit_lens[257 + s] and dist_lens[dist_sym(d)], "the code has no pattern for this token"
            w.put(lc[257 + s], lit_lens[257 + s])
            w.put(n - LEN_BASE[s], LEN_EXTRA[s])
            ds = dist_sym(d)
            w.put(dc[ds], dist_lens[ds])
            w.put(d - DIST_BASE[ds], DIST_EXTRA[ds])
        else:
            assert lit_lens[t]
            w.put(lc[t], lit_lens[t])
    w.put(lc[256], lit_lens[256])


def fixed(w, tokens, final=0):
    w.put(final, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LIT, FIXED_DIST)


def run_length(seq, repeat_nonzero=True):
    """code lengths -> code-length symbols [(sym, extra)], maximal runs over the WHOLE sequence (a run may cross from the literal/length
    lengths into the distance lengths)"""
    toks, i = [], 0
    while i < len(seq):
        v, j = seq[i], i + 1
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                c = min(n, 138)
                toks.append((18, c - 11))
                n -= c
            if n >= 3:
                toks.append((17, n - 3))
                n = 0
            toks += [(0, 0)] * n
        else:
            toks.append((v, 0))
            n -= 1
            while n >= 3 and repeat_nonzero:
                c = min(n, 6)
                toks.append((16, c - 3))
                n -= c
            toks += [(v, 0)] * n
        i = j
    return toks


def dynamic(w, tokens, lit_lens, dist_lens, final=0, cl_lens=None, hclen=None, plain_header=False, repeat_nonzero=True):
    """A dynamic block with the given code lengths (lit_lens[0 .. nlen), dist_lens[0 .. ndist), trailing zeros kept: they set HLIT / HDIST).
    cl_lens: the code-length code (default: 5 bits for every symbol the header uses, which is complete for 1, 2, 4, 8, 16 symbols only -- so
    the default pads to a complete code); plain_header: no repeat symbols."""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    seq = lit_lens + dist_lens
    toks = [(v, 0) for v in seq] if plain_header else run_length(seq, repeat_nonzero)
    if cl_lens is None:
        used = sorted({s for s, _ in toks})
        cl_lens = [0] * 19
        size = 1
        while size < len(used):
            size *= 2
        pad = [s for s in range(19) if s not in used][:size - len(used)]
        bits = max(1, size.bit_length() - 1)
        for s in used + pad:
            cl_lens[s] = bits
    if hclen is None:
        hclen = 19
        while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
            hclen -= 1
    assert all(cl_lens[CL_ORDER[k]] == 0 for k in range(hclen, 19))
    cc = canonical_codes(cl_lens)
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    for s, extra in toks:
        assert cl_lens[s]
        w.put(cc[s], cl_lens[s])
        w.put(extra, CL_EXTRA_BITS.get(s, 0))
    put_tokens(w, tokens, lit_lens + [0] * (288 - len(lit_lens)), dist_lens + [0] * (30 - len(dist_lens)))


def expand(tokens, out=b""):
    out = bytearray(out)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            assert d <= len(out)
            for _ in range(n):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out)


def zlib_wrap(deflate_bytes, data, adler=None):
    return b"\x78\x01" + deflate_bytes + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def lits(data):
    return list(data)


def _lens(pairs, n):
    out = [0] * n
    for s, l in pairs:
        out[s] = l
    return out


def handwritten():
    """[(name, zlib stream, the bytes it holds)] -- each stream is checked against zlib.decompress by the CPU tests"""
    rng = np.random.default_rng(5)
    out = []

    def add(name, w, data):
        out.append((name, zlib_wrap(w.bytes(), data), data))

    noise = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = Bits()
    stored(w, noise)
    t = [(10, 32768), (258, 32768)]
    fixed(w, t, 1)
    add("distance_32768", w, expand(t, noise))

    head = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    w = Bits()
    t = lits(head) + [(258, 300), (3, 3), (3, 558), (258, 1)]
    fixed(w, t, 1)
    add("length_258_and_3", w, expand(t))

    for d in (1, 2, 3, 63, 64, 65):
        w = Bits()
        t = lits(head[:d + 2]) + [(258, d), (max(3, d + 1), d), (100, d)]
        fixed(w, t, 1)
        add("distance_%d_below_length" % d, w, expand(t))

    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    w = Bits()
    fixed(w, lits(b"ab"))                                # ends off a byte boundary: the stored blocks pad
    stored(w, b"")
    fixed(w, lits(b"c"))
    stored(w, big, 1)
    add("stored_0_and_65535_unaligned", w, b"abc" + big)

    two = _lens([(0, 1), (256, 1)], 257)
    w = Bits()
    dynamic(w, [], two, [0])                             # an empty dynamic block
    fixed(w, lits(b"after the empty block"), 1)
    add("empty_dynamic_block", w, b"after the empty block")

    # HCLEN = 4 (the field; eight code-length codes: 16 17 18 0 8 7 9 6): 64 codes of 6 bits
    six = _lens([(s, 6) for s in range(32, 95)] + [(256, 6)], 257)
    cl = _lens([(0, 2), (6, 2), (17, 2), (18, 2)], 19)
    msg = bytes(range(32, 95)) * 3
    w = Bits()
    dynamic(w, lits(msg), six, [0], 1, cl_lens=cl, hclen=8, repeat_nonzero=False)
    assert (w.vals[4], w.bits[4]) == (4, 4)
    add("hclen_4", w, msg)

    # HLIT = 29: the zeros of symbols 258 .. 285 run on into the distance lengths (one repeat symbol 18 covers both)
    lit = _lens([(s, 8) for s in range(254)] + [(254, 9), (255, 9), (256, 9), (257, 9)], 286)
    dist = [0, 0, 0, 0, 1, 1]
    assert (18, 32 - 11) in run_length(lit + dist)
    w = Bits()
    t = lits(head[:20]) + [(3, 5), (3, 8)]
    dynamic(w, t, lit, dist, 1)
    add("repeat_crosses_into_distances", w, expand(t))

    w = Bits()
    t = lits(b"xy") + [(3, 1), (3, 1)]
    dynamic(w, t, _lens([(120, 2), (121, 2), (256, 2), (257, 2)], 258), [1], 1)
    add("single_distance_code", w, expand(t))

    w = Bits()
    dynamic(w, lits(b"xyxxy"), _lens([(120, 1), (121, 2), (256, 2)], 257), [0], 1)
    add("no_distance_code", w, b"xyxxy")

    deep = _lens([(65 + k, k + 1) for k in range(14)] + [(80, 15), (256, 15)], 257)
    msg = bytes([80, 65, 78, 80, 66, 77, 80])
    w = Bits()
    dynamic(w, lits(msg), deep, [0], 1, plain_header=True)
    add("code_of_15_bits", w, msg)

    w = Bits()
    stored(w, head[:40])
    t1 = lits(head[40:60]) + [(20, 60)]
    fixed(w, t1)
    t2 = lits(b"xyxy") + [(3, 1)]
    dynamic(w, t2, _lens([(120, 2), (121, 2), (256, 2), (257, 2)], 258), [1], 1)
    add("stored_fixed_dynamic", w, expand(t2, expand(t1, head[:40])))
    return out


def damaged():
    """[(name, zlib stream, the length a file around it promises)] -- each is rejected by zlib.decompress or inflates to another length,
    except ``filter_byte_5``, whose stream is sound and whose scanlines are not"""
    rng = np.random.default_rng(9)
    body = bytearray(rng.integers(0, 64, 600, dtype=np.uint8).tobytes())
    body[0], body[200], body[400] = 0, 1, 4              # three rows of a 199-pixel gray file
    body = bytes(body)
    good = compress(body, "default")
    out = [("truncated_at_a_third", good[:len(good) // 3], 600)]
    w = Bits()
    w.put(1, 1)
    w.put(3, 2)
    w.align()
    out.append(("block_type_3", zlib_wrap(w.bytes() + b"\x00" * 8, body), 600))
    w = Bits()
    stored(w, body, 1)
    s = bytearray(w.bytes())
    s[3] ^= 1
    out.append(("len_nlen_mismatch", zlib_wrap(bytes(s), body), 600))
    w = Bits()
    dynamic(w, [0], _lens([(0, 1), (1, 1), (256, 1)], 257), [0], 1, plain_header=True)
    out.append(("oversubscribed_code", zlib_wrap(w.bytes(), b"\x00"), 600))
    w = Bits()
    dynamic(w, [0], _lens([(0, 2), (256, 2)], 257), [0], 1, plain_header=True)
    out.append(("incomplete_code", zlib_wrap(w.bytes(), b"\x00"), 600))
    w = Bits()
    w.put(1, 1)
    w.put(1, 2)
    put_tokens(w, [0, (3, 5)], FIXED_LIT, FIXED_DIST)
    out.append(("distance_too_far", zlib_wrap(w.bytes(), b"\x00" * 4), 600))
    out.append(("wrong_adler", good[:-4] + struct.pack(">I", zlib.adler32(body) ^ 0x10000), 600))
    out.append(("one_byte_too_many", compress(body + b"\x07", "default"), 600))
    out.append(("one_byte_too_few", compress(body[:-1], "default"), 600))
    bad = bytearray(body)
    bad[200] = 5                                         # the filter byte of the second row
    out.append(("filter_byte_5", compress(bytes(bad), "default"), 600))
    return out


def wrap_stream(z, length, rows=1):
    """a zlib stream that holds ``length`` bytes as a gray 8-bit file of ``rows`` rows (the damage list: 3 rows of 199 pixels)"""
    assert length % rows == 0
    return png_bytes(length // rows - 1, rows, 8, 0, [z])


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # x0, y0, dx, dy per pass


def adam7_file(img):
    """uint8 [H,W] or [H,W,3] -> an Adam7 file of it (Pillow writes none): the plan refuses it, Pillow reads it"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    stream = b""
    for x0, y0, dx, dy in ADAM7:
        sub = img[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            stream += b"".join(b"\x00" + row.tobytes() for row in sub)
    return png_bytes(w, h, 8, 0 if img.ndim == 2 else 2, [zlib.compress(stream)], lace=1)
