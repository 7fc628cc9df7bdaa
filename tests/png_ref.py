"""The device PNG writer (csrc/pngenc.hip + csrc/pngenc.cpp) restated in numpy / Python: the definition the device is held to, byte for byte.

A page (uint8 [H,W] gray or [H,W,3] RGB) becomes a lossless 8-bit PNG file:

A. ``filter_stream``: per row the five PNG filters over the raw neighbours; the one with the smallest sum of ``abs(int8(x))`` wins, ties
   to the lowest filter number; the stream is ``[filter byte][row]`` per row.
B. ``chunk_tokens``: the stream is cut into chunks of ``CHUNK`` bytes, each a deflate block of its own.  Inside a chunk a maximal run of L
   equal bytes is its first byte as a literal, then -- R = L - 1 -- while R >= 3 a match of min(R, 258) at distance 1, then the last 0 .. 2
   bytes as literals.
C. ``code_lengths``: length-limited Huffman code lengths as a pure integer function of the histogram (the rule is in its docstring);
   ``header_tokens``: the lengths run-length coded with the code-length symbols 16 / 17 / 18.
D. ``encode_chunk``: dynamic header + tokens + end of block + an empty stored block (000, pad, 00 00 FF FF); a stored block when that is not
   shorter.  No block is final.
``deflate``: zlib header 78 01, the chunks' blocks, the final empty fixed block 03 00, Adler-32.  ``png_file``: signature, IHDR, iCCP (the
profile in stored blocks), one IDAT, IEND.
"""
import struct
import zlib

import numpy as np

CHUNK = 16384
LITLEN, CL = 286, 19
HIST_ROW, REC = 288, 320
STORED, DYNAMIC = 0, 1
LIMIT15, LIMIT7 = 1, 2
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: length symbol 257 + s covers LEN_BASE[s] .. with LEN_EXTRA[s] extra bits; 258 has its own symbol
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_SYM = np.zeros(259, np.int64)
for _s in range(28):
    LEN_SYM[LEN_BASE[_s]:LEN_BASE[_s] + (1 << LEN_EXTRA[_s])] = _s
LEN_SYM[258] = 28
LEN_EXTRA_A, LEN_BASE_A = np.array(LEN_EXTRA, np.int64), np.array(LEN_BASE, np.int64)


# ------------------------------------------------------------------------------------------------ stage A
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img):
    """-> (filter number per row, filtered rows uint8 [H, W*c])"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    h = img.shape[0]
    bpp = 1 if img.ndim == 2 else 3
    raw = img.reshape(h, -1).astype(np.int64)
    up = np.vstack([np.zeros((1, raw.shape[1]), np.int64), raw[:-1]])
    left = np.hstack([np.zeros((h, bpp), np.int64), raw[:, :-bpp]])
    upleft = np.hstack([np.zeros((h, bpp), np.int64), up[:, :-bpp]])
    cand = np.stack([raw, raw - left, raw - up, raw - ((left + up) >> 1), raw - _paeth(left, up, upleft)]) & 255      # [5, H, n]
    cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                                                           # [5, H]
    best = np.argmin(cost, axis=0)                                                                                      # first minimum: lowest number
    return best.astype(np.uint8), cand[best, np.arange(h)].astype(np.uint8)


def filter_stream(img):
    best, rows = filter_rows(img)
    return np.hstack([best[:, None], rows]).tobytes()


# ------------------------------------------------------------------------------------------------ stage B
def chunk_tokens(c):
    """The tokens of one chunk (uint8 array), in order: ``(sym, length)`` arrays -- a literal has its byte as ``sym`` and length 0, a match
    its length symbol (257 ..) and its length."""
    c = np.asarray(c, np.uint8)
    n = len(c)
    brk = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    L = np.diff(np.concatenate([brk, [n]]))
    v = c[brk].astype(np.int64)
    R = L - 1
    nfull = R // 258
    rem = R - 258 * nfull
    tail_match = rem >= 3
    tail_lits = np.where(tail_match, 0, rem)
    cnt = 1 + nfull + tail_match + tail_lits
    run = np.repeat(np.arange(len(L)), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    full = (k >= 1) & (k <= nfull[run])
    tail = (k == nfull[run] + 1) & tail_match[run]
    length = np.where(full, 258, np.where(tail, rem[run], 0))
    sym = np.where(length > 0, 257 + LEN_SYM[length], v[run])
    return sym, length


def histogram(sym, length):
    """uint32 [288]: the 286 literal/length counts (end of block: 1), the match count, the token count"""
    h = np.zeros(HIST_ROW, np.int64)
    h[:LITLEN] = np.bincount(sym, minlength=LITLEN)
    h[256] = 1
    h[286] = int((length > 0).sum())
    h[287] = len(sym)
    return h


# ------------------------------------------------------------------------------------------------ stage C
def code_lengths(freq, maxbits):
    """Length-limited code lengths of the symbols with freq > 0 -> (lengths, limited):
    1. the used symbols sorted by (count, symbol) ascending;
    2. Huffman's tree by the two-queue merge: leaves in that order, internal nodes in the order made; of two equal heads the leaf is taken;
    3. depths above maxbits are cut to maxbits (limited = True); while the Kraft sum exceeds 1, one leaf of the longest length below
       maxbits moves one level down and takes a leaf of length maxbits with it as its sibling (each step lowers the sum by 2^-maxbits);
    4. the lengths, longest first, go to the symbols in the order of 1.
    A single used symbol gets length 1."""
    freq = [int(f) for f in freq]
    lens = [0] * len(freq)
    order = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    m = len(order)
    if m == 1:
        lens[order[0]] = 1
    if m < 2:
        return lens, False
    w = [freq[s] for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, nn = 0, m, m
    for _ in range(m - 1):
        pick = []
        for _h in range(2):
            if li < m and (ii >= nn or w[li] <= w[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        w[nn] = w[pick[0]] + w[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nn
        nn += 1
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, m - 1, -1):
        depth[i] = depth[parent[i]] + 1
    bl = [0] * (maxbits + 1)
    limited = False
    for i in range(m):
        d = depth[parent[i]] + 1
        if d > maxbits:
            d, limited = maxbits, True
        bl[d] += 1
    excess = sum(bl[d] << (maxbits - d) for d in range(1, maxbits + 1)) - (1 << maxbits)
    while excess > 0:
        d = maxbits - 1
        while bl[d] == 0:
            d -= 1
        bl[d] -= 1
        bl[d + 1] += 2
        bl[maxbits] -= 1
        excess -= 1
    i = 0
    for d in range(maxbits, 0, -1):
        for _ in range(bl[d]):
            lens[order[i]] = d
            i += 1
    return lens, limited


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> the codes, bit-reversed (deflate packs Huffman codes from their most significant bit)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lens:
        if l:
            out.append(int(format(nxt[l], "0%db" % l)[::-1], 2))
            nxt[l] += 1
        else:
            out.append(0)
    return out


def header_tokens(litlen, dist):
    """The header's code lengths as code-length symbols -> (nlit, [(sym, extra value)]): the HLIT + 257 literal/length lengths and the
    one distance length as ONE sequence, cut into maximal runs of equal values.  n zeros: while n >= 11 symbol 18 takes min(n, 138); then
    3 .. 10 left: symbol 17; 1 .. 2 left: symbols 0.  n lengths v > 0: v, then while n >= 3 symbol 16 takes min(n, 6), then the rest as v."""
    nlit = LITLEN
    while nlit > 257 and litlen[nlit - 1] == 0:
        nlit -= 1
    seq = list(litlen[:nlit]) + [dist]
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
            while n >= 3:
                c = min(n, 6)
                toks.append((16, c - 3))
                n -= c
            toks += [(v, 0)] * n
        i = j
    return nlit, toks


CL_EXTRA_BITS = {16: 2, 17: 3, 18: 7}


# ------------------------------------------------------------------------------------------------ stage D
def _pack(vals, nbits):
    """values (least significant bit first) of nbits bits each, back to back -> bytes, the last byte padded with zeros"""
    vals, nbits = np.asarray(vals, np.int64), np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    tok = np.repeat(np.arange(len(vals)), nbits)
    pos = np.arange(total) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    return np.packbits(((vals[tok] >> pos) & 1).astype(np.uint8), bitorder="little").tobytes()


class Chunk:
    """everything the model knows about one chunk: hist [288], litlen [286], dist, cl [19], flags, kind, block (its bytes), sums (A, B)"""


def encode_chunk(c):
    c = np.asarray(c, np.uint8)
    n = len(c)
    assert 1 <= n <= CHUNK
    o = Chunk()
    sym, length = chunk_tokens(c)
    o.hist = histogram(sym, length)
    o.litlen, lim15 = code_lengths(o.hist[:LITLEN], 15)
    o.dist = 1 if o.hist[286] else 0
    nlit, toks = header_tokens(o.litlen, o.dist)
    clfreq = np.bincount([s for s, _ in toks], minlength=CL)
    o.cl, lim7 = code_lengths(clfreq, 7)
    o.flags = (LIMIT15 if lim15 else 0) | (LIMIT7 if lim7 else 0)
    hclen = CL
    while hclen > 4 and o.cl[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    lcode, ccode = canonical_codes(o.litlen), canonical_codes(o.cl)
    vals = [0, 2, nlit - 257, 0, hclen - 4] + [o.cl[CL_ORDER[k]] for k in range(hclen)]
    bits = [1, 2, 5, 5, 4] + [3] * hclen
    for s, extra in toks:
        vals.append(ccode[s] | (extra << o.cl[s]))
        bits.append(o.cl[s] + CL_EXTRA_BITS.get(s, 0))
    ll, lc = np.array(o.litlen, np.int64), np.array(lcode, np.int64)
    s28 = np.where(length > 0, sym - 257, 0)
    extra_bits = np.where(length > 0, LEN_EXTRA_A[s28], 0)
    tv = lc[sym] | (np.where(length > 0, length - LEN_BASE_A[s28], 0) << ll[sym])          # code, extra bits, the distance code's 0 bit
    tb = ll[sym] + extra_bits + (length > 0)
    vals = np.concatenate([np.array(vals, np.int64), tv, [lcode[256], 0]])
    bits = np.concatenate([np.array(bits, np.int64), tb, [o.litlen[256], 3]])
    dyn_bytes = (int(bits.sum()) + 7) // 8 + 4
    a = int(c.astype(np.int64).sum()) % 65521
    b = int((c.astype(np.int64) * (n - np.arange(n))).sum()) % 65521
    o.sums = (a, b)
    if dyn_bytes >= 5 + n:
        o.kind = STORED
        o.block = b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + c.tobytes()
    else:
        o.kind = DYNAMIC
        o.block = _pack(vals, bits) + b"\x00\x00\xff\xff"
        assert len(o.block) == dyn_bytes
    return o


def chunks_of(data):
    a = np.frombuffer(bytes(data), np.uint8)
    return [encode_chunk(a[i:i + CHUNK]) for i in range(0, len(a), CHUNK)]


def deflate(data, chunks=None):
    """the zlib stream of the byte string: 78 01, the chunks' blocks, 03 00, Adler-32"""
    chunks = chunks_of(data) if chunks is None else chunks
    return b"\x78\x01" + b"".join(c.block for c in chunks) + b"\x03\x00" + struct.pack(">I", zlib.adler32(bytes(data)))


def stage_arrays(data, chunks=None):
    """bbocr_op_png_stage's stages 1, 2, 3 of a byte stream: uint32 [chunks,288], uint8 [chunks,320], int64 [chunks+1]"""
    chunks = chunks_of(data) if chunks is None else chunks
    hist = np.array([c.hist for c in chunks], np.uint32).reshape(len(chunks), HIST_ROW)
    rec = np.zeros((len(chunks), REC), np.uint8)
    for k, c in enumerate(chunks):
        rec[k, 0], rec[k, 1] = c.kind, c.flags
        rec[k, 2:2 + LITLEN] = c.litlen
        rec[k, 2 + LITLEN] = c.dist
        rec[k, 3 + LITLEN:3 + LITLEN + CL] = c.cl
    off = np.concatenate([[0], np.cumsum([len(c.block) for c in chunks])]).astype(np.int64)
    return hist, rec, off


# ------------------------------------------------------------------------------------------------ the file
def _png_chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def stored_zlib(data):
    """the zlib stream of stored blocks the iCCP chunk carries the profile in"""
    out = b"\x78\x01"
    for i in range(0, len(data), 65535):
        part = data[i:i + 65535]
        out += bytes([1 if i + 65535 >= len(data) else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    return out + struct.pack(">I", zlib.adler32(data))


def png_file(img, icc=None, chunks=None):
    img = np.asarray(img)
    h, w = img.shape[:2]
    out = b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if img.ndim == 2 else 2, 0, 0, 0))
    if icc:
        out += _png_chunk(b"iCCP", b"ICC Profile\x00\x00" + stored_zlib(bytes(icc)))
    return out + _png_chunk(b"IDAT", deflate(filter_stream(img), chunks)) + _png_chunk(b"IEND", b"")


def encode_bound(h, w, channels, icc_bytes=0):
    """bbocr_png_encode_bound"""
    if h < 1 or w < 1 or channels not in (1, 3):
        return 0
    stream = h * (1 + w * channels)
    icc = 31 + icc_bytes + 5 * -(-icc_bytes // 65535) if icc_bytes else 0
    if 2 + -(-stream // CHUNK) * 5 + stream + 6 > 2 ** 31 - 1 or icc - 12 > 2 ** 31 - 1:
        return 0
    return 59 + icc + -(-stream // CHUNK) * 5 + stream + 2 + 4


def deflate_bound(n):
    return 2 + -(-n // CHUNK) * 5 + n + 6


def idat_payload(png):
    """the concatenated IDAT payloads of a PNG file"""
    at, out = 8, b""
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        if kind == b"IDAT":
            out += png[at + 8:at + 8 + n]
        at += 12 + n
    return out
