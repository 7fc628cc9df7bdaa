"""A transcoder for baseline JPEG files, not an encoder: ``forge(data, **options)`` reads the quantised coefficients of a file Pillow wrote
(grey, 4:2:0, 4:4:4, 4:2:2 or 4:4:0) with the restatement (jpeg_chroma_ref.decode_coefficients, which is jpeg_entropy_ref's over any of
those MCU layouts) and writes them out again in a dialect no libjpeg encoder speaks: other Huffman tables, table and component ids, DHT /
DQT layouts, restart intervals, fill bytes, padding, extra segments.  The coefficients and the quantisation tables do not change, so a
forged file's pixels are the source's; Pillow's decoder is the independent judge of the syntax (test_jpeg_forge_cpu.py).

Tables are ``(counts[16], vals)`` pairs, T.81's BITS and HUFFVAL.  The builders: ``standard``, ``flat``, ``unary``, ``optimal``, ``skewed``
and ``invalid_tables``.  Where ``forge`` takes a table it also takes a function of the symbol frequencies ``{symbol: count}`` of the
components that select it, for the builders that need them."""
from __future__ import annotations

import struct

import jpeg_chroma_ref as K
import jpeg_encode_ref as E
import jpeg_entropy_ref as J

DC_SYMBOLS = list(range(12))
AC_SYMBOLS = sorted(E.AC_LUM[1])                                  # the 162 run/size symbols of 8-bit baseline data
RST = "rst"                                                       # key of ``fill``: every RSTn marker
EOI = 0xD9


# ------------------------------------------------------------------------------------------------ table builders
def standard(cls, chroma=False):
    """T.81 K.3's typical table of class ``cls`` (0 DC, 1 AC)"""
    return ((E.DC_LUM, E.DC_CHROM), (E.AC_LUM, E.AC_CHROM))[cls][chroma]


def flat(length, symbols):
    """every symbol a code of ``length`` bits"""
    assert len(symbols) < (1 << length)
    counts = [0] * 16
    counts[length - 1] = len(symbols)
    return counts, list(symbols)


def unary(symbols):
    """one code per length 1, 2, .. k (0, 10, 110, ..) in the order of ``symbols``, the rest at 16 bits; k the largest that leaves them room"""
    n = len(symbols)
    k = next(k for k in range(min(n, 16), -1, -1) if k == n or (k < 16 and n - k < (1 << (16 - k))))
    counts = [1] * k + [0] * (16 - k)
    counts[15] += n - k
    return counts, list(symbols)


def optimal(freq):
    """jchuff.c::jpeg_gen_optimal_table for the frequencies ``{symbol: count}``: Huffman's code, limited to 16 bits, all-ones reserved"""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    f[256] = 1
    size, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2                                           # chain c2's tree onto c1's
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * (max(size) + 2)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = min(16, len(bits) - 1)
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                  # the pseudo-symbol 256 held the all-ones code
    order = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    return (bits[1:17] + [0] * 16)[:16], order


def skewed(freq, counts, symbols):
    """the code lengths of ``counts`` handed out against the frequencies: the rarest of ``symbols`` get the shortest codes, the most
    frequent the longest"""
    assert sum(counts) == len(symbols)
    return list(counts), sorted(symbols, key=lambda s: (freq.get(s, 0), s))


def invalid_tables():
    """{name: (class, (counts, vals))}: tables jdhuff.c::jpeg_make_d_derived_tbl refuses (JERR_BAD_HUFF_TABLE)"""
    return {
        "dc-sixteen-4-bit-codes": (0, ([0, 0, 0, 16] + [0] * 12, list(range(16)))),                  # 1111 is a code
        "dc-two-1-bit-codes": (0, ([2] + [0] * 15, [0, 1])),                                          # 1 is a code
        "ac-all-ones-at-16": (1, ([1] * 15 + [2], AC_SYMBOLS[:17])),                                  # 0, 10, .. and both 16-bit codes left
        "ac-oversubscribed": (1, ([3] + [0] * 15, [0, 1, 2])),                                        # three 1-bit codes
        "dc-category-16": (0, ([0, 0, 0, 13] + [0] * 12, list(range(12)) + [16])),                    # a prefix code, of a symbol no DC table holds
    }


def codes_of(spec):
    """{symbol: (code, length)} (Annex C)"""
    return E._codes(spec)


# ------------------------------------------------------------------------------------------------ symbols
def _nbits(v):
    return abs(v).bit_length()


def _block(zz, pred):
    """jchuff.c::encode_one_block: [(class, symbol, extra bits, their number)] of one block in zig-zag order"""
    diff = zz[0] - pred
    n = _nbits(diff)
    out = [(0, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)]
    r = 0
    for k in range(1, 64):
        v = zz[k]
        if v == 0:
            r += 1
            continue
        while r > 15:
            out.append((1, 0xF0, 0, 0))
            r -= 16
        n = _nbits(v)
        out.append((1, (r << 4) + n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
        r = 0
    if r:
        out.append((1, 0x00, 0, 0))
    return out


def _pack(pairs):
    """(value, bits) pairs MSB first, the last byte filled with 1-bits, then stuffed"""
    acc = n = 0
    out = bytearray()
    for v, l in pairs:
        acc = (acc << l) | v
        n += l
        while n >= 8:
            out.append((acc >> (n - 8)) & 0xFF)
            n -= 8
        acc &= (1 << n) - 1
    if n:
        out.append(((acc << (8 - n)) | ((1 << (8 - n)) - 1)) & 0xFF)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def segment_symbols(data, ri=None):
    """-> (plan, comp of every block in an MCU, [segment][(component, class, symbol, extra, n)]) for the restart interval ``ri`` (None:
    the file's own, 0: none)"""
    plan = K.parse(data)
    assert plan["supported"] or plan["chroma"], plan
    coef, _ = K.decode_coefficients(data, plan)
    st = K.Stream(data, plan)
    zz = coef[:, J.ZIGZAG].tolist()
    ri = plan["restart_interval"] if ri is None else ri
    per = (ri or st.nmcu) * st.bpm
    segs = []
    for a in range(0, len(zz), per):
        pred = [0, 0, 0]
        syms = []
        for b in range(a, min(a + per, len(zz))):
            c = st.comp[b % st.bpm]
            syms += [(c,) + s for s in _block(zz[b], pred[c])]
            pred[c] = zz[b][0]
        segs.append(syms)
    return plan, st.comp, segs


def frequencies(data, ri=None, select=None):
    """{(class, id): {symbol: count}} of the file's symbols under the restart interval ``ri`` and the table selection ``select``"""
    plan, _, segs = segment_symbols(data, ri)
    select = select or plan["tables"]
    freq = {}
    for syms in segs:
        for c, cls, sym, _, _ in syms:
            f = freq.setdefault((cls, select[c][cls]), {})
            f[sym] = f.get(sym, 0) + 1
    return freq


# ------------------------------------------------------------------------------------------------ the file
def _seg(marker, body):
    assert len(body) + 2 <= 65535
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def _wrong(spec):
    """a valid table that is not ``spec``: its symbols in the opposite order"""
    return spec[0], list(reversed(spec[1]))


def forge(data, *, tables=None, select=None, dht="each", dht_twice=None, dht_where="after", dht_override=None, dqt_ids=None, dqt="each",
          dqt_twice=False, dqt16=False, comp_ids=None, sos_order=None, marking="jfif", dri=None, fill=None, pad=None, extra=(),
          trailer=b""):
    """The file ``data`` written again.  Options (defaults: the source's own choice, Pillow's layout):
    tables      {(class, id): table or function of the frequencies}: the Huffman tables, under the ids they are sent with
    select      [(DC id, AC id)] per component: what SOS names
    dht         "each": one DHT segment per table; "one": one for all
    dht_twice   "after" / "before": every table is sent twice, the first copy wrong, behind / in front of SOF0
    dht_where   "after" / "before": the (right) tables behind / in front of SOF0
    dht_override {(class, id): table}: written in DHT in place of the table the scan is coded with (invalid tables)
    dqt_ids     quantisation table id per component; dqt "each" / "one" segment; dqt_twice: every table defined wrong in front of SOF0 and
                again, right, behind it; dqt16: 16-bit entries (refused)
    comp_ids    component ids of SOF0 and SOS; sos_order: the order SOS names the components in (refused unless the frame's)
    marking     "jfif", "adobe1" / "adobe0" (APP14 with that transform, no JFIF), "none"
    dri         the DRI values sent, in order (a number: that one); the last one holds and the data are cut by it.  None: the source's
    fill        {marker: n}: n fill bytes FF in front of every such marker (``RST``: every RSTn, ``EOI``)
    pad         (segment, bytes without FF): bytes behind the last MCU of that restart segment
    extra       [(before, marker, body bytes)]: a segment of ``marker`` in front of the first ``before`` segment
    trailer     bytes behind EOI"""
    dri = [dri] if isinstance(dri, int) else dri
    ri = None if dri is None else dri[-1]
    plan, comp, segs = segment_symbols(data, ri)
    nc = plan["components"]
    if dri is None:
        dri = [plan["restart_interval"]] if plan["restart_interval"] else []
    select = [tuple(s) for s in (select or plan["tables"])]
    assert len(select) == nc
    if tables is None:
        assert all(((0, d) in plan["huff"] and (1, a) in plan["huff"]) for d, a in select)
        tables = {k: v for k, v in plan["huff"].items() if any(s[k[0]] == k[1] for s in select)}
    freq = {}
    for syms in segs:
        for c, cls, sym, _, _ in syms:
            f = freq.setdefault((cls, select[c][cls]), {})
            f[sym] = f.get(sym, 0) + 1
    tables = {k: (t(freq.get(k, {})) if callable(t) else t) for k, t in tables.items()}
    codes = {k: codes_of(t) for k, t in tables.items()}
    fill = fill or {}

    def marker(m):
        return b"\xff" * fill.get(RST if 0xD0 <= m <= 0xD7 else m, 0) + bytes([0xFF, m])

    # the entropy-coded data
    scan = b""
    for i, syms in enumerate(segs):
        pairs = []
        for c, cls, sym, bits, n in syms:
            pairs.append(codes[(cls, select[c][cls])][sym])
            if n:
                pairs.append((bits, n))
        scan += _pack(pairs)
        if pad and pad[0] % len(segs) == i:
            assert 0xFF not in pad[1]
            scan += bytes(pad[1])
        if i + 1 < len(segs):
            scan += marker(0xD0 + i % 8)
    # the headers
    head = []                                                     # (marker, body)
    if marking == "jfif":
        head.append((0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"))
    elif marking in ("adobe0", "adobe1"):
        head.append((0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([int(marking[-1])])))
    dqt_ids = list(dqt_ids or [0, 1, 1][:nc])
    quant = {}
    for c in range(nc):
        assert quant.setdefault(dqt_ids[c], plan["quant"][c]) == plan["quant"][c], "components that share a table id must share the table"

    def dqt_segments(wrong):
        bodies = []
        for tid, q in quant.items():
            vals = [(q[z] % 255) + 1 if wrong else q[z] for z in J.ZIGZAG]
            bodies.append(bytes([0x10 | tid]) + b"".join(struct.pack(">H", v) for v in vals) if dqt16 else bytes([tid]) + bytes(vals))
        return [(0xDB, b"".join(bodies))] if dqt == "one" else [(0xDB, b) for b in bodies]

    def dht_segments(wrong):
        bodies = []
        for (cls, tid), t in tables.items():
            t = (dht_override or {}).get((cls, tid), t)
            t = _wrong(t) if wrong else t
            bodies.append(bytes([(cls << 4) | tid]) + bytes(t[0]) + bytes(t[1]))
        return [(0xC4, b"".join(bodies))] if dht == "one" else [(0xC4, b) for b in bodies]

    if dqt_twice:
        head += dqt_segments(True)
    if dht_twice == "before":
        head += dht_segments(True)
    if dht_where == "before":
        head += dht_segments(False)
    if not dqt_twice:
        head += dqt_segments(False)
    cids = list(comp_ids or [1, 2, 3][:nc])
    samp = plan["sampling"] if nc == 3 else [(1, 1)]
    head.append((0xC0, struct.pack(">BHHB", 8, plan["height"], plan["width"], nc) +
                 b"".join(bytes([cids[c], (samp[c][0] << 4) | samp[c][1], dqt_ids[c]]) for c in range(nc))))
    if dqt_twice:
        head += dqt_segments(False)
    if dht_twice == "after":
        head += dht_segments(True)
    if dht_where == "after":
        head += dht_segments(False)
    head += [(0xDD, struct.pack(">H", v)) for v in dri]
    order = list(sos_order or range(nc))
    head.append((0xDA, bytes([nc]) + b"".join(bytes([cids[c], (select[c][0] << 4) | select[c][1]]) for c in order) + b"\x00\x3f\x00"))
    out = b"\xff\xd8"
    extra = list(extra)
    for m, body in head:
        for e in [e for e in extra if e[0] == m]:
            out += marker(e[1])[:-2] + _seg(e[1], e[2])
            extra.remove(e)
        out += marker(m)[:-2] + _seg(m, body)
    assert not extra, extra
    return out + scan + marker(EOI) + bytes(trailer)


def replace_dht(data, cls, tid, table):
    """``data`` with the first DHT segment that holds exactly the table (cls, tid) rewritten to hold ``table``"""
    p = 2
    while data[p + 1] != 0xDA:
        L = struct.unpack(">H", data[p + 2:p + 4])[0]
        if data[p + 1] == 0xC4 and data[p + 4] == ((cls << 4) | tid) and L == 2 + 17 + sum(data[p + 5:p + 21]):
            return data[:p] + _seg(0xC4, bytes([(cls << 4) | tid]) + bytes(table[0]) + bytes(table[1])) + data[p + 2 + L:]
        p += 2 + L
    raise ValueError("no such DHT segment")
