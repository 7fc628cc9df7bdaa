"""Progressive JPEG files (SOF2) restated in numpy: the definition csrc/jpegprog.h's scan decoder and csrc/jpeg_parse.h's plan are held
to, itself held to the installed Pillow / libjpeg-turbo (test_jpeg_progressive_cpu.py).

``parse`` walks the markers of a whole file -- frame, tables as they stand at every SOS, restart interval in force, the segments of every
scan -- and checks the scan script by T.81 G.1.1 and for completeness; ``decode_coefficients`` runs the scans in file order into one
coefficient array ``int32 [blocks][64]`` (natural order, blocks in MCU order: jpeg_chroma_ref's layout), each scan kind as jdphuff.c
carries it out; the samples come from jpeg_chroma_ref's IDCT and upsampling.  A non-interleaved scan walks its component's own block
raster, ``ceil(ceil(W * h / hmax) / 8)`` blocks a row, which is narrower than the MCU raster of the array whenever the picture does not
fill its last MCU; its restart interval counts those blocks.

``write`` is the other direction, for scripts Pillow never writes: quantised coefficients + a script -> a progressive file coded with
near-flat Huffman tables (jcphuff.c's symbols, end-of-band runs and buffered correction bits)."""
from __future__ import annotations

import struct

import numpy as np

import jpeg_chroma_ref as K
import jpeg_entropy_ref as J

ZZ = J.ZIGZAG
MAX_SCANS = 64
(OK, NOT_JPEG, TRUNCATED, NO_EOI, SOF, PRECISION, COMPONENTS, SAMPLING, COLORSPACE, MULTISCAN, TABLES, RESTART, SCRIPT, SCANS) = range(14)


# ------------------------------------------------------------------------------------------------ the plan
def comp_raster(plan, c):
    """(blocks a row, block rows, blocks across an MCU, blocks down an MCU) of component c's own raster"""
    nc = plan["components"]
    hmax, vmax = plan["sampling"][0] if nc == 3 else (1, 1)
    h, v = plan["sampling"][c] if nc == 3 else (1, 1)
    return -(-(-(-plan["width"] * h // hmax)) // 8), -(-(-(-plan["height"] * v // vmax)) // 8), h, v


def scan_units(plan, scan):
    if len(scan["comps"]) > 1:
        return plan["mcu_cols"] * plan["mcu_rows"]
    bw, bh, _, _ = comp_raster(plan, scan["comps"][0])
    return bw * bh


def _segments(data, start):
    """([(first, end)] of the restart segments of the entropy-coded data at ``start``, offset of the marker that ends it) or a reason;
    a segment ends at the first FF of the run of fill bytes its marker closes"""
    q, a, n, segs = start, start, len(data), []

    def first_ff(q):
        while q > a and data[q - 1] == 0xFF:
            q -= 1
        return q

    while q < n:
        q = data.find(b"\xFF", q)
        if q < 0 or q + 1 >= n:
            break
        b = data[q + 1]
        if b == 0:
            q += 2
        elif b == 0xFF:
            q += 1
        elif 0xD0 <= b <= 0xD7:
            if b - 0xD0 != len(segs) % 8:
                return RESTART
            segs.append((a, first_ff(q)))
            q += 2
            a = q
        else:
            segs.append((a, first_ff(q)))
            return segs, q
    return NO_EOI


def _walk(data, plan):
    n = len(data)
    if n < 4 or data[:2] != b"\xFF\xD8":
        return NOT_JPEG
    p = 2
    qt, huff = {}, {}
    sof = jfif = False
    adobe, dri = -1, 0
    ids, tq = [], []
    bits = None
    scans = plan["scans"]
    while True:
        while True:
            if p + 2 > n or data[p] != 0xFF:
                return NO_EOI if scans else TRUNCATED
            if data[p + 1] == 0xFF:
                p += 1
                continue
            break
        m = data[p + 1]
        p += 2
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            break
        if p + 2 > n:
            return TRUNCATED
        L = (data[p] << 8) | data[p + 1]
        if L < 2 or p + L > n:
            return TRUNCATED
        s = data[p + 2:p + L]
        if m == 0xC2:
            if sof or len(s) < 6:
                return SOF
            if s[0] != 8:
                return PRECISION
            H, W, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if H == 0 or W == 0 or len(s) < 6 + 3 * nc:
                return SOF
            ids = [s[6 + 3 * i] for i in range(nc)]
            tq = [s[8 + 3 * i] for i in range(nc)]
            plan.update(width=W, height=H, components=nc, sampling=[(s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15) for i in range(min(nc, 3))])
            sof = True
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8):
            return SOF
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    return TABLES
                tc, th = s[q] >> 4, s[q] & 15
                counts = list(s[q + 1:q + 17])
                if tc > 1 or th > 3 or sum(counts) > 256 or q + 17 + sum(counts) > len(s):
                    return TABLES
                huff[(tc, th)] = (counts, list(s[q + 17:q + 17 + sum(counts)]))
                q += 17 + sum(counts)
        elif m == 0xDB:
            if scans:
                return MULTISCAN
            q = 0
            while q < len(s):
                if s[q] >> 4:
                    return PRECISION
                if (s[q] & 15) > 3 or q + 65 > len(s):
                    return TABLES
                t = [0] * 64
                for k in range(64):
                    t[ZZ[k]] = s[q + 1 + k]
                qt[s[q] & 15] = t
                q += 65
        elif m == 0xDD:
            if len(s) < 2:
                return TRUNCATED
            dri = (s[0] << 8) | s[1]
        elif m == 0xE0 and s[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and len(s) >= 12 and s[:5] == b"Adobe":
            adobe = s[11]
        elif m == 0xDA:
            if not sof:
                return SOF
            nc = plan["components"]
            if not scans:
                if nc not in (1, 3):
                    return COMPONENTS
                if nc == 3:
                    if not jfif and adobe != 1:
                        return COLORSPACE
                    samp = plan["sampling"]
                    if samp == [(2, 2), (1, 1), (1, 1)]:
                        plan["chroma"] = 0
                    else:
                        plan["chroma"] = next((c for c, hv in K.LUMA.items() if samp == [hv, (1, 1), (1, 1)]), 0)
                        if not plan["chroma"]:
                            return SAMPLING
                if any(t > 3 or t not in qt for t in tq):
                    return TABLES
                plan["quant"] = [qt[t] for t in tq]
                h, v = plan["sampling"][0] if nc == 3 else (1, 1)
                plan["mcu_cols"], plan["mcu_rows"] = -(-plan["width"] // (8 * h)), -(-plan["height"] // (8 * v))
                bits = [[-1] * 64 for _ in range(nc)]
            if len(scans) == MAX_SCANS:
                return SCANS
            ns = s[0] if len(s) >= 1 else 0
            if ns < 1 or ns > 3 or ns > nc or len(s) < 1 + 2 * ns + 3:
                return MULTISCAN
            comps, dct, act = [], [], []
            for i in range(ns):
                if s[1 + 2 * i] not in ids:
                    return MULTISCAN
                c = ids.index(s[1 + 2 * i])
                if comps and c <= comps[-1]:
                    return MULTISCAN
                comps.append(c)
                dct.append(s[2 + 2 * i] >> 4)
                act.append(s[2 + 2 * i] & 15)
            ss, se, ah, al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15
            if (se != 0) if ss == 0 else (ns != 1 or se < ss or se > 63):
                return SCRIPT
            if ah > 13 or al > 13:
                return SCRIPT
            tabs = []
            for i, c in enumerate(comps):
                if ss > 0 and bits[c][0] < 0:
                    return SCRIPT
                for k in range(ss, se + 1):
                    if (ah != 0) if bits[c][k] < 0 else (ah != bits[c][k] or al != ah - 1):
                        return SCRIPT
                    bits[c][k] = al
                if not (ss == 0 and ah > 0):
                    key = (0, dct[i]) if ss == 0 else (1, act[i])
                    if key[1] > 3 or key not in huff or not J.table_ok(*huff[key], dc=ss == 0):
                        return TABLES
                    tabs.append(huff[key])
            scan = dict(comps=comps, dc_table=dct, ac_table=act, ss=ss, se=se, ah=ah, al=al, restart_interval=dri, offset=p + L, huff=tabs)
            units = scan_units(plan, scan)
            ri = dri or units
            got = _segments(data, p + L)
            if isinstance(got, int):
                return got
            segs, end = got
            if len(segs) != -(-units // ri):
                return RESTART
            scan.update(segments=segs, bytes=end - (p + L))
            scans.append(scan)
            p = end
            continue
        p += L
    if not scans:
        return TRUNCATED
    if any(b != 0 for row in bits for b in row):
        return SCRIPT
    return OK


def parse(data: bytes) -> dict:
    """The plan of a file: ``supported`` / ``reason``, the frame (width, height, components, sampling, mcu_cols, mcu_rows, chroma, quant)
    and ``scans``, each ``dict(comps, dc_table, ac_table, ss, se, ah, al, restart_interval, offset, bytes, segments [(first, end)], huff
    [(counts, values) per scan component])`` -- those read before the refusal when the file is refused"""
    plan = dict(width=0, height=0, components=0, sampling=[], mcu_cols=0, mcu_rows=0, chroma=0, scans=[])
    reason = _walk(bytes(data), plan)
    plan.update(supported=reason == OK, reason=reason)
    return plan


# ------------------------------------------------------------------------------------------------ entropy decoding
class Bits:
    """The bits of one restart segment without stuffing; past the end: ones"""

    def __init__(self, raw: bytes):
        raw = raw.replace(b"\xFF\x00", b"\xFF")
        self.n = len(raw) * 8
        self.v = int.from_bytes(raw + b"\xFF" * 8, "big")
        self.total = self.n + 64
        self.p = 0

    def peek16(self):
        if self.p + 16 > self.total:
            raise ValueError("the segment ends before its blocks")
        return (self.v >> (self.total - self.p - 16)) & 0xFFFF

    def get(self, n):
        v = self.peek16() >> (16 - n)
        self.p += n
        return v


def _decoder(spec):
    """{(length, code): symbol} of a table given as (counts, values)"""
    counts, vals = spec
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def _symbol(dec, st: Bits):
    v = st.peek16()
    for l in range(1, 17):
        s = dec.get((l, v >> (16 - l)))
        if s is not None:
            st.p += l
            return s
    raise ValueError("a bit pattern without a code")


def _extend(bits, n):
    return bits if bits >= (1 << (n - 1)) else bits - (1 << n) + 1


def block_of(plan, scan, u, ci=0, j=0):
    """The array's block of unit u of a scan (block j of scan component ci of MCU u when it interleaves)"""
    nc = plan["components"]
    h, v = plan["sampling"][0] if nc == 3 else (1, 1)
    bpm = h * v + 2 if nc == 3 else 1
    c = scan["comps"][ci]
    off = 0 if nc == 1 or c == 0 else h * v + c - 1
    if len(scan["comps"]) > 1:
        return u * bpm + off + j
    bw, _, ch, cv = comp_raster(plan, c)
    by, bx = divmod(u, bw)
    return ((by // cv) * plan["mcu_cols"] + bx // ch) * bpm + off + (by % cv) * ch + bx % ch


def decode_scan(data: bytes, plan: dict, k: int, coef: np.ndarray, stats: dict = None):
    """Scan k of the file into ``coef`` (in place).  ``stats["eobrun"]``: the longest end-of-band run met, in blocks."""
    scan = plan["scans"][k]
    ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
    nc = plan["components"]
    h, v = plan["sampling"][0] if nc == 3 else (1, 1)
    units = scan_units(plan, scan)
    ri = scan["restart_interval"] or units
    decs = [_decoder(t) for t in scan["huff"]]
    p1 = 1 << al
    for g, (a, b) in enumerate(scan["segments"]):
        st = Bits(data[a:b])
        pred = [0, 0, 0]
        eobrun = 0
        for u in range(g * ri, min((g + 1) * ri, units)):
            if ss == 0:
                for ci, c in enumerate(scan["comps"]):
                    nb = h * v if len(scan["comps"]) > 1 and c == 0 and nc == 3 else 1
                    for j in range(nb):
                        blk = block_of(plan, scan, u, ci, j)
                        if ah == 0:
                            sz = _symbol(decs[ci], st)
                            if sz > 15:
                                raise ValueError("a DC category above 15")
                            if sz:
                                pred[ci] += _extend(st.get(sz), sz)
                            coef[blk, 0] = pred[ci] << al
                        elif st.get(1):
                            coef[blk, 0] |= p1
                continue
            row = coef[block_of(plan, scan, u)]
            kk = ss
            if ah == 0:
                if eobrun > 0:
                    eobrun -= 1
                    continue
                while kk <= se:
                    sym = _symbol(decs[0], st)
                    r, sz = sym >> 4, sym & 15
                    if sz:
                        kk += r
                        val = _extend(st.get(sz), sz)
                        if kk > 63:
                            raise ValueError("a coefficient behind the block")
                        row[ZZ[kk]] = val << al
                    elif r == 15:
                        kk += 15
                    else:
                        eobrun = (1 << r) - 1 + (st.get(r) if r else 0)
                        if stats is not None:
                            stats["eobrun"] = max(stats.get("eobrun", 0), eobrun + 1)
                        break
                    kk += 1
                continue

            def correct(z):
                if st.get(1) and (row[z] & p1) == 0:
                    row[z] += p1 if row[z] >= 0 else -p1

            if eobrun == 0:
                while kk <= se:
                    sym = _symbol(decs[0], st)
                    r, sz = sym >> 4, sym & 15
                    val = 0
                    if sz:
                        if sz != 1:
                            raise ValueError("a refinement symbol of size %d" % sz)
                        val = p1 if st.get(1) else -p1
                    elif r != 15:
                        eobrun = (1 << r) + (st.get(r) if r else 0)
                        if stats is not None:
                            stats["eobrun"] = max(stats.get("eobrun", 0), eobrun)
                        break
                    while kk <= se:
                        if row[ZZ[kk]] != 0:
                            correct(ZZ[kk])
                        else:
                            r -= 1
                            if r < 0:
                                break
                        kk += 1
                    if val:
                        if kk > se:
                            raise ValueError("a coefficient behind the band")
                        row[ZZ[kk]] = val
                    kk += 1
            if eobrun > 0:
                while kk <= se:
                    if row[ZZ[kk]] != 0:
                        correct(ZZ[kk])
                    kk += 1
                eobrun -= 1
        if eobrun != 0 or st.p > st.n or st.n - st.p >= 8:
            raise ValueError("segment %d of scan %d does not end with its blocks" % (g, k))


def n_blocks(plan):
    nc = plan["components"]
    h, v = plan["sampling"][0] if nc == 3 else (1, 1)
    return plan["mcu_cols"] * plan["mcu_rows"] * (h * v + 2 if nc == 3 else 1)


def decode_coefficients(data: bytes, plan: dict, n_scans: int = 0, stats: dict = None, each=None) -> np.ndarray:
    """int32 [blocks][64] after the first ``n_scans`` scans (0: all).  ``each(k, coef)`` is called behind every scan."""
    coef = np.zeros((n_blocks(plan), 64), np.int32)
    for k in range(n_scans or len(plan["scans"])):
        decode_scan(data, plan, k, coef, stats)
        if each:
            each(k, coef)
    return coef


def decode_pixels(data: bytes, plan: dict = None) -> np.ndarray:
    """uint8 [H,W,3] YCbCr triples (colour files) or [H,W] samples (grey files): what libjpeg hands Pillow"""
    plan = plan or parse(data)
    return K.planes_to_pixels(K.component_planes(decode_coefficients(data, plan), plan), plan)


# ------------------------------------------------------------------------------------------------ the scan writer
FLAT_DC = ([0, 0, 0, 0, 16] + [0] * 11, list(range(16)))                           # sixteen 5-bit codes
FLAT_AC = ([0] * 7 + [255, 1] + [0] * 7, list(range(256)))                         # 255 codes of 8 bits, one of 9: no code of ones only


def _codes(spec):
    counts, vals = spec
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


class _Out:
    def __init__(self):
        self.acc = self.n = 0
        self.out = bytearray()

    def put(self, code, length):
        if not length:
            return
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _nbits(v):
    return int(abs(int(v))).bit_length()


def _write_scan(coef, plan, scan, ri):
    """The entropy-coded bytes of one scan (stuffed, restart markers between its segments): jcphuff.c"""
    ss, se, ah, al = scan["ss"], scan["se"], scan["ah"], scan["al"]
    nc = plan["components"]
    h, v = plan["sampling"][0] if nc == 3 else (1, 1)
    dc, ac = _codes(FLAT_DC), _codes(FLAT_AC)
    units = scan_units(plan, scan)
    ri = ri or units
    o = _Out()
    st = dict(eobrun=0, be=[])

    def emit_eobrun():
        if st["eobrun"]:
            nb = st["eobrun"].bit_length() - 1
            o.put(*ac[nb << 4])
            o.put(st["eobrun"], nb)
            st["eobrun"] = 0
        for b in st["be"]:
            o.put(b, 1)
        st["be"] = []

    for g in range(-(-units // ri)):
        pred = [0, 0, 0]
        for u in range(g * ri, min((g + 1) * ri, units)):
            if ss == 0:
                for ci, c in enumerate(scan["comps"]):
                    nb = h * v if len(scan["comps"]) > 1 and c == 0 and nc == 3 else 1
                    for j in range(nb):
                        x = int(coef[block_of(plan, scan, u, ci, j), 0])
                        if ah:
                            o.put((x >> al) & 1, 1)
                            continue
                        t = x >> al
                        d = t - pred[ci]
                        pred[ci] = t
                        n = _nbits(d)
                        o.put(*dc[n])
                        o.put(d if d >= 0 else d - 1, n)
                continue
            row = [int(coef[block_of(plan, scan, u), ZZ[k]]) for k in range(64)]
            if ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    t = abs(row[k]) >> al
                    if t == 0:
                        r += 1
                        continue
                    emit_eobrun()
                    while r > 15:
                        o.put(*ac[0xF0])
                        r -= 16
                    n = _nbits(t)
                    o.put(*ac[(r << 4) + n])
                    o.put(t if row[k] >= 0 else ~t, n)
                    r = 0
                if r:
                    st["eobrun"] += 1
                    if st["eobrun"] == 0x7FFF:
                        emit_eobrun()
                continue
            absv = [abs(x) >> al for x in row]
            eob = max([k for k in range(ss, se + 1) if absv[k] == 1], default=0)
            r, br = 0, []
            for k in range(ss, se + 1):
                t = absv[k]
                if t == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    o.put(*ac[0xF0])
                    r -= 16
                    for b in br:
                        o.put(b, 1)
                    br = []
                if t > 1:
                    br.append(t & 1)
                    continue
                emit_eobrun()
                o.put(*ac[(r << 4) + 1])
                o.put(0 if row[k] < 0 else 1, 1)
                for b in br:
                    o.put(b, 1)
                br = []
                r = 0
            if r or br:
                st["eobrun"] += 1
                st["be"] += br
                if st["eobrun"] == 0x7FFF or len(st["be"]) > 937:
                    emit_eobrun()
        emit_eobrun()
        o.flush()
        if (g + 1) * ri < units:
            o.out += bytes([0xFF, 0xD0 + g % 8])
    return bytes(o.out)


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def write(coef: np.ndarray, plan: dict, script, restart=None, head: bytes = b"") -> bytes:
    """A progressive file of the frame ``plan`` (width, height, components, sampling, quant, mcu_cols, mcu_rows) whose coefficients are
    ``coef`` (int [blocks][64], natural order, MCU block order), coded scan by scan as ``script`` says: ``[(components, Ss, Se, Ah, Al)]``.
    ``restart``: None, one interval for every scan, or one per scan (a DRI sits in front of each scan whose interval differs from the one
    in force).  ``head``: marker segments placed behind JFIF (an EXIF block)."""
    nc = plan["components"]
    out = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00") + head
    for c in range(nc):
        out += _segment(0xDB, bytes([c]) + bytes(int(plan["quant"][c][z]) for z in ZZ))
    samp = plan["sampling"] if nc == 3 else [(1, 1)]
    out += _segment(0xC2, struct.pack(">BHHB", 8, plan["height"], plan["width"], nc) +
                    b"".join(bytes([c + 1, (samp[c][0] << 4) | samp[c][1], c]) for c in range(nc)))
    out += _segment(0xC4, bytes([0x00]) + bytes(FLAT_DC[0]) + bytes(FLAT_DC[1]))
    out += _segment(0xC4, bytes([0x10]) + bytes(FLAT_AC[0]) + bytes(FLAT_AC[1]))
    in_force = 0
    for i, (comps, ss, se, ah, al) in enumerate(script):
        ri = (restart[i] if isinstance(restart, (list, tuple)) else restart) or 0
        if ri != in_force:
            out += _segment(0xDD, struct.pack(">H", ri))
            in_force = ri
        scan = dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al)
        out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, 0x00]) for c in comps) + bytes([ss, se, (ah << 4) | al]))
        out += _write_scan(coef, plan, scan, ri)
    return out + b"\xFF\xD9"
