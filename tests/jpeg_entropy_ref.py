"""Restatement of the entropy half of a baseline JPEG decoder (ITU T.81 Annex F.2.2 / libjpeg's jdmarker.c + jdhuff.c), in plain Python.

Three parts, each the yardstick of one layer of csrc/jpegdec.*:
  * ``parse``      the marker parser: what ``bbocr_host_jpeg_plan`` must report (geometry, sampling, restart interval, scan range,
                   ``supported`` + reason); a Huffman table the scan names and libjpeg refuses (``table_ok``) is TABLES, and fill bytes
                   in front of RSTn or the closing marker belong to no restart segment;
  * ``decode_coefficients``  the sequential Huffman decoder: quantised coefficients per block in natural order (DC terms absolute), and
                   the exact state at the first symbol boundary at or after every ``S``-bit subsequence start;
  * ``device_model``  the passes of the device decoder on the same bits: speculative decode of every subsequence from the assumed state,
                   synchronisation to a fixed point (inside groups of ``group`` lanes, then across them), exclusive scan of the block
                   counts, write pass -- and the status word the write pass raises (``ERR_*``).
``decode_pixels`` completes the coefficients to samples with tests/jpeg_ref.py (ISLOW IDCT, range limit, fancy upsampling).
"""
from __future__ import annotations

import numpy as np

import jpeg_ref

# reason codes of bbocr_jpeg_plan::reason (include/bbocr.h)
OK, NOT_JPEG, TRUNCATED, NO_EOI, SOF, PRECISION, COMPONENTS, SAMPLING, COLORSPACE, MULTISCAN, TABLES, RESTART = range(12)

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


def _parse(data: bytes) -> dict:
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Refused(NOT_JPEG)
    p = 2
    qt, huff = {}, {}
    sof = None
    dri = 0
    jfif = False
    adobe = None
    while True:
        while True:                                            # next marker: any number of FF fill bytes
            if p + 2 > n:
                raise Refused(TRUNCATED)
            if data[p] != 0xFF:
                raise Refused(TRUNCATED)
            if data[p + 1] == 0xFF:
                p += 1
                continue
            break
        m = data[p + 1]
        p += 2
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            raise Refused(TRUNCATED)                           # EOI before any scan
        if p + 2 > n:
            raise Refused(TRUNCATED)
        L = (data[p] << 8) | data[p + 1]
        if L < 2 or p + L > n:
            raise Refused(TRUNCATED)
        s = data[p + 2:p + L]
        if m == 0xC0:
            if sof is not None or len(s) < 6:
                raise Refused(SOF)
            if s[0] != 8:
                raise Refused(PRECISION)
            H, W, nc = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            if H == 0 or W == 0 or len(s) < 6 + 3 * nc:
                raise Refused(SOF)
            sof = dict(height=H, width=W, comps=[(s[6 + 3 * i], s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15, s[8 + 3 * i]) for i in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Refused(SOF)                                 # extended, progressive, lossless, arithmetic
        elif m == 0xCC:
            raise Refused(SOF)
        elif m == 0xC4:
            q = 0
            while q < len(s):
                if q + 17 > len(s):
                    raise Refused(TABLES)
                tc, th = s[q] >> 4, s[q] & 15
                counts = list(s[q + 1:q + 17])
                tot = sum(counts)
                if tc > 1 or th > 1 or tot > 256 or q + 17 + tot > len(s):
                    raise Refused(TABLES)
                huff[(tc, th)] = (counts, list(s[q + 17:q + 17 + tot]))
                q += 17 + tot
        elif m == 0xDB:
            q = 0
            while q < len(s):
                if s[q] >> 4:
                    raise Refused(PRECISION)                   # 16-bit table
                if (s[q] & 15) > 3 or q + 65 > len(s):
                    raise Refused(TABLES)
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = s[q + 1 + k]
                qt[s[q] & 15] = t
                q += 65
        elif m == 0xDD:
            if len(s) < 2:
                raise Refused(TRUNCATED)
            dri = (s[0] << 8) | s[1]
        elif m == 0xE0 and s[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and s[:5] == b"Adobe" and len(s) >= 12:
            adobe = s[11]
        elif m == 0xDA:
            if sof is None:
                raise Refused(SOF)
            nc = len(sof["comps"])
            if nc not in (1, 3):
                raise Refused(COMPONENTS)
            if nc == 3:
                if not jfif and adobe != 1:
                    raise Refused(COLORSPACE)
                if [(c[1], c[2]) for c in sof["comps"]] != [(2, 2), (1, 1), (1, 1)]:
                    raise Refused(SAMPLING)
            if len(s) < 1 or s[0] != nc or len(s) < 1 + 2 * nc + 3:
                raise Refused(MULTISCAN)
            tabs = []
            for i in range(nc):
                cid, t = s[1 + 2 * i], s[2 + 2 * i]
                if cid != sof["comps"][i][0]:
                    raise Refused(MULTISCAN)
                td, ta = t >> 4, t & 15
                if (0, td) not in huff or (1, ta) not in huff or sof["comps"][i][3] not in qt:
                    raise Refused(TABLES)
                if not table_ok(*huff[(0, td)], dc=True) or not table_ok(*huff[(1, ta)]):
                    raise Refused(TABLES)                      # jdhuff.c::jpeg_make_d_derived_tbl: JERR_BAD_HUFF_TABLE
                tabs.append((td, ta))
            scan_off = p + L
            break
        p += L
    # the entropy-coded segment: byte ranges between restart markers
    nc = len(sof["comps"])
    mcu = 16 if nc == 3 else 8
    mcux, mcuy = -(-sof["width"] // mcu), -(-sof["height"] // mcu)
    nmcu = mcux * mcuy
    segs = []
    q = start = scan_off
    end = None

    def first_ff(q):
        """a marker's FF at q: the first FF of the run of fill bytes (T.81 B.1.1.2) it closes; the segment ends there"""
        while q > start and data[q - 1] == 0xFF:
            q -= 1
        return q

    while q < n:
        q = data.find(b"\xff", q)
        if q < 0 or q + 1 >= n:
            break
        b = data[q + 1]
        if b == 0x00:
            q += 2
        elif b == 0xFF:
            q += 1
        elif 0xD0 <= b <= 0xD7:
            if b - 0xD0 != len(segs) % 8:
                raise Refused(RESTART)
            segs.append((start, first_ff(q)))
            q += 2
            start = q
        else:
            segs.append((start, first_ff(q)))
            end = q
            break
    if end is None:
        raise Refused(NO_EOI)
    if data[end + 1] != 0xD9:
        raise Refused(MULTISCAN)
    ri = dri if dri else nmcu
    if len(segs) != -(-nmcu // ri):
        raise Refused(RESTART)
    return dict(width=sof["width"], height=sof["height"], components=nc, sampling=[(c[1], c[2]) for c in sof["comps"]],
                restart_interval=dri, mcu_cols=mcux, mcu_rows=mcuy, segments=segs, scan_offset=scan_off, scan_bytes=end - scan_off,
                quant=[qt[c[3]] for c in sof["comps"]], huff=huff, tables=tabs, supported=True, reason=OK)


def table_ok(counts, vals, dc=False):
    """jdhuff.c::jpeg_make_d_derived_tbl's two checks: behind the codes of every length the next code still has that length (no code
    is all ones, none lies beyond), and a DC table names no category above 15"""
    code = 0
    for l in range(1, 17):
        code += counts[l - 1]
        if code >= (1 << l):
            return False
        code <<= 1
    return not dc or all(v <= 15 for v in vals)


def parse(data: bytes) -> dict:
    """The plan of a file; ``supported`` False + ``reason`` for everything outside the decoder's scope."""
    try:
        return _parse(bytes(data))
    except Refused as r:
        return dict(supported=False, reason=r.reason)


# ------------------------------------------------------------------------------------------------ Huffman decoding
_LOOKUPS = {}


def _lookup16(counts, vals):
    """For every 16-bit look-ahead: (code lengths, symbols) as lists; length 0 = no code (Annex C code assignment)."""
    key = (tuple(counts), tuple(vals))
    if key not in _LOOKUPS:
        _LOOKUPS[key] = tuple(a.tolist() for a in _lookup16_arrays(counts, vals))
    return _LOOKUPS[key]


def _lookup16_arrays(counts, vals):
    ln = np.zeros(65536, np.int32)
    sy = np.zeros(65536, np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            if code >= (1 << l):
                return ln, sy                                  # over-subscribed table: the rest has no code
            lo = code << (16 - l)
            ln[lo:lo + (1 << (16 - l))] = l
            sy[lo:lo + (1 << (16 - l))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return ln, sy


class Stream:
    """The unstuffed bytes of all restart segments, one after the other; reads past a segment's end return 1-bits."""

    def __init__(self, data: bytes, plan: dict):
        parts = [data[a:b].replace(b"\xff\x00", b"\xff") for a, b in plan["segments"]]
        self.seg_byte = np.cumsum([0] + [len(x) for x in parts]).tolist()
        self.bytes = b"".join(parts)
        nc = plan["components"]
        self.bpm = 6 if nc == 3 else 1
        self.comp = [0, 0, 0, 0, 1, 2] if nc == 3 else [0]
        self.dc = [_lookup16(*plan["huff"][(0, plan["tables"][c][0])]) for c in range(nc)]
        self.ac = [_lookup16(*plan["huff"][(1, plan["tables"][c][1])]) for c in range(nc)]
        self.seg_bytes = [self.bytes[a:b] + b"\xff" * 8 for a, b in zip(self.seg_byte[:-1], self.seg_byte[1:])]
        nmcu = plan["mcu_cols"] * plan["mcu_rows"]
        self.ri = plan["restart_interval"] or nmcu
        self.nmcu = nmcu

    def seg_blocks(self, s):
        return min(self.ri, self.nmcu - s * self.ri) * self.bpm


def _run(st: Stream, s: int, state, end, max_blocks, out=None, first_block=0):
    """Decode segment ``s`` from ``state`` = (bit, block in MCU, zig-zag position) while bit < end and fewer than ``max_blocks`` blocks
    are complete.  Bits are segment-relative.  -> (state, blocks completed, ok); ``ok`` False: a look-ahead without a code was met
    (the decode stops there with bit = end).  ``out`` [blocks][64]: coefficients are stored (DC terms as differences)."""
    B = st.seg_bytes[s]                                         # followed by one-bits: a read past the end sees those
    last = len(B) - 4
    frm = int.from_bytes
    p, b, z = state
    n = 0
    while p < end and n < max_blocks:
        c = st.comp[b]
        ln, sy = (st.dc if z == 0 else st.ac)[c]
        k = min(p >> 3, last)
        v = (frm(B[k:k + 4], "big") >> (16 - (p & 7))) & 0xFFFF if k < last else 0xFFFF
        l = ln[v]
        if l == 0:
            return (end, b, z), n, False
        sym = sy[v]
        p += l
        if z == 0:
            sz = sym & 15
            r = 0
        else:
            r, sz = sym >> 4, sym & 15
            if sz == 0:
                z = z + 16 if r == 15 else 64
                if z > 63:
                    z, b, n = 0, (b + 1) % st.bpm, n + 1
                continue
            z += r
        if sz:
            k = min(p >> 3, last)
            bits = (frm(B[k:k + 4], "big") >> (32 - (p & 7) - sz)) & ((1 << sz) - 1) if k < last else (1 << sz) - 1
            p += sz
            val = bits if bits >= (1 << (sz - 1)) else bits - (1 << sz) + 1
        else:
            val = 0
        if out is not None and z <= 63:
            out[first_block + n][ZIGZAG[z]] = val
        z += 1
        if z > 63:
            z, b, n = 0, (b + 1) % st.bpm, n + 1
    return (p, b, z), n, True


def subsequences(st: Stream, S: int):
    """[(segment, first bit, end bit)] (segment-relative bits) of every subsequence, segment after segment"""
    subs = []
    for s in range(len(st.seg_byte) - 1):
        nbits = (st.seg_byte[s + 1] - st.seg_byte[s]) * 8
        for a in range(0, max(nbits, 1), S):
            subs.append((s, a, min(a + S, nbits)))
    return subs


def decode_coefficients(data: bytes, plan: dict, S: int = 1024):
    """Sequential decode.  -> (coef int32 [blocks][64] natural order, DC absolute; entry states int64 [subsequences][4] =
    (bit in the unstuffed stream, block in MCU, zig-zag position, first output block))"""
    st = Stream(data, plan)
    nblocks = st.nmcu * st.bpm
    coef = np.zeros((nblocks, 64), np.int32)
    entries = []
    blk0 = 0
    for s in range(len(st.seg_byte) - 1):
        nbits = (st.seg_byte[s + 1] - st.seg_byte[s]) * 8
        want = st.seg_blocks(s)
        state, done = (0, 0, 0), 0
        for a in range(0, max(nbits, 1), S):
            entries.append((st.seg_byte[s] * 8 + state[0], state[1], state[2], blk0 + done))
            state, n, ok = _run(st, s, state, min(a + S, nbits), want - done, coef, blk0 + done)
            done += n
        if done != want:
            raise ValueError("segment %d holds %d blocks, expected %d" % (s, done, want))
        blk0 += want
    _dc_sums(coef, st)
    return coef, np.array(entries, np.int64)


def _dc_sums(coef, st: Stream):
    """DC differences -> DC terms: per component and restart segment, the running sum"""
    nblocks = coef.shape[0]
    comp = np.array(st.comp)[np.arange(nblocks) % st.bpm]
    seg = (np.arange(nblocks) // st.bpm) // st.ri
    for c in set(st.comp):
        for s in range(len(st.seg_byte) - 1):
            m = (comp == c) & (seg == s)
            coef[m, 0] = np.cumsum(coef[m, 0])


ERR_SYNC, ERR_CODE, ERR_COUNT = 1, 2, 4                          # kernels.h JD_ERR_*: the bits of the write pass's status word


def device_model(data: bytes, plan: dict, S: int = 1024, group: int = 64, status: bool = False, stream: Stream = None):
    """The device's passes.  -> (coef, entry states) as ``decode_coefficients`` returns them, and the number of cross-group passes;
    ``status``: and the status word of the write pass, by jpeg_spec.h::jpeg_write_pass's three rules on the model's own counts and
    states.  ``stream``: the file's Stream when it is not this module's (another MCU layout)."""
    st = stream or Stream(data, plan)
    subs = subsequences(st, S)
    n = len(subs)
    first = [i == 0 or subs[i - 1][0] != subs[i][0] for i in range(n)]
    big = 1 << 60
    # 1. speculative decode from the assumed state (block 0 of the MCU, coefficient 0)
    entry = [(a, 0, 0) for (_, a, _) in subs]
    res = [_run(st, s, e, end, big) for (s, _, end), e in zip(subs, entry)]
    exits, counts = [r[0] for r in res], [r[1] for r in res]

    def relax(lo, hi, bound):
        """lanes lo..hi-1 take their left neighbour's exit state until nothing changes (at most ``bound`` rounds)"""
        any_change = False
        base = max(lo, 1) - 1
        for _ in range(bound):
            prev = exits[base:hi]                                  # the round reads the exit states of the round before
            changed = False
            for i in range(base + 1, hi):
                if not first[i] and prev[i - 1 - base] != entry[i]:
                    entry[i] = prev[i - 1 - base]
                    exits[i], counts[i], _ok = _run(st, subs[i][0], entry[i], subs[i][2], big)
                    changed = True
            if not changed:
                break
            any_change = True
        return any_change

    # 2. inside every group (the group's first lane keeps its assumed state), then across groups until a pass changes nothing
    groups = [(g, min(g + group, n)) for g in range(0, n, group)]
    for lo, hi in groups:
        relax(lo + 1, hi, group)
    passes = 0
    for _ in range(len(groups) + 1):
        passes += 1
        snapshot = list(exits)
        changed = False
        for lo, hi in groups:
            if lo > 0 and not first[lo] and snapshot[lo - 1] != entry[lo]:
                entry[lo] = snapshot[lo - 1]
                exits[lo], counts[lo], _ok = _run(st, subs[lo][0], entry[lo], subs[lo][2], big)
                changed = True
            changed |= relax(lo + 1, hi, group)
        if not changed:
            break
    # 3. exclusive scan of the block counts, per segment
    first_block, run = [], 0
    for i in range(n):
        if first[i]:
            run = subs[i][0] * st.ri * st.bpm
        first_block.append(run)
        run += counts[i]
    # 4. write pass, and what it checks: the neighbour's exit state is the entry state (SYNC), every look-ahead has a code (CODE), the
    # blocks written are the blocks counted, and a segment's last subsequence ends on the segment's last block, at a block's start (COUNT)
    nblocks = st.nmcu * st.bpm
    coef = np.zeros((nblocks, 64), np.int32)
    word = 0
    for i, (s, _, end) in enumerate(subs):
        seg_end = s * st.ri * st.bpm + st.seg_blocks(s)
        room = max(seg_end - first_block[i], 0)
        state, wrote, ok = _run(st, s, entry[i], end, room, coef, first_block[i])
        if not first[i] and exits[i - 1] != entry[i]:
            word |= ERR_SYNC
        if not ok:
            word |= ERR_CODE
        if wrote != counts[i]:
            word |= ERR_COUNT
        if (i + 1 == n or first[i + 1]) and (first_block[i] + wrote != seg_end or state[1:] != (0, 0)):
            word |= ERR_COUNT
    _dc_sums(coef, st)
    states = np.array([(st.seg_byte[subs[i][0]] * 8 + entry[i][0], entry[i][1], entry[i][2], first_block[i]) for i in range(n)], np.int64)
    return (coef, states, passes, word) if status else (coef, states, passes)


# ------------------------------------------------------------------------------------------------ coefficients -> samples
def component_planes(coef: np.ndarray, plan: dict):
    """Dequantise + ISLOW IDCT: the component planes before upsampling, cropped to the component's size"""
    nc = plan["components"]
    mx, my = plan["mcu_cols"], plan["mcu_rows"]
    H, W = plan["height"], plan["width"]
    c = coef.astype(np.int64).reshape(my, mx, 6 if nc == 3 else 1, 8, 8)

    def idct(blocks, q):                                        # [by, bx, 8, 8]
        d = blocks * np.array(q, np.int64).reshape(8, 8)
        r = jpeg_ref._idct_1d(d, 2, True)
        r = jpeg_ref.range_limit(jpeg_ref._idct_1d(r, 3, False))
        return r.transpose(0, 2, 1, 3).reshape(r.shape[0] * 8, r.shape[1] * 8)

    if nc == 1:
        return [idct(c[:, :, 0], plan["quant"][0])[:H, :W]]
    y = c[:, :, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * 2, mx * 2, 8, 8)
    ch, cw = -(-H // 2), -(-W // 2)
    return [idct(y, plan["quant"][0])[:H, :W], idct(c[:, :, 4], plan["quant"][1])[:ch, :cw], idct(c[:, :, 5], plan["quant"][2])[:ch, :cw]]


def decode_pixels(data: bytes, plan: dict = None) -> np.ndarray:
    """uint8 [H,W,3] YCbCr triples (colour files) or [H,W] samples (grey files): what libjpeg hands Pillow"""
    plan = plan or parse(data)
    coef, _ = decode_coefficients(data, plan)
    return planes_to_pixels(component_planes(coef, plan), plan)


def planes_to_pixels(planes, plan):
    H, W = plan["height"], plan["width"]
    if plan["components"] == 1:
        return planes[0].astype(np.uint8)
    return np.stack([planes[0], jpeg_ref.upsample(planes[1], H, W), jpeg_ref.upsample(planes[2], H, W)], axis=2).astype(np.uint8)
