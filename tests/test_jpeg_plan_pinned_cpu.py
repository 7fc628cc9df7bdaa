"""The two JPEG plan functions pinned on a small corpus, no GPU: ``bbocr_host_jpeg_plan`` and ``bbocr_host_jpeg_progressive_plan`` must
answer every case below exactly as the library did when tests/golden/jpeg_plans/recording.json was made -- return code, ``reason`` and a
SHA-256 of the plan structure's bytes.  The recording was made by the commit BEFORE the two marker walks were given their shared pieces
(csrc/jpeg_parse.h), so it holds what the walks did while they were two, refusals and their order included.

The corpus is eight stored files (tests/golden/jpeg_plans/*.jpg: Pillow's version plays no part) and, derived here from each of them,
every truncation inside the headers, every marker before the first scan turned into another, and a few rearranged copies.

    python tests/test_jpeg_plan_pinned_cpu.py --record     # writes recording.json with the library BBOCR_LIB_PATH names (or the tree's)
    python tests/test_jpeg_plan_pinned_cpu.py --corpus     # writes the eight files again (needs Pillow; their bytes depend on its version)
"""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "golden", "jpeg_plans")
RECORDING = os.path.join(DIR, "recording.json")
FILES = ["grey", "c420", "c444_restart", "c422_optimised", "exif6", "prog420", "prog_grey", "prog_restart"]
CODES = [0xC0, 0xC1, 0xC2, 0xC4, 0xDA, 0xDB, 0xD9, 0xE0]
# a DHT segment's payload for table class 0, id `th`: jpeg_progressive_ref.FLAT_DC's counts and values
FLAT_DC = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12)))


def segment(code, payload):
    return bytes([0xFF, code]) + (len(payload) + 2).to_bytes(2, "big") + payload


def markers(data):
    """[(offset of the FF, code, offset behind the segment)] of the markers up to and including the first SOS"""
    out, p = [(0, 0xD8, 2)], 2
    while True:
        assert data[p] == 0xFF and data[p + 1] not in (0x00, 0xFF), p
        end = p + 2 + int.from_bytes(data[p + 2:p + 4], "big")
        out.append((p, data[p + 1], end))
        if data[p + 1] == 0xDA:
            return out
        p = end


def scan_end(data, p):
    """offset of the FF of the marker that ends the entropy-coded data starting at p"""
    while not (data[p] == 0xFF and data[p + 1] not in (0x00, 0xFF) and not 0xD0 <= data[p + 1] <= 0xD7):
        p += 1
    return p


def cases(data):
    """[(name, bytes)] of one corpus file, in a fixed order"""
    ms = markers(data)
    sos_at, sos_end = ms[-1][0], ms[-1][2]
    out = [("whole", data)]
    out += [("cut %d" % n, data[:n]) for n in range(1, sos_end + 1)]
    for at, code, _ in ms:                                                 # the SOS itself included
        out += [("marker %d %02X to %02X" % (at, code, c), data[:at + 1] + bytes([c]) + data[at + 2:]) for c in CODES if c != code]
    for th in (2, 4):                                                      # a third id (the progressive walk takes it) and a fifth (neither does)
        out.append(("DHT id %d" % th, data[:sos_at] + segment(0xC4, bytes([th]) + FLAT_DC[0] + FLAT_DC[1]) + data[sos_at:]))
    dqt = b"".join(data[a:e] for a, c, e in ms if c == 0xDB)
    without = b"".join(data[a:e] for a, c, e in ms if c != 0xDB)
    assert dqt and len(without) + len(dqt) == sos_end
    end = scan_end(data, sos_end)
    out.append(("DQT moved behind the first scan", without + data[sos_end:end] + dqt + data[end:]))
    out.append(("DQT again behind the first scan", data[:end] + dqt + data[end:]))
    assert data[-2:] == b"\xFF\xD9"
    out.append(("EOI removed", data[:-2]))
    return out


def load_corpus():
    return [(name, open(os.path.join(DIR, name + ".jpg"), "rb").read()) for name in FILES]


def answers(lib, data):
    """[[return code, reason, SHA-256 of the plan's bytes]] of the baseline and the progressive plan function"""
    from bb_ocr_amd import _lib

    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    out = []
    for fn, T in ((lib.bbocr_host_jpeg_plan, _lib.bbocr_jpeg_plan), (lib.bbocr_host_jpeg_progressive_plan, _lib.bbocr_jpeg_progressive_plan)):
        plan = T()
        C.memset(C.byref(plan), 0xA5, C.sizeof(plan))                      # a byte the function leaves alone shows in the hash
        rc = fn(buf, len(data), C.byref(plan))
        out.append([rc, plan.reason, hashlib.sha256(bytes(plan)).hexdigest()])
    return out


def record(lib):
    """{"answers": the distinct answers, "files": {file: {"cases": names, "plan": indices, "progressive": indices}}}"""
    table, files = {}, {}
    for name, data in load_corpus():
        cs = cases(data)
        rows = [answers(lib, d) for _, d in cs]
        idx = [[table.setdefault(tuple(r[k]), len(table)) for r in rows] for k in (0, 1)]
        files[name] = {"cases": [n for n, _ in cs], "plan": idx[0], "progressive": idx[1]}
    return {"answers": [list(a) for a in table], "files": files}


@pytest.fixture(scope="module")
def lib():
    from bb_ocr_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def recording():
    with open(RECORDING) as f:
        return json.load(f)


def test_the_corpus_is_what_it_says():
    corpus = dict(load_corpus())
    assert all(len(d) < 2048 for d in corpus.values())
    sof = {n: next(c for _, c, _ in markers(d) if 0xC0 <= c <= 0xC2) for n, d in corpus.items()}
    assert [sof[n] for n in FILES] == [0xC0] * 5 + [0xC2] * 3
    dri = {n for n, d in corpus.items() if any(c == 0xDD for _, c, _ in markers(d))}
    assert dri == {"c444_restart", "prog_restart"}
    assert any(c == 0xE1 for _, c, _ in markers(corpus["exif6"]))
    total = sum(len(cases(d)) for d in corpus.values())
    assert total > 3000


@pytest.mark.parametrize("name", FILES)
def test_both_plans_answer_as_recorded(lib, recording, name):
    data = dict(load_corpus())[name]
    rec = recording["files"][name]
    cs = cases(data)
    assert [n for n, _ in cs] == rec["cases"]                              # the derivation is the recording's
    for k, (case, d) in enumerate(cs):
        got = answers(lib, d)
        want = [recording["answers"][rec["plan"][k]], recording["answers"][rec["progressive"][k]]]
        assert got == want, (name, case)


def test_the_recording_holds_every_reason_the_walks_differ_in(recording):
    """the corpus reaches the refusals the two walks do not share: a plan pinned on accepted files alone would pin little"""
    reasons = [{recording["answers"][i][1] for f in recording["files"].values() for i in f[k]} for k in ("plan", "progressive")]
    # BBOCR_JPEG_*: OK 0, NOT_JPEG 1, TRUNCATED 2, NO_EOI 3, SOF 4, SAMPLING 7 (a file of a chroma class), MULTISCAN 9, TABLES 10
    assert {0, 1, 2, 3, 4, 7, 9, 10} <= reasons[0], reasons[0]
    assert {0, 1, 2, 3, 4, 9, 10} <= reasons[1], reasons[1]
    assert all(a[0] == 0 for a in recording["answers"])


def make_corpus():
    import io

    import numpy as np
    from PIL import Image

    def picture(w, h, mode, seed):
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 5 + y * 3) % 256, (x * 2 + 90) % 256, (y * 7 + 30) % 256], -1) + rng.integers(0, 24, (h, w, 3))
        img = Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))
        return img if mode == "RGB" else img.convert("L")

    def save(img, **kw):
        buf = io.BytesIO()
        img.save(buf, "JPEG", **kw)
        return buf.getvalue()

    tiff = b"MM\x00\x2A\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01\x00\x06\x00\x00\x00\x00\x00\x00"
    files = {
        "grey": save(picture(24, 16, "L", 1), quality=40),
        "c420": save(picture(48, 32, "RGB", 2), quality=30, subsampling=2),
        "c444_restart": save(picture(32, 16, "RGB", 3), quality=30, subsampling=0, restart_marker_blocks=3),
        "c422_optimised": save(picture(40, 24, "RGB", 4), quality=30, subsampling=1, optimize=True),
        "exif6": save(picture(32, 24, "RGB", 5), quality=30, subsampling=2, exif=b"Exif\x00\x00" + tiff),
        "prog420": save(picture(32, 32, "RGB", 6), quality=30, subsampling=2, progressive=True),
        "prog_grey": save(picture(16, 16, "L", 7), quality=40, progressive=True),
        "prog_restart": save(picture(32, 16, "RGB", 8), quality=30, subsampling=0, progressive=True, restart_marker_blocks=2),
    }
    os.makedirs(DIR, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(DIR, name + ".jpg"), "wb") as f:
            f.write(data)
        print(name, len(data), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if "--corpus" in sys.argv:
        make_corpus()
    if "--record" in sys.argv:
        from bb_ocr_amd import _lib

        rec = record(_lib.load())
        with open(RECORDING, "w") as f:
            json.dump(rec, f, separators=(",", ":"))
        print(sum(len(v["cases"]) for v in rec["files"].values()), "cases,", len(rec["answers"]), "distinct answers ->", RECORDING)
