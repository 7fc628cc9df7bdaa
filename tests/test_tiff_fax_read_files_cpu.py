"""The ``tiff_decode`` levels of ``extractor_batch.read_files`` without a card: with ``"fax"`` the CCITT files of a directory become ``"tiff"``
pages beside the LZW / Deflate ones and share their decode calls; with ``True`` they keep the host decode as before and every call is
what it was; the level reaches the pages from the keyword, from the Reader and with ``mixed``.  Pinned with the recording double of
test_tiff_read_files_cpu.py (CPU tensors stand for device memory, Pillow for the card; ``tiff_fax_plan`` needs the built library)."""
import numpy as np
import pytest

import tiff_fax_ref as F
from test_read_files_cpu import KW, FakeDeviceReader, FakeReader
from test_tiff_read_files_cpu import TiffDouble, calls_of

A, B = (48, 64), (30, 40)
# 4 + 2 CCITT files (A: 4, B: 2), 3 plain TIFF files (A: 2, B: 1), a CCITT file the fax plan refuses (uncompressed-mode bit), a JPEG
SPEC = [("group4", A)] * 3 + [("group3", A), ("tiff_ccitt", B), ("group4", B), ("tiff_lzw", A), ("tiff_adobe_deflate", A), ("tiff_lzw", B),
        ("refused", A), ("jpg", A)]
MAX_BATCH = 4


class FaxDouble(TiffDouble):
    """... that notes which pages of a decode call are CCITT pages"""

    def _planes(self, pages):
        self._note("fax_pages", (sum(bool(p.fax) for p in pages), len(pages)))
        return super()._planes(pages)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("tiff_fax_read_files")
    rng = np.random.default_rng(9)
    paths = []
    for i, (kind, (h, w)) in enumerate(SPEC):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "tiff"))
        if kind == "jpg":
            Image.fromarray(a).save(p)
        elif kind == "refused":
            p.write_bytes(F.fax_file((a[..., 0] > 200).astype(np.uint8), 3, 2))
        elif kind.startswith("tiff_") and kind != "tiff_ccitt":
            Image.fromarray(a if i % 2 else a[..., 0]).save(p, compression=kind)
        else:
            Image.fromarray(a[..., 0] > 200).save(p, compression=kind)
        paths.append(p)
    plans = [F.fax_plan(open(p, "rb").read()) for p in paths]
    assert [pl["supported"] for pl, _ in plans] == [1] * 9 + [0, 0] and [fx["scheme"] for _, fx in plans] == [4, 4, 4, 3, 2, 4, 0, 0, 0, 3, 0]
    ref = FakeReader()
    return paths, {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}


def same_calls(a, b):
    """the same calls, in whatever order the decode threads made them"""
    return sorted(map(repr, a.calls)) == sorted(map(repr, b.calls))


def run(reader, paths, **kw):
    from bb_ocr_amd import extractor_batch

    return extractor_batch.read_files(reader, paths, None, MAX_BATCH, 4, **kw, **KW)


def test_fax_level_sends_ccitt_files_to_the_decode_calls(files):
    paths, want = files
    r = FaxDouble()
    assert run(r, paths, tiff_decode="fax") == want
    # groups of one shape, closed at MAX_BATCH pages: A 4 + 2, B 3 -- CCITT and plain pages side by side
    assert calls_of(r, "decode_tiff_batch") == [(2, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    assert calls_of(r, "fax_pages") == [(0, 2), (2, 3), (4, 4)]
    # (the two single pages: the CCITT file the fax plan refuses, uploaded as host pixels, and the JPEG file)
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (2, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    assert not calls_of(r, "readtext_arrays")
    lvl = FaxDouble()
    lvl.tiff_decode = "fax"                                                # the Reader's level, no keyword
    assert run(lvl, paths) == want and same_calls(lvl, r)


def test_true_routes_as_before(files):
    paths, want = files
    on = FaxDouble()                                                       # tiff_decode = True: the Reader's
    assert run(on, paths) == want
    assert calls_of(on, "decode_tiff_batch") == [(1, 30, 40, 3), (2, 48, 64, 3)] and calls_of(on, "fax_pages") == [(0, 1), (0, 2)]
    kw = FaxDouble()
    assert run(kw, paths, tiff_decode=True) == want and same_calls(kw, on)
    one = FaxDouble()
    assert run(one, paths, tiff_decode="1") == want and same_calls(one, on)      # any other string: the plain level
    off = FaxDouble()
    assert run(off, paths, tiff_decode=False) == want and not calls_of(off, "decode_tiff_batch")
    plain = FakeDeviceReader()                                             # a Reader without the attribute: today's path
    assert run(plain, paths) == want
    assert same_calls(plain, off)


def test_status_and_retry_of_a_ccitt_page(files):
    paths, want = files
    r = FaxDouble(bad_files={open(paths[1], "rb").read(), open(paths[4], "rb").read()})
    assert run(r, paths, tiff_decode="fax") == want
    assert calls_of(r, "decode_tiff_batch") == [(2, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    # the two pages of non-zero status are not read from the batch: each takes the host decode of its bytes, alone
    assert calls_of(r, "readtext_arrays") == [(1, 30, 40, 3), (1, 48, 64, 3)]
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (2, 30, 40, 3), (2, 48, 64, 3), (3, 48, 64, 3)]


def test_mixed_batches_decode_every_page_in_one_call(files, monkeypatch):
    paths, want = files
    monkeypatch.setattr(FaxDouble, "readtext_pages", lambda self, pages, **kw: (self._note("readtext_pages", (len(pages),), kw), self.texts_of(pages))[1],
                        raising=False)
    monkeypatch.setattr(FaxDouble, "texts_of", lambda self, pages: [self.texts(p[0][None].numpy(), p[1][None].numpy())[0] for p in pages], raising=False)
    from bb_ocr_amd import extractor_batch

    r = FaxDouble()
    assert extractor_batch.read_files(r, paths, None, 64, 4, mixed=True, tiff_decode="fax", **KW) == want
    assert calls_of(r, "decode_tiff_pages") == [(9,)] and calls_of(r, "fax_pages") == [(6, 9)] and not calls_of(r, "decode_tiff_batch")
    t = FaxDouble()
    assert extractor_batch.read_files(t, paths, None, 64, 4, mixed=True, tiff_decode=True, **KW) == want
    assert calls_of(t, "decode_tiff_pages") == [(3,)] and calls_of(t, "fax_pages") == [(0, 3)]


def test_ocr_input_and_extract_texts_pass_the_level(files):
    from bb_ocr_amd import extractor_batch as E

    paths, _ = files
    g4, lzw, refused = str(paths[0]), str(paths[6]), str(paths[9])
    assert E._tiff_page(g4) is None and E._tiff_page(g4, True) is None and E._tiff_page(g4, "fax")[1].fax
    assert E._tiff_page(lzw, "fax")[1].fax is False and E._tiff_page(lzw)[0] == "tiff" and E._tiff_page(refused, "fax") is None
    assert E._tiff_level(FaxDouble(), None) is True and E._tiff_level(FaxDouble(), "fax") == "fax" and E._tiff_level(FaxDouble(), False) is False
    assert E._tiff_level(FakeDeviceReader(), None) is False and E._tiff_level(FakeDeviceReader(), "FAX") == "fax"
    assert E._plain_input_device(g4, 0, False, False, "fax")[0] == "tiff" and E._plain_input_device(g4, 0, False, False, True)[0] != "tiff"
