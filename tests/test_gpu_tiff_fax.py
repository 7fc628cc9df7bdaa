"""-m gpu: the CCITT codec of the device TIFF decoder (bbocr_tiff_decode_fax, bbocr_op_tiff_fax_decode_stage; csrc/tiff_fax.h under
csrc/tiffdec.hip's wave policy) against tests/tiff_fax_ref.py byte for byte -- the strips' stream and both planes -- and against
``reader.decode_file``; one call that mixes CCITT files with raw, LZW and Deflate files of other shapes, into strided destinations between
guard bytes; the damage list beside good files; the plain entry points' refusal; and the callers with ``tiff_decode="fax"``.
(tools/tiff_fax_hostcheck.py has run every file here through the same decoder under a sanitizer on the host; a damaged file is an input
the decoder answers with a status.)"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import tiff_decode_ref as R
import tiff_fax_ref as F

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
ERR_ARG, ERR_DATA = -1, -7                                                # bbocr.h BBOCR_ERR_*


@pytest.fixture(scope="module")
def good():
    """[(name, file, the restatement's decode)]: the designed pages in their variants, the hand-built files, the hand-written streams:
    computed once, shared, never changed"""
    return [(n, f, F.decode(f)) for n, f in F.designed_files() + F.handbuilt() + F.handwritten_files()]


def host_decode(f):
    from bb_ocr_amd.reader import decode_file

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return decode_file(f)


def pages_of(files):
    from bb_ocr_amd import reader as M

    pages = [M.tiff_page(f, fax=True) for f in files]
    assert all(p is not None for p in pages)
    return pages


def decode_guarded(reader, files, extra=(5, 3)):
    """ONE decode call of files of any shapes into one device buffer: per file and plane GUARD bytes, H rows at a pitch larger than the
    row, GUARD bytes.  -> (status, the buffer, [(rgb offset, rgb pitch, gray offset, gray pitch, H, W)])"""
    pages = pages_of(files)
    lay, at = [], 0
    for p in pages:
        H, W, _ = p.shape
        pr, pg = 3 * W + extra[0], W + extra[1]
        lay.append((at + GUARD, pr, at + 2 * GUARD + H * pr, pg, H, W))
        at += 3 * GUARD + H * (pr + pg)
    buf = torch.full((at,), FILL, dtype=torch.uint8, device=reader.device)
    base = buf.data_ptr()
    status = reader._tiff_decode_into(pages, [base + l[0] for l in lay], [l[1] for l in lay], [base + l[2] for l in lay], [l[3] for l in lay])
    return status, buf.cpu().numpy(), lay


def expected_buffer(size, lay, planes):
    """the buffer decode_guarded must leave: FILL everywhere but in the rows' pixels; planes[k] None: that file's region is not compared"""
    want = np.full(size, FILL, np.uint8)
    mask = np.ones(size, bool)
    for (o_rgb, pr, o_gray, pg, H, W), pl in zip(lay, planes):
        rows = np.arange(H)[:, None]
        i_rgb, i_gray = (o_rgb + rows * pr + np.arange(3 * W)[None]).ravel(), (o_gray + rows * pg + np.arange(W)[None]).ravel()
        if pl is None:
            mask[i_rgb] = mask[i_gray] = False
        else:
            want[i_rgb], want[i_gray] = pl[0].ravel(), pl[1].ravel()
    return want, mask


def test_the_pages_hold_what_the_names_say(good):
    plans = [(d["plan"], d["fax"]) for _, _, d in good]
    assert {fx["scheme"] for _, fx in plans} == {2, 3, 4} and {fx["fill_order"] for _, fx in plans} == {1, 2}
    assert {pl["photometric"] for pl, _ in plans} == {0, 1} and {fx["t4_options"] for _, fx in plans if fx["scheme"] == 3} == {0, 1, 4, 5}
    assert {1, 7, 8, 9, 63, 64, 65, 1728, 2561} <= {pl["width"] for pl, _ in plans} and max(pl["width"] for pl, _ in plans) > 5120
    assert {1, 2, 3} <= {pl["strips"] for pl, _ in plans}
    for colour in (0, 1):                                                  # every terminating length and every make-up multiple, both colours
        codes = []
        for name, f, d in good:
            if name.startswith("every_length-c2"):
                pl, fx, strips = F.fax_walk(f)
                for o, c in strips:
                    F.decode_strip(f[o:o + c], pl["width"], pl["height"], 2, codes=codes)
        assert {r for c, r in codes if c == colour} == set(range(64)) | {64 * k for k in range(1, 41)}
    modes = []                                                             # every mode of the 2-D coding
    for name, f, d in good:
        if name.startswith("modes-c4") and d["plan"]["strips"] == 1:
            pl, fx, strips = F.fax_walk(f)
            F.decode_strip(f[strips[0][0]:sum(strips[0])], pl["width"], pl["height"], 4, codes=modes)
    assert set(F.MODES) <= set(m for m in modes if isinstance(m, str))


def test_stages_equal_the_restatement_and_decode_file(reader, good):
    for name, f, d in good:
        s0, st = reader.tiff_fax_decode_stage(f, 0)
        assert st == 0 and s0.tobytes() == d["stage0"], name
        (rgb, gray), st = reader.tiff_fax_decode_stage(f, 2)
        assert st == 0 and np.array_equal(rgb, d["rgb"]) and np.array_equal(gray, d["gray"]), name
        h_rgb, h_gray = host_decode(f)
        assert np.array_equal(rgb, h_rgb) and np.array_equal(gray, h_gray), name


def test_one_call_mixes_fax_and_plain_files_between_guards(reader, good):
    plain = [(n, f, R.decode(f)) for n, f in R.matrix()[5::9] if R.plan(f)["compression"] in (1, 5, 8)]
    assert {d["plan"]["compression"] for _, _, d in plain} == {1, 5, 8}
    mix = []
    for k, item in enumerate(good):                                       # a plain file after every twentieth fax file
        mix.append(item)
        if k % 20 == 0 and k // 20 < len(plain):
            mix.append(plain[k // 20])
    files = [f for _, f, _ in mix]
    status, buf, lay = decode_guarded(reader, files)
    assert status == [0] * len(files)
    exp, _ = expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in mix])
    assert np.array_equal(buf, exp)                                       # every plane exact, guards and the bytes behind every row untouched
    status2, buf2, _ = decode_guarded(reader, files)
    assert status2 == status and np.array_equal(buf2, buf)                # two consecutive calls: identical bytes


def test_damaged_files_beside_good_ones(reader, good):
    bad = F.damaged()
    pick = good[3::7][:len(bad) + 1]
    assert len(pick) == len(bad) + 1
    files, planes, is_bad = [], [], []
    for k, (_, f, d) in enumerate(pick):                                  # good, bad, good, bad, ... good
        files.append(f)
        planes.append((d["rgb"], d["gray"]))
        is_bad.append(False)
        if k < len(bad):
            files.append(bad[k][1])
            planes.append(None)
            is_bad.append(True)
    status, buf, lay = decode_guarded(reader, files)
    assert [s != 0 for s in status] == is_bad and all(s in (0, ERR_DATA) for s in status), list(zip(status, is_bad))
    exp, mask = expected_buffer(buf.size, lay, planes)
    assert np.array_equal(buf[mask], exp[mask])                           # the good files exact; no byte outside any destination's rows
    for name, f in bad:                                                   # ... and each alone, through the entry points of the callers
        assert reader.decode_tiff_device([f], fax=True) == [None], name
        assert reader.tiff_fax_decode_stage(f, 0)[1] == ERR_DATA, name
    status, buf, lay = decode_guarded(reader, [f for _, f, _ in pick])    # the context serves a further call
    assert status == [0] * len(pick)
    assert np.array_equal(buf, expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in pick])[0])


def test_the_plain_entry_points_keep_refusing(reader, good):
    f = good[0][1]
    page = pages_of([f])[0]
    H, W, _ = page.shape
    rgb = torch.full((H * W * 3,), FILL, dtype=torch.uint8, device=reader.device)
    gray = torch.full((H * W,), FILL, dtype=torch.uint8, device=reader.device)
    page.fax = False                                                      # (so that _tiff_decode_into takes bbocr_tiff_decode)
    assert reader._tiff_decode_into([page], [rgb.data_ptr()], [3 * W], [gray.data_ptr()], [W]) == [ERR_ARG]
    assert bool((rgb == FILL).all()) and bool((gray == FILL).all())
    st = C.c_int()
    dst = torch.zeros(4 * H * W + 64, dtype=torch.uint8, device=reader.device)
    plain = reader._lib.bbocr_op_tiff_decode_stage(reader._h, f, len(f), 0, C.c_void_p(dst.data_ptr()), dst.numel(), C.byref(st))
    fax = reader._lib.bbocr_op_tiff_fax_decode_stage(reader._h, f, len(f), 0, C.c_void_p(dst.data_ptr()), dst.numel(), C.byref(st))
    assert plain == ERR_ARG and fax == 0 and st.value == 0
    assert reader.decode_tiff_device([f], fax=False) == [None] and reader.decode_tiff_device([f], fax=True)[0] is not None
    for name, file, _, _ in F.fax_refusals():                             # what the fax plan refuses, the fax entry point refuses
        assert reader._lib.bbocr_op_tiff_fax_decode_stage(reader._h, file, len(file), 0, C.c_void_p(dst.data_ptr()), dst.numel(), C.byref(st)) == ERR_ARG, name


# ------------------------------------------------------------------------------------------------ the callers
def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[0], np.float64), np.asarray(y[0], np.float64)) and x[1] == y[1] and x[2] == y[2]
                                    for x, y in zip(a, b))


def test_callers_with_the_fax_level(reader, tmp_path, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import extractor_batch, synth

    paths = []
    for i, comp in enumerate(("group4", "group3", "tiff_lzw")):
        img = synth.page(60 + i, width=320, height=192, lines=3, margin=24)[0]
        p = tmp_path / ("p%d.tiff" % i)
        Image.fromarray(img[..., 1] > 128).save(p, compression=comp)
        paths.append(str(p))
    pixels = [host_decode(p) for p in paths]
    assert [F.fax_plan(open(p, "rb").read())[1]["scheme"] for p in paths] == [4, 3, 0]
    decoded = []
    real_batch, real_pages = reader.decode_tiff_batch, reader.decode_tiff_pages
    monkeypatch.setattr(reader, "decode_tiff_batch", lambda pages: (decoded.append(len(list(pages))), real_batch(pages))[1])
    monkeypatch.setattr(reader, "decode_tiff_pages", lambda pages: (decoded.append(len(list(pages))), real_pages(pages))[1])
    off = reader.readtext_files(paths, tiff_decode=False)            # (a 1-bit page may hold no box for this detector: the pixels are compared below)
    assert len(off) == 3 and not decoded
    for mixed in (False, True):
        del decoded[:]
        on = reader.readtext_files(paths, tiff_decode="fax", mixed=mixed)
        assert all(same_results(a, b) for a, b in zip(on, off)) and decoded == [3], (mixed, decoded)
        del decoded[:]
        plain = reader.readtext_files(paths, tiff_decode=True, mixed=mixed)                  # True: the LZW file alone goes to the card
        assert all(same_results(a, b) for a, b in zip(plain, off)) and decoded == [1], (mixed, decoded)
        res = extractor_batch.read_files(reader, paths, tiff_decode="fax", mixed=mixed)
        assert all(same_results(res[i], off[i]) for i in range(3))
        assert extractor_batch.extract_texts(reader, paths, tiff_decode="fax", mixed=mixed) == extractor_batch.extract_texts(reader, paths, tiff_decode=False, mixed=mixed)
    # readtext of a Group 4 file (path and bytes) with the option on = the same call on its pixels
    one = reader.readtext(paths[0])
    del decoded[:]
    monkeypatch.setattr(reader, "tiff_decode", "fax")
    data = open(paths[0], "rb").read()
    assert same_results(reader.readtext(paths[0]), one)
    assert same_results(reader.readtext(data), reader.readtext(np.ascontiguousarray(pixels[0][0])))
    assert sum(decoded) == 2
    for got, want in zip(reader.decode_tiff_device(paths), pixels):      # what the callers above were given: decode_file's planes
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
