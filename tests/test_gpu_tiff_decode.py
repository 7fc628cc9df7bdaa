"""-m gpu: the device TIFF decoder (bbocr_tiff_decode, bbocr_op_tiff_decode_stage; csrc/tiffdec.hip) against tests/tiff_decode_ref.py byte
for byte -- the strips' stream, the stream behind the predictor, both planes -- and against ``reader.decode_file`` + upload; batches that
mix codecs and shapes; strided destinations between guard bytes; the status of damaged files beside good ones; and the callers with
``tiff_decode=True``.  (tools/tiffdec_hostcheck.py has run every file here through the same strip decoders under a sanitizer on the
host; a damaged file is an input the decoder answers with a status.)"""
import io

import numpy as np
import pytest
import torch

import tiff_decode_ref as R

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
ERR_ARG, ERR_DATA = -1, -7                                                # bbocr.h BBOCR_ERR_*


@pytest.fixture(scope="module")
def good():
    """[(name, file, the restatement's decode)]: Pillow's matrix, the hand-built files, the hand-written streams: computed once, shared,
    never changed"""
    return [(n, f, R.decode(f)) for n, f in R.matrix() + R.handbuilt() + R.handwritten_files()]


def pages_of(files):
    from bb_ocr_amd import reader as M

    return [M.TiffPage(f, M.tiff_plan(f)) for f in files]


def decode_guarded(reader, files, extra=(5, 3)):
    """ONE bbocr_tiff_decode call of files of any shapes into one device buffer: per file and plane GUARD bytes, H rows at a pitch larger
    than the row, GUARD bytes.  -> (status, the buffer, [(rgb offset, rgb pitch, gray offset, gray pitch, H, W)])"""
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


def test_stages_equal_the_restatement(reader, good):
    for name, f, d in good:
        s0, st = reader.tiff_decode_stage(f, 0)
        assert st == 0 and s0.tobytes() == d["stage0"], name
        s1, st = reader.tiff_decode_stage(f, 1)
        assert st == 0 and s1.tobytes() == d["stage1"], name
        (rgb, gray), st = reader.tiff_decode_stage(f, 2)
        assert st == 0 and np.array_equal(rgb, d["rgb"]) and np.array_equal(gray, d["gray"]), name


def test_stage_arguments(reader):
    import ctypes as C

    f = R.tiff_file(bytes(range(64)), 8, 8, compression=5, rows_per_strip=3)
    dst = torch.zeros(4 * 64, dtype=torch.uint8, device=reader.device)
    st = C.c_int()
    call = lambda data, stage, room: reader._lib.bbocr_op_tiff_decode_stage(reader._h, data, len(data), stage, C.c_void_p(dst.data_ptr()), room, C.byref(st))
    assert call(f, 2, 4 * 64) == 0 and call(f, 2, 4 * 64 - 1) == ERR_ARG and call(f, 3, 4 * 64) == ERR_ARG and call(f, 0, 63) == ERR_ARG
    assert call(f, 0, 64) == 0 and call(R.refusals()[-1][1], 0, 4 * 64) == ERR_ARG


def test_one_call_mixes_codecs_and_shapes_between_guards(reader, good):
    """the full call against decode_file: every good file -- four codecs, two predictors, five modes, both byte orders, four shapes and the
    hand-written streams' -- in ONE batch, into strided destinations whose guard bytes and row tails must stay untouched"""
    from bb_ocr_amd.reader import decode_file

    files = [f for _, f, _ in good]
    assert {R.plan(f)["compression"] for f in files} == {1, 5, 8, 32946, 32773} and len({R.plan(f)["width"] for f in files}) > 4
    status, buf, lay = decode_guarded(reader, files)
    assert status == [0] * len(files)                                     # no supported file is refused
    exp, _ = expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in good])
    assert np.array_equal(buf, exp)                                       # every plane exact, guards and the bytes behind every row untouched
    for name, f, d in good[::7]:                                          # (the restatement's planes ARE decode_file's: the CPU tests; a sample here)
        rgb, gray = decode_file(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
    status2, buf2, _ = decode_guarded(reader, files)
    assert status2 == status and np.array_equal(buf2, buf)                # two consecutive calls: identical bytes


def test_batch_and_device_entry_points(reader, good):
    groups = {}
    for name, f, d in good:
        groups.setdefault(d["rgb"].shape, []).append((name, f, d))
    for shape, group in groups.items():                                   # one uniform batch per shape, whatever the codecs in it
        (rgb, gray), status = reader.decode_tiff_batch(pages_of([f for _, f, _ in group]))
        assert status == [0] * len(group) and tuple(rgb.shape) == (len(group),) + shape, shape
        assert np.array_equal(rgb.cpu().numpy(), np.stack([d["rgb"] for _, _, d in group])), shape
        assert np.array_equal(gray.cpu().numpy(), np.stack([d["gray"] for _, _, d in group])), shape
    with pytest.raises(ValueError):
        reader.decode_tiff_batch(pages_of([good[0][1], good[1][1]]))
    sources = [f for _, f, _ in good] + [R.refusals()[-1][1], b"\xff\xd8\xff\xe0"]
    got = reader.decode_tiff_device(sources)
    assert got[-1] is None and got[-2] is None
    for k, (g, (_, _, d)) in enumerate(zip(got, good)):
        assert g is not None and np.array_equal(g[0].cpu().numpy(), d["rgb"]) and np.array_equal(g[1].cpu().numpy(), d["gray"]), k


def test_damaged_files_beside_good_ones(reader, good):
    bad = R.damaged()
    pick = good[2::9][:len(bad) + 1]
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
        assert reader.decode_tiff_device([f]) == [None], name
        assert reader.tiff_decode_stage(f, 0)[1] == ERR_DATA, name
    status, buf, lay = decode_guarded(reader, [f for _, f, _ in pick])    # the context serves a further call
    assert status == [0] * len(pick)
    assert np.array_equal(buf, expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in pick])[0])


def test_argument_errors_per_file(reader, good):
    f = good[5][1]
    page = pages_of([f])[0]
    H, W, _ = page.shape
    rgb = torch.full((H * W * 3 + 8,), FILL, dtype=torch.uint8, device=reader.device)
    gray = torch.full((H * W + 8,), FILL, dtype=torch.uint8, device=reader.device)
    refused = pages_of([f])[0]
    refused.data = R.refusals()[-1][1]
    short = reader._tiff_decode_into([page, page, refused, page], [rgb.data_ptr()] * 4, [3 * W - 1, 3 * W, 3 * W, 3 * W], [gray.data_ptr()] * 4, [W, W - 1, W, W])
    assert short == [ERR_ARG, ERR_ARG, ERR_ARG, 0]
    assert bool((rgb[H * W * 3:] == FILL).all()) and bool((gray[H * W:] == FILL).all())


def test_raw_strips_above_one_piece(reader):
    """an uncompressed strip is copied in pieces of 64 KB: strips of one piece, of exactly one (65536 bytes), of two with a short last
    one, and of three; a stored strip one byte short of its rows, and one that ends inside its first piece, are damage"""
    from bb_ocr_amd.reader import decode_file

    rgb = np.random.default_rng(1).integers(0, 256, (200, 200, 3), dtype=np.uint8)
    rgba = np.random.default_rng(2).integers(0, 256, (200, 200, 4), dtype=np.uint8)
    whole = np.random.default_rng(3).integers(0, 256, (128, 128, 4), dtype=np.uint8)      # 65536 bytes: exactly one piece
    files = [R.tiff_file(rgb.tobytes(), 200, 200, samples=3, photometric=2, rows_per_strip=r) for r in (None, 120, 109, 110)]
    files.append(R.tiff_file(rgba.tobytes(), 200, 200, samples=4, photometric=2, extra_samples=[2]))
    files.append(R.tiff_file(whole.tobytes(), 128, 128, samples=4, photometric=2, extra_samples=[0]))
    short = [R.tiff_file(None, 200, 200, samples=3, photometric=2, strips=[rgb.tobytes()[:-1]]),
             R.tiff_file(None, 200, 200, samples=3, photometric=2, strips=[rgb.tobytes()[:50000]])]
    status, buf, lay = decode_guarded(reader, files[:3] + short + files[3:])
    assert status == [0, 0, 0, ERR_DATA, ERR_DATA, 0, 0, 0]
    planes = [decode_file(f) for f in files]
    exp, mask = expected_buffer(buf.size, lay, planes[:3] + [None, None] + planes[3:])
    assert np.array_equal(buf[mask], exp[mask])
    assert np.array_equal(planes[0][0], rgb) and np.array_equal(planes[4][0], rgba[..., :3]) and np.array_equal(planes[5][0], whole[..., :3])


# ------------------------------------------------------------------------------------------------ the callers
def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[0], np.float64), np.asarray(y[0], np.float64)) and x[1] == y[1] and x[2] == y[2]
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """TIFF pages of all four codecs and JPEG pages of two shapes, a 16-bit TIFF (the plan refuses it) and a TIFF with a strip cut short
    -> (paths, kinds)"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("tiff_callers")
    shapes = {"A": dict(width=320, height=192, lines=3, margin=24), "B": dict(width=256, height=160, lines=2, margin=20)}
    spec = [("tiff_lzw", "A"), ("jpg", "A"), ("tiff_packbits_L", "B"), ("tiff_raw", "A"), ("16bit", "A"), ("tiff_1bit", "A"), ("jpg", "B"),
            ("tiff_tiff_adobe_deflate_L", "B"), ("cut", "A"), ("tiff_tiff_lzw_p2", "B"), ("jpg", "A"), ("tiff_tiff_adobe_deflate", "A")]
    paths = []
    for i, (kind, shape) in enumerate(spec):
        img = synth.page(40 + i, **shapes[shape])[0]
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "tiff"))
        H, W = img.shape[:2]
        if kind == "jpg":
            Image.fromarray(img).save(p, quality=92)
        elif kind == "16bit":
            Image.fromarray(img[..., 1].astype(np.uint16) * 257).save(p)
        elif kind == "cut":
            strips = [R.lzw_encode(img[r:r + 64].tobytes()) for r in range(0, H, 64)]
            strips[1] = strips[1][: len(strips[1]) // 2]
            p.write_bytes(R.tiff_file(None, W, H, samples=3, photometric=2, compression=5, rows_per_strip=64, strips=strips))
        elif kind == "tiff_1bit":
            Image.fromarray(img[..., 1] > 128).save(p, compression="tiff_lzw")
        elif kind == "tiff_tiff_lzw_p2":
            p.write_bytes(R.pillow_file(Image.fromarray(img), "tiff_lzw", 2, "few"))
        else:
            comp = {"tiff_lzw": "tiff_lzw", "tiff_packbits_L": "packbits", "tiff_raw": "raw", "tiff_tiff_adobe_deflate_L": "tiff_adobe_deflate",
                    "tiff_tiff_adobe_deflate": "tiff_adobe_deflate"}[kind]
            p.write_bytes(R.pillow_file(Image.fromarray(img[..., 1] if kind.endswith("_L") else img), comp, 1, "few"))
        paths.append(str(p))
    return paths, [k for k, _ in spec]


def test_callers_with_the_option_on(reader, directory, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import extractor_batch

    paths, kinds = directory
    assert reader.tiff_decode is False                                   # off unless asked for
    off = reader.readtext_files(paths, tiff_decode=False)
    # most pages hold text, so the comparisons below compare results (not all: the 16-bit page is white once Pillow has clipped it to
    # 8 bits, and the cut file is whatever the host path makes of it)
    assert sum(bool(r) for r in off) >= 8
    decoded = []
    real_batch, real_pages = reader.decode_tiff_batch, reader.decode_tiff_pages
    monkeypatch.setattr(reader, "decode_tiff_batch", lambda pages: (decoded.append(len(list(pages))), real_batch(pages))[1])
    monkeypatch.setattr(reader, "decode_tiff_pages", lambda pages: (decoded.append(len(list(pages))), real_pages(pages))[1])
    for mixed in (False, True):
        del decoded[:]
        on = reader.readtext_files(paths, tiff_decode=True, mixed=mixed)
        assert all(same_results(a, b) for a, b in zip(on, off)), mixed
        # the eight TIFF files the plan supports (the cut one among them) went through the device decoder: one call per shape group, or,
        # mixed, one call for all of them
        assert sorted(decoded) == ([8] if mixed else [3, 5]), decoded
        res = extractor_batch.read_files(reader, paths, tiff_decode=True, mixed=mixed, device_decode=True)
        assert all(same_results(res[i], off[i]) for i in range(len(paths)))
        texts = extractor_batch.extract_texts(reader, paths, tiff_decode=True, mixed=mixed)
        assert texts == extractor_batch.extract_texts(reader, paths, tiff_decode=False, mixed=mixed)
    del decoded[:]
    assert extractor_batch.read_files(reader, paths, mixed=False).keys() == set(range(len(paths))) and not decoded      # the Reader's default: off
    one = [reader.readtext(p) for p in paths[:6]]
    monkeypatch.setattr(reader, "tiff_decode", True)
    del decoded[:]
    for p, want in zip(paths[:6], one):
        assert same_results(reader.readtext(p), want), p                  # readtext(path) of a TIFF: the host path's result
        data = open(p, "rb").read()
        assert same_results(reader.readtext(data), reader.readtext(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))    # bytes: the array rule
    assert sum(decoded) == 2 * sum(k.startswith("tiff") for k in kinds[:6])


def test_readtext_of_a_tiff_equals_readtext_of_its_pixels(reader, directory, monkeypatch):
    from bb_ocr_amd.reader import decode_file

    paths, kinds = directory
    monkeypatch.setattr(reader, "tiff_decode", True)
    for p, kind in zip(paths, kinds):
        if kind in ("tiff_lzw", "tiff_raw", "tiff_tiff_adobe_deflate"):   # RGB pages: an array's gray plane is derived from its colours
            rgb, _ = decode_file(p)
            assert same_results(reader.readtext(open(p, "rb").read()), reader.readtext(rgb)), p
