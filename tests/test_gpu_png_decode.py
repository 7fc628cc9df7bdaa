"""-m gpu: the device PNG decoder (bbocr_png_decode, bbocr_op_png_decode_stage; csrc/pngdec.hip) against tests/png_decode_ref.py byte for
byte -- the inflated stream, the unfiltered scanlines, both planes -- and against ``reader.decode_file`` + upload; the status of damaged
files beside good ones; the round trip through the device PNG writer; and the callers with ``png_decode=True``."""
import glob
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_decode_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_images", "*.png")))
GUARD, FILL = 64, 0xEE
ERR_ARG, ERR_DATA = -1, -7                                                # bbocr.h BBOCR_ERR_*


@pytest.fixture(scope="module")
def matrix():
    """[(name, file, the restatement's decode)] at the GPU tests' widths and heights: computed once, shared, never changed"""
    return [(n, f, R.decode(f)) for n, f in R.matrix(R.GPU_WIDTHS, R.GPU_HEIGHTS)]


@pytest.fixture(scope="module")
def text_pages():
    """one 1280 x 960 synthetic text page as RGB, L and 1-bit files -> [(name, file)]"""
    from PIL import Image

    from bb_ocr_amd import synth

    img = synth.page(21, width=1280, height=960, lines=14, margin=32)[0]
    out = []
    for name, pil in (("rgb", Image.fromarray(img)), ("L", Image.fromarray(img[..., 1])), ("1bit", Image.fromarray(img[..., 1] > 128))):
        b = io.BytesIO()
        pil.save(b, "PNG")
        out.append(("page_" + name, b.getvalue()))
    assert [R.plan(f)["bit_depth"] for _, f in out] == [8, 8, 1]
    return out


def pages_of(files):
    from bb_ocr_amd import reader as M

    return [M.PngPage(f, M.png_plan(f)) for f in files]


def decode_guarded(reader, files, extra=(5, 3)):
    """ONE bbocr_png_decode call of files of any shapes into one device buffer: per file and plane GUARD bytes, H rows at a pitch larger
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
    status = reader._png_decode_into(pages, [base + l[0] for l in lay], [l[1] for l in lay], [base + l[2] for l in lay], [l[3] for l in lay])
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


def test_stages_equal_the_restatement(reader, matrix):
    for name, f, d in matrix:
        s0, st = reader.png_decode_stage(f, 0)
        assert st == 0 and s0.tobytes() == d["stage0"], name
        s1, st = reader.png_decode_stage(f, 1)
        assert st == 0 and np.array_equal(s1.reshape(d["stage1"].shape), d["stage1"]), name
        (rgb, gray), st = reader.png_decode_stage(f, 2)
        assert st == 0 and np.array_equal(rgb, d["rgb"]) and np.array_equal(gray, d["gray"]), name


def test_stage_0_of_the_handwritten_streams(reader):
    for name, z, data in R.handwritten():
        s0, st = reader.png_decode_stage(R.wrap_stream(z, len(data)), 0)
        assert st == 0 and s0.tobytes() == data, name


def test_stage_arguments(reader):
    import ctypes as C

    f = R.case((8, 2), 8, 8, ("all", 4), "default", "one", 0)
    dst = torch.zeros(4 * 64, dtype=torch.uint8, device=reader.device)
    st = C.c_int()
    call = lambda data, stage, room: reader._lib.bbocr_op_png_decode_stage(reader._h, data, len(data), stage, C.c_void_p(dst.data_ptr()), room, C.byref(st))
    assert call(f, 2, 4 * 64) == 0 and call(f, 2, 4 * 64 - 1) == ERR_ARG and call(f, 3, 4 * 64) == ERR_ARG and call(f, 0, 8 * 25 - 1) == ERR_ARG
    assert call(R.adam7_file(np.zeros((8, 8), np.uint8)), 0, 4 * 64) == ERR_ARG


def test_planes_status_guards_and_pitches(reader, matrix, text_pages):
    from bb_ocr_amd.reader import decode_file

    files = [f for _, f, _ in matrix] + [open(p, "rb").read() for p in GOLDEN] + [f for _, f in text_pages]
    want = [(d["rgb"], d["gray"]) for _, _, d in matrix] + [decode_file(f) for f in files[len(matrix):]]
    status, buf, lay = decode_guarded(reader, files)
    assert status == [0] * len(files)                                     # no supported file is refused
    exp, _ = expected_buffer(buf.size, lay, want)
    assert np.array_equal(buf, exp)                                       # every plane exact, guards and the bytes behind every row untouched
    status2, buf2, _ = decode_guarded(reader, files)
    assert status2 == status and np.array_equal(buf2, buf)                # two consecutive calls: identical bytes


def test_batch_and_device_entry_points(reader, matrix, text_pages):
    from bb_ocr_amd.reader import decode_file

    pages = pages_of([f for _, f in text_pages])                          # RGB, L and 1-bit files of one shape: one uniform batch
    (rgb, gray), status = reader.decode_png_batch(pages)
    assert status == [0, 0, 0] and tuple(rgb.shape) == (3, 960, 1280, 3) and tuple(gray.shape) == (3, 960, 1280)
    for k, (_, f) in enumerate(text_pages):
        w_rgb, w_gray = decode_file(f)
        assert np.array_equal(rgb[k].cpu().numpy(), w_rgb) and np.array_equal(gray[k].cpu().numpy(), w_gray)
    with pytest.raises(ValueError):
        reader.decode_png_batch(pages + pages_of([matrix[0][1]]))
    groups = {}                                                           # the matrix: every file, one uniform batch per shape (all 11 pairs in each)
    for name, f, d in matrix:
        groups.setdefault(d["rgb"].shape, []).append((name, f, d))
    assert len(groups) == len(R.GPU_WIDTHS) * len(R.GPU_HEIGHTS) and all(len(g) == len(R.PAIRS) for g in groups.values())
    for shape, group in groups.items():
        (rgb, gray), status = reader.decode_png_batch(pages_of([f for _, f, _ in group]))
        assert status == [0] * len(group) and tuple(rgb.shape) == (len(group),) + shape, shape
        assert np.array_equal(rgb.cpu().numpy(), np.stack([d["rgb"] for _, _, d in group])), shape
        assert np.array_equal(gray.cpu().numpy(), np.stack([d["gray"] for _, _, d in group])), shape
    sources = [f for _, f, _ in matrix] + GOLDEN + [R.adam7_file(np.zeros((9, 9), np.uint8)), b"\xff\xd8\xff\xe0"]
    want = [(d["rgb"], d["gray"]) for _, _, d in matrix] + [decode_file(p) for p in GOLDEN]      # (the restatement's planes ARE decode_file's: the CPU tests)
    got = reader.decode_png_device(sources)
    assert got[-1] is None and got[-2] is None
    for k, (g, w) in enumerate(zip(got, want)):
        assert g is not None and np.array_equal(g[0].cpu().numpy(), w[0]) and np.array_equal(g[1].cpu().numpy(), w[1]), k


def test_damaged_files_beside_good_ones(reader, matrix):
    """(tools/pngdec_hostcheck.py has run these files through the same inflate under a sanitizer on the host.)"""
    bad = [(n, R.wrap_stream(z, length, 3)) for n, z, length in R.damaged()]
    idx = R.content(9, 5, 2, 3, 1)                                        # a palette of 3 entries under indices up to 3
    assert idx.max() == 3
    pal3 = R.png_bytes(9, 5, 2, 3, [zlib.compress(R.apply_filters(R.pack_rows(idx, 2), np.zeros(5, np.int64), 1))], palette=R.palette_of(2, 1)[:9])
    assert R.plan(pal3)["supported"] == 1 and R.plan(pal3)["palette_entries"] == 3
    with pytest.raises(R.Refused):
        R.decode(pal3)
    bad.append(("palette_index", pal3))
    good = matrix[3::23][:len(bad) + 1]
    files, planes, is_bad = [], [], []
    for k, (_, f, d) in enumerate(good):                                  # good, bad, good, bad, ... good
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
    for name, f in bad:                                                   # ... and each alone, through the entry point of the callers
        assert reader.decode_png_device([f]) == [None], name
    status, buf, lay = decode_guarded(reader, [f for _, f, _ in good])    # the context serves a further call
    assert status == [0] * len(good)
    assert np.array_equal(buf, expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in good])[0])


def test_argument_errors_per_file(reader, matrix):
    import ctypes as C

    f = matrix[5][1]
    page = pages_of([f])[0]
    H, W, _ = page.shape
    rgb = torch.full((H * W * 3 + 8,), FILL, dtype=torch.uint8, device=reader.device)
    gray = torch.full((H * W + 8,), FILL, dtype=torch.uint8, device=reader.device)
    refused = pages_of([f])[0]
    refused.data = R.adam7_file(np.zeros((H, W), np.uint8))
    short = reader._png_decode_into([page, page, refused, page], [rgb.data_ptr()] * 4, [3 * W - 1, 3 * W, 3 * W, 3 * W], [gray.data_ptr()] * 4, [W, W - 1, W, W])
    assert short == [ERR_ARG, ERR_ARG, ERR_ARG, 0]
    assert bool((rgb[H * W * 3:] == FILL).all()) and bool((gray[H * W:] == FILL).all())


def test_round_trip_through_the_device_writer(reader):
    rng = np.random.default_rng(4)
    gray = np.repeat(rng.integers(0, 256, (75, 20), dtype=np.uint8), 5, axis=1)
    rgb = rng.integers(0, 256, (67, 131, 3), dtype=np.uint8)
    rgb[20:40, 10:90] = (250, 3, 128)
    for page in (gray, rgb):
        dev = torch.from_numpy(page).to(reader.device)
        f = reader.encode_png(dev)
        got = reader.decode_png_device([f])[0]
        assert got is not None
        if page.ndim == 2:
            assert torch.equal(got[1], dev) and torch.equal(got[0], dev[..., None].expand(-1, -1, 3))
        else:
            assert torch.equal(got[0], dev)


# ------------------------------------------------------------------------------------------------ the callers
def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[0], np.float64), np.asarray(y[0], np.float64)) and x[1] == y[1] and x[2] == y[2]
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """PNG and JPEG pages of two shapes, an Adam7 file (the plan refuses it) and a PNG whose zlib stream is cut short -> (paths, names)"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("png_callers")
    shapes = {"A": dict(width=320, height=192, lines=3, margin=24), "B": dict(width=256, height=160, lines=2, margin=20)}
    spec = [("png_rgb", "A"), ("jpg", "A"), ("png_L", "B"), ("png_rgb", "A"), ("adam7", "A"), ("png_1bit", "A"), ("jpg", "B"), ("png_L", "B"),
            ("cut", "A"), ("png_rgb", "B"), ("jpg", "A"), ("png_rgb", "A")]
    paths = []
    for i, (kind, shape) in enumerate(spec):
        img = synth.page(40 + i, **shapes[shape])[0]
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "png"))
        if kind == "jpg":
            Image.fromarray(img).save(p, quality=92)
        elif kind == "adam7":
            p.write_bytes(R.adam7_file(img))
        elif kind == "cut":
            b = io.BytesIO()
            Image.fromarray(img).save(b, "PNG")
            _, idat, _ = R.walk(b.getvalue())
            z = b"".join(idat)
            p.write_bytes(R.png_bytes(img.shape[1], img.shape[0], 8, 2, [z[:len(z) // 2]]))
        else:
            pil = Image.fromarray(img if kind == "png_rgb" else (img[..., 1] if kind == "png_L" else img[..., 1] > 128))
            pil.save(p)
        paths.append(str(p))
    return paths, [k for k, _ in spec]


def test_callers_with_the_option_on(reader, directory, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import extractor_batch

    paths, kinds = directory
    assert reader.png_decode is False                                    # off unless asked for
    off = reader.readtext_files(paths, png_decode=False)
    assert sum(bool(r) for r in off) >= len(paths) - 2                   # the pages hold text
    decoded = []
    real = reader.decode_png_batch
    monkeypatch.setattr(reader, "decode_png_batch", lambda pages: (decoded.append(len(list(pages))), real(pages))[1])
    for mixed in (False, True):
        del decoded[:]
        on = reader.readtext_files(paths, png_decode=True, mixed=mixed)
        assert all(same_results(a, b) for a, b in zip(on, off)), mixed
        # the eight PNG files the plan supports (the cut one among them) went through the device decoder: one call per shape group
        assert sorted(decoded) == [3, 5], decoded
        res = extractor_batch.read_files(reader, paths, png_decode=True, mixed=mixed, device_decode=True)
        assert all(same_results(res[i], off[i]) for i in range(len(paths)))
        texts = extractor_batch.extract_texts(reader, paths, png_decode=True, mixed=mixed)
        assert texts == extractor_batch.extract_texts(reader, paths, png_decode=False, mixed=mixed)
    del decoded[:]
    assert extractor_batch.read_files(reader, paths, mixed=False).keys() == set(range(len(paths))) and not decoded      # the Reader's default: off
    one = [reader.readtext(p) for p in paths[:6]]
    monkeypatch.setattr(reader, "png_decode", True)
    del decoded[:]
    for p, want in zip(paths[:6], one):
        assert same_results(reader.readtext(p), want), p
        data = open(p, "rb").read()
        assert same_results(reader.readtext(data), reader.readtext(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))    # bytes: the array rule
    assert sum(decoded) == 2 * sum(k.startswith("png") for k in kinds[:6])
