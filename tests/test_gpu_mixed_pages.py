"""GPU: pages of mixed shapes in one device call (bbocr_readtext_pages, csrc/pages.hip, the page-table variants of the crop kernels) and
its callers.  Every comparison is equality: one call over n pages returns what n one-page calls return, bit for bit."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 0xA5
# (H, W, lines): 250 x 500 is off the detector's 32-pixel grid and 250 * 500 is no multiple of 16; 192 x 320 comes twice, not adjacent;
# page 5 carries no text
SIX = [(256, 384, 4), (250, 500, 4), (192, 320, 3), (288, 416, 5), (192, 320, 2), (224, 352, 0)]


def _page(seed, H, W, lines, colour=False):
    from bb_ocr_amd import synth

    if lines == 0:
        return np.full((H, W, 3), 236, np.uint8)
    return synth.page(seed, width=W, height=H, lines=lines, margin=20, line_pitch=38, colour=colour)[0]


_CACHE = {}


def _six():
    """The six pages on the card (made once, never written)"""
    if "six" not in _CACHE:
        _CACHE["six"] = [torch.from_numpy(_page(91_000 + k, H, W, n, colour=bool(k & 1))).cuda() for k, (H, W, n) in enumerate(SIX)]
    return _CACHE["six"]


def _single(reader, page, gray=None, **kw):
    return reader.readtext_device(page[None], None if gray is None else gray[None], **kw)[0]


def _singles(reader, name, pages, **kw):
    """Page-by-page reference of a page list, computed once per (reader, list, keywords)"""
    key = (id(reader), name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CACHE:
        _CACHE[key] = [_single(reader, p, **kw) for p in pages]
    return _CACHE[key]


@pytest.fixture(params=["bf16", "fp16"])
def rd(request, reader, reader_fp16):
    return reader if request.param == "bf16" else reader_fp16


def test_mixed_pages_equal_one_page_calls(rd):
    pages = _six()
    want = _singles(rd, "six", pages)
    assert sum(len(w) for w in want) >= 10 and want[5] == [] and want[2] != want[4]
    assert rd.readtext_pages(pages) == want
    assert rd.readtext_pages(pages[::-1]) == want[::-1]                      # another order: other groups, another pass order
    assert rd.readtext_pages(pages[2:3]) == want[2:3]                        # n = 1


def test_canvas_resize_in_the_mix(rd):
    """canvas_size = 256: the six pages are resized by the detector, a 160 x 256 page is not"""
    if "small" not in _CACHE:
        _CACHE["small"] = torch.from_numpy(_page(91_100, 160, 256, 3)).cuda()
    pages = _six() + [_CACHE["small"]]
    assert rd.detect_dims(160, 256, 256)[4] == 1.0 and rd.detect_dims(256, 384, 256)[4] < 1.0
    want = _singles(rd, "six+small", pages, canvas_size=256)
    assert any(want) and want[6]
    assert rd.readtext_pages(pages, canvas_size=256) == want


def test_strided_views_and_given_gray_planes(reader):
    """Pages as non-contiguous views of a larger device tensor (odd x offset: rows start unaligned), some with a gray plane given -- the
    plane of ANOTHER text page of the same shape, so that a wrong plane changes the text -- equal readtext_device on contiguous copies"""
    from bb_ocr_amd.reader import _gray_bgr2gray

    host = [_page(92_000 + k, H, W, n, colour=True) for k, (H, W, n) in enumerate([(192, 320, 3), (192, 320, 3), (250, 500, 4), (256, 384, 4)])]
    big = torch.full((620, 1111, 3), GUARD, dtype=torch.uint8, device="cuda")
    bigg = torch.full((620, 1111), GUARD, dtype=torch.uint8, device="cuda")
    spots = [(3, 7), (3, 401), (210, 5), (330, 611)]                         # (y0, x0), x0 odd
    views, grays = [], []
    for (y0, x0), a in zip(spots, host):
        H, W = a.shape[:2]
        big[y0:y0 + H, x0:x0 + W] = torch.from_numpy(a).cuda()
        views.append(big[y0:y0 + H, x0:x0 + W])
    # page 0 reads page 1's plane (strided, odd offset), page 3 its own plane (contiguous), pages 1 and 2 none
    g1 = torch.from_numpy(_gray_bgr2gray(host[1])).cuda()
    bigg[5:5 + 192, 9:9 + 320] = g1
    g3 = torch.from_numpy(_gray_bgr2gray(host[3])).cuda()
    grays = [bigg[5:5 + 192, 9:9 + 320], None, None, g3]
    assert not views[0].is_contiguous() and not grays[0].is_contiguous()
    want = [_single(reader, v.contiguous(), None if g is None else g.contiguous()) for v, g in zip(views, grays)]
    assert all(want) and want[0] != _single(reader, views[0].contiguous())   # the foreign plane does change page 0's text
    assert reader.readtext_pages(list(zip(views, grays))) == want
    # a view whose pixels are not packed (channel flip) is made contiguous by the Reader
    flipped = views[2].flip(2)
    assert reader.readtext_pages([flipped]) == [_single(reader, flipped.contiguous())]


def _plan(reader, arr, n):
    ro, go, sb = (C.c_longlong * n)(), (C.c_longlong * n)(), (C.c_longlong * 2)()
    assert reader._lib.bbocr_host_pages_plan(arr, n, None, None, None, ro, go, None, sb) == 0
    return list(ro), list(go), list(sb)


def test_pack_stage_alone(reader):
    """bbocr_op_pack_pages: staging bytes == source pages on the 16-byte and on the byte path, derived gray == the uniform path's, guard
    bands around the source views and around the staging buffers unchanged"""
    from bb_ocr_amd import _lib
    from bb_ocr_amd.reader import _gray_bgr2gray

    rng = np.random.default_rng(5)
    big = torch.full((700, 912, 3), GUARD, dtype=torch.uint8, device="cuda")           # pitch 2736 = 16 * 171
    bigg = torch.full((700, 912), GUARD, dtype=torch.uint8, device="cuda")
    srcs = []                                                                           # (rgb tensor, gray tensor or None)

    def tight(H, W, gray=False):
        a = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        g = torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).cuda() if gray else None
        srcs.append((a, g))

    def view(y0, x0, H, W, gray=False):
        big[y0:y0 + H, x0:x0 + W] = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
        g = None
        if gray:
            bigg[y0:y0 + H, x0:x0 + W] = torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8)).cuda()
            g = bigg[y0:y0 + H, x0:x0 + W]
        srcs.append((big[y0:y0 + H, x0:x0 + W], g))

    tight(256, 384)                  # 16-byte path, derived gray
    tight(250, 500)                  # 125000 pixels: 16-byte path + the last 8 pixels byte by byte
    tight(250, 500, gray=True)       # second page of its group: staging offset 375000 is no multiple of 16 -> byte path; given gray
    view(3, 7, 100, 333)             # odd x offset: byte path
    view(110, 16, 120, 320)          # aligned view, W % 16 == 0: 16-byte path with a pitch
    view(240, 48, 90, 160, True)     # the same with a given, aligned gray view
    view(340, 5, 77, 201, True)      # byte path, given gray at an odd offset
    tight(256, 384, gray=True)       # 16-byte path, given gray; shares the first page's group
    tight(33, 5000)                  # more than one tile per row
    n = len(srcs)
    arr = (_lib.bbocr_page * n)()
    for k, (a, g) in enumerate(srcs):
        arr[k].dev_rgb, arr[k].H, arr[k].W, arr[k].rgb_pitch = a.data_ptr(), a.shape[0], a.shape[1], a.stride(0)
        if g is not None:
            arr[k].dev_gray, arr[k].gray_pitch = g.data_ptr(), g.stride(0)
    ro, go, sb = _plan(reader, arr, n)
    pad = 4096
    st_rgb = torch.full((sb[0] + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    st_gray = torch.full((sb[1] + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    big0, bigg0 = big.clone(), bigg.clone()
    torch.cuda.synchronize()
    reader._check(reader._lib.bbocr_op_pack_pages(reader._h, arr, n, C.c_void_p(st_rgb.data_ptr() + pad), C.c_void_p(st_gray.data_ptr() + pad)))
    got_rgb, got_gray = st_rgb.cpu().numpy(), st_gray.cpu().numpy()
    want_rgb, want_gray = np.full_like(got_rgb, GUARD), np.full_like(got_gray, GUARD)
    for k, (a, g) in enumerate(srcs):
        H, W = a.shape[:2]
        an = a.cpu().numpy()
        want_rgb[pad + ro[k]:pad + ro[k] + H * W * 3] = an.reshape(-1)
        if g is None:
            # what the uniform path derives: launch_gray on the contiguous page (pre-processing stage 6) -- and cv2's formula
            d = torch.empty((H, W), dtype=torch.uint8, device="cuda")
            src = a.contiguous()
            torch.cuda.synchronize()
            reader._check(reader._lib.bbocr_op_preprocess_stage(reader._h, 6, C.c_void_p(src.data_ptr()), H, W, C.c_void_p(d.data_ptr()), H, W, 0.0))
            gn = d.cpu().numpy()
            assert np.array_equal(gn, _gray_bgr2gray(an))
        else:
            gn = g.cpu().numpy()
        want_gray[pad + go[k]:pad + go[k] + H * W] = gn.reshape(-1)
    # (whole buffers: the pages, the 256-byte padding between groups and the guard bands on both sides)
    assert np.array_equal(got_rgb, want_rgb)
    assert np.array_equal(got_gray, want_gray)
    assert torch.equal(big, big0) and torch.equal(bigg, bigg0)


def test_pack_stage_with_staging_at_any_byte(reader):
    """Caller-owned staging buffers that start at an odd address: pages whose offsets, pointers and pitches are all multiples of 16 must
    then take the byte path (the 16-byte path is chosen from the address a copy really has), and the bytes are the same"""
    from bb_ocr_amd import _lib

    rng = np.random.default_rng(6)
    srcs = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for H, W in ((64, 96), (80, 160), (64, 96))]
    n = len(srcs)
    arr = (_lib.bbocr_page * n)()
    for k, a in enumerate(srcs):
        arr[k].dev_rgb, arr[k].H, arr[k].W = a.data_ptr(), a.shape[0], a.shape[1]
    ro, go, sb = _plan(reader, arr, n)
    assert all(v % 16 == 0 for v in ro + go)
    got = {}
    for shift in (0, 1, 7):
        st_rgb = torch.full((sb[0] + 64,), GUARD, dtype=torch.uint8, device="cuda")
        st_gray = torch.full((sb[1] + 64,), GUARD, dtype=torch.uint8, device="cuda")
        assert st_rgb.data_ptr() % 16 == 0 and st_gray.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        reader._check(reader._lib.bbocr_op_pack_pages(reader._h, arr, n, C.c_void_p(st_rgb.data_ptr() + 16 + shift), C.c_void_p(st_gray.data_ptr() + 16 + shift)))
        r, g = st_rgb.cpu().numpy(), st_gray.cpu().numpy()
        assert (r[:16 + shift] == GUARD).all() and (g[:16 + shift] == GUARD).all()
        assert (r[16 + shift + sb[0]:] == GUARD).all() and (g[16 + shift + sb[1]:] == GUARD).all()
        got[shift] = (r[16 + shift:16 + shift + sb[0]], g[16 + shift:16 + shift + sb[1]])
    for k, a in enumerate(srcs):
        assert np.array_equal(got[0][0][ro[k]:ro[k] + a.numel()], a.cpu().numpy().reshape(-1))
    for shift in (1, 7):
        assert np.array_equal(got[shift][0], got[0][0]) and np.array_equal(got[shift][1], got[0][1])


def _crop_case():
    """Three gray pages of three shapes with horizontal and free boxes; some touch or cross the page border"""
    from bb_ocr_amd.reader import _gray_bgr2gray

    shapes = [(192, 320), (250, 500), (288, 416)]
    grays = [_gray_bgr2gray(_page(93_000 + k, H, W, 4, colour=True)) for k, (H, W) in enumerate(shapes)]
    hori, free = [], []
    for H, W in shapes:
        hori.append([[20, 180, 18, 50], [-6, W + 9, 60, 92], [W - 70, W + 30, H - 28, H + 6], [0, 40, 0, 64], [30, 60, 20, 140]])
        free.append([[[30.0, 100.0], [200.0, 84.0], [204.0, 118.0], [34.0, 134.0]],
                     [[W - 90.0, H - 60.0], [W + 12.0, H - 50.0], [W + 8.0, H - 10.0], [W - 94.0, H - 20.0]],      # runs over the right edge
                     [[-8.0, -5.0], [120.0, 4.0], [118.0, 40.0], [-10.0, 31.0]]])                                    # and over the top-left corner
    return shapes, grays, hori, free


def test_crop_stage_alone(rd):
    """bbocr_op_crops_pages == bbocr_op_crops page by page: the page-table variants of the crop kernels read each page with its own bounds"""
    from bb_ocr_amd import _lib

    shapes, grays, hori, free = _crop_case()
    big = torch.full((300, 777), GUARD, dtype=torch.uint8, device="cuda")
    dev = [torch.from_numpy(g).cuda() for g in grays]
    big[7:7 + 288, 11:11 + 416] = dev[2]
    dev[2] = big[7:7 + 288, 11:11 + 416]                                        # the third page: a strided view, read in place
    lib, h = rd._lib, rd._h
    hflat = [int(v) for page in hori for b in page for v in b]
    fflat = [float(v) for page in free for q in page for p in q for v in p]
    harr, farr = (C.c_int * len(hflat))(*hflat), (C.c_double * len(fflat))(*fflat)
    hoff = (C.c_int * 4)(*np.concatenate([[0], np.cumsum([len(p) for p in hori])]).tolist())
    foff = (C.c_int * 4)(*np.concatenate([[0], np.cumsum([len(p) for p in free])]).tolist())
    arr = (_lib.bbocr_page * 3)()
    for k, g in enumerate(dev):
        arr[k].dev_gray, arr[k].H, arr[k].W, arr[k].gray_pitch = g.data_ptr(), g.shape[0], g.shape[1], g.stride(0)
    nbox = len(hflat) // 4 + len(fflat) // 8
    for imgW, mode, contrast in ((256, 1, 0.0), (256, 1, 0.5), (320, 3, 0.0), (128, 0, 0.0), (192, 0, 0.5)):
        want, counts = [], []
        for k, g in enumerate(dev):
            out = torch.zeros((len(hori[k]) + len(free[k]), 64, imgW), dtype=torch.int16, device="cuda")
            gc = g.contiguous()
            ph = (C.c_int * (4 * len(hori[k])))(*[int(v) for b in hori[k] for v in b])
            pf = (C.c_double * (8 * len(free[k])))(*[float(v) for q in free[k] for p in q for v in p])
            n_out = C.c_int()
            torch.cuda.synchronize()
            rd._check(lib.bbocr_op_crops(h, C.c_void_p(gc.data_ptr()), g.shape[0], g.shape[1], ph, len(hori[k]), pf, len(free[k]), imgW, contrast,
                                         C.c_void_p(out.data_ptr()), C.byref(n_out), mode))
            want.append(out[:n_out.value].cpu())
            counts.append(n_out.value)
        out = torch.zeros((nbox, 64, imgW), dtype=torch.int16, device="cuda")
        n_out = C.c_int()
        torch.cuda.synchronize()
        rd._check(lib.bbocr_op_crops_pages(h, arr, 3, harr, hoff, farr, foff, imgW, contrast, C.c_void_p(out.data_ptr()), C.byref(n_out), mode))
        assert n_out.value == sum(counts) and (mode == 0 or n_out.value == nbox), (imgW, mode, counts)
        assert torch.equal(out[:n_out.value].cpu(), torch.cat(want)), (imgW, mode, contrast)
    assert sum(counts) > 0                                                       # (the last, per-box-width case took some boxes too)


def _low_contrast(seed, H, W, lines):
    """A page scaled to low contrast where the recogniser reads it: synth's faint ink on every line.  The green channel -- what the designed
    detector reads -- keeps its dark strokes, red and blue are set so that cv2's gray plane shows ink 123 on paper 163 instead of 30 on 235.
    (Scaling all three channels alike cannot serve: the fixtures' recogniser is a seeded random CRNN whose confidence stays at 0.2 .. 0.5
    on such a page, above contrast_ths = 0.1, and under a stronger scaling the paper enters the detector's ink range.)  On the fp32 CPU
    oracle this page's three lines have first-pass confidences 0.005, 0.014 and 0.033, and the retry raises them to 0.18, 0.65 and 0.28."""
    from bb_ocr_amd import synth

    return synth.page(seed, width=W, height=H, lines=lines, margin=20, line_pitch=38, faint=1.0)[0]


@pytest.mark.parametrize("kw", [dict(rotation_info=[90, 180, 270]), dict(decoder="beamsearch"), dict(allowlist="0123456789"), dict(paragraph=True), {}],
                         ids=["rotation", "beamsearch", "allowlist", "paragraph", "contrast_retry"])
def test_modes_equal_page_by_page(reader, kw):
    """A two-shape mix (one page scaled to low contrast) in each of readtext's modes"""
    if "modes" not in _CACHE:
        host = [_page(94_000, 192, 320, 3), _low_contrast(94_011, 250, 500, 4), _page(94_002, 192, 320, 2, colour=True)]
        _CACHE["modes"] = [torch.from_numpy(a).cuda() for a in host]
    pages = _CACHE["modes"]
    want = _singles(reader, "modes", pages, **kw)
    assert all(want)
    if not kw:      # the contrast retry changes the low-contrast page's result: shown on the page alone
        first = _single(reader, pages[1], contrast_ths=0.0)
        print("first-pass confidences", [c for _, _, c in first], "with the retry", [c for _, _, c in want[1]])
        assert first != want[1]
    assert reader.readtext_pages(pages, **kw) == want


def _twelve():
    shapes = [(192 + 8 * (k % 5) + 32 * (k // 6), 288 + 24 * k) for k in range(12)]
    assert len(set(shapes)) == 12
    if "twelve" not in _CACHE:
        _CACHE["twelve"] = [torch.from_numpy(_page(95_000 + k, H, W, 2 + k % 4, colour=bool(k & 1))).cuda() for k, (H, W) in enumerate(shapes)]
    return _CACHE["twelve"]


def test_twelve_shapes_in_one_call(rd):
    pages = _twelve()
    want = _singles(rd, "twelve", pages)
    assert rd.readtext_pages(pages) == want
    st = rd.stage_times()
    assert st["total"] > 0 and st["detector_net"] > 0 and st["ccl_device"] > 0 and st["recognizer_net"] > 0 and st["total"] >= st["detector_net"]


def test_two_calls_in_flight_equal_the_serial_path(reader_fp16):
    """Two threads share the Reader and call with different mixes: each call returns what it returns alone, whichever slot it ran in"""
    from concurrent.futures import ThreadPoolExecutor

    r = reader_fp16
    six, twelve = _six(), _twelve()
    mixes = [six, twelve[:7] + six[1:3], six[::-1] + twelve[5:]]
    serial = [r.readtext_pages(m) for m in mixes]
    assert serial[0] != serial[1]

    def call(k):
        return r.readtext_pages(mixes[k % 3]), r.stage_times()

    with ThreadPoolExecutor(max_workers=2) as ex:
        par = list(ex.map(call, range(8)))
    for k, (out, st) in enumerate(par):
        assert out == serial[k % 3], k
        assert st["total"] > 0 and st["detector_net"] > 0


def test_callers_in_mixed_mode(reader, tmp_path, monkeypatch):
    from PIL import Image

    from bb_ocr_amd.extractor_batch import extract_texts

    shapes = [(192, 320), (250, 500), (256, 384), (192, 320), (288, 416), (250, 500), (224, 352)]
    imgs = [_page(96_000 + k, H, W, 2 + k % 3, colour=bool(k & 1)) for k, (H, W) in enumerate(shapes)]
    want = reader.readtext_batched(imgs)
    assert all(want)
    assert reader.readtext_batched(imgs, mixed=True) == want
    monkeypatch.setenv("BBOCR_MAX_DEVICE_BATCH", "3")                          # batches closed by page count: [3, 3, 1], two in flight
    assert reader.readtext_batched(imgs, mixed=True) == want
    monkeypatch.setenv("BBOCR_MIXED_BATCH", "1")                               # the environment switch behind mixed=None
    monkeypatch.setenv("BBOCR_MIXED_PIXEL_BUDGET", str(300_000))               # ... and by the pixel budget
    assert reader.readtext_batched(imgs) == want
    monkeypatch.delenv("BBOCR_MIXED_BATCH")
    monkeypatch.delenv("BBOCR_MIXED_PIXEL_BUDGET")
    monkeypatch.delenv("BBOCR_MAX_DEVICE_BATCH")
    paths = []
    for k, a in enumerate(imgs[:6]):
        p = tmp_path / (f"p{k}.jpg" if k % 3 != 2 else f"p{k}.png")
        Image.fromarray(a).save(p, quality=92) if p.suffix == ".jpg" else Image.fromarray(a).save(p)
        paths.append(str(p))
    for dd in (False, True):
        base = extract_texts(reader, paths, device_decode=dd)
        assert sum(bool(t) for t in base.values()) >= 5
        assert extract_texts(reader, paths, device_decode=dd, mixed=True) == base
    assert reader.readtext_files(paths, mixed=True) == reader.readtext_files(paths)


def test_argument_errors_leave_the_reader_usable(reader):
    pages = _six()
    want = _singles(reader, "six", pages)
    good = pages[0]
    with pytest.raises(ValueError):
        reader.readtext_pages([])
    for bad in (good.cpu(), good.to(torch.int16), good[..., :2], good[0], torch.zeros((0, 8, 3), dtype=torch.uint8, device="cuda"), "page.png"):
        with pytest.raises(ValueError):
            reader.readtext_pages([good, bad])
    with pytest.raises(ValueError):
        reader.readtext_pages([(good, pages[1][..., 0])])                      # a gray plane of another shape
    with pytest.raises(ValueError):
        reader.readtext_pages([(good, good[..., 0].to(torch.float32))])
    # refused by the library before anything is queued: a page that collapses to zero size under canvas_size
    thin = torch.zeros((2, 2000, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="collapses"):
        reader.readtext_pages([good, thin], canvas_size=256)
    with pytest.raises((ValueError, RuntimeError)):
        reader.readtext_pages([good], rotation_info=[45])
    assert reader.readtext_pages(pages) == want
