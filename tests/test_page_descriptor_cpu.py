"""``preprocess.page_descriptor``: the one rule of a valid device page that ``auto_crop_box_device``, ``ocr_thumbnail_device`` and
``orient_page_device`` share, on CPU tensors (being on the reader's device is a separate check)."""
import pytest
import torch

from bb_ocr_amd.preprocess import PAGE_BGR, PAGE_GRAY, PAGE_RGB, PAGE_YCBCR3, PAGE_YCBCR4, page_descriptor

ANY = (PAGE_GRAY, PAGE_BGR, PAGE_RGB, PAGE_YCBCR4, PAGE_YCBCR3)


def _desc(t, layouts):
    return page_descriptor(t.shape, t.stride(), t.dtype, layouts)


def test_accepts_packed_pages_and_row_strided_views():
    gray = torch.zeros((5, 9), dtype=torch.uint8)
    bgr = torch.zeros((5, 9, 3), dtype=torch.uint8)
    assert _desc(gray, (PAGE_GRAY,)) == (5, 9, 9, 1)
    assert _desc(gray, (PAGE_GRAY, PAGE_BGR)) == (5, 9, 9, 1)
    for layout in (PAGE_BGR, PAGE_RGB, PAGE_YCBCR3):
        assert _desc(bgr, (layout,)) == (5, 9, 27, 3)
    assert _desc(bgr, (PAGE_GRAY, PAGE_BGR)) == (5, 9, 27, 3)
    assert _desc(torch.zeros((5, 9, 4), dtype=torch.uint8), (PAGE_YCBCR4,)) == (5, 9, 36, 4)
    crop = torch.zeros((12, 20, 3), dtype=torch.uint8)[2:9, 3:17]               # a crop read in place: the pitch is the parent's
    assert _desc(crop, (PAGE_BGR,)) == (7, 14, 60, 3)
    assert _desc(torch.zeros((12, 20), dtype=torch.uint8)[2:9, 3:17], (PAGE_GRAY,)) == (7, 14, 20, 1)


def test_rejects_everything_else():
    gray = torch.zeros((5, 9), dtype=torch.uint8)
    bgr = torch.zeros((5, 9, 3), dtype=torch.uint8)
    bad = [
        (bgr.to(torch.int32), ANY), (bgr.float(), ANY), (gray.float(), ANY),     # dtype
        (bgr[:, :, :2], ANY),                                                    # two channels: no such layout
        (bgr[:, ::2], ANY), (gray[:, ::2], ANY),                                 # pixels not packed along a row
        (bgr.permute(1, 0, 2), ANY), (gray.t(), ANY),                            # rows and columns swapped
        (bgr[:0], ANY), (gray[:0], ANY), (bgr[:, :0], ANY),                      # empty
        (bgr, (PAGE_GRAY,)), (gray, (PAGE_BGR,)), (bgr, (PAGE_YCBCR4,)),         # channels against the declared layout
        (bgr, (5,)), (bgr, (-1,)), (gray, (7,)), (bgr, ()),                      # a layout outside 0 .. 4, or none
        (torch.zeros((9,), dtype=torch.uint8), ANY), (torch.zeros((2, 5, 9, 3), dtype=torch.uint8), ANY),
    ]
    for t, layouts in bad:
        with pytest.raises(ValueError):
            _desc(t, layouts)
