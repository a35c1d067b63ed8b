"""Geometry and form choice of the device Resize(S) + CenterCrop(S) (csrc/preprocess.hip, prep_geometry() in csrc/mcm_api.hip),
restated in plain Python (numpy only, no GPU), plus the inputs the bit-exact tests share: a Pillow-only restatement of
torchvision's transform, hostile image contents and, per crop size S, a table of image sizes that reaches every branch the
kernel can take at that S.

The kernel picks a form per workgroup (8 output rows of one image).  form_branches() names what it picks:
  copy          no axis is resampled (short side == S, both sides): the fused form as a plain crop copy
  fused-taps    more than 16 taps on an axis (2 * ceil(scale) + 1: scale factor above 7): the fused form
  T8-rs8|4|2|1  LDS form, 8-tap tables (both axes at most 8 taps), 8 / 4 / 2 / 1 output rows per LDS pass
  T16-rs8|4|2|1 LDS form, 16-tap tables
  T8-nofit, T16-nofit   not even single rows fit the LDS budget: the workgroup falls through to the fused form
  fused-T8, fused-T16   S % 4 != 0: the LDS form is never entered; the image runs the fused form although its taps would
                        have let it in (the label says which table width it would have had)
tests/test_resize_forms.py pins, on the CPU, which labels every table reaches and that no other label is reachable at
that S; the GPU tests (tests/test_gpu_preprocess_sizes.py) then run the tables.  Whoever changes the choice in
preprocess.hip changes form_branches() with it.
"""
from __future__ import annotations

import math
import os
import re

import numpy as np

# preprocess.hip
KMAX = 64                     # taps per output coordinate the fused form holds
ROWS = 8                      # output rows per workgroup
FT = 16                       # taps per output coordinate the LDS form holds
LDS_FORM_BYTES = 56 * 1024    # staged source window + horizontal-pass rows

CONTENT_KINDS = ("rand", "c0", "c255", "c100", "checker", "stripes", "extremes")


def prep_ring() -> int:
    """mcm_handle::PREP_RING, the staging slots mcm_resize_crop_u8 rotates over, read from csrc/mcm_api.hip."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "mcm_amd", "csrc", "mcm_api.hip")) as f:
        return int(re.search(r"static constexpr int PREP_RING = (\d+);", f.read()).group(1))


def _round_half_even(v: float) -> int:
    f = math.floor(v)
    d = v - f
    if d < 0.5:
        return int(f)
    if d > 0.5:
        return int(f) + 1
    return int(f) if int(f) % 2 == 0 else int(f) + 1


def prep_geometry(H: int, W: int, S: int):
    """(nh, nw, top, left) of an H x W image for a square target S, or None where the resized image is smaller than the crop
    (mcm_api.hip prep_geometry): short side -> S, long side int(S * long / short), untouched when short == S; crop origin
    round((n - S) / 2), half to even."""
    shrt, lng = (W, H) if W <= H else (H, W)
    if shrt == S:
        nh, nw = H, W
    else:
        nl = int(float(S) * float(lng) / float(shrt))
        nw, nh = (S, nl) if W <= H else (nl, S)
    if nh < S or nw < S:
        return None
    return nh, nw, _round_half_even((nh - S) / 2.0), _round_half_even((nw - S) / 2.0)


def resample_limits(in_size: int, out_size: int, first: int, count: int):
    """(xmin, n) of preprocess.hip resample_coeffs (Pillow's precompute_coeffs, bilinear) for output coordinates
    first .. first + count: first contributing input sample and number of taps.  Same double operations in the same order."""
    xx = np.arange(first, first + count, dtype=np.float64)
    scale = float(in_size) / float(out_size)
    support = 1.0 * (1.0 if scale < 1.0 else scale)
    center = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    return xmin, np.minimum(xmax - xmin, KMAX)


def _taps(n_in: int, n_out: int) -> int:
    return 2 * int(math.ceil(max(float(n_in) / float(n_out), 1.0))) + 1 if n_in != n_out else 1


def form_branches(H: int, W: int, S: int) -> set:
    """Labels of the forms the kernel's workgroups take for one H x W image at crop size S (resize_crop_kernel / lds_form)."""
    geo = prep_geometry(H, W, S)
    if geo is None:
        raise ValueError(f"{H}x{W} is smaller than the crop after Resize({S})")
    nh, nw, top, left = geo
    rx, ry = nw != W, nh != H
    if not (rx or ry):
        return {"copy"}
    taps_x, taps_y = _taps(W, nw), _taps(H, nh)
    if taps_x > KMAX or taps_y > KMAX:
        raise ValueError(f"{H}x{W}: downscale factor above 31 is refused by mcm_resize_crop_u8")
    if taps_x > FT or taps_y > FT:
        return {"fused-taps"}
    TB = 8 if taps_x <= 8 and taps_y <= 8 else 16
    if S % 4:
        return {f"fused-T{TB}"}
    if rx:
        xmin, nx = resample_limits(W, nw, left, S)
    else:
        xmin, nx = np.arange(left, left + S), np.ones(S, dtype=np.int64)
    if ry:
        ymin, ny = resample_limits(H, nh, top, S)
    else:
        ymin, ny = np.arange(top, top + S), np.ones(S, dtype=np.int64)
    wbytes = int(xmin[S - 1] + nx[S - 1] - xmin[0]) * 3
    wstride = ((wbytes + 15 + 15) // 16 + 1) * 16
    out = set()
    for y0 in range(0, S, ROWS):
        nrow = min(ROWS, S - y0)
        ym, yn = ymin[y0:y0 + nrow], ny[y0:y0 + nrow]
        rs = ROWS
        while rs >= 1:
            worst = 0
            for r0 in range(0, nrow, rs):
                r1 = min(r0 + rs, nrow) - 1
                worst = max(worst, int(ym[r1] + yn[r1] - ym[r0]))
            if worst * (wstride + 3 * S) <= LDS_FORM_BYTES:
                break
            rs >>= 1
        out.add(f"T{TB}-rs{rs}" if rs >= 1 and wbytes > 0 else f"T{TB}-nofit")
    return out


def pillow_resize_crop(img: np.ndarray, S: int) -> np.ndarray:
    """torchvision's Resize(S, BILINEAR) + CenterCrop(S) on a uint8 [H, W, 3] array, with Pillow alone
    (torchvision/transforms/functional.py resize / center_crop; the resized image is never smaller than the crop here)."""
    from PIL import Image

    im = Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8), "RGB")
    w, h = im.size
    short, long = (w, h) if w <= h else (h, w)
    if short != S:
        new_short, new_long = S, int(S * long / short)
        new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
        im = im.resize((new_w, new_h), Image.BILINEAR)
    w, h = im.size
    top, left = int(round((h - S) / 2.0)), int(round((w - S) / 2.0))
    return np.asarray(im.crop((left, top, left + S, top + S)))


def content(kind: str, h: int, w: int, rng: np.random.Generator) -> np.ndarray:
    """uint8 [h, w, 3] of one of CONTENT_KINDS: what a resampling or clamping mistake shows on (constants: every weight sum
    must come back to the same byte; 0 / 255 patterns: the largest steps a filter meets, at the clamps' two ends)."""
    if kind == "rand":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind in ("c0", "c255", "c100"):
        return np.full((h, w, 3), int(kind[1:]), dtype=np.uint8)
    yy, xx, cc = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "checker":     # per-pixel checkerboard, neighbouring channels in antiphase
        return (((yy + xx + cc) % 2) * 255).astype(np.uint8)
    if kind == "stripes":     # vertical stripes of period 3, rolled by one column per channel
        return ((((xx + cc) % 3) == 0) * 255).astype(np.uint8)
    if kind == "extremes":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    raise ValueError(kind)


# (H, W) per crop size.  64 / 224 / 336 are the shipped sizes; 70 (S % 4 == 2: fused form only, last row group of 6) and
# 84 (S % 8 == 4: LDS form with a last row group of 4) reach the row-group tails no shipped size has.
SIZES = {
    64: [(16, 16), (211, 211), (352, 352), (64, 64), (467, 467), (64, 90), (1, 1), (2, 700)],
    70: [(21, 21), (277, 290), (70, 70), (70, 99), (411, 300), (613, 700), (1, 3)],
    84: [(21, 21), (277, 277), (411, 411), (537, 537), (84, 84), (613, 613), (85, 84), (300, 84)],
    224: [(56, 56), (649, 649), (739, 739), (816, 806), (1097, 1097), (1433, 1433), (1635, 1635), (224, 224), (768, 1024)],
    336: [(84, 84), (772, 772), (974, 974), (1108, 1108), (1411, 1411), (1646, 1646), (2452, 2452), (336, 336), (337, 336),
          (1008, 1018)],
}

# What each table reaches, and (tests/test_resize_forms.py's search) all that is reachable at that S
EXPECTED_BRANCHES = {
    64: {"copy", "fused-taps", "T8-rs8", "T16-rs8", "T16-rs4"},
    70: {"copy", "fused-taps", "fused-T8", "fused-T16"},
    84: {"copy", "fused-taps", "T8-rs8", "T16-rs8", "T16-rs4", "T16-rs2"},
    224: {"copy", "fused-taps", "T8-rs8", "T8-rs4", "T16-rs4", "T16-rs2", "T16-rs1", "T16-nofit"},
    336: {"copy", "fused-taps", "T8-rs8", "T8-rs4", "T8-rs2", "T16-rs2", "T16-rs1", "T16-nofit"},
}


def branches_of_table(S: int) -> set:
    out = set()
    for h, w in SIZES[S]:
        out |= form_branches(h, w, S)
    return out
