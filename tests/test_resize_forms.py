"""CPU side of the Resize + CenterCrop size sweep (tests/resize_forms.py): the C oracle equals a Pillow-only restatement of
torchvision's transform at every crop size, image size and content the GPU tests run; the size tables reach every branch of
the kernel's form choice that is reachable at their S (a table that stops covering a branch fails here, without a GPU);
prep_geometry() agrees with the oracle and with the rules pinned in tests/test_preprocess_oracle.py.  Integer work: every
comparison is exact."""
import ctypes

import numpy as np
import pytest

from tests import resize_forms as rf

PIL = pytest.importorskip("PIL")


@pytest.mark.parametrize("S", sorted(rf.SIZES))
def test_oracle_equals_pillow_on_every_table_entry_and_content(S):
    from oracle import oracle as orc

    rng = np.random.default_rng(1000 + S)
    n = 0
    for h, w in rf.SIZES[S]:
        for kind in rf.CONTENT_KINDS:
            img = rf.content(kind, h, w, rng)
            np.testing.assert_array_equal(orc.resize_crop_u8(img, S), rf.pillow_resize_crop(img, S), err_msg=f"S={S} {h}x{w} {kind}")
            n += 1
    assert n == len(rf.SIZES[S]) * len(rf.CONTENT_KINDS)


def test_contents_are_what_they_say():
    rng = np.random.default_rng(0)
    for kind in rf.CONTENT_KINDS:
        a = rf.content(kind, 5, 7, rng)
        assert a.shape == (5, 7, 3) and a.dtype == np.uint8, kind
    assert (rf.content("c100", 3, 3, rng) == 100).all() and (rf.content("c255", 3, 3, rng) == 255).all()
    assert not rf.content("c0", 3, 3, rng).any()
    c = rf.content("checker", 4, 4, rng)
    assert c[0, 0].tolist() == [0, 255, 0] and c[0, 1].tolist() == [255, 0, 255] and c[1, 0].tolist() == [255, 0, 255]
    s = rf.content("stripes", 2, 6, rng)
    assert s[0, :, 0].tolist() == [255, 0, 0, 255, 0, 0] and s[1, :, 1].tolist() == [0, 0, 255, 0, 0, 255]
    assert set(np.unique(rf.content("extremes", 16, 16, rng)).tolist()) == {0, 255}


# at least these, per crop size (the kernel's choices all depend on S: taps, rows per pass, window stride)
MUST_REACH = {
    64: {"copy", "fused-taps", "T8-rs8", "T16-rs8", "T16-rs4"},
    84: {"copy", "fused-taps", "T8-rs8", "T16-rs8", "T16-rs4", "T16-rs2"},
    224: {"copy", "fused-taps", "T8-rs8", "T8-rs4", "T16-rs4", "T16-rs2", "T16-rs1", "T16-nofit"},
    336: {"copy", "fused-taps", "T8-rs8", "T8-rs4", "T8-rs2", "T16-rs2", "T16-rs1", "T16-nofit"},
}


@pytest.mark.parametrize("S", sorted(rf.SIZES))
def test_table_reaches_every_reachable_branch(S):
    got = rf.branches_of_table(S)
    print(f"S={S}: table reaches {sorted(got)}")
    assert got == rf.EXPECTED_BRANCHES[S]
    assert got >= MUST_REACH.get(S, set())
    if S % 4:
        assert all(b in ("copy", "fused-taps") or b.startswith("fused-T") for b in got)
    # nothing else is reachable: every short side up to 8.6 x S (past 7 x S everything is `fused-taps`) at S <= 84, every third
    # at 224, every fourth at 336, and S itself (the only short side that is not resampled), x aspects 1 .. 4, both orientations
    reach = set()
    for s in sorted(set(range(1, int(8.6 * S) + 1, 1 if S <= 84 else (3 if S <= 224 else 4))) | {S}):
        for asp in (1.0, 1.01, 1.1, 1.25, 4.0 / 3.0, 1.5, 2.0, 3.0, 4.0):
            lng = max(s, int(round(s * asp)))
            reach |= rf.form_branches(s, lng, S) | rf.form_branches(lng, s, S)
    assert reach == got, (sorted(reach - got), sorted(got - reach))


def test_8_tap_tables_never_need_2_rows_per_pass_at_224():
    """Every short side whose filters fit 8 taps at S = 224 (scale factor up to 3), three aspects, both orientations: four rows
    per pass always fit the LDS budget, so `T8-rs2` (and below) does not exist at 224 — 17 source rows of at most
    2080 + 672 bytes are 46.8 KB of the 56.  At 336 it does (the table holds such an image)."""
    seen = set()
    for s in range(1, 3 * 224 + 1):
        for asp in (1.0, 4.0 / 3.0, 4.0):
            lng = max(s, int(round(s * asp)))
            for hw in ((s, lng), (lng, s)):
                seen |= rf.form_branches(*hw, 224)
    # (a long side just past 3 x its resized length takes 16-tap tables: int() shortens the resized long side)
    assert {b for b in seen if b.startswith("T8")} == {"T8-rs8", "T8-rs4"}, seen


def test_form_choice_by_hand():
    """A few choices worked out by hand from preprocess.hip."""
    assert rf.form_branches(224, 224, 224) == {"copy"}
    assert rf.form_branches(224, 301, 224) == {"copy"}                 # crop only
    assert rf.form_branches(112, 112, 224) == {"T8-rs8"}               # upscaling: 3 taps, a 10-row window of 2 * 672-byte rows
    assert rf.form_branches(1569, 1569, 224) == {"fused-taps"}         # scale 7.004: 2 * 8 + 1 taps
    assert rf.form_branches(1568, 1568, 224) == {"T16-nofit"}          # scale 7: 15 taps, and 17 source rows of 5.4 KB
    assert rf.form_branches(672, 672, 224) <= {"T8-rs8", "T8-rs4"}     # scale 3: 7 taps
    assert all(b.startswith("T16") for b in rf.form_branches(673, 673, 224))   # scale 3.004: 9 taps
    assert rf.form_branches(300, 300, 70) == {"fused-T16"} and rf.form_branches(140, 140, 70) == {"fused-T8"}
    with pytest.raises(ValueError):
        rf.form_branches(7200, 7100, 224)                              # scale factor above 31


def test_resample_limits_equal_pillows_window():
    """(first tap, taps) against a literal scalar transcription of Resample.c precompute_coeffs."""
    for in_size, out_size in ((500, 224), (224, 500), (1635, 224), (2452, 336), (21, 84), (1, 70), (700, 22400)):
        first, count = (0, out_size) if out_size < 1000 else (out_size // 2 - 32, 64)
        xmin, n = rf.resample_limits(in_size, out_size, first, count)
        scale = in_size / out_size
        support = max(scale, 1.0)
        for i in range(count):
            center = (first + i + 0.5) * scale
            lo = max(int(center - support + 0.5), 0)
            hi = min(int(center + support + 0.5), in_size)
            assert (int(xmin[i]), int(n[i])) == (lo, hi - lo), (in_size, out_size, first + i)
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()   # what lds_form's window relies on


def test_prep_geometry_agrees_with_the_oracle_and_the_pinned_rules():
    from oracle import oracle as orc

    def orc_size(h, w, s):
        nh, nw = ctypes.c_int32(), ctypes.c_int32()
        orc.lib().orc_resized_size(h, w, s, ctypes.byref(nh), ctypes.byref(nw))
        return nh.value, nw.value

    # tests/test_preprocess_oracle.py::test_resized_size_rules / test_identity_and_crop_only
    assert rf.prep_geometry(375, 500, 224)[:2] == (224, 298)
    assert rf.prep_geometry(500, 333, 224)[:2] == (336, 224)
    assert rf.prep_geometry(224, 300, 224)[:2] == (224, 300)
    assert rf.prep_geometry(64, 48, 224)[:2] == (298, 224)
    assert rf.prep_geometry(231, 517, 224)[:2] == (224, 501)
    assert rf.prep_geometry(224, 301, 224) == (224, 301, 0, 38)   # 38.5 -> 38 (half to even)
    assert rf.prep_geometry(299, 224, 224) == (299, 224, 38, 0)   # 37.5 -> 38
    rng = np.random.default_rng(9)
    cases = [(h, w, S) for S in rf.SIZES for h, w in rf.SIZES[S]]
    cases += [(int(rng.integers(1, 900)), int(rng.integers(1, 900)), int(S)) for S in (64, 70, 84, 224, 336) for _ in range(40)]
    for h, w, S in cases:
        nh, nw, top, left = rf.prep_geometry(h, w, S)
        assert (nh, nw) == orc_size(h, w, S), (h, w, S)
        assert min(nh, nw) == S and 0 <= top <= nh - S and 0 <= left <= nw - S
        assert top == int(round((nh - S) / 2.0)) and left == int(round((nw - S) / 2.0))
    # the crop origin, where nothing is resampled: the oracle's crop is the source window prep_geometry names
    for (h, w), S in (((64, 90), 64), ((70, 99), 70), ((85, 84), 84), ((300, 84), 84), ((337, 336), 336), ((224, 301), 224)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw, top, left = rf.prep_geometry(h, w, S)
        assert (nh, nw) == (h, w)
        out = orc.resize_crop_u8(img, S)
        assert out.shape == (S, S, 3)
        np.testing.assert_array_equal(out, img[top:top + S, left:left + S])


def test_prep_ring_is_read_from_the_library_source():
    assert rf.prep_ring() == 4   # what tests/test_gpu_preprocess_sizes.py::test_ring_reuse_without_synchronisation states
