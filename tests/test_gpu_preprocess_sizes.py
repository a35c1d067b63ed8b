"""mcm_resize_crop_u8 against the C oracle (== Pillow: tests/test_resize_forms.py) at every crop size, form and content:
S = 64, 224, 336 (shipped), 70 (S % 4 != 0: fused form only, last row group of 6) and 84 (S % 8 == 4: LDS form with a last row
group of 4), on the size tables of tests/resize_forms.py, which reach every branch of the kernel's form choice at their S, and
on constant, saturated and alternating 0 / 255 images next to random bytes.  Also: the fused form forced on images the LDS
form takes (harness library), packed sources at every byte alignment, the staging ring past its length without a
synchronisation, a full batch.  Integer work: every comparison is bit-exact.  The towers never run here."""
import dataclasses

import numpy as np
import pytest

from tests import resize_forms as rf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_BATCH = 16
_cache = {}


def _case(S, kind, h, w, salt=0):
    """(image, oracle crop) of one table entry; computed once, shared by every test, never written to."""
    key = (S, kind, h, w, salt)
    if key not in _cache:
        from oracle import oracle as orc

        seed = [S, rf.CONTENT_KINDS.index(kind), h, w, salt]
        img = rf.content(kind, h, w, np.random.default_rng(seed))
        ref = orc.resize_crop_u8(img, S)
        img.setflags(write=False)
        ref.setflags(write=False)
        _cache[key] = (img, ref)
    return _cache[key]


def _geo(S):
    from mcm_amd.config import geometry

    if S == 64:
        return geometry("tiny")
    if S == 224:
        return geometry("B16-2L")
    return dataclasses.replace(geometry("tiny"), name=f"tiny-{S}", image_size=S, patch_size=14)


@pytest.fixture(scope="module")
def handle():
    """handle(S, harness=False): one NativeCLIP per crop size and library, made on first use, closed with the module."""
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    nets = {}

    def get(S, harness=False):
        if (S, harness) not in nets:
            geo = _geo(S)
            nets[(S, harness)] = NativeCLIP(geo, synth_state_dict(geo, seed=0), precision="bf16", max_batch=MAX_BATCH,
                                            max_prompt_tokens=1024, harness=harness)
        return nets[(S, harness)]

    yield get
    for n in nets.values():
        n.close()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # (a copy: the shared inputs are read-only)


def _run_table(net, S, kind):
    cases = [_case(S, kind, h, w) for h, w in rf.SIZES[S]]
    assert len(cases) <= MAX_BATCH
    out = net.resize_crop([_dev(img) for img, _ in cases]).cpu().numpy()   # one launch: LDS-form, fused-form and copy images
    assert out.shape == (len(cases), S, S, 3) and out.dtype == np.uint8
    return out, cases


@pytest.mark.parametrize("kind", rf.CONTENT_KINDS)
@pytest.mark.parametrize("S", sorted(rf.SIZES))
def test_every_size_and_content_matches_oracle(handle, S, kind):
    out, cases = _run_table(handle(S), S, kind)
    for (h, w), (_, ref), got in zip(rf.SIZES[S], cases, out):
        np.testing.assert_array_equal(got, ref, err_msg=f"S={S} {h}x{w} {kind} {sorted(rf.form_branches(h, w, S))}")


@pytest.mark.parametrize("S", [64, 84, 224, 336])
def test_fused_form_equals_lds_form(handle, S):
    """The fused form on every image of the table, also those the LDS form takes by default (harness switch
    mcm_debug_resize_fused_only), and the default choice: both the oracle's bytes, so each other's."""
    net = handle(S, harness=True)
    lib = net._lib
    assert any(b.startswith("T") and not b.endswith("nofit") for b in rf.branches_of_table(S))   # the switch changes something
    try:
        for kind in rf.CONTENT_KINDS:
            lib.mcm_debug_resize_fused_only(1)
            fused, cases = _run_table(net, S, kind)
            lib.mcm_debug_resize_fused_only(0)
            lds, _ = _run_table(net, S, kind)
            for (h, w), (_, ref), a, b in zip(rf.SIZES[S], cases, fused, lds):
                np.testing.assert_array_equal(a, ref, err_msg=f"fused form S={S} {h}x{w} {kind}")
                np.testing.assert_array_equal(b, ref, err_msg=f"default choice S={S} {h}x{w} {kind}")
                np.testing.assert_array_equal(a, b, err_msg=f"fused vs default S={S} {h}x{w} {kind}")
    finally:
        lib.mcm_debug_resize_fused_only(0)


PACKED = {   # the small and medium entries of the tables, twice over where 16 images need it
    84: [(21, 21), (277, 277), (411, 411), (537, 537), (84, 84), (613, 613), (85, 84), (300, 84)],
    336: [(84, 84), (772, 772), (974, 974), (1108, 1108), (336, 336), (337, 336), (1008, 1018), (1411, 1411)],
}


@pytest.mark.parametrize("S", sorted(PACKED))
def test_packed_images_at_every_alignment_match_oracle(handle, S):
    """tests/test_gpu_preprocess.py::test_packed_images_at_unaligned_offsets_match_oracle at S = 336 and 84: 16 images back to
    back in one allocation, image i at an offset of residue (1 + i) mod 16 (every residue; the first one byte into the
    allocation), the last one ending it, the bytes between images non-zero."""
    sizes = PACKED[S] + PACKED[S]
    assert len(sizes) == 16 == MAX_BATCH
    cases = [_case(S, rf.CONTENT_KINDS[i % len(rf.CONTENT_KINDS)], h, w, salt=1 + i // 8) for i, (h, w) in enumerate(sizes)]
    offsets, cur = [], 1
    for i, (img, _) in enumerate(cases):
        cur += (1 + i - cur) % 16             # a gap of 0 .. 15 bytes
        offsets.append(cur)
        cur += img.size
    host = np.random.default_rng(S).integers(1, 256, cur, dtype=np.uint8)
    for o, (img, _) in zip(offsets, cases):
        host[o:o + img.size] = img.reshape(-1)
    assert offsets[0] == 1 and offsets[-1] + cases[-1][0].size == host.size and {o % 16 for o in offsets} == set(range(16))
    out = handle(S).resize_crop_packed(torch.from_numpy(host).cuda(), offsets, [h for h, _ in sizes],
                                       [w for _, w in sizes]).cpu().numpy()
    for i, ((h, w), (_, ref), got) in enumerate(zip(sizes, cases, out)):
        np.testing.assert_array_equal(got, ref, err_msg=f"S={S} image {i} {h}x{w} at offset {offsets[i]}")


def test_ring_reuse_without_synchronisation(handle):
    """mcm_resize_crop_u8 rotates its pinned geometry records and per-slot coefficient tables over PREP_RING = 4 slots.
    2 * PREP_RING + 1 = 9 calls back to back on one stream, nothing synchronised in between, each with its own mix of
    sizes, batch size and output: call k runs the S = 224 table rotated by k places, so that a record (and its coefficient
    table) that held an LDS-form image is a `fused-taps` image's the next time its slot comes round, and the reverse."""
    ring = rf.prep_ring()
    assert ring == 4   # as the docstring states it; the mixes below are built from whatever it is
    S, table = 224, rf.SIZES[224]
    n = len(table)
    mixes = [[table[(b + k) % n] for b in range(n - k % 3)] for k in range(2 * ring + 1)]

    def lds(hw):
        return all(b.startswith("T") and not b.endswith("nofit") for b in rf.form_branches(*hw, S))

    def fused(hw):
        return rf.form_branches(*hw, S) == {"fused-taps"}

    pairs = [(mixes[k][b], mixes[k + ring][b]) for k in range(ring + 1) for b in range(min(len(mixes[k]), len(mixes[k + ring])))]
    assert any(lds(a) and fused(b) for a, b in pairs) and any(fused(a) and lds(b) for a, b in pairs)
    assert len({tuple(m) for m in mixes}) == len(mixes)
    net = handle(S)
    dev = {hw: _dev(_case(S, "rand", *hw)[0]) for hw in table}
    net.resize_crop([dev[table[0]]])    # the first call of a handle allocates (synchronously): not part of the run
    torch.cuda.synchronize()
    outs = [net.resize_crop([dev[hw] for hw in mix]) for mix in mixes]   # back to back
    torch.cuda.synchronize()
    for k, (mix, out) in enumerate(zip(mixes, outs)):
        got = out.cpu().numpy()
        for b, hw in enumerate(mix):
            np.testing.assert_array_equal(got[b], _case(S, "rand", *hw)[1], err_msg=f"call {k} image {b} {hw}")


def test_full_batch_and_single_image_at_336(handle):
    S, table = 336, rf.SIZES[336]
    net = handle(S)
    sizes = [table[i % len(table)] for i in range(MAX_BATCH)]
    cases = [_case(S, "rand" if i < len(table) else "extremes", h, w) for i, (h, w) in enumerate(sizes)]
    assert len(cases) == net.max_batch
    out = net.resize_crop([_dev(img) for img, _ in cases]).cpu().numpy()
    for i, ((h, w), (_, ref)) in enumerate(zip(sizes, cases)):
        np.testing.assert_array_equal(out[i], ref, err_msg=f"image {i} {h}x{w}")
    for hw in ((974, 974), (2452, 2452)):
        img, ref = _case(S, "rand", *hw)
        np.testing.assert_array_equal(net.resize_crop([_dev(img)]).cpu().numpy()[0], ref, err_msg=f"alone: {hw}")
