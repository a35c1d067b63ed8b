"""The bank walk that knn.hip and neglabel.hip share (bank_sim.hpp), frozen: both scores on unit-norm inputs must give, bit for
bit, what the commit before the walk was shared gave on an MI355X (tests/golden/bank_walk_frozen.npz, recorded there by
tests/golden/make_bank_walk_frozen.py).  Unit rows, not lattices: on a lattice every summation order gives the same bits, so the
exact tests of tests/test_gpu_knn.py would not notice a changed MFMA order or staging; here any change of either moves low bits.
Shapes: 70 queries (a second query tile of 6 rows); 600 bank rows for k-NN and 70 + 7 * 75 = 595 for NegLabel (three tiles, the
last ragged; ranges across tile edges and, with three splits, across split edges); k = 300 is more than the 200 rows of a split
(the -inf tail).  Widths: 512, and 100 for a ragged last 32-column chunk: every width tests/test_gpu_knn.py and
tests/test_gpu_neglabel.py build nets for (64, 512, 768, 1024) is a multiple of 32, so the ragged one is the 100 of
tests/test_gpu_maha_fit.py.  An output larger than 4 KiB (the k = 300 lists) is held by the SHA-256 of its bytes."""
import dataclasses
import hashlib
import os

import numpy as np
import pytest

from tests import knn_budget as kb
from tests import neglabel_budget as nb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bank_walk_frozen.npz")
REGENERATE = ("to regenerate: check out the commit whose bits are to be kept, build it, and run "
              "`python tests/golden/make_bank_walk_frozen.py --commit HASH` there on an MI355X (with this module and that script "
              "copied in)")
WIDTHS = [512, 100]
B, N_KNN, KS = 70, 600, [5, 300]
K, G, GS = 70, 7, 75
SPLITS = [1, 3]
TEMPS = [0.01, 1.0]


def _net(P):
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry("tiny")
    if P != geo.proj_dim:
        geo = dataclasses.replace(geo, name=f"tiny-P{P}", proj_dim=P)
    return NativeCLIP(geo, synth_state_dict(geo, 0), precision="fp16", max_batch=8, max_prompt_tokens=256)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy()).view(np.int32)


def _put(out, name, bits):
    if bits.nbytes <= 4096:
        out[name] = bits
    else:
        out[name + "/sha256"] = np.frombuffer(hashlib.sha256(bits.tobytes()).digest(), dtype=np.uint8)


def frozen_outputs():
    """{name: int32 view (or digest) of an output} over every case, as the library in the tree computes them."""
    out = {}
    for P in WIDTHS:
        net = _net(P)
        try:
            f, bank = kb.unit_case(B, N_KNN, P, seed=P)
            fd, bd = _dev(f), _dev(bank)
            for k in KS:
                for splits in SPLITS:
                    s, v = net.knn_scores(fd, bd, k, splits=splits, return_values=True)
                    _put(out, f"knn/P{P}/k{k}/S{splits}/scores", _bits(s))
                    _put(out, f"knn/P{P}/k{k}/S{splits}/topv", _bits(v))
            f, bank = nb.unit_case(B, K, G, GS, P, seed=P)
            fd, bd = _dev(f), _dev(bank)
            for T in TEMPS:
                for splits in SPLITS:
                    s, g = net.neglabel_scores(fd, bd, K, G, GS, T=T, splits=splits, return_groups=True)
                    _put(out, f"neglabel/P{P}/T{T}/S{splits}/scores", _bits(s))
                    _put(out, f"neglabel/P{P}/T{T}/S{splits}/groups", _bits(g))
        finally:
            net.close()
    return out


def test_both_scores_keep_the_recorded_bits():
    want = np.load(FIXTURE)
    got = frozen_outputs()
    made_with = (f"(fixture made at commit {want['commit'].item()} with ROCm {want['rocm'].item()}; this is ROCm "
                 f"{torch.version.hip}; {REGENERATE})")
    names = sorted(n for n in want.files if n not in ("rocm", "commit"))
    assert names == sorted(got), made_with
    for name in names:
        w, g = want[name], got[name]
        assert w.dtype == g.dtype and w.shape == g.shape, (name, made_with)
        assert np.array_equal(w, g), (name, int((w != g).sum()), "element(s) differ", made_with)
    print(f"FROZEN bank walk: {len(names)} arrays bit-equal to the recorded ones")
