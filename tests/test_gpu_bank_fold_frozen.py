"""The online log-sum-exp fold that neglabel.hip, vim.hip and glmcm.hip share (bank_sim.hpp lse_fold, lse_merge and the open
pairs behind the tile), frozen for the two scores tests/test_gpu_bank_walk_frozen.py does not hold: the ViM score and the GL-MCM
local score on unit-norm inputs must give, bit for bit, what the commit before the fold was shared gave on an MI355X
(tests/golden/bank_fold_frozen.npz, recorded there by tests/golden/make_bank_walk_frozen.py --which fold).  Unit rows, not
lattices, for the reason given there: on a lattice every summation order gives the same bits.
Common: widths 512, and 100 for a ragged last 32-column chunk; T in {0.01, 1.0}.
ViM: 70 queries (a second query tile of 6 rows), splits in {1, 3}, off given and None, alpha = 1.5, the parts returned.  Two banks
of 595 rows (three tiles, the last ragged): (K, R) = (70, 525), the cut inside the first tile; (300, 295): with three splits of
199 rows the prompts span splits 0 and 1 and the basis spans splits 1 and 2, and row 300, the cut, lies inside tile 256..454 of
the one-split walk and inside split 1's first tile.
GL-MCM local: 3 images of 49 rows = 147 query rows (three query tiles, the last of 19 rows; images straddle tiles), 600 prompts
(three tiles, the last ragged), the patch values returned.
An output larger than 4 KiB is held by the SHA-256 of its bytes."""
import os

import numpy as np
import pytest

from tests import glmcm_budget as gb
from tests import vim_budget as vb
from tests.test_gpu_bank_walk_frozen import _bits, _dev, _net, _put

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bank_fold_frozen.npz")
REGENERATE = ("to regenerate: check out the commit whose bits are to be kept, build it, and run "
              "`python tests/golden/make_bank_walk_frozen.py --which fold --commit HASH` there on an MI355X (with this module, "
              "tests/test_gpu_bank_walk_frozen.py and that script copied in)")
WIDTHS = [512, 100]
TEMPS = [0.01, 1.0]
B_VIM, VIM_BANKS, SPLITS, ALPHA = 70, [(70, 525), (300, 295)], [1, 3], 1.5
B_GLM, R_GLM, K_GLM = 3, 49, 600


def frozen_outputs():
    """{name: int32 view (or digest) of an output} over every case, as the library in the tree computes them."""
    out = {}
    for P in WIDTHS:
        net = _net(P)
        try:
            for K, R in VIM_BANKS:
                f, bank = vb.unit_case(B_VIM, K, R, P, seed=P + K)
                fd, bd = _dev(f), _dev(bank)
                for off in (None, torch.from_numpy(vb.lattice_off(R, seed=P + K))):
                    for T in TEMPS:
                        for splits in SPLITS:
                            s, p = net.vim_scores(fd, bd, K, T=T, alpha=ALPHA, off=off, splits=splits, return_parts=True)
                            name = f"vim/P{P}/K{K}/{'off' if off is not None else 'nooff'}/T{T}/S{splits}"
                            _put(out, name + "/scores", _bits(s))
                            _put(out, name + "/parts", _bits(p))
            local, text, _, _ = gb.unit_case(B_GLM, R_GLM, K_GLM, P, seed=P)
            ld, td = _dev(local), _dev(text)
            for T in TEMPS:
                s, p = net.local_scores(ld, td, T=T, return_patches=True)
                _put(out, f"glmcm/P{P}/T{T}/scores", _bits(s))
                _put(out, f"glmcm/P{P}/T{T}/patches", _bits(p))
        finally:
            net.close()
    return out


def test_vim_and_local_scores_keep_the_recorded_bits():
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
    print(f"FROZEN bank fold: {len(names)} arrays bit-equal to the recorded ones")
