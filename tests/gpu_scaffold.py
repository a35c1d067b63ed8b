"""What the GPU test modules share: the tiny geometry widened to a proj_dim and the cache of such handles, host -> device and
bit-view helpers, and the reporter of the fp64 error budgets.  A plain module: the fixtures stay in the test modules, under
their own names, and delegate here.  torch is imported where it is used, so importing this module needs no GPU."""
import ctypes
import dataclasses

import numpy as np
import pytest

from tests import error_budget as eb


def widened_net(P=None, geo="tiny", seed=0, precision="fp16", max_batch=8, max_prompt_tokens=256, **kw):
    """A NativeCLIP of the `geo` geometry with seeded weights, widened to proj_dim = P where P is given and differs."""
    from mcm_amd.config import geometry
    from mcm_amd.engine import NativeCLIP
    from mcm_amd.weights import synth_state_dict

    geo = geometry(geo)
    if P is not None and P != geo.proj_dim:
        geo = dataclasses.replace(geo, name=f"{geo.name}-P{P}", proj_dim=P)
    return NativeCLIP(geo, synth_state_dict(geo, seed), precision=precision, max_batch=max_batch,
                      max_prompt_tokens=max_prompt_tokens, **kw)


def net_cache(make=widened_net):
    """The body of a module-scoped fixture: yields get(key) -> make(key), one handle per key, all closed at teardown."""
    nets = {}

    def get(key):
        if key not in nets:
            nets[key] = make(key)
        return nets[key]

    yield get
    for n in nets.values():
        n.close()


def dev(a):
    """A host array as a contiguous fp32 device tensor."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    """The int32 view of a host array of 32-bit numbers."""
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b, rows=slice(None), keys=()):
    """Whether two dicts of host arrays hold the same bits under every key, in `rows`."""
    return all(np.array_equal(bits(a[k][rows]), bits(b[k][rows])) for k in keys)


def check_budget(what, prec, got, ref, bud, where="", finite_budget=False):
    """Print "BUDGET <what> <prec> <worst ratio> <where>", fail with the worst element where |got - ref| exceeds its budget, and
    return the ratio.  `finite_budget`: also require every budget to be finite."""
    if finite_budget:
        assert np.isfinite(bud).all(), f"{what} {prec} {where}: a non-finite budget"
    r, i = eb.worst(got, ref, bud)
    print(f"BUDGET {what} {prec} {r:.3f} {where}")
    if r > 1.0:
        idx = np.unravel_index(i, np.shape(ref))
        pytest.fail(f"{what} {prec} {where}: max|got - ref| / budget = {r:.3g} at {idx}: got "
                    f"{np.asarray(got).flat[i]!r} ref {ref.flat[i]!r} budget {bud.flat[i]:.3g}")
    return r
