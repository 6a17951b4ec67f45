"""Golden cases of the rational-quadratic spline through the REFERENCE's own layer (build container only):

    python tests/golden/make_golden_spline.py

Imports layers/activations.py SplineActivation from the reference and runs it on the CPU for the configurations of
tests/spline_cases.py (shared and individual weights, 5 and 8 bins, tail_bound 10 and 3).  The parameters are drawn at UNIT scale
(randn as fp32 values; the constructor's 0.01 * randn makes the spline the identity to four digits, which tests nothing) and the
inputs are 6 * randn with planted elements: exactly +-tail_bound, exactly 0, +-1.2 tail_bound, and one element inside every bin,
chosen from the float64 knots.  Recorded in float64 and float32: `forward`, its log-det, `reverse(forward)`.  Recorded in float64
only: autograd's gradients of (out * r).sum() + (logdet * s).sum() for the input and the three parameters.  Checked here: the
reference runs these inputs as they stand (it masks before it range-checks, so +-tail_bound and beyond raise nothing), and its float64
round trip is within 2e-12.  Arrays only, one .npz.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fastflow"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
from spline_cases import CONFIGS, GOLDEN, knots64, planted_inputs  # noqa: E402

import torch  # noqa: E402
from layers.activations import SplineActivation  # noqa: E402

torch.set_num_threads(1)


def layer(shape, K, tb, individual, params, dtype):
    m = SplineActivation(shape[1:], n_bins=K, tail_bound=tb, individual_weights=individual).to(dtype)
    with torch.no_grad():
        for p, v in zip((m.unnormalized_widths, m.unnormalized_heights, m.unnormalized_derivatives), params):
            p.copy_(torch.from_numpy(v).to(dtype).reshape(p.shape))
    return m


def make(seed, name, arrays):
    shape, K, tb, individual = CONFIGS[name]
    rng = np.random.default_rng(seed)
    lead = (1, *shape[1:]) if individual else ()
    params = [rng.standard_normal(lead + (n,)).astype(np.float32) for n in (K, K, K - 1)]
    x = planted_inputs(rng, shape, knots64(*params, tb)[0], tb)
    r = rng.standard_normal(shape).astype(np.float32)
    s = rng.standard_normal(shape[0]).astype(np.float32)
    out = dict(uw=params[0], uh=params[1], ud=params[2], x=x, r=r, s=s)
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        m = layer(shape, K, tb, individual, params, dtype)
        with torch.no_grad():
            y, ld = m(torch.from_numpy(x).to(dtype))
            rev = m.reverse(y)
        out.update({"y" + tag: y.numpy(), "logdet" + tag: ld.numpy(), "rev" + tag: rev.numpy()})
    assert np.abs(out["rev64"] - x.astype(np.float64)).max() <= 2e-12, name
    m = layer(shape, K, tb, individual, params, torch.float64)
    leaf = torch.from_numpy(x).double().requires_grad_(True)
    y, ld = m(leaf)
    ((y * torch.from_numpy(r).double()).sum() + (ld * torch.from_numpy(s).double()).sum()).backward()
    out.update(grad_x=leaf.grad.numpy(), grad_uw=m.unnormalized_widths.grad.numpy(), grad_uh=m.unnormalized_heights.grad.numpy(),
               grad_ud=m.unnormalized_derivatives.grad.numpy())
    print(name, "fp32 vs float64: y %.2e logdet %.2e round trip %.2e" % (
        np.abs(out["y32"] - out["y64"]).max(), np.abs(out["logdet32"] - out["logdet64"]).max(), np.abs(out["rev32"] - x).max()))
    arrays.update({f"{name}/{k}": v for k, v in out.items()})


if __name__ == "__main__":
    arrays = {}
    for seed, name in enumerate(CONFIGS):
        make(100 + seed, name, arrays)
    path = os.path.join(OUT, GOLDEN)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path) // 1024, "KiB")
