"""Golden cases of ActNorm through the REFERENCE's own layer (build container only):

    python tests/golden/make_golden_actnorm.py

Imports layers/actnorm.py from the reference and runs it in float64 on the CPU: the data-dependent initialisation of the first
forward (layers/actnorm.py:17-23), `out` and `ldj` of that forward (:34, :57-65), `reverse(out)` (:51), and autograd's gradients
of sum(out * gy) + sum(ldj * gl) for the input and both parameters, taken on a second forward with the initialised parameters.
The inputs come from tests/actnorm_cases.py (integer-hash arithmetic, the same fp32 values everywhere) and are stored as fp32
(float64 copies of them are what the reference sees); everything else is float64.  The largest case stores its per-channel
results whole and its activation-sized ones for two images, with a checksum of the input that a test rebuilds.  Arrays only.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fastflow"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
from actnorm_cases import BIG, BIG_IMAGES, CASES, inputs  # noqa: E402

import torch  # noqa: E402
from layers.actnorm import ActNorm  # noqa: E402

torch.set_num_threads(1)

def make(name):
    x, gy, gl = (torch.from_numpy(a) for a in inputs(name))
    B, C, H, W = x.shape
    m = ActNorm(C).double()
    x64 = x.double()
    with torch.no_grad():
        out, ldj = m(x64)                                        # initialises
        rev = m.reverse(out)
    assert int(m.initialized) == 1
    leaf = x64.clone().requires_grad_(True)
    o2, l2 = m(leaf)
    ((o2 * gy.double()).sum() + (l2 * gl.double()).sum()).backward()
    keep = (lambda a: a[list(BIG_IMAGES)]) if name == BIG else (lambda a: a)
    arrays = dict(translation=m.translation.detach().numpy(), log_scale=m.log_scale.detach().numpy(), out=keep(out.numpy()),
                  ldj=ldj.numpy().copy(), rev=keep(rev.numpy()), gl=gl.numpy(), grad_x=keep(leaf.grad.numpy()),
                  grad_log_scale=m.log_scale.grad.numpy(), grad_translation=m.translation.grad.numpy(),
                  x_channel_sums=x64.sum(dim=(0, 2, 3)).numpy(), shape=np.asarray(x.shape))
    if name != BIG:
        arrays.update(x=x.numpy(), gy=gy.numpy())
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(name, os.path.getsize(path) // 1024, "KiB", "log_scale", arrays["log_scale"].min(), arrays["log_scale"].max())


if __name__ == "__main__":
    for name in CASES:
        make(name)
