"""Golden cases of the element-wise activations through the REFERENCE's own layers (build container only):

    python tests/golden/make_golden_activations.py

Imports layers/activations.py SmoothLeakyRelu, LeakyRelu, LearnableLeakyRelu and SmoothTanh from the reference and runs them on the
CPU at their default parameters, in float64 and float32, on [3, 2, 4, 5] inputs of 4 * randn with planted 0.0, -0.0, +-1e-6 and +-30
(tests/activation_cases.py): `forward`, its log-det, `reverse` of the forward's output and `reverse` of the inputs themselves, each
with the reference's 100 Newton steps.  Also recorded: SmoothTanh(3, 0.05).reverse of the inputs, in which the reference's
unbracketed iteration CYCLES -- a record of that, not a yardstick: the tests compare that case with float64 bisection and only report
the reference's figure.  Arrays only, one .npz.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/fastflow"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(OUT))
from activation_cases import GOLDEN, GOLDEN_SHAPE, KINDS, planted  # noqa: E402

import torch  # noqa: E402
from layers import activations as ref  # noqa: E402

torch.set_num_threads(1)
CLASSES = dict(zip(KINDS, (ref.SmoothLeakyRelu, ref.LeakyRelu, ref.LearnableLeakyRelu, ref.SmoothTanh)))

if __name__ == "__main__":
    rng = np.random.default_rng(7)
    x = planted((4 * rng.standard_normal(GOLDEN_SHAPE)).astype(np.float32))
    arrays = {"x": x}
    for kind, cls in CLASSES.items():
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            m = cls().to(dtype)
            v = torch.from_numpy(x).to(dtype)
            with torch.no_grad():
                y, ld = m(v)
                arrays.update({f"{kind}/y{tag}": y.numpy(), f"{kind}/logdet{tag}": ld.numpy(), f"{kind}/rev{tag}": m.reverse(y).numpy(),
                               f"{kind}/rev_of_x{tag}": m.reverse(v).numpy()})
        print(kind, "fp32 vs float64: y %.2e logdet %.2e round trip %.2e" % (
            np.abs(arrays[kind + "/y32"] - arrays[kind + "/y64"]).max(), np.abs(arrays[kind + "/logdet32"] - arrays[kind + "/logdet64"]).max(),
            np.abs(arrays[kind + "/rev32"] - x).max()))
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        with torch.no_grad():
            arrays["smooth_tanh_3_0.05/rev_of_x" + tag] = ref.SmoothTanh(3, 0.05).reverse(torch.from_numpy(x).to(dtype)).numpy()
    path = os.path.join(OUT, GOLDEN)
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path) // 1024, "KiB")
