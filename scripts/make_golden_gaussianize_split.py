#!/usr/bin/env python3
"""tests/golden/gaussianize_split.npz: the reference's own `Split(12)` (fastflow/layers/split.py) in float64 on a [2, 12, 4, 5] input
-- randomised weights, the input, x1, z2, logdet and the inverse of (x1, z2).  `make_golden_gaussianize_split.py REFERENCE_ROOT`;
the reference's module is imported by path, nothing of it is copied.  tests/test_gauss_split_host.py reads the file."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(root):
    spec = importlib.util.spec_from_file_location("reference_split", os.path.join(root, "fastflow", "layers", "split.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gen = torch.Generator().manual_seed(116)
    layer = mod.Split(12).double()
    with torch.no_grad():
        for name, p in layer.named_parameters():       # 0.05, and 0.1 for the bias and the log-scale: exp(+-logs) stays O(1)
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * (0.1 if name.endswith(("bias", "log_scale_factor")) else 0.05))
        x = torch.randn(2, 12, 4, 5, generator=gen, dtype=torch.float64)
        x1, z2, logdet = layer(x)
        back, logdet_inv = layer.inverse(x1, z2)
    assert float((back - x).abs().max()) <= 1e-14 and float((logdet + logdet_inv).abs().max()) <= 1e-12
    out = {"state." + k: v.numpy() for k, v in layer.state_dict().items()}
    out.update(x=x.numpy(), x1=x1.numpy(), z2=z2.numpy(), logdet=logdet.numpy(), inverse=back.numpy())
    path = os.path.join(REPO, "tests", "golden", "gaussianize_split.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", sorted(out))


if __name__ == "__main__":
    main(sys.argv[1])
