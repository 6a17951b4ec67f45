"""Inputs and the float64 reference of the PLU-parametrised 1x1 convolution (glow.Conv1x1LU), shared by
tests/test_plu_host.py and tests/test_gpu_plu.py.  A helper, not collected.

The reference has no such layer: the yardstick is float64 autograd on the CPU through the written-out composition (`ref64`), with
`torch.inverse` and `torch.slogdet` of the composed matrix as independent checks of W^-1 and the log-det.  Inputs: the constructor's
factorisation of the orthogonal matrix it draws, plus 0.05 N(0,1) on the strict triangles and 0.1 N(0,1) on log_s from a seeded
generator -- at C = 192 (cond(W) about 2,000) the float32 PyTorch lines stay within 2.6e-6 of float64 in helpers.rel_err, at C <= 96
within 9e-7 -- and the unperturbed initialisation, where W is the drawn matrix again."""
import numpy as np
import torch

from helpers import rel_err, report

BAR = 1e-5          # the project's bar for every kernel (helpers.rel_err)


def make_layer(C, perturb=True, seed=0):
    """A fresh glow.Conv1x1LU on the CPU in float32 (np.random seeded per width)."""
    from fincflow_amd import glow
    np.random.seed(1000 + C + seed)
    m = glow.Conv1x1LU(C)
    if perturb:
        g = torch.Generator().manual_seed(77 + C + seed)
        with torch.no_grad():
            m.lower.add_(0.05 * torch.randn(C, C, generator=g).tril(-1))
            m.upper.add_(0.05 * torch.randn(C, C, generator=g).triu(1))
            m.log_s.add_(0.1 * torch.randn(C, generator=g))
    return m


def factors(m):
    return m.lower, m.upper, m.log_s, m.sign_s, m.perm


def ref64(lower, upper, log_s, sign_s, perm):
    """(w, w_inv, logdet) in float64 on the CPU, differentiable in lower, upper, log_s: the composition written out, W^-1 and the
    log-det from the dense matrix."""
    C = log_s.numel()
    eye = torch.eye(C, dtype=torch.float64)
    L = torch.tril(lower, -1) + eye
    Ut = torch.triu(upper, 1) + torch.diag(sign_s * torch.exp(log_s))
    w = (L @ Ut)[perm.long()]
    return w, torch.inverse(w), torch.slogdet(w)[1]


def leaves64(m):
    """The layer's five tensors on the CPU, the parameters as float64 leaves."""
    lower, upper, log_s = (p.detach().cpu().double().requires_grad_(True) for p in (m.lower, m.upper, m.log_s))
    return lower, upper, log_s, m.sign_s.detach().cpu().double(), m.perm.detach().cpu()


def judge(case, names, got, want, bar=BAR, **fields):
    """helpers.rel_err per tensor against float64, every figure printed and appended to the parity report (kind `plu`) before the
    assertion."""
    errs = {}
    for n, g, w in zip(names, got, want):
        g, w = g.detach().cpu().double().numpy(), w.detach().cpu().double().numpy()
        assert g.shape == w.shape, (n, g.shape, w.shape)
        errs[n] = rel_err(g, w) if np.any(w) else (0.0 if not np.any(g) else float("inf"))
    worst = max(errs, key=errs.get)
    report("plu", case=case, worst=errs[worst], at=worst, bar=bar, **fields)
    print("plu %s %s: %s" % (case, fields, {n: "%.2e" % e for n, e in errs.items()}))
    assert all(e <= bar for e in errs.values()), (case, fields, errs, bar)
    return errs
