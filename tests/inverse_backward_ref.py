"""The fp64 CPU reference of the backward through the unit's inverse, shared by tests/test_inverse_backward_host.py and
tests/test_gpu_inverse_backward.py.

`solve` is a differentiable restatement of x = inverse(z): H + W - 1 sweeps of x <- L^-1 (z - N x), written from F.pad, F.conv2d,
torch.flip and einsum.  It is exact: N (every tap but the pixel's own) reads strictly earlier anti-diagonals, so sweep k fixes
anti-diagonal k - 1 for good.  Autograd through it is the reference for grad_z and for the gradients of the STORED banks.  The free
autograd gradient is non-zero on the corner tap's masked entries (the diagonal and above): compare under `stored_mask`.

`adjoint_identity` restates the library's route in numpy fp64: the adjoint bank, the complemented orientation, the
oracle's fp64 inverse, the lead product, minus the forward's weight gradient.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _flip(t, o):
    dims = [d for d, bit in ((3, 1), (2, 2)) if o & bit]
    return torch.flip(t, dims) if dims else t


def group_orient(orient, g):
    return (orient >> (2 * g)) & 3


def canonical(w_stored, G, orient):
    """[G*Cq, Cq, KH, KW] stored -> canonical, in the graph (torch.flip per group)."""
    Cq = w_stored.shape[0] // G
    return torch.cat([_flip(w_stored[g * Cq:(g + 1) * Cq], group_orient(orient, g)) for g in range(G)], 0)


def stored_mask(G, Cq, KH, KW, orient):
    """1 where a stored weight is trainable (layers/conv.py:81-96), as a float64 tensor [G*Cq, Cq, KH, KW]."""
    m = torch.ones(Cq, Cq, KH, KW, dtype=torch.float64)
    for c in range(Cq):
        m[c, c:, -1, -1] = 0.0
    return torch.cat([_flip(m, group_orient(orient, g)) for g in range(G)], 0)


def forward(x, w_stored, G, orient):
    """z = forward(x): per group, flip to canonical, pad the top-left corner, cross-correlate, flip back."""
    Cq = w_stored.shape[0] // G
    wc = canonical(w_stored, G, orient)
    KH, KW = wc.shape[2:]
    outs = []
    for g in range(G):
        o = group_orient(orient, g)
        xc = _flip(x[:, g * Cq:(g + 1) * Cq], o)
        outs.append(_flip(F.conv2d(F.pad(xc, (KW - 1, 0, KH - 1, 0)), wc[g * Cq:(g + 1) * Cq]), o))
    return torch.cat(outs, 1)


def solve(z, w_stored, G, orient):
    """x = inverse(z), differentiable in z and w_stored."""
    Cq = w_stored.shape[0] // G
    wc = canonical(w_stored, G, orient)
    KH, KW = wc.shape[2:]
    H, W = z.shape[2:]
    corner = torch.zeros(1, 1, KH, KW, dtype=wc.dtype)
    corner[..., -1, -1] = 1.0
    outs = []
    for g in range(G):
        o = group_orient(orient, g)
        w = wc[g * Cq:(g + 1) * Cq]
        eye = torch.eye(Cq, dtype=w.dtype)
        linv = torch.linalg.solve_triangular(w[:, :, -1, -1], eye, upper=False)
        w_rest = w * (1.0 - corner)
        zc = _flip(z[:, g * Cq:(g + 1) * Cq], o)
        x = torch.zeros_like(zc)
        for _ in range(H + W - 1):
            x = torch.einsum("oc,bchw->bohw", linv, zc - F.conv2d(F.pad(x, (KW - 1, 0, KH - 1, 0)), w_rest))
        outs.append(_flip(x, o))
    return torch.cat(outs, 1)


def reference_grads(z, w_stored, g_x, G, orient):
    """(x, grad_z, grad_w_stored) of <g_x, solve(z, w_stored)> by autograd, numpy fp64; grad_w is the FREE gradient (unmasked)."""
    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w_stored, dtype=np.float64), requires_grad=True)
    x = solve(zt, wt, G, orient)
    gz, gw = torch.autograd.grad(x, (zt, wt), torch.tensor(np.asarray(g_x, dtype=np.float64)))
    return x.detach().numpy(), gz.numpy(), gw.numpy()


def forward_vjp(x, w_stored, y, G, orient):
    """(grad_x, grad_w_stored) of the FORWARD conv at input x for grad_output y, numpy fp64 (free gradient)."""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    wt = torch.tensor(np.asarray(w_stored, dtype=np.float64), requires_grad=True)
    gx, gw = torch.autograd.grad(forward(xt, wt, G, orient), (xt, wt), torch.tensor(np.asarray(y, dtype=np.float64)))
    return gx.numpy(), gw.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the identity, in numpy fp64
# ---------------------------------------------------------------------------------------------------------------------
def adjoint_bank(w_canon, G):
    """(w_adj [G*Cq, Cq, KH, KW], lead_t [C, C]) in float64: what finc_adjoint_weights_f32 computes."""
    w = np.asarray(w_canon, dtype=np.float64)
    C, Cq, KH, KW = w.shape
    w_adj = np.zeros_like(w)
    lead_t = np.zeros((C, C))
    for g in range(G):
        wg = w[g * Cq:(g + 1) * Cq]                                    # [k][i][kh][kw]
        linv = np.linalg.inv(wg[:, :, -1, -1])                         # [o][k]
        a = np.einsum("kihw,ok->iohw", wg, linv)
        a[:, :, -1, -1] = np.eye(Cq)
        w_adj[g * Cq:(g + 1) * Cq] = a
        lead_t[g * Cq:(g + 1) * Cq, g * Cq:(g + 1) * Cq] = linv.T
    return w_adj, lead_t


def complement(orient, G):
    return orient ^ ((1 << (2 * G)) - 1)


def np_flip(a, o):
    if o & 1:
        a = a[..., ::-1]
    if o & 2:
        a = a[..., ::-1, :]
    return a


def adjoint_identity(z, w_stored, g_x, G, orient, inverse_f64):
    """(x, grad_z, grad_w_stored masked) by the library's route in float64.  `inverse_f64(t, w_canon, G)`: a canonical-orientation
    fp64 inverse (oracle.inverse_f64)."""
    ws = np.asarray(w_stored, dtype=np.float64)
    C, Cq, KH, KW = ws.shape
    wc = np.concatenate([np_flip(ws[g * Cq:(g + 1) * Cq], group_orient(orient, g)) for g in range(G)], 0)

    def inv(t, bank, orient_bits):
        tc = np.concatenate([np_flip(t[:, g * Cq:(g + 1) * Cq], group_orient(orient_bits, g)) for g in range(G)], 1)
        xc = inverse_f64(np.ascontiguousarray(tc), np.ascontiguousarray(bank), G)
        return np.concatenate([np_flip(xc[:, g * Cq:(g + 1) * Cq], group_orient(orient_bits, g)) for g in range(G)], 1)

    x = inv(np.asarray(z, dtype=np.float64), wc, orient)
    w_adj, lead_t = adjoint_bank(wc, G)
    v = inv(np.asarray(g_x, dtype=np.float64), w_adj, complement(orient, G))
    y = np.einsum("oc,bchw->bohw", lead_t, v)
    gw = -forward_vjp(x, ws, y, G, orient)[1] * stored_mask(G, Cq, KH, KW, orient).numpy()
    return x, y, gw
