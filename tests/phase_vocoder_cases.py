"""Shared by test_phase_vocoder_cpu.py and test_phase_vocoder_gpu.py: the float64 textbook phase vocoder (angles, wrap,
expected advance, cumsum: torchaudio.functional.phase_vocoder restated in the package's time-major layout), float64
restatements of what csrc/phase_vocoder.hip computes (the phasor product forward, the downward gather backward), the
spectra, the sweep and the metric."""
import math

import torch

RATES = (0.5, 0.8, 1 / 1.1, 1.3, 2.0, 3.0, 100.0)
BATCHES = (1, 2, 64, 65)          # 64: the threshold of the clip-per-block layout
BINS = (1, 257, 512, 513, 1025)
FRAMES = (1, 2, 9, 33)
TOL = 1e-5                        # the library's normwise bound; the fp32 phasor product is 1.4e-6 .. 3.1e-6 off at 690 frames


def normwise(a, b):
    """|| a - b || / || b || over all elements (complex or real)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    a = a.to(torch.complex128 if a.is_complex() else torch.float64)
    b = b.to(a.dtype)
    den = float(torch.linalg.vector_norm(b))
    return float(torch.linalg.vector_norm(a - b)) / (den if den > 0 else 1.0)


def spectrum(shape, seed):
    """complex-normal, complex64 (what the kernels read), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def steps(T, rate):
    """The step rule, written out: (idx list, alpha list in float64)"""
    idx, alpha, j = [], [], 0
    while j * float(rate) < T:
        s = j * float(rate)
        idx.append(int(math.floor(s)))
        alpha.append(s - math.floor(s))
        j += 1
    return idx, alpha


def textbook(X, rate, hop):
    """float64: X (..., T, F) complex128 -> (..., N, F) complex128.  Differentiable by torch autograd."""
    T, F = X.shape[-2], X.shape[-1]
    idx, alpha = steps(T, rate)
    i0 = torch.tensor(idx, dtype=torch.long)
    al = torch.tensor(alpha, dtype=torch.float64).unsqueeze(-1)
    advance = torch.linspace(0, math.pi * hop, F, dtype=torch.float64)
    phase_0 = X[..., :1, :].angle()
    Xp = torch.cat([X, torch.zeros(X.shape[:-2] + (2, F), dtype=X.dtype)], -2)
    X0, X1 = Xp.index_select(-2, i0), Xp.index_select(-2, i0 + 1)
    a0, a1, n0, n1 = X0.angle(), X1.angle(), X0.abs(), X1.abs()
    ph = a1 - a0 - advance
    ph = ph - 2 * math.pi * torch.round(ph / (2 * math.pi))
    ph = ph + advance
    acc = torch.cumsum(torch.cat([phase_0, ph[..., :-1, :]], -2), -2)
    return torch.polar(al * n1 + (1 - al) * n0, acc)


def textbook_with_grad(X32, g32, rate, hop=256):
    """(Z, dL/dX) in float64 of the complex64 input X32 for L = Re sum conj(g) Z: what a backward hands to X.grad"""
    X = X32.to(torch.complex128).requires_grad_()
    Z = textbook(X, rate, hop)
    (gX,) = torch.autograd.grad(Z, X, grad_outputs=g32.to(torch.complex128))
    return Z.detach(), gX


def _unit(z):
    m = z.abs()
    zero = m == 0
    return torch.where(zero, torch.ones_like(z), z / torch.where(zero, torch.ones_like(m), m)), m


def phasor_product(X, idx, alpha):
    """The kernel's forward in the dtype of X: p_0 = u(X[0]), p_{j+1} = p_j u(X[idx_j + 1]) conj(u(X[idx_j])),
    Z[j] = (alpha_j |X[idx_j + 1]| + (1 - alpha_j) |X[idx_j]|) p_j, frame T a frame of zeros.  Returns (Z, p_N)."""
    F = X.shape[-1]
    Xp = torch.cat([X, torch.zeros(X.shape[:-2] + (1, F), dtype=X.dtype)], -2)
    u, m = _unit(Xp)
    p = u[..., 0, :]
    rows = []
    for i, a in zip(idx, alpha):
        rows.append((a * m[..., i + 1, :] + (1 - a) * m[..., i, :]) * p)
        p = p * u[..., i + 1, :] * u[..., i, :].conj()
    return torch.stack(rows, -2), p


def gather_backward(X, g, idx, alpha, fin):
    """The kernel's backward, walked as the kernel walks it: j downwards, p_j back from the final phasor by the conjugate
    step, a running suffix sum S, the two frames of the step with their own G_abs / G_ang, a frame written when idx moves
    past it, zeros in frames no step reads."""
    T, F = X.shape[-2], X.shape[-1]
    Xp = torch.cat([X, torch.zeros(X.shape[:-2] + (1, F), dtype=X.dtype)], -2)
    u, m = _unit(Xp)
    real = m.dtype
    gX = torch.full_like(X, float("nan"))             # every element must be written

    def flush(i, acc):
        if i < T:
            ga, gp = acc
            x, mi = Xp[..., i, :], m[..., i, :]
            safe = torch.where(mi == 0, torch.ones_like(mi), mi)
            val = ga * u[..., i, :] + gp * torch.complex(-x.imag, x.real) / safe ** 2
            gX[..., i, :] = torch.where(mi == 0, torch.zeros_like(val), val)

    def fresh():
        return [torch.zeros(X.shape[:-2] + (F,), dtype=real), torch.zeros(X.shape[:-2] + (F,), dtype=real)]

    p, S = fin, torch.zeros(X.shape[:-2] + (F,), dtype=real)
    cur, lo, hi = None, None, None
    for j in range(len(idx) - 1, -1, -1):
        i, a = idx[j], alpha[j]
        if cur is None:
            for t in range(i + 2, T):
                gX[..., t, :] = 0
            lo, hi = fresh(), fresh()
        elif cur - i == 1:
            flush(cur + 1, hi)
            lo, hi = fresh(), lo
        elif cur != i:
            flush(cur + 1, hi)
            flush(cur, lo)
            for t in range(i + 2, cur):
                gX[..., t, :] = 0
            lo, hi = fresh(), fresh()
        cur = i
        p = p * (u[..., i + 1, :] * u[..., i, :].conj()).conj()
        Z = (a * m[..., i + 1, :] + (1 - a) * m[..., i, :]) * p
        gphi = (Z.conj() * g[..., j, :]).imag
        gm = (p.conj() * g[..., j, :]).real
        hi[1] = hi[1] + S
        lo[1] = lo[1] - S
        lo[0] = lo[0] + (1 - a) * gm
        hi[0] = hi[0] + a * gm
        S = S + gphi
    lo[1] = lo[1] + S
    flush(cur + 1, hi)
    flush(cur, lo)
    for t in range(cur):
        gX[..., t, :] = 0
    return gX
