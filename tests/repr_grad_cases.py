"""The forward backward of the phase-side representations (at_phase_scan_backward, at_cartesian_pack_backward,
csrc/repr_grad.hip; autograd.PhaseScanFunction and its neighbours): the kernel sweep of test_repr_grad_gpu.py, the
launcher's grid cap, float64 restatements of the reference's expressions (utils/misc.py:12-26, 65-81;
spectral_repr.py:21-140, 215-226, 318-335, 403-428) built from the modules' buffers, and the formulas the kernels
implement.  Shared by test_repr_grad_cpu.py and test_repr_grad_gpu.py; everything here is float64 on the CPU."""
import itertools
import math

# ---- the launcher (repr_grad.hip: flat_blocks, kScanBwdMaxBlocks) ------------------------------------------------------
BLOCK = 256
GRID_CAP_BLOCKS = 256 * 64          # beyond GRID_CAP_BLOCKS * BLOCK elements the threads of the flat pass loop


def grid_blocks(n):
    return min(-(-n // BLOCK), GRID_CAP_BLOCKS)


def loop_trips(n):
    """(trips of the busiest thread, trips of the idlest) of the flat pass over n elements."""
    threads = grid_blocks(n) * BLOCK
    return -(-n // threads), n // threads


# threads loop 3 or 4 times (the last trip is partial): 36 * 690 * 513 = 12 742 920 > 3 * 16384 * 256 = 12 582 912
GRID_LOOP_SHAPE = (36, 690, 513)

# ---- the kernel sweep -------------------------------------------------------------------------------------------------
MODES = ["unwrap", "forward", "backward", "central", "angle"]
IF_MODES = ("forward", "backward", "central")
SWEEP_T = [1, 2, 3, 4, 9]
SWEEP_F = [1, 7, 513]
SWEEP_B = [1, 3]
# options crossed with the shapes: frame window, Normalize scale, g inside a stacked (.., T, 2, F) tensor, the accumulated
# gradient (none / a tensor of its own / the output itself), the output over X
OPTION_NAMES = ("window", "scale", "stacked", "accum", "out_is_x")
OPTIONS = [o for o in itertools.product([False, True], [False, True], [False, True], ["none", "separate", "out"],
                                        [False, True])
           if not (o[3] == "out" and o[4])]         # out == accum == X would make the accumulated gradient X itself


def kernel_cases():
    """Every mode x T x F x B (a single frame has no central difference: the module builds that case from other pieces),
    each with one of the option rows; test_repr_grad_cpu.py checks that every pair of values of any two factors that can
    meet does meet.  A window goes with the IF modes only (at_phase_scan_backward refuses it for angle / unwrap)."""
    cases = []
    k = 0
    for mode, T, F, B in itertools.product(MODES, SWEEP_T, SWEEP_F, SWEEP_B):
        if mode == "central" and T == 1:
            continue
        opt = dict(zip(OPTION_NAMES, OPTIONS[(7 * k + k // len(OPTIONS)) % len(OPTIONS)]))
        if mode not in IF_MODES:
            opt["window"] = False
        cases.append(dict(mode=mode, T=T, F=F, B=B, **opt))
        k += 1
    return cases


# ---- the reference's expressions, float64 torch --------------------------------------------------------------------------

def ref_unwrap(ph):
    """utils/misc.py:12-26, statement by statement (out of place): the phase correction is ddmod - diff, zeroed where
    |diff| < pi, and summed along time."""
    import torch
    diff = ph[..., 1:, :] - ph[..., :-1, :]
    ddmod = torch.remainder(diff + math.pi, 2 * math.pi) - math.pi
    ddmod = torch.where((ddmod == -math.pi) & (diff > 0), torch.full_like(ddmod, math.pi), ddmod)
    corr = ddmod - diff
    corr = torch.where(diff.abs() < math.pi, torch.zeros_like(corr), corr)
    return torch.cat([ph[..., :1, :], ph[..., 1:, :] + torch.cumsum(corr, -2)], -2)


def ref_fdiff(u, method):
    """utils/misc.py:65-81 with the row scaling of IF.get_if (spectral_repr.py:321-329).  A single frame gives two rows
    with "central", as the reference's cat does."""
    import torch
    if method == "forward":
        d = torch.cat([u[..., :1, :], (u[..., 1:, :] - u[..., :-1, :]) / 2], -2)
        return torch.cat([d[..., :-1, :] / math.pi, d[..., -1:, :]], -2)
    if method == "backward":
        v = u.flip(-2)
        d = torch.cat([v[..., :1, :], (v[..., 1:, :] - v[..., :-1, :]) / 2], -2).flip(-2)
        return torch.cat([d[..., :1, :], d[..., 1:, :] / (-math.pi)], -2)
    if method == "central":
        d = torch.cat([u[..., :1, :], (u[..., 2:, :] - u[..., :-2, :]) / 4, u[..., -1:, :]], -2)
        return torch.cat([d[..., :1, :], d[..., 1:-1, :] / (2 * math.pi), d[..., -1:, :]], -2)
    raise AttributeError(method)


def ref_scan(X, mode, window=None, offset=None, scale=None):
    """What at_phase_scan computes of a complex spectrum X (..., T, F): angle / unwrap / IF, the frame weight, the
    Normalize affine."""
    ph = X.angle()
    if mode == "angle":
        y = ph
    elif mode == "unwrap":
        y = ref_unwrap(ph)
    else:
        y = ref_fdiff(ref_unwrap(ph), mode)
    if window is not None:
        y = window.reshape(-1, 1) * y
    if offset is not None:
        y = (y - offset) / scale
    return y


def ref_normalise(y, affine):
    off, sc = affine
    return (y - off) / sc if off is not None else y


def ref_cartesian(X, re_affine, im_affine):
    import torch
    return torch.stack([ref_normalise(X.real, re_affine), ref_normalise(X.imag, im_affine)], -2)


def affine_of(rep):
    """(offset, scale) of a module with a .norm, as float64 scalars, or (None, None)."""
    norm = getattr(rep, "norm", rep)
    if getattr(norm, "mode", None) is None or not hasattr(norm, "offset"):
        return None, None
    return float(norm.offset.double()), float(norm.scale.double())


def ref_magnitude(X, mod):
    """Magnitude.forward (spectral_repr.py:215-226) from the module's buffers."""
    import torch
    a = X.abs()
    if mod.mel:
        a = torch.matmul(a, mod.mel_bank[0].detach().cpu().double())
    eps = float(mod.eps)
    if mod.contrast_mode == "log1p":
        a = torch.log(1 + a)
    elif mod.contrast_mode == "log":
        a = torch.log(torch.clamp(a, eps, None))
    elif mod.contrast_mode == "log10":
        a = torch.log10(torch.clamp(a, eps, None))
    a = ref_normalise(a, affine_of(mod))
    return a if mod.keep_nyquist else a[..., 1:]


def ref_forward(rep):
    """fn(X complex128) -> the float64 forward of a representation module, by class name."""
    import torch
    name = type(rep).__name__
    if name == "Normalize":
        return lambda x: ref_normalise(x, affine_of(rep))
    if name == "Real":
        return lambda X: ref_normalise((X if rep.keep_nyquist else X[..., 1:]).real, affine_of(rep))
    if name == "Imaginary":
        return lambda X: (lambda y: y if rep.keep_nyquist else y[..., 1:])(ref_normalise(X.imag, affine_of(rep)))
    if name == "Phase":
        def phase(X):
            y = ref_scan(X, "unwrap" if rep.unwrap else "angle", None, *affine_of(rep))
            return y if rep.keep_nyquist else y[..., 1:]
        return phase
    if name == "IF":
        def inst_f(X):
            y = ref_fdiff(ref_unwrap(X.angle()), rep.method)
            if rep.weighted:
                y = rep._get_weighted_window(y).detach().cpu().double().reshape(-1, 1) * y
            y = ref_normalise(y, affine_of(rep))
            return y if rep.keep_nyquist else y[..., 1:]
        return inst_f
    if name == "Magnitude":
        return lambda X: ref_magnitude(X, rep)
    if name in ("Cartesian", "Polar", "PolarIF"):
        first, second = ref_forward(rep.magnitude), ref_forward(rep.phase)

        def both(X):
            a, b = first(X), second(X)
            return torch.stack([a, b], rep.stack) if rep.stack is not None else (a, b)
        return both
    raise TypeError(name)


def autograd_of(fn, x, grads):
    """x.grad of fn(x) fed `grads` (a tensor, or a tuple for a tuple result), in float64 / complex128."""
    import torch
    leaf = x.detach().cpu().to(torch.complex128 if x.is_complex() else torch.float64).requires_grad_()
    out = fn(leaf)
    outs = out if isinstance(out, tuple) else (out,)
    grads = grads if isinstance(grads, tuple) else (grads,)
    torch.autograd.backward(list(outs), [g.detach().cpu().double().reshape(o.shape) for o, g in zip(outs, grads)])
    return leaf.grad


# ---- the kernels' formulas, float64 numpy ---------------------------------------------------------------------------------

def row_scales(mode, T):
    import numpy as np
    s = np.ones(T)
    if mode == "forward":
        s[:T - 1] = 1 / math.pi
    elif mode == "backward":
        s[1:] = -1 / math.pi
    elif mode == "central":
        s[1:T - 1] = 1 / (2 * math.pi)
    return s


def formula_scan_backward(X, g, mode, window=None, scale=None, accum=None):
    """at_phase_scan_backward on numpy arrays: X (..., T, F) complex128, g (..., T, F) float64."""
    import numpy as np
    T = X.shape[-2]
    k = row_scales(mode, T) * (np.asarray(window, dtype=np.float64) if window is not None else 1.0)
    a = g * k[:, None] / (scale if scale is not None else 1.0)
    gu = np.zeros_like(a)
    if mode in ("angle", "unwrap") or (mode == "central" and T == 1):
        gu = a.copy()
    elif mode == "forward":
        c = np.full(T, 0.5)
        c[0] = 1.0
        gu = c[:, None] * a
        gu[..., :T - 1, :] -= a[..., 1:, :] / 2
    elif mode == "backward":
        c = np.full(T, 0.5)
        c[T - 1] = 1.0
        gu = c[:, None] * a
        gu[..., 1:, :] -= a[..., :T - 1, :] / 2
    else:
        gu[..., 0, :] += a[..., 0, :]
        gu[..., T - 1, :] += a[..., T - 1, :]
        gu[..., 2:, :] += a[..., 1:T - 1, :] / 4          # a_{t-1}, 1 <= t-1 <= T-2
        gu[..., :T - 2, :] -= a[..., 1:T - 1, :] / 4      # a_{t+1}, 1 <= t+1 <= T-2
    d = X.real ** 2 + X.imag ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        gX = np.where(d == 0, 0.0, gu * (-X.imag + 1j * X.real) / d)
    return gX + accum if accum is not None else gX


def formula_cartesian_forward(g, re_scale=None, im_scale=None):
    """at_cartesian_pack_backward: g (..., 2, F) float64 -> (..., F) complex128."""
    return g[..., 0, :] / (re_scale if re_scale is not None else 1.0) \
        + 1j * g[..., 1, :] / (im_scale if im_scale is not None else 1.0)
