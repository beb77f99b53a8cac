"""The dispatch of the Magnitude.invert / Polar.invert backward (at_magnitude_invert_backward,
csrc/invert_grad.hip: launch_magnitude_invert_backward, launch_maginv_form; csrc/persistent_launch.h: persistent_launch), restated for
the CPU, and the sweep of test_invert_grad_gpu.py that drives every path of it.

test_invert_grad_cases_cpu.py checks that the sweep reaches every class named here, for both forms; the GPU file runs
it.  The bank shapes are those of grad_cases.MAG_CASES."""
import grad_cases as G

LDS_BUDGET = 160 * 1024          # kBandLdsBudget (csrc/band_plan.h)
LDS_PER_CU = 160 * 1024          # gfx950
THREADS_PER_CU = 2048            # 8 waves on each of 4 SIMDs
CUS = 256


def pads(K, N):
    return (K + 63) // 64 * 64, (N + 63) // 64 * 64


def per_wave_bytes(K, N, polar):
    """A wave's LDS slice: g of the row (N floats); the polar form keeps gM there, next to c(z) and c'(z) (K each)."""
    k_pad, n_pad = pads(K, N)
    return 4 * (n_pad + 2 * k_pad if polar else n_pad)


def table_floats(K, N, t_nnz, f_nnz, polar):
    """start / len / off and weights of the transposed inverse bank (K columns) and, polar, of the bank (N columns)."""
    return ((3 * (N + K) + f_nnz if polar else 3 * K) + t_nnz + 3) // 4 * 4


def launch_plan(K, N, t_nnz, f_nnz=None, polar=False):
    """(class, waves per workgroup, dynamic LDS bytes) of one call; t_nnz = None: mel=False."""
    if t_nnz is None:
        return "pointwise", 4, 0
    per_wave = per_wave_bytes(K, N, polar)
    tab = table_floats(K, N, t_nnz, f_nnz, polar)
    if tab * 4 + 4 * per_wave <= LDS_BUDGET:
        lds = tab * 4 + 4 * per_wave
        return ("lds_big" if lds > 64 * 1024 else "lds"), 4, lds
    if per_wave > LDS_BUDGET:
        return "unsupported", 0, 0
    wpb = min(4, LDS_BUDGET // per_wave)
    return "global_w%d" % wpb, wpb, per_wave * wpb


def grid_blocks(rows, wpb, lds, cus=CUS):
    """persistent_launch's grid: the workgroups the chip holds at once (bounded here by LDS and by the wave slots; the
    occupancy query may answer fewer when registers bind, which only adds trips), at most one per group of wpb rows."""
    per_cu = max(min(LDS_PER_CU // lds, THREADS_PER_CU // (64 * wpb)), 1)
    return min(per_cu * cus, -(-rows // wpb))


def row_loop_trips(rows, wpb, lds, cus=CUS):
    """(trips of the kernel's row loop that the busiest workgroup makes, groups of the last trip)."""
    groups = -(-rows // wpb)
    blocks = grid_blocks(rows, wpb, lds, cus)
    return -(-groups // blocks), groups % blocks


# the classes each form can reach at the n_fft the library takes (<= 16384).  Real form: a wave's slice is g alone, at
# most 8256 floats, so four waves always fit the budget and "fewer waves" does not exist there; polar form: three arrays
# per wave, so its global-memory classes run 4, 3 and 1 waves in this sweep.
REAL_CLASSES = {"pointwise", "lds", "lds_big", "global_w4"}
POLAR_CLASSES = {"lds", "lds_big", "global_w4", "global_w3", "global_w1"}

MAG_CASES = G.MAG_CASES
MAG_MODES = G.MAG_MODES


def polar_eligible(kw):
    """A MAG_CASES entry whose bank is square (F x F) and whose module the stacked Polar tensor can hold."""
    return kw.get("mel", True) and kw.get("keep_nyquist", True) and "n_mels" not in kw and "bank_dtype" not in kw


POLAR_CASES = [c for c in MAG_CASES if polar_eligible(c[1])]

# many rows: at least three trips of the row loop on a 256-CU device, the last one partial
MANY_ROWS = {"real": ({"n_fft": 1024, "n_mels": 128}, (31, 690)), "polar": ({"n_fft": 1024}, (15, 690))}


def module_plan(mod, polar=False):
    """launch_plan of a Magnitude, from bank_columns of its inverse bank (as autograd._inverse_bank_tables builds them)."""
    from acids_transforms_amd.utils.banded import bank_columns
    F = mod.n_fft // 2 + 1
    if not mod.mel:
        return launch_plan(F, F, None)
    bank = mod.inverse_mel_bank
    K, N = bank.shape[-2], bank.shape[-1]
    t_nnz = len(bank_columns(bank.transpose(-2, -1))[3])
    f_nnz = len(bank_columns(bank)[3]) if polar else None
    return launch_plan(K, N, t_nnz, f_nnz, polar)


# ---- the reference's expressions (spectral_repr.py:203-213, 229-240, 441-452, 497-508) and the kernels' formulas -------
# shared by the CPU and GPU tests; everything in float64 on the CPU

def magnitude_params(mod):
    """What Magnitude.invert reads of a module, as float64 CPU values: the reference expression is built from the
    module's own buffers."""
    norm = mod.norm.mode is not None
    return {"contrast": mod.contrast_mode, "eps": float(mod.eps), "keep_nyquist": mod.keep_nyquist,
            "W": mod.inverse_mel_bank.detach().cpu().double()[0] if mod.mel else None,
            "offset": float(mod.norm.offset) if norm else None, "scale": float(mod.norm.scale) if norm else None}


def affine_params(rep):
    """(offset, scale) of a Real / Imaginary / Phase, or (None, None)."""
    if rep.norm.mode is None:
        return None, None
    return float(rep.norm.offset), float(rep.norm.scale)


def ref_invert_contrast(z, contrast, eps):
    import torch
    if contrast == "log1p":
        return torch.exp(z) - 1
    if contrast == "log":
        return torch.exp(z) - eps
    if contrast == "log10":
        return torch.tensor(10, dtype=z.dtype).pow(z)
    return z


def ref_affine_invert(y, offset, scale, keep_nyquist=True):
    import torch
    out = y * scale + offset if offset is not None else y
    if not keep_nyquist:
        out = torch.cat([out, torch.zeros(out.shape[:-1] + (1,), dtype=out.dtype)], -1)
    return out


def ref_magnitude_invert(y, p):
    import torch
    z = ref_affine_invert(y, p["offset"], p["scale"], p["keep_nyquist"])
    x = ref_invert_contrast(z, p["contrast"], p["eps"])
    return torch.matmul(x, p["W"]) if p["W"] is not None else x


def ref_polar_invert(y, p, ph_offset, ph_scale):
    import torch
    mag = ref_magnitude_invert(y[..., 0, :], p)
    phase = ref_affine_invert(y[..., 1, :], ph_offset, ph_scale)
    return mag * torch.exp(1j * phase)


def ref_cartesian_invert(y, re_affine, im_affine):
    return ref_affine_invert(y[..., 0, :], *re_affine) + 1j * ref_affine_invert(y[..., 1, :], *im_affine)


def autograd_of(fn, y, g):
    """y.grad of fn(y) fed the gradient g (complex g: torch's convention), float64."""
    import torch
    leaf = y.detach().clone().double().requires_grad_()
    out = fn(leaf)
    out.backward(g.to(out.dtype).reshape(out.shape))
    return leaf.grad


def _cprime(z, contrast):
    import numpy as np
    if contrast in ("log1p", "log"):
        return np.exp(z)
    if contrast == "log10":
        return np.log(10.0) * 10.0 ** z
    return np.ones_like(z)


def formula_magnitude_invert(y, g, p):
    """at_magnitude_invert_backward's real form on float64 numpy arrays: y (rows, K - pad), g (rows, N)."""
    import numpy as np
    sc = p["scale"] if p["scale"] is not None else 1.0
    z = y * sc + p["offset"] if p["offset"] is not None else y
    back = g @ p["W"].numpy().T if p["W"] is not None else g          # sum_n W[k, n] g[n]
    if not p["keep_nyquist"]:
        back = back[..., :-1]                                             # the padded column's gradient is dropped
    return sc * _cprime(z, p["contrast"]) * back


def formula_polar_invert(y, gX, p, ph_offset, ph_scale):
    """The polar form: y (rows, 2, F), gX (rows, F) complex -> dy (rows, 2, F)."""
    import numpy as np
    ps = ph_scale if ph_scale is not None else 1.0
    phi = y[..., 1, :] * ps + (ph_offset if ph_offset is not None else 0.0)
    sc = p["scale"] if p["scale"] is not None else 1.0
    z = y[..., 0, :] * sc + p["offset"] if p["offset"] is not None else y[..., 0, :]
    eps = p["eps"]
    cz = {"log1p": lambda v: np.exp(v) - 1, "log": lambda v: np.exp(v) - eps, "log10": lambda v: 10.0 ** v}.get(
        p["contrast"], lambda v: v)(z)
    M = cz @ p["W"].numpy()
    gM = gX.real * np.cos(phi) + gX.imag * np.sin(phi)
    dphase = ps * M * (gX.imag * np.cos(phi) - gX.real * np.sin(phi))
    dmag = formula_magnitude_invert(y[..., 0, :], gM, p)
    return np.stack([dmag, dphase], -2)


def formula_polar_to_complex(gX, mag, phase):
    import numpy as np
    return (gX.real * np.cos(phase) + gX.imag * np.sin(phase),
            mag * (gX.imag * np.cos(phase) - gX.real * np.sin(phase)))


def formula_cartesian(gX, re_scale, im_scale):
    import numpy as np
    return np.stack([gX.real * (re_scale if re_scale is not None else 1.0),
                     gX.imag * (im_scale if im_scale is not None else 1.0)], -2)
