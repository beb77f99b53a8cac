"""For test_spectral_distance_cpu.py and test_mel_distance_cpu.py: CPU stand-ins for the ops behind autograd's two
distance Functions, so that the Python driver they share runs, and can be watched, without a GPU."""
import torch

from spectral_distance_cases import frames


def stub_ops(monkeypatch, autograd):
    """Replaces the ops that autograd's two distance Functions call by CPU stand-ins and wraps the shared driver
    (autograd._dist_sums, autograd._DistBackward) in counters.  Returns the log: a list of (name, detail) in call order.
    stft_forward gives zeros of the right shape; the sums ops write S_D = 1, S_B = 2, S_L = 3; the backward ops leave
    the spectrum alone; stft_backward fills its `out` with n_fft, so that a gradient shows what was written where."""
    log = []

    def stft_forward(x, w, n, hop, center=True):
        log.append(("stft_forward", (x.shape[0], n, hop)))
        return torch.zeros((x.shape[0], frames(n, hop, x.shape[-1]), n // 2 + 1), dtype=torch.complex64)

    def sums(name):
        def op(A, Bm, eps, out=None):
            log.append((name, tuple(A.shape)))
            out.copy_(torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64).expand_as(out))
            return out
        return op

    def mel_rows(X, cols):
        log.append(("mel_rows", tuple(X.shape)))
        return torch.zeros(tuple(X.shape[:-1]) + (cols[0].numel(),))

    def stft_backward(G, w, n, hop, L, out=None):
        log.append(("stft_backward", (G.shape[0], n, out.data_ptr())))
        out.fill_(float(n))
        return out

    def backward(name):
        return lambda *a: log.append((name, (a[0].shape[0], a[-1])))

    for name, fn in (("stft_forward", stft_forward), ("spectral_distance_sums", sums("spectral_distance_sums")),
                     ("mel_distance_sums", sums("mel_distance_sums")), ("mel_rows", mel_rows), ("stft_backward", stft_backward),
                     ("spectral_distance_backward", backward("spectral_distance_backward")),
                     ("mel_distance_backward", backward("mel_distance_backward"))):
        monkeypatch.setattr(autograd.ops, name, fn)
    real_sums, real_bwd = autograd._dist_sums, autograd._DistBackward

    def dist_sums(*a, **k):
        log.append(("_dist_sums", None))
        return real_sums(*a, **k)

    class DistBackward(real_bwd):
        def __init__(self, *a, **k):
            log.append(("_DistBackward", None))
            super().__init__(*a, **k)
    monkeypatch.setattr(autograd, "_dist_sums", dist_sums)
    monkeypatch.setattr(autograd, "_DistBackward", DistBackward)
    return log
