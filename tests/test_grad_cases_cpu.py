"""The backward sweeps of test_grad_paths_gpu.py reach every path of the STFT adjoint and of the Magnitude backward
(grad_cases.py restates the dispatch).  CPU only: this turns the GPU file's coverage claims into checked facts."""
import pytest

import grad_cases as C
from acids_transforms_amd import _lib


def _sweep_classes():
    out = []
    for n, h in C.ADJ_SWEEP:
        for L in C.adj_lengths(n, h):
            out.append(((n, h, L), C.adjoint_class(n, h, 2, L)))
    for n, h, L in C.FAST_HOP_DIVIDES:
        out.append(((n, h, L), C.adjoint_class(n, h, 2, L)))
    return out


def test_family_and_chunk_restatement():
    assert [C.irfft_family(n) for n in (2, 4, 6, 8, 64, 128, 256, 400, 512, 1024, 8192)] == \
        ["mixed", "mixed", "mixed", "generic", "generic", "small", "small", "mixed", "512", "1024", "generic"]
    # test_autograd_cpu.py's pinned values of the library
    assert C.workspace_bytes(4, 10, 1024) == 4096 + 4 * 10 * 1024 * 4
    assert C.chunk_clips(1024, 690, 1024) == 379
    assert C.frames(441, 110, 221) == 3 and C.frames(1024, 256, 16384) == 65


def test_adjoint_sweep_reaches_every_irfft_family():
    hit = {c["family"] for _, c in _sweep_classes()}
    assert C.ADJ_FAMILIES <= hit, sorted(C.ADJ_FAMILIES - hit)


def test_adjoint_sweep_reaches_every_fold_path():
    cases = _sweep_classes()
    # vec4 groups in the interior at every residue of L - P - 1, one of them with hop | L (the residue-3 group then
    # holds the right-fold term that reads the last padded sample)
    for r in range(4):
        assert any(c["vec4_interior"] and c["residue"] == r for _, c in cases), r
    assert any(c["vec4_interior"] and c["residue"] == 3 and c["hop_divides_L"] for _, c in cases)
    # the scalar interior path at an even n_fft: hop % 4 != 0
    assert any(n % 8 == 0 and h % 4 != 0 and not c["vec4"] and L > 2 * n for (n, h, L), c in cases)
    # frames that leave samples uncovered, and frames that overlap at every sample
    assert {"below", "equal", "above"} <= {c["hop_vs_n"] for _, c in cases}
    assert any(h == 1 for (_, h, _), _c in cases)
    # both folds overlapping one frame (L = P + 1)
    assert any(L == n // 2 + 1 for (n, _, L), _ in cases)
    # odd sizes (no Nyquist bin) at every irFFT family that takes them
    assert any(n % 2 == 1 and n > 8000 for (n, _, _), _ in cases)


def test_big_adjoint_cases_cut_the_chunks_they_claim():
    n, h, L, B, clips = C.BIG_ADJ["three_chunks"]
    c = C.adjoint_class(n, h, B, L)
    assert c["n_chunks"] >= 3 and c["last_chunk"] < c["chunk"], c
    assert (c["chunk"], c["n_chunks"], c["last_chunk"]) == (378, 3, 44)
    # the clips on both sides of every chunk boundary, and the last clip
    for k in range(1, c["n_chunks"]):
        assert k * c["chunk"] - 1 in clips and k * c["chunk"] in clips
    assert B - 1 in clips

    n, h, L, B, clips = C.BIG_ADJ["chunk_of_one"]
    c = C.adjoint_class(n, h, B, L)
    assert c["T"] * n > C.CHUNK_FLOATS and c["chunk"] == 1 and c["n_chunks"] == B == len(clips)

    n, h, L, B, clips = C.BIG_ADJ["clip_loop"]
    c = C.adjoint_class(n, h, B, L)
    assert c["n_chunks"] == 1 and c["clip_loop"] and B > 2 * C.GRID_Y          # the clip loop runs three times
    for k in (1, 2):
        assert k * C.GRID_Y - 1 in clips and k * C.GRID_Y in clips
    assert B - 1 in clips


@pytest.mark.parametrize("case", ["three_chunks", "chunk_of_one", "clip_loop"])
def test_chunk_restatement_matches_the_library(case):
    n, h, L, B, _ = C.BIG_ADJ[case]
    T = C.frames(n, h, L)
    lib = _lib.lib()
    got = lib.at_stft_backward_workspace_bytes(B, T, n, h)
    assert got == C.workspace_bytes(B, T, n)
    window_slot = (n * 4 + 255) // 256 * 256
    assert (got - window_slot) // (T * n * 4) == C.chunk_clips(B, T, n)
    assert (got - window_slot) % (T * n * 4) == 0


def test_chunk_restatement_matches_the_library_on_the_sweep():
    lib = _lib.lib()
    for (n, h, L), c in _sweep_classes():
        for B in (1, 2, 1000):
            T = C.frames(n, h, L)
            assert lib.at_stft_backward_workspace_bytes(B, T, n, h) == C.workspace_bytes(B, T, n), (n, h, L, B)


def test_magnitude_sweep_reaches_every_class():
    hit = {}
    for name, kw, _ in C.MAG_CASES:
        hit.setdefault(C.module_class(C.magnitude_module(kw)), []).append(name)
    for kw, _ in C.MANY_ROWS.values():
        hit.setdefault(C.module_class(C.magnitude_module(kw)), []).append("many_rows")
    assert C.MAG_CLASSES <= set(hit), sorted(C.MAG_CLASSES - set(hit))
    assert "unsupported" not in hit


@pytest.mark.parametrize("name,want", [("n256", "lds_kit9"), ("n1024_m520", "lds_kit9"), ("n1536", "lds_kit0"),
                                       ("n2048_m80", "lds_kit0"), ("n2048_m128", "lds_kit0"), ("n2048", "lds_kit0_big"),
                                       ("n3000", "lds_kit0_big"), ("n4096_m128", "lds_kit0_big"),
                                       ("n8192", "global_w4"), ("n16384", "global_w2"), ("n1024_dense", "global_w4"),
                                       ("n1024_off", "pointwise")])
def test_magnitude_case_class(name, want):
    kw = next(k for n, k, _ in C.MAG_CASES if n == name)
    assert C.module_class(C.magnitude_module(kw)) == want


def test_magnitude_bank_edges_are_in_the_sweep():
    mods = {name: C.magnitude_module(kw) for name, kw, _ in C.MAG_CASES if name in ("n1024_m1", "n1024_m520")}
    assert mods["n1024_m1"].mel_bank.shape[-1] == 1
    bank = mods["n1024_m520"].mel_bank[0]
    assert bank.shape[-1] > bank.shape[-2] and bool((bank.sum(0) == 0).any())     # empty filters: f_len = 0
    # a row count below a workgroup's waves, and row counts that leave its last group part full
    rows = {r[0] * r[1] for _, _, r in C.MAG_CASES}
    assert {1, 3, 5} <= rows


def test_many_rows_need_several_grid_passes():
    # the banded grid is capped at occupancy x CUs; 256 CUs x 8 workgroups x 4 waves is far below 200000 rows, and
    # the pointwise grid's 65536 x 256 threads is below 300 x 690 x 513 elements
    for kw, shape in C.MANY_ROWS.values():
        assert shape[0] * shape[1] >= 200000
    kw, shape = C.MANY_ROWS["pointwise"]
    assert shape[0] * shape[1] * (kw["n_fft"] // 2 + 1) > 65536 * 256
