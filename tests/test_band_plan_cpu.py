"""The one row plan of the banded kernels (csrc/band_plan.h: band_plan), run on the host against the three restatements
the case files keep: grad_cases.magnitude_bwd_class (launch_magnitude_backward), invert_grad_cases.launch_plan
(launch_maginv_form, real and polar) and mel_distance_cases.plan (launch_mel_rows, launch_mel_distance_backward).

tests/band_plan_main.cpp is compiled with the host compiler of the ROCm toolchain that the library's Makefile needs
anyway.  What goes into the plan -- the floats of the tables a launcher stages and the bytes of one wave's rows -- is
formed here as each launcher forms it; everything compared is an integer.
"""
import subprocess

import pytest

import grad_cases as G
import host_program
import invert_grad_cases as IG
import mel_distance_cases as MD
from acids_transforms_amd.utils.banded import bank_columns

BUDGET = 160 * 1024


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program.build("band_plan_main.cpp", str(tmp_path_factory.mktemp("band_plan") / "band_plan"))


def _plans(prog, cases):
    """band_plan of every (table floats, per-wave bytes) as (class, waves per workgroup, LDS bytes, staged floats)."""
    text = "".join("%d %d\n" % c for c in cases)
    out = subprocess.run([prog], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    plans = []
    for line in out:
        ok, tab_lds, wpb, tab, lds = (int(v) for v in line.split())
        cls = "unsupported" if not ok else ("lds_big" if lds > 64 * 1024 else "lds") if tab_lds else "global_w%d" % wpb
        plans.append((cls, wpb, lds, tab))
    return plans


def test_constants_and_roundings(prog):
    out = subprocess.run([prog, "--consts"], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [BUDGET, 9, 64, 64, 128, 8]
    assert BUDGET == G.LDS_BUDGET == IG.LDS_BUDGET == MD.LDS_BUDGET


def _banks(mod_kw):
    mod = G.magnitude_module(mod_kw)
    return mod, (mod.mel_bank if mod.mel else None)


def test_magnitude_backward_cases(prog):
    """launch_magnitude_backward: both banks' tables, K + N floats per wave; the class names add the register row."""
    cases, want, Ks = [], [], []
    for _, kw, _ in G.MAG_CASES + [("many", G.MANY_ROWS["banked"][0], None)]:
        mod, bank = _banks(kw)
        if bank is None:
            continue
        K, N = bank.shape[-2], bank.shape[-1]
        f_nnz, t_nnz = len(bank_columns(bank)[3]), len(bank_columns(bank.transpose(-2, -1))[3])
        cases.append((3 * (N + K) + f_nnz + t_nnz, 4 * (MD.pad64(K) + MD.pad64(N))))
        want.append(G.magnitude_bwd_class(K, N, f_nnz, t_nnz))
        Ks.append(K)
    got = []
    for (cls, wpb, lds, tab), K, (floats, per_wave) in zip(_plans(prog, cases), Ks, cases):
        if cls in ("lds", "lds_big"):             # the restatement names the class only: waves and bytes from the rule
            assert (wpb, tab, lds) == (4, (floats + 3) // 4 * 4, 4 * ((floats + 3) // 4 * 4) + 4 * per_wave)
            cls = "lds_kit9" if K <= 9 * 64 else ("lds_kit0_big" if cls == "lds_big" else "lds_kit0")
        elif cls != "unsupported":
            assert (tab, lds) == (0, wpb * per_wave) and wpb == min(4, BUDGET // per_wave)
        got.append(cls)
    assert got == want
    assert set(want) == G.MAG_CLASSES - {"pointwise"}


@pytest.mark.parametrize("polar", [False, True])
def test_invert_backward_cases(prog, polar):
    """launch_maginv_form: the transposed inverse bank's tables and N floats per wave; polar adds the bank's tables and
    2 K floats."""
    cases, want = [], []
    for _, kw, _ in (IG.POLAR_CASES if polar else IG.MAG_CASES) + [("many", IG.MANY_ROWS["polar" if polar else "real"][0], None)]:
        mod = G.magnitude_module(kw)
        if not mod.mel:
            continue
        bank = mod.inverse_mel_bank
        K, N = bank.shape[-2], bank.shape[-1]
        t_nnz = len(bank_columns(bank.transpose(-2, -1))[3])
        f_nnz = len(bank_columns(bank)[3]) if polar else None
        k_pad, n_pad = IG.pads(K, N)
        cases.append(((3 * (N + K) + f_nnz if polar else 3 * K) + t_nnz, 4 * (n_pad + 2 * k_pad if polar else n_pad)))
        want.append(IG.launch_plan(K, N, t_nnz, f_nnz, polar))
        assert want[-1] == IG.module_plan(mod, polar)
    assert [p[:3] for p in _plans(prog, cases)] == want
    assert {w[0] for w in want} == (IG.POLAR_CLASSES if polar else IG.REAL_CLASSES - {"pointwise"})


def test_mel_distance_cases(prog):
    """launch_mel_rows (the bank's tables, K floats per wave) and launch_mel_distance_backward (both banks', K + N)."""
    cases, want, Ks = [], [], []
    for _, _, F, N in MD.OP_SHAPES + (MD.many_rows_shape(),):
        W = MD.bank(F, N)
        f_nnz, t_nnz = bank_columns(W)[3].size, bank_columns(W.t())[3].size
        cases += [(3 * N + f_nnz, 4 * MD.pad64(F)), (3 * N + f_nnz + 3 * F + t_nnz, 4 * (MD.pad64(F) + MD.pad64(N)))]
        want += [MD.plan(F, N, f_nnz), MD.plan(F, N, f_nnz, t_nnz)]
        Ks += [F, F]
        assert tuple(want[-2:]) == MD.bank_plans(W)
    got = _plans(prog, cases)
    assert [p[:3] for p in got] == [w[:3] for w in want]
    # the register row: next to staged tables only, K <= 64 kBandKit
    assert [w[3] for w in want] == [p[0] in ("lds", "lds_big") and K <= 9 * 64 for p, K in zip(got, Ks)]
    assert {w[0] for w in want} == {"lds", "global_w4"}


def test_budget_boundaries(prog):
    """Around the budget, through invert_grad_cases.launch_plan's real form (K = N = 64: 256 bytes per wave, 192 + t_nnz
    table floats) where it reaches, and with the rule's own numbers where one byte matters."""
    def real(t_nnz, N=64):
        return (3 * 64 + t_nnz, 4 * IG.pads(64, N)[1]), IG.launch_plan(64, N, t_nnz)
    named = [
        real(40512),            # tables + 4 waves exactly at the budget
        real(40513),            # one float over: the staged tables grow by a float4, and leave LDS
        real(15936),            # exactly 64 KiB: below the line of the big classes
        real(15937),            # one float4 over it
        real(200000, 40960),    # a wave's rows exactly at the budget: one wave
        real(200000, 40961),    # the next padded row: refused
        real(200000, 20480),    # half the budget: two waves
        real(200000, 20481),    # a row past half of it: one
        real(200000, 13632),    # three rows fit (3 x 54 528 = 163 584), a fourth does not
    ]
    got = _plans(prog, [c for c, _ in named])
    want = [w for _, w in named]
    assert [p[:3] for p in got] == want
    assert want == [("lds_big", 4, BUDGET), ("global_w4", 4, 1024), ("lds", 4, 65536), ("lds_big", 4, 65552),
                    ("global_w1", 1, BUDGET), ("unsupported", 0, 0), ("global_w2", 2, BUDGET), ("global_w1", 1, 82176),
                    ("global_w3", 3, 163584)]
    assert [p[3] for p in got] == [40704, 0, 16128, 16132, 0, 0, 0, 0, 0]       # staged floats: a multiple of four, or none
    # one byte: per_wave at the budget and one over it, with tables that do not fit; tables + 4 waves at the budget
    # and one float4 over it, with rows of 16 bytes
    raw = _plans(prog, [(200000, BUDGET), (200000, BUDGET + 1), (BUDGET // 4 - 16, 16), (BUDGET // 4 - 15, 16)])
    assert raw == [("global_w1", 1, BUDGET, 0), ("unsupported", 0, 0, 0), ("lds_big", 4, BUDGET, BUDGET // 4 - 16),
                   ("global_w4", 4, 64, 0)]
