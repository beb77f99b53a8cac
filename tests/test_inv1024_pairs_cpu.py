"""The paired layout of the n_fft-1024 inverse kernels (csrc/inv1024_pairs.h), checked on the host for all 64 lanes.

Lane L loads bin L + 64 m into register m < 4 and bin (64 - L) + 64 m into register m >= 4, so that registers m and
7 - m hold a mirror pair (X[k], X[512 - k]) in every lane and the real-FFT split computes each pair once, with one
W1024 twiddle.  The expectations below restate that layout from the header's comment; tests/inv1024_pairs_main.cpp is
compiled with the host compiler of the ROCm toolchain that the library's Makefile needs anyway.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acids_transforms_amd", "csrc")


def _host_compiler():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for root in filter(None, roots):
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++", "bin/amdclang++"):
            if os.path.exists(os.path.join(root, sub)):
                return os.path.join(root, sub)
    pytest.fail("no host compiler of the ROCm toolchain found under %s" % [r for r in roots if r])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inv1024_pairs") / "inv1024_pairs")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "inv1024_pairs_main.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def _table(prog, *args):
    out = subprocess.run([prog] + list(args), check=True, capture_output=True, text=True).stdout
    return np.array([l.split() for l in out.splitlines()], dtype=np.int64)


@pytest.fixture(scope="module")
def layout(prog):
    t = _table(prog, "--layout")
    assert t.shape == (64 * 8, 8)
    names = ["lane", "m", "load_bin", "partner_reg", "exchange_lane", "rotated_bin", "final_bin", "twiddle_bin"]
    c = {n: t[:, i].reshape(64, 8) for i, n in enumerate(names)}
    assert np.array_equal(c["lane"], np.arange(64)[:, None] + np.zeros((1, 8), dtype=np.int64))
    assert np.array_equal(c["m"], np.zeros((64, 1), dtype=np.int64) + np.arange(8)[None, :])
    return c


def test_every_bin_is_loaded_once(layout):
    lane, m, b = layout["lane"], layout["m"], layout["load_bin"]
    assert np.array_equal(b[:, :4], (lane + 64 * m)[:, :4])
    assert np.array_equal(b[:, 4:], (64 - lane + 64 * m)[:, 4:])
    # bins 0..512 except 256, each exactly once; 256 is in no register (lane 0's extra element)
    assert sorted(b.ravel().tolist()) == [k for k in range(513) if k != 256]
    assert b[0].tolist() == [0, 64, 128, 192, 320, 384, 448, 512]
    # one load instruction = one register over the 64 lanes = 64 consecutive bins, ascending below 4, descending from 4 on
    for r in range(8):
        col = b[:, r]
        assert np.array_equal(np.sort(col), np.arange(col.min(), col.min() + 64))
        assert np.all(np.diff(col) == (1 if r < 4 else -1))
    assert [int(b[:, r].min()) for r in range(8)] == [0, 64, 128, 192, 257, 321, 385, 449]


def test_registers_m_and_7_minus_m_are_mirror_partners(layout):
    b, pr = layout["load_bin"], layout["partner_reg"]
    assert np.array_equal(pr, 7 - layout["m"])
    for lane in range(64):
        for r in range(8):
            assert b[lane, r] + b[lane, pr[lane, r]] == 512
    # the pair's one twiddle is that of its member below 256
    assert np.array_equal(layout["twiddle_bin"][:, :4], b[:, :4])
    assert layout["twiddle_bin"][:, :4].max() < 256


def test_rotation_and_exchange_give_the_natural_order(layout):
    lane, m = layout["lane"], layout["m"]
    x = layout["exchange_lane"]
    assert np.array_equal(x, (64 - lane) % 64)
    assert x[0, 0] == 0 and x[32, 0] == 32                       # lanes 0 and 32 address themselves
    assert np.array_equal(x[x[:, 0], 0], np.arange(64))          # a swap of two lanes
    # after the split and lane 0's rotation (bin 256 into its register 4): registers 0..3 hold the lane's own column,
    # registers 4..7 column (64 - lane) & 63, each at its natural index -- lane 0 the whole of column 0
    r = layout["rotated_bin"]
    assert np.array_equal(r[:, :4], (lane + 64 * m)[:, :4])
    assert np.array_equal(r[:, 4:], (x + 64 * m)[:, 4:])
    assert r[0].tolist() == [0, 64, 128, 192, 256, 320, 384, 448]
    # after the exchange: what fft512<true> takes
    assert np.array_equal(layout["final_bin"], lane + 64 * m)
    assert np.array_equal(layout["final_bin"][:, 4:], r[x[:, 0]][:, 4:])


def test_w1024_table_is_antisymmetric(prog):
    """W1024^(512-k) = -conj(W1024^k) bit for bit, k = 1..255: what lets one twiddle serve both members of a pair."""
    t = _table(prog, "--table")
    assert np.array_equal(t[:, 0], np.arange(512))
    re = t[:, 1].astype(np.uint32).view(np.float32)
    im = t[:, 2].astype(np.uint32).view(np.float32)
    k = np.arange(512)
    assert np.abs(re - np.cos(2 * np.pi * k / 1024)).max() < 1e-7 and np.abs(im + np.sin(2 * np.pi * k / 1024)).max() < 1e-7
    k = np.arange(1, 256)
    sign = np.uint32(0x80000000)
    assert np.array_equal(t[512 - k, 1].astype(np.uint32), t[k, 1].astype(np.uint32) ^ sign)     # Re: negated
    assert np.array_equal(t[512 - k, 2], t[k, 2])                                                # Im: the same
    assert re[0] == 1.0 and im[256] == -1.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pair_split_is_the_bin_by_bin_split_bit_for_bit(prog, seed):
    """fp32 model with the kernels' operation order: each pair split once through the layout against every bin split on
    its own with its own table entry."""
    t = _table(prog, "--split", str(seed))
    assert np.array_equal(t[:, 0], np.arange(512))
    ref = t[:, 1:3].astype(np.uint32)
    got = t[:, 3:5].astype(np.uint32)
    assert np.count_nonzero(ref.view(np.float32)) > 1000        # a real spectrum went through
    assert np.array_equal(got, ref)
