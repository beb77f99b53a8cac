"""The source of the streaming time-domain stages (csrc/stream_source.h: StreamSource), run on the host against numpy's
concatenate([state or zeros(H), x, zeros]).  tests/stream_source_main.cpp is compiled with the host compiler of the ROCm
toolchain, as tests/band_plan_main.cpp is; every value is a small integer, so the comparison is exact.
"""
import subprocess

import numpy as np
import pytest

import host_program

# (C, H): no state to carry; an empty chunk; a tail that reaches back into the state; C == H; C > H
SHAPES = [(4, 0), (0, 0), (0, 3), (2, 5), (1, 2), (5, 5), (7, 3)]
CASES = [(C, H, s) for C, H in SHAPES for s in (0, 1)]
TAPS = np.array([1.0, 10.0, 100.0, 1000.0])


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = host_program.build("stream_source_main.cpp", str(tmp_path_factory.mktemp("stream_source") / "stream_source"))
    text = "".join("%d %d %d\n" % c for c in CASES)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(CASES)
    return {c: [np.array(part.split(), dtype=np.float64) for part in line.split("|")] for c, line in zip(CASES, out)}


def _source(C, H, has_state):
    state = np.arange(1, H + 1, dtype=np.float64) if has_state else np.zeros(H)
    return state, np.arange(101, 101 + C, dtype=np.float64)


@pytest.mark.parametrize("C,H,has_state", CASES)
def test_at_and_tail_are_numpys_concatenate(lines, C, H, has_state):
    state, x = _source(C, H, has_state)
    s = np.concatenate([np.zeros(2), state, x, np.zeros(3)])      # places -H - 2 .. C + 2
    got = lines[(C, H, has_state)][0]
    assert got.size == s.size + H
    assert np.array_equal(got[:s.size], s)
    assert np.array_equal(got[s.size:], np.concatenate([state, x])[C:])      # the last H of [state | chunk]


@pytest.mark.parametrize("C,H,has_state", CASES)
def test_dot_is_the_chain_over_at_for_every_window(lines, C, H, has_state):
    """Windows of four taps from five places before the state to one past the chunk: every change of source (zeros, state,
    chunk, zeros) falls at every tap of some window.  The sums are integers below 2^24: exact in float32."""
    state, x = _source(C, H, has_state)
    s = np.concatenate([np.zeros(5), state, x, np.zeros(5)])      # places -H - 5 .. C + 4
    got = lines[(C, H, has_state)][1].reshape(-1, 2)
    want = np.array([0.5 + TAPS @ s[i:i + 4] for i in range(H + C + 7)])      # first = -H - 5 .. C + 1
    assert got.shape == (want.size, 2)
    assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want)
