"""The aligned row stream of the sliding-window forwards (csrc/row_stream.h: RowStream) and the runs' cut (run_units), run
on the host.  tests/row_stream_main.cpp is compiled with the host compiler of the ROCm toolchain, as
tests/stream_source_main.cpp is: 64 lane instances of RowStream<NB> in lockstep store into a recorder, the value of an
element being its own index, so every count below is exact.
"""
import subprocess

import pytest

import host_program
import plan_cases as P

NBS = (4, 8, 16, 32)                      # n_fft 512, 1024, 2048, 4096
LENGTHS = (1, 2, 3, 63, 64, 65, 130)      # frames per run: below, at and past one turn of the rotation, and two turns


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return host_program.build("row_stream_main.cpp", str(tmp_path_factory.mktemp("row_stream") / "row_stream"))


@pytest.fixture(scope="module")
def stream_cases(exe):
    out = subprocess.run([exe, "stream"], check=True, capture_output=True, text=True).stdout.splitlines()
    cases = {}
    for line in out:
        nb, g0, n, good, bad, outside = (int(v) for v in line.split())
        cases[(nb, g0, n)] = (good, bad, outside)
    return cases


def test_every_start_and_length_is_run(stream_cases):
    assert set(stream_cases) == {(nb, g0, n) for nb in NBS for g0 in range(64) for n in LENGTHS}
    assert len(stream_cases) == 1792


@pytest.mark.parametrize("nb", NBS)
def test_a_run_writes_its_elements_once_and_nothing_else(stream_cases, nb):
    """Every element of [e0, e0 + n F), e0 = g0 F, is written exactly once and with its own index; nothing is written
    outside the range -- the run's first and last blocks are masked where the neighbouring run owns them.  Two adjacent
    runs therefore tile the stream."""
    F = 64 * nb + 1
    for g0 in range(64):
        for n in LENGTHS:
            assert stream_cases[(nb, g0, n)] == (n * F, 0, 0), (nb, g0, n)


def test_run_units_is_the_cut_of_plan_cases(exe):
    """run_units against plan_cases.runs: units 1 .. 41 at the forced run lengths 8, 9, 13 and one run per clip; the run
    after a clip's last one has no units."""
    cases = [(units, v) for units in range(1, 42) for v in (8, 9, 13, P.ONE_RUN)]
    text = "".join("%d %d\n" % (units, P.forced_run_length(v, units)) for units, v in cases)
    out = subprocess.run([exe, "cut"], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (units, v), line in zip(cases, out):
        parts = line.split()
        assert parts[-1] == "-"
        got = [tuple(int(x) for x in part.split(":")) for part in parts[:-1]]
        assert got == P.runs(units, v), (units, v)
