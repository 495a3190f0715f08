"""draw_group_rows (pydream_amd/csrc/dz_draw_groups.h): the archive row count each generation of a draw group samples from.

The persistent kernel's <.., KC, PLAIN> instantiations make the slot draws of G = 64 / nslots consecutive generations in one pass (G = 3 at five tries) and
turn them into archive row numbers in the same pass, so every lane needs the row count of its OWN generation: a history append inside the group raises it
by N for the generations behind it.  The kernel and this test compile the same lines; the host side is held here to the generation loop written out plainly
(dz_megakernel.h: `app = gi == next_app; Mn = app ? M + N : M; if (app) next_app += thin`), for thin 1..12, the first append at every generation of the first
thin-cycle and absent, groups of 1..4 generations, and launch lengths that end on a full and on a short group."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pydream_amd", "csrc", "dz_draw_groups.h")

SOURCE = """
#include "%s"
extern "C" unsigned rows(unsigned M, unsigned N, int next_app, int thin, int gi0, int j) { return dz::draw_group_rows(M, N, next_app, thin, gi0, j); }
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("draw_groups")
    src, lib = str(tmp / "rows.cpp"), str(tmp / "librows.so")
    with open(src, "w") as f:
        f.write(SOURCE % HEADER)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-shared", "-fPIC", src, "-o", lib])
    fn = ctypes.CDLL(lib).rows
    fn.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    fn.restype = ctypes.c_uint32
    return fn


def plain_loop(M0, N, first_app, thin, ngen):
    """-> per generation index: (rows it samples from, next_app as the loop holds it at the top of that generation)"""
    out, M, next_app = [], M0, first_app
    for gi in range(ngen):
        out.append((M, next_app))
        if gi == next_app:
            M += N
            next_app += thin
    return out


@pytest.mark.parametrize("G", [3, 1, 2, 4])
def test_rows_of_every_generation_of_every_group(rows, G):
    M0, N = 1000, 4096
    checked = appends_inside = 0
    for thin in range(1, 13):
        for first_app in [-1] + list(range(thin)):
            for ngen in range(1, 2 * thin + 2 * G + 2):         # every launch length up to two thin-cycles and two groups: full and short last groups
                ref = plain_loop(M0, N, first_app, thin, ngen)
                for gi0 in range(0, ngen, G):                   # a group starts with the state the loop holds at its first generation
                    Mg, na = ref[gi0]
                    for j in range(min(G, ngen - gi0)):
                        got = rows(Mg, N, na, thin, gi0, j)
                        assert got == ref[gi0 + j][0], (thin, first_app, ngen, gi0, j, got, ref[gi0 + j][0])
                        checked += 1
                        appends_inside += got != Mg
    assert checked > 1000
    assert (appends_inside > 0) == (G > 1)                      # the row count did change inside groups


def test_every_append_position_in_a_group_of_three(rows):
    # the first append on each of the three positions of a group, the second one `thin` behind it: inside the same group for thin 1 and 2
    M, N, gi0 = 700, 3073, 9
    for pos in range(3):
        for thin in range(1, 13):
            want = [M, M + N * (pos < 1) + N * (pos + thin < 1), M + N * (pos < 2) + N * (pos + thin < 2)]
            assert [rows(M, N, gi0 + pos, thin, gi0, j) for j in range(3)] == want, (pos, thin)
    assert [rows(M, N, -1, 4, gi0, j) for j in range(3)] == [M, M, M]                    # no append at all
    assert [rows(M, N, gi0 + 3, 1, gi0, j) for j in range(3)] == [M, M, M]               # the next append lies behind the group
    assert [rows(M, N, gi0, 1, gi0, j) for j in range(4)] == [M, M + N, M + 2 * N, M + 3 * N]      # thin 1: every generation appends


def test_row_counts_wrap_as_the_kernels_unsigned_arithmetic_does(rows):
    assert rows(0xFFFFF000, 0x2000, 5, 10, 5, 1) == 0x1000
