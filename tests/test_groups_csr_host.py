"""The CSR walk of the series-group kernels (``csrc/ftn_groups.h``) is plain C++: a stand-alone program that includes
the header is built with the host compiler under AddressSanitizer and UBSan and does what a workgroup does - the
``cfirst`` prologue thread by thread and phase by phase, the lookup of chunks 0 .. C - 1 with the reads of ``order``,
the combine range of every group with a read of each chunk sum - on arrays of exactly the kernels' sizes.

For a device CSR that agrees with the host copy the walk must visit every group's members in their order in chunks of
32, and ``cfirst`` must be the exclusive prefix sum of the chunk counts.  For one that disagrees (the device words are
not validated) the program must end clean under the sanitizers with every index it reports inside the arrays: this is
where the kernels' promise that such a CSR addresses nothing outside x, order, out and LDS is established - no test
hands one to a kernel on the GPU."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

import groups_checks as gc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flow-timesnet_amd" / "csrc"
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1

# stdin: G M C nthreads, the G + 1 device offsets, the M device members  ->  "cfirst ..", per chunk "chunk c g start n
# members..", per group "combine g k0 k1"
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ftn_groups.h"
static int next_int() { int v; if (scanf("%d", &v) != 1) exit(2); return v; }
int main() {
  const int G = next_int(), M = next_int(), C = next_int(), nthreads = next_int();
  if (G < 1 || M < 0 || C < 0 || nthreads < 1) return 2;
  int* offsets = (int*)malloc(sizeof(int) * (G + 1));           // exact sizes: an overrun is the sanitizer's to report
  int* order = (int*)malloc(sizeof(int) * M);
  int* cfirst = (int*)malloc(sizeof(int) * (G + 1));
  int* part = (int*)malloc(sizeof(int) * nthreads);
  int* g0 = (int*)malloc(sizeof(int) * nthreads);               // a thread's registers across the barrier
  int* g1 = (int*)malloc(sizeof(int) * nthreads);
  double* csum = (double*)calloc(C, sizeof(double));
  for (int g = 0; g <= G; ++g) offsets[g] = next_int();
  for (int i = 0; i < M; ++i) order[i] = next_int();
  const FtnGroupCsr s = {order, offsets, G, M, C};
  for (int t = 0; t < nthreads; ++t) part[t] = ftn_csr_count(s, t, nthreads, &g0[t], &g1[t]);
  for (int t = 0; t < nthreads; ++t) ftn_csr_first(s, t, nthreads, g0[t], g1[t], part, cfirst);    // after the barrier
  printf("cfirst");
  for (int g = 0; g <= G; ++g) printf(" %d", cfirst[g]);
  printf("\n");
  for (int c = 0; c < C; ++c) {
    const FtnGroupChunk k = ftn_csr_chunk(s, cfirst, c);
    const int n = k.len < 0 ? 0 : k.len < FTN_GROUP_CHUNK ? k.len : FTN_GROUP_CHUNK;   // the kernels' j < len, j < 32
    printf("chunk %d %d %d %d", c, k.g, k.start, n);
    for (int j = 0; j < n; ++j) printf(" %d", order[k.start + j]);
    printf("\n");
  }
  double sink = 0.0;
  for (int g = 0; g < G; ++g) {
    for (int k = cfirst[g]; k < cfirst[g + 1]; ++k) sink += csum[k];
    printf("combine %d %d %d\n", g, cfirst[g], cfirst[g + 1]);
  }
  free(offsets); free(order); free(cfirst); free(part); free(g0); free(g1); free(csum);
  return sink == 0.0 ? 0 : 3;
}
"""


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"))
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("groups_csr")
    (tmp / "walk.cpp").write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", str(CSRC), str(tmp / "walk.cpp"), "-o", str(tmp / "walk")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp / "walk"


def _walk(program, offsets, order, C, nthreads):
    """``(cfirst, [(c, g, start, members)], [(g, k0, k1)])`` of the program for the device CSR and the host's C."""
    G, M = len(offsets) - 1, len(order)
    text = " ".join(map(str, [G, M, C, nthreads, *offsets, *order]))
    r = subprocess.run([str(program)], input=text, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]      # a sanitizer report ends the program with an error
    cfirst, chunks, combines = None, [], []
    for line in r.stdout.splitlines():
        kind, *v = line.split()
        v = [int(w) for w in v]
        if kind == "cfirst":
            cfirst = v
        elif kind == "chunk":
            assert len(v) == 4 + v[3]
            chunks.append((v[0], v[1], v[2], v[4:]))
        else:
            combines.append(tuple(v))
    assert len(cfirst) == G + 1 and [c for c, *_ in chunks] == list(range(C)) and [g for g, *_ in combines] == list(range(G))
    return cfirst, chunks, combines


def _csr(members):
    offsets = [0]
    for m in members:
        offsets.append(offsets[-1] + len(m))
    return offsets, [i for m in members for i in m]


def _check_agreeing(program, members, nthreads):
    offsets, order = _csr(members)
    per = [(len(m) + gc.CHUNK - 1) // gc.CHUNK for m in members]
    C = sum(per)
    cfirst, chunks, combines = _walk(program, offsets, order, C, nthreads)
    assert cfirst == [sum(per[:g]) for g in range(len(members) + 1)] and cfirst[-1] == C
    assert combines == [(g, cfirst[g], cfirst[g + 1]) for g in range(len(members))]
    seen = [[] for _ in members]
    for c, g, start, got in chunks:
        assert cfirst[g] <= c < cfirst[g + 1]
        k = c - cfirst[g]
        assert start == offsets[g] + k * gc.CHUNK and got == members[g][k * gc.CHUNK:(k + 1) * gc.CHUNK] and got
        seen[g] += got
    assert seen == [list(m) for m in members]


def _sized(sizes):
    """Member lists of the given sizes, the series taken in descending order."""
    total, out = sum(sizes), []
    for s in sizes:
        out.append(list(range(total - 1, total - 1 - s, -1)))
        total -= s
    return out


@pytest.mark.parametrize("N", [5, 33, 193])
def test_agreeing_csr_walks_every_layout(walk_program, N):
    for name, members in gc.layouts(N).items():
        G = len(members)
        for nthreads in sorted({1, 2, G - 1, G, G + 1, 2 * G + 3, 256} - {0}):
            _check_agreeing(walk_program, members, nthreads)


SIZES = [(0,), (1,), (31,), (32,), (33,), (65,),
         (31, 32, 33), (0, 65, 1), (0, 0, 0), (33, 0, 0), (0, 0, 33),
         (0, 1, 31, 32), (33, 65, 0, 1), (32, 32, 32, 32), (65, 0, 0, 33), (0, 0, 0, 0)]


@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: "-".join(map(str, s)))
def test_agreeing_csr_around_the_chunk_edge(walk_program, sizes):
    """nthreads below, equal to and above G; 3 threads for 4 groups take 2 + 2 + 0: the last thread has no group and
    still writes cfirst[G]."""
    for nthreads in (1, 2, 3, 4, 5, 7, 64):
        _check_agreeing(walk_program, _sized(sizes), nthreads)


# the host copy the launches below were sized from, and device words that disagree with it
HOSTS = {"g4": _sized((33, 0, 65, 31)), "g1": _sized((65,)), "g3": _sized((32, 1, 0))}
BAD_OFFSETS = {
    "g4": {"negative": [[0, -5, 33, -1, 129], [-1, -2, -3, -4, -5], [INT_MIN, 33, INT_MIN, 98, 129]],
           "above_M": [[0, 33, 500, 98, 1 << 30], [INT_MAX] * 5, [130, 131, 132, 133, 134], [0, 33, 33, 98, 130]],
           "decreasing": [[129, 98, 33, 33, 0], [0, 98, 33, 129, 64], [0, INT_MAX, INT_MIN, INT_MAX, INT_MIN]],
           "all_zero": [[0] * 5],
           "more_chunks": [[0, 1, 2, 3, 129], [0, 129, 0, 129, 0], [0, 1, 34, 67, 129], [0, 129, 0, 129, 129]],
           "fewer_chunks": [[0, 129, 129, 129, 129], [0, 0, 0, 0, 32], [0, 0, 0, 0, 1], [7, 7, 7, 7, 7]]},
    "g1": {"negative": [[-9, -3], [-9, 65]], "above_M": [[0, 200], [66, INT_MAX]], "decreasing": [[65, 0], [5, 3]],
           "all_zero": [[0, 0]], "more_chunks": [], "fewer_chunks": [[0, 1], [3, 35], [64, 65]]},
    "g3": {"negative": [[-1, -1, 33, 33]], "above_M": [[0, 32, 34, 40]], "decreasing": [[33, 32, 1, 0]],
           "all_zero": [[0] * 4], "more_chunks": [[0, 1, 2, 33], [0, 33, 0, 33]], "fewer_chunks": [[0, 32, 32, 32]]}}
KINDS = ["negative", "above_M", "decreasing", "all_zero", "more_chunks", "fewer_chunks"]


def _check_inside(program, offsets, order, host_members, nthreads):
    M, C = sum(len(m) for m in host_members), gc.chunks(host_members)
    cfirst, chunks, combines = _walk(program, offsets, order, C, nthreads)
    assert all(0 <= v <= C for v in cfirst), cfirst
    for c, g, start, got in chunks:
        assert 0 <= g < len(host_members) and (not got or (0 <= start and start + len(got) <= M)), (c, g, start, len(got))
    for g, k0, k1 in combines:
        assert all(0 <= k < C for k in range(k0, k1)), (g, k0, k1)
    return cfirst


@pytest.mark.parametrize("kind", KINDS)
def test_disagreeing_offsets_stay_inside(walk_program, kind):
    for host, members in HOSTS.items():
        _, order = _csr(members)
        per = [(len(m) + gc.CHUNK - 1) // gc.CHUNK for m in members]
        for offsets in BAD_OFFSETS[host][kind]:
            lim = [max(0, min(o, len(order))) for o in offsets]
            device = sum((b - a + gc.CHUNK - 1) // gc.CHUNK for a, b in zip(lim, lim[1:]) if b > a)
            if kind == "more_chunks":                           # the case is what its name says
                assert device > sum(per)
            if kind == "fewer_chunks":
                assert device < sum(per)
            for nthreads in (1, 3, 4, 256):
                cfirst = _check_inside(walk_program, offsets, order, members, nthreads)
                assert cfirst[-1] == min(device, sum(per))


def test_members_outside_the_series_are_only_read(walk_program):
    """The walk hands a member on as it is (the kernels test it against N where they use it): words outside
    0 .. N - 1 change no index into ``order``."""
    for members in HOSTS.values():
        offsets, order = _csr(members)
        N = len(order)
        bad = [(-1, N, INT_MAX, INT_MIN, N + 1000)[i % 5] if i % 3 == 0 else v for i, v in enumerate(order)]
        for nthreads in (1, 4, 256):
            _check_inside(walk_program, offsets, bad, members, nthreads)
            _, chunks, _ = _walk(walk_program, offsets, bad, gc.chunks(members), nthreads)
            assert [v for *_, got in chunks for v in got] == bad
