"""Which rows a fast-conv workgroup owns (``csrc/ftn_conv_walk.h``) is plain arithmetic shared by host and device: a
stand-alone program that includes the header is built with the host compiler under AddressSanitizer and UBSan and
prints, for every workgroup, the stretches ``ftn_conv_walk_next`` yields and the row range ``ftn_conv_walk_row`` gives
its positions.  Over tile counts x batch sizes x workgroup counts x switch charges:

* every (tile, batch row) lies in exactly one stretch of exactly one workgroup, stretches stay inside their tile,
  ascend, and a workgroup's rows are one contiguous range of the tile-major sequence - the one ``ftn_conv_walk_row``
  reports (what ``tools/stamps.py`` reads from the stamp record);
* a workgroup owns at most ``ceil(V / n)`` positions of the ``V = tiles (B + sw)``, and one that walks on into
  another tile owns at least ``sw`` rows fewer than that per switch;
* with ``sw = 0`` the rows are ``[R w / n, R (w + 1) / n)`` with ``R = tiles B``: the equal split the kernel computed
  before the header existed, which the branch split of ``ftn_conv_split.h`` was fitted to (row totals 0, 1, 2, 7, 15,
  120, 255, 260, 1280 and 5120 are among the cases)."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flow-timesnet_amd" / "csrc"
# (tiles, B): row totals R = 0, 1, 2, 7, 15, 120, 255, 260, 1280 (the bench shape: 5 x 256), 5120, and one tile of 1280
SHAPES = ((0, 4), (1, 1), (2, 1), (1, 2), (7, 1), (5, 3), (5, 24), (1, 255), (5, 52), (5, 256), (20, 256), (1, 1280))
NWGS = (1, 2, 54, 80, 122, 256)
SWITCH = (0, 1, 2, 3)

# argv: tiles B sw n  ->  one line per workgroup: row_lo row_hi, then tile b_begin b_end of every stretch.  The
# position pair sits on the heap at its exact size: a write past it is the sanitizer's to report
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ftn_conv_walk.h"
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int tiles = atoi(argv[1]), B = atoi(argv[2]), sw = atoi(argv[3]), n = atoi(argv[4]);
  if (tiles < 0 || B < 1 || sw < 0 || n < 1) return 2;
  for (int w = 0; w < n; ++w) {
    int* pos = (int*)malloc(2 * sizeof(int));
    ftn_conv_walk(tiles, B, sw, n, w, pos);
    if (pos[0] < pos[1]) printf("%lld %lld", ftn_conv_walk_row(B, sw, pos[0]), ftn_conv_walk_row(B, sw, pos[1]));
    else printf("0 0");
    int tile, b0, b1;
    for (int v = pos[0]; ftn_conv_walk_next(B, sw, &v, pos[1], &tile, &b0, &b1);) printf(" %d %d %d", tile, b0, b1);
    printf("\n");
    free(pos);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"))
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("conv_walk")
    (tmp / "walk.cpp").write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(CSRC), str(tmp / "walk.cpp"), "-o", str(tmp / "walk")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp / "walk"


def _walk(program, tiles, B, sw, n):
    """Per workgroup: ((row_lo, row_hi), [(tile, b_begin, b_end), ...])."""
    r = subprocess.run([str(program), str(tiles), str(B), str(sw), str(n)], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]      # a sanitizer report ends the program with an error
    out = []
    for line in r.stdout.splitlines():
        v = [int(t) for t in line.split()]
        assert len(v) >= 2 and (len(v) - 2) % 3 == 0, line
        out.append(((v[0], v[1]), [tuple(v[i:i + 3]) for i in range(2, len(v), 3)]))
    assert len(out) == n
    return out


@pytest.mark.parametrize("sw", SWITCH)
@pytest.mark.parametrize("n", NWGS)
def test_walk_shares_out_every_row_once(walk_program, n, sw):
    for tiles, B in SHAPES:
        R, V = tiles * B, tiles * (B + sw)
        share = -(-V // n)
        owners = [0] * R
        for w, ((lo, hi), stretches) in enumerate(_walk(walk_program, tiles, B, sw, n)):
            ctx = (tiles, B, sw, n, w, lo, hi, stretches)
            rows = []
            for tile, b0, b1 in stretches:
                assert 0 <= tile < tiles and 0 <= b0 < b1 <= B, ctx
                rows.extend(range(tile * B + b0, tile * B + b1))
            for row in rows:
                owners[row] += 1
            assert rows == list(range(lo, hi)), ctx               # ascending, contiguous, as the stamp record says
            assert [s[0] for s in stretches] == sorted({s[0] for s in stretches}), ctx    # one stretch per tile
            assert all(s[2] == B for s in stretches[:-1]) and all(s[1] == 0 for s in stretches[1:]), ctx
            assert len(rows) + sw * (len(stretches) - 1) <= share, ctx
            if sw == 0:
                assert (lo, hi) == (R * w // n, R * (w + 1) // n) or (lo == hi == 0 and R * w // n == R * (w + 1) // n), ctx
        assert owners == [1] * R, (tiles, B, sw, n, [i for i, c in enumerate(owners) if c != 1][:8])


def test_bench_shape_crossings_own_fewer_rows(walk_program):
    """256 batch rows x 5 tiles on the pinned split [54, 80, 122] with the charges the launch derives (2, 1, 1): no
    workgroup owns more rows than under the equal split (24 / 16 / 11), the 3x3 and 7x7 workgroups that cross a tile
    boundary own 22 and 10, and the 80 5x5 workgroups keep their 16 rows inside one tile.  With no charge the four 7x7
    workgroups that cross own 11."""
    for n, sw, most, crossing in ((54, 2, 24, [22] * 4), (80, 1, 16, []), (122, 1, 11, [10] * 4)):
        walks = _walk(walk_program, 5, 256, sw, n)
        assert max(hi - lo for (lo, hi), _ in walks) == most
        assert [hi - lo for (lo, hi), st in walks if len(st) > 1] == crossing
    assert [hi - lo for (lo, hi), st in _walk(walk_program, 5, 256, 0, 54) if len(st) > 1] == [23, 24, 24, 23]
    assert [hi - lo for (lo, hi), st in _walk(walk_program, 5, 256, 0, 122) if len(st) > 1] == [11, 11, 11, 11]
