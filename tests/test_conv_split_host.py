"""The branch split of the fast conv launch (``csrc/ftn_conv_split.h``) is plain host arithmetic: a stand-alone program
that includes the header is built with the host compiler under AddressSanitizer and UBSan and run over CU counts x
kernel sets x input groups x row estimates.  Every split must give each virtual branch a workgroup, use exactly the
CU count, and - with a row estimate - be no worse than the proportional shares under the model it minimises,
``max_k ceil(rows / nwg[k]) * cost[k]``.  The split of the bench shape is pinned."""
import math
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "flow-timesnet_amd" / "csrc"
CUS = (16, 64, 256, 304)
KSETS = {"k3": (3,), "k35": (3, 5), "k357": (3, 5, 7), "k3579": (3, 5, 7, 9)}
NCIS = (1, 2)
ROWS = (0, 1, 7, 255, 256, 1280, 5120)

# argv: ncu nci rows_est k...  ->  one line with nwg[]; a virtual branch is (branch, output tile) and the fast path
# has as many output tiles as input groups
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ftn_conv_split.h"
int main(int argc, char** argv) {
  if (argc < 5 || argc - 4 > FTN_MAXBR) return 2;
  const int ncu = atoi(argv[1]), nci = atoi(argv[2]), rows_est = atoi(argv[3]), nbr = argc - 4;
  const int nvb = nbr * nci;
  if (nci < 1 || nvb > FTN_CONV_MAXVB) return 2;
  int* slabs = (int*)malloc(sizeof(int) * nvb);                  // exact sizes: an overrun is the sanitizer's to report
  int* nwg = (int*)malloc(sizeof(int) * nvb);
  for (int v = 0; v < nvb; ++v) { const int k = atoi(argv[4 + v / nci]); slabs[v] = (k * k + 1) / 2; }
  ftn_conv_split(ncu, nvb, slabs, nci, rows_est, nwg);
  for (int v = 0; v < nvb; ++v) printf("%d ", nwg[v]);
  printf("\n");
  free(slabs); free(nwg);
  return 0;
}
"""


@pytest.fixture(scope="module")
def split_program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"))
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("conv_split")
    (tmp / "split.cpp").write_text(PROGRAM)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", str(CSRC), str(tmp / "split.cpp"), "-o", str(tmp / "split")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return tmp / "split"


def _split(program, ncu, ks, nci, rows_est):
    r = subprocess.run([str(program), str(ncu), str(nci), str(rows_est), *map(str, KSETS[ks])], capture_output=True,
                       text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]      # a sanitizer report ends the program with an error
    return [int(v) for v in r.stdout.split()]


def _model_time(nwg, cost, rows):
    return max(math.ceil(rows / n) * c for n, c in zip(nwg, cost))


@pytest.mark.parametrize("nci", NCIS)
@pytest.mark.parametrize("ks", list(KSETS))
@pytest.mark.parametrize("ncu", CUS)
def test_split_covers_the_cus(split_program, ncu, ks, nci):
    # the cost model of the header, restated: per batch row 3.17 + 0.281 per K-32 slab and input group
    cost = [3.17 + 0.281 * ((k * k + 1) // 2) * nci for k in KSETS[ks] for _ in range(nci)]
    proportional = _split(split_program, ncu, ks, nci, 0)
    for rows in ROWS:
        nwg = proportional if rows == 0 else _split(split_program, ncu, ks, nci, rows)
        assert len(nwg) == len(cost)
        assert all(n >= 1 for n in nwg), (rows, nwg)
        assert sum(nwg) == ncu, (rows, nwg)
        if rows > 0:
            assert _model_time(nwg, cost, rows) <= _model_time(proportional, cost, rows), (rows, nwg, proportional)


def test_bench_shape_split_is_pinned(split_program):
    """256 CUs, 3x3 / 5x5 / 7x7, one input group, 256 batch rows x 5 groups x 1 tile."""
    assert _split(split_program, 256, "k357", 1, 256 * 5 * 1) == [54, 80, 122]
