#!/usr/bin/env python3
"""Instruction census of one HIP unit: compile it to gfx950 assembly and count, per kernel and per basic block, the
MFMA, VALU, LDS and vector-memory instructions, next to the kernel's VGPR and spill counts.

    tools/isa_census.py flow-timesnet_amd/csrc/stagec_pos.hip -DFTN_POS_DEV=1 --kernel k_mlp_pos --min-mfma 4
    tools/isa_census.py UNIT.hip --kernel PATTERN --count v_perm_b32 --count v_lshrrev_b32

Everything after the unit that is not an option of this tool goes to hipcc.  `census()` is the importable form
(tests/test_stagec_isa.py).  The classes are the issue ports of a CDNA SIMD: what a loop that is bound by instruction
issue pays for."""
from __future__ import annotations

import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ARCH = "gfx950"
CLASSES = ("mfma", "valu", "lds", "vmem", "salu")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_ENCODING = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")      # the encoding suffix is not part of the mnemonic
_VMEM = ("global_", "buffer_", "flat_", "scratch_", "tbuffer_", "image_")


def find_hipcc() -> str | None:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.access(cand, os.X_OK):
            return cand
    return None


def classify(mnemonic: str) -> str | None:
    if mnemonic.startswith(("v_mfma_", "v_smfmac_")):
        return "mfma"
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(_VMEM):
        return "vmem"
    if mnemonic.startswith("s_"):
        return "salu"
    return None


def demangle(names: list[str]) -> dict[str, str]:
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        dem = out.strip().splitlines()
        if len(dem) == len(names):
            return {n: re.sub(r"^void ", "", d).split("(")[0] for n, d in zip(names, dem)}
    except (OSError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def parse_asm(text: str) -> dict[str, dict]:
    """{mangled kernel name: {"blocks": [{"label", mfma, valu, lds, vmem, salu}], "mnemonics": Counter, resources}}"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out: dict[str, dict] = {}
    cur = block = None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = _LABEL.match(line)
        if m:
            name = m.group(1)
            if name in kernels:
                cur = out[name] = {"blocks": [], "mnemonics": collections.Counter()}
                block = None
            elif name.startswith(".Lfunc_end"):
                cur = None
            if cur is not None:
                block = dict.fromkeys(CLASSES, 0)
                block["label"] = "entry" if name in kernels else name
                cur["blocks"].append(block)
            continue
        if cur is None or line.startswith("."):
            continue
        mnemonic = _ENCODING.sub("", line.split()[0])
        cls = classify(mnemonic)
        if cls is None:
            continue
        block[cls] += 1
        cur["mnemonics"][mnemonic] += 1
    # resources: the amdhsa.kernels metadata (one "- .agpr_count:" entry per kernel)
    meta = text.split("amdhsa.kernels:", 1)
    if len(meta) == 2:
        for entry in re.split(r"^\s*-\s+(?=\.agpr_count:)", meta[1], flags=re.M):
            nm = re.search(r"^\s*\.name:\s+(\S+)", entry, re.M)
            if not nm or nm.group(1) not in out:
                continue
            for key in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                        "private_segment_fixed_size"):
                v = re.search(rf"^\s*\.{key}:\s+(\d+)", entry, re.M)
                out[nm.group(1)][key] = int(v.group(1)) if v else None
    for k in out.values():
        for c in CLASSES:
            k[c] = sum(b[c] for b in k["blocks"])
    return out


def census(unit: str | os.PathLike, flags: list[str] | tuple[str, ...] = (), hipcc: str | None = None) -> dict[str, dict]:
    """Compile `unit` for gfx950 (device code only) and return parse_asm() keyed by DEMANGLED kernel name."""
    hipcc = hipcc or find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    unit = Path(unit).resolve()
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / (unit.stem + ".s")
        cmd = [hipcc, "-O3", "-std=c++17", f"--offload-arch={ARCH}", "--offload-device-only", "-S",
               "-I", str(unit.parent), *flags, str(unit), "-o", str(asm)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
        parsed = parse_asm(asm.read_text())
    names = demangle(list(parsed))
    return {names[k]: v for k, v in parsed.items()}


def report(kernels: dict[str, dict], pattern: str = "", min_mfma: int = 0, count: list[str] | tuple[str, ...] = (),
           file=sys.stdout) -> None:
    for name, k in kernels.items():
        if pattern not in name:
            continue
        print(f"{name}\n  VGPRs {k.get('vgpr_count')}  AGPRs {k.get('agpr_count')}  spilled VGPRs {k.get('vgpr_spill_count')}"
              f"  spilled SGPRs {k.get('sgpr_spill_count')}  scratch {k.get('private_segment_fixed_size')} B/lane", file=file)
        print("  total      " + "  ".join(f"{c} {k[c]}" for c in CLASSES), file=file)
        for mn in count:
            print(f"  {mn}: {k['mnemonics'].get(mn, 0)}", file=file)
        for b in k["blocks"]:
            if b["mfma"] >= min_mfma:
                print(f"  {b['label']:12s}" + "  ".join(f"{c} {b[c]}" for c in CLASSES), file=file)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("unit")
    ap.add_argument("--kernel", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--min-mfma", type=int, default=0, help="only basic blocks with at least this many MFMAs")
    ap.add_argument("--count", action="append", default=[], help="also print the count of this mnemonic (repeatable)")
    args, flags = ap.parse_known_args()
    report(census(args.unit, flags), args.kernel, args.min_mfma, args.count)
    return 0


if __name__ == "__main__":
    sys.exit(main())
