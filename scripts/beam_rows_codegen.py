#!/usr/bin/env python3
"""Code generation of the row-staged beam kernels (csrc/beam_fat.hip) for gfx950, without a GPU:

    python scripts/beam_rows_codegen.py [--prologue] [CSRC_DIR] > kernels.json

compiles beam_fat.hip of CSRC_DIR (default: this tree's) to device assembly with the flags of openpystruct_amd/build.py (the per-file
ones included) and prints, per kernel: the number of kernel-argument dwords the hardware preloads into SGPRs at wave launch, user SGPRs,
VGPRs, SGPRs, private-segment (scratch) bytes, LDS bytes and the number of instructions.  --prologue adds the instructions from the entry
the hardware jumps to (behind the load prologue kept for firmware without preloading) up to the first vector-memory load."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openpystruct_amd import build  # noqa: E402

FILE = "beam_fat.hip"


def kernels(asm: str, prologue: bool) -> dict:
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = [ln.split(";")[0].strip() for ln in body[:body.rindex("s_endpgm")].split("\n")]
        code = [ln for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")] + ["s_endpgm"]
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))   # noqa: E731
        pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        pretty = pretty[5:] if pretty.startswith("void ") else pretty
        pretty = pretty[:pretty.index(">(") + 1] if ">(" in pretty else pretty.split("(")[0]
        rec = dict(kernarg_preload_dwords=field("user_sgpr_kernarg_preload_length"), user_sgprs=field("user_sgpr_count"),
                   vgpr=field("next_free_vgpr"), sgpr=field("next_free_sgpr"), private_segment=field("private_segment_fixed_size"),
                   lds=field("group_segment_fixed_size"), instructions=len(code))
        if prologue:
            start = next((i + 1 for i, ln in enumerate(code) if ln.startswith("s_branch")), 0) if rec["kernarg_preload_dwords"] else 0
            stop = next((i for i in range(start, len(code)) if code[i].startswith(("buffer_load", "global_load"))), len(code) - 1)
            rec["to_first_vector_load"] = code[start:stop + 1]
        out[pretty.replace("opsamd::", "")] = rec
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--prologue"]
    csrc = args[0] if args else build.CSRC
    src = os.path.join(csrc, FILE)
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "beam_fat.s")
        subprocess.check_call([build.hipcc_path()] + build._flags() + build._file_flags(src) + ["--offload-device-only", "-S", "-o", s, src])
        out = kernels(open(s).read(), "--prologue" in sys.argv[1:])
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
