#!/usr/bin/env python3
"""Code generation of the frame streaming kernels (csrc/frame_vjp.hip, frame_sizing_grad.hip, frame_loads.hip) for gfx950, without a GPU:

    python scripts/frame_stream_codegen.py [CSRC_DIR] > kernels.json

compiles the three files of CSRC_DIR (default: this tree's) to device assembly with the flags of openpystruct_amd/build.py and prints,
per kernel: VGPRs, SGPRs, private-segment bytes, the number of f64 arithmetic instructions (v_*_f64 other than comparisons), the number of
instructions, and a hash of the instruction stream with labels and symbol names removed (equal hashes: the same code)."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openpystruct_amd import build  # noqa: E402

FILES = ("frame_vjp", "frame_sizing_grad", "frame_loads")


def kernels(asm: str) -> dict:
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = [ln.split(";")[0].strip() for ln in body[:body.index("s_endpgm")].split("\n")]
        code = [ln for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")] + ["s_endpgm"]
        f64 = [ln for ln in code if re.match(r"v_\w+_f64", ln) and not ln.startswith("v_cmp")]
        stream = "\n".join(re.sub(r"\.LBB\w+|_Z\w+", "L", ln) for ln in code)
        pretty = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
        out[pretty] = dict(vgpr=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           sgpr=int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", body).group(1)),
                           private_segment=int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                           f64_arithmetic=len(f64), instructions=len(code), stream_sha1=hashlib.sha1(stream.encode()).hexdigest()[:12])
    return out


def main():
    csrc = sys.argv[1] if len(sys.argv) > 1 else build.CSRC
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in FILES:
            s = os.path.join(tmp, f + ".s")
            subprocess.check_call([build.hipcc_path()] + build._flags() + ["--offload-device-only", "-S", "-o", s, os.path.join(csrc, f + ".hip")])
            out.update(kernels(open(s).read()))
    json.dump(out, sys.stdout, indent=1)


if __name__ == "__main__":
    main()
