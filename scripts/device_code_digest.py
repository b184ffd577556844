#!/usr/bin/env python3
"""SHA-256 of the gfx950 device assembly of every file of build.SOURCES, without a GPU:

    python scripts/device_code_digest.py [TREE] > digests.json              # one tree (default: this one)
    python scripts/device_code_digest.py PARENT_TREE THIS_TREE > both.json  # two trees and whether they agree

Each file is compiled with `hipcc --offload-device-only -S`, the tree's own build._flags() and the file's FILE_FLAGS; lines containing
`__hip_cuid_` (a symbol that is random per compile) are dropped and the rest is hashed.  Equal digests: the same device code.  A
host-only refactor (launch epilogues, argument checks) is shown to leave every kernel alone by running this on the parent's checkout
and on the new tree."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digests(tree: str) -> dict:
    spec = importlib.util.spec_from_file_location("_build_of_tree", os.path.join(tree, "openpystruct_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)

    def one(src):
        rel = os.path.relpath(src, tree)   # (relative, from the tree's root: no path of the checkout enters the assembly)
        asm = subprocess.run([build.hipcc_path()] + build._flags() + build._file_flags(src) + ["--offload-device-only", "-S", "-o", "-", rel],
                             cwd=tree, check=True, capture_output=True, text=True).stdout
        kept = "".join(ln for ln in asm.splitlines(True) if "__hip_cuid_" not in ln)
        return os.path.basename(src), hashlib.sha256(kept.encode()).hexdigest()

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 2)) as ex:
        return dict(ex.map(one, build.SOURCES))


def main():
    trees = [os.path.abspath(t) for t in sys.argv[1:]] or [ROOT]
    if len(trees) == 1:
        out = digests(trees[0])
    else:
        parent, this = digests(trees[0]), digests(trees[1])
        differing = sorted(f for f in set(parent) | set(this) if parent.get(f) != this.get(f))
        out = {"what": "SHA-256 of the gfx950 device assembly of every file of build.SOURCES in two trees: hipcc --offload-device-only -S with "
                       "build._flags() and the file's FILE_FLAGS, the lines containing __hip_cuid_ (random per compile) dropped",
               "how": "python scripts/device_code_digest.py PARENT_TREE THIS_TREE (no GPU)",
               "files": len(this), "identical": not differing, "differing": differing, "parent": parent, "this": this}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
