"""Generates tests/golden/beam_rows_parent_bits.npz: what the build at hand computes on the GPU for the cases of
tests/beam_rows_bits.py, bit for bit.  Recorded ONCE, on the commit before the rows kernel's instruction stream was trimmed
(44ced76); tests/test_gpu_beam_rows_bits.py holds every later build to it.  Run it again only when a change is MEANT to move
results, and say so in that change.

Every array is stored as raw bits (uint64 / uint32 / uint8) under "<case>_<array>".  The two runs of case (d) are stored as
their XOR with case (a), run on the same inputs: equal or nearly equal results then cost next to nothing in the compressed file.

Run (needs the GPU):  python tests/golden/make_beam_rows_parent_bits.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import beam_rows_bits as rb  # noqa: E402

PATH = os.path.join(HERE, "beam_rows_parent_bits.npz")


def pack(got):
    out = {}
    for case, arrays in got.items():
        for k, z in arrays.items():
            out[f"{case}_{k}"] = z ^ got["a"][k] if case in ("d16", "d8r") else z
    return out


def unpack(npz):
    got = {}
    for key in npz.files:
        case, k = key.split("_", 1)
        got.setdefault(case, {})[k] = npz[key]
    for case in ("d16", "d8r"):
        got[case] = {k: z ^ got["a"][k] for k, z in got[case].items()}
    return got


def main():
    got = rb.run_all()
    for case in ("a", "b", "d16", "d8r"):
        assert not got[case]["status"].any(), (case, got[case]["status"])
    assert got["c"]["status"].tolist() == [0, 0, 1, 0], got["c"]["status"]
    np.savez_compressed(PATH, **pack(got))
    back = unpack(np.load(PATH))
    assert all(np.array_equal(back[c][k], z) for c, arrays in got.items() for k, z in arrays.items())
    for case in ("d16", "d8r"):
        print(case, "entries that differ from (a):", {k: int((z != got["a"][k]).sum()) for k, z in got[case].items()})
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
