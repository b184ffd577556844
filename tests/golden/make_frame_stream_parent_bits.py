"""Generates tests/golden/frame_stream_parent_bits.npz: what the build at hand computes on the GPU for the cases of
tests/frame_stream_bits.py, bit for bit.  Recorded ONCE, on the commit before the frame streaming kernels' node walk, end-node
contraction and launch were each stated once (9a1c99c); tests/test_gpu_frame_stream_bits.py holds every later build to it.  Run it
again only when a change is MEANT to move results, and say so in that change.

Every array is stored as raw bits (uint64) under "<case>__<array>".  The case "big" runs the inputs of "g10x6" in every replica and
is stored as its XOR with that case: equal results then cost next to nothing in the compressed file.

Run (needs the GPU):  python tests/golden/make_frame_stream_parent_bits.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import frame_stream_bits as fb  # noqa: E402

PATH = os.path.join(HERE, "frame_stream_parent_bits.npz")


def pack(got):
    return {f"{case}__{k}": z ^ got["g10x6"][k] if case == "big" and k != "replicas" else z
            for case, arrays in got.items() for k, z in arrays.items()}


def unpack(npz):
    got = {}
    for key in npz.files:
        case, k = key.split("__", 1)
        got.setdefault(case, {})[k] = npz[key]
    got["big"] = {k: z if k == "replicas" else z ^ got["g10x6"][k] for k, z in got["big"].items()}
    return got


def main():
    got = fb.run_all()
    assert got["big"]["replicas"].tolist() == [0], got["big"]["replicas"]
    np.savez_compressed(PATH, **pack(got))
    back = unpack(np.load(PATH))
    assert all(np.array_equal(back[c][k], z) for c, arrays in got.items() for k, z in arrays.items())
    print("big: entries that differ from g10x6:", {k: int((z != got["g10x6"][k]).sum()) for k, z in got["big"].items() if k != "replicas"})
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
