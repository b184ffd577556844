"""Generates tests/golden/sizing_loops_parent_bits.npz: what the build at hand computes on the GPU for the cases of
tests/sizing_loops_bits.py, bit for bit.  Recorded ONCE, on the commit before the host side of the sizing loops (optimiser state,
step-size table, loop driver, aggregate check) was stated once (d26c410); tests/test_gpu_sizing_loops_bits.py holds every later
build to it.  Run it again only when a change is MEANT to move results, and say so in that change.

Every array is stored as raw bits under "<case>__<array>.<dtype>".  Before anything is written, every loop case must satisfy
`sizing_loops_bits.loop_condition`: rows that stop at different epochs, one of them before a poll the loop went past.

Run (needs the GPU):  python tests/golden/make_sizing_loops_parent_bits.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import sizing_loops_bits as lb  # noqa: E402

PATH = os.path.join(HERE, "sizing_loops_parent_bits.npz")


def pack(got):
    return {f"{case}__{k}": z for case, arrays in got.items() for k, z in arrays.items()}


def unpack(npz):
    got = {}
    for key in npz.files:
        case, k = key.split("__", 1)
        got.setdefault(case, {})[k] = npz[key]
    return got


def main():
    got = lb.run_all()
    for case, arrays in got.items():
        if case not in lb.NOT_LOOPS:
            ep = lb.epochs_of(arrays).tolist()
            print(case, "epochs", ep)
            assert all(lb.loop_condition(arrays)), (case, ep, lb.loop_condition(arrays))
    np.savez_compressed(PATH, **pack(got))
    back = unpack(np.load(PATH))
    assert all(np.array_equal(back[c][k], z) and back[c][k].dtype == z.dtype for c, arrays in got.items() for k, z in arrays.items())
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
