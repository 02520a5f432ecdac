"""Writes tests/golden/decode_fold_parent.npz: the bit patterns (outputs, stash rows, (max, sum)) that the library in the tree
leaves for every case of tests/test_gpu_decode_fold.py.  Run ONCE on the MI355X on a checkout of the commit BEFORE a change to
the decode step's final fold (with the test module of the change copied in: it holds the case list); the test then pins the
change to these bits.  Inputs are the oracle's counter-based synthetic tensors: nothing depends on a device generator.

    python tools/make_decode_fold_golden.py [output.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_decode_fold as T  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    g = {}
    for dt, d, team in T.GROUPS:
        for key, (out, stash, lse) in T.run_group(dt, d, team).items():
            g[f"{key}__out"], g[f"{key}__stash"], g[f"{key}__lse"] = T.bits(out), T.bits(stash), T.bits(lse)
    for case in T.DOMINANT:
        out, stash, lse = T.run_dominant(*case)
        key = T.dominant_key(*case)
        g[f"{key}__out"], g[f"{key}__stash"], g[f"{key}__lse"] = T.bits(out), T.bits(stash), T.bits(lse)
    for n in T.CHAIN_LENS:
        (chained, _), _ = T.run_chain(n)
        for l, (out, stash) in enumerate(chained):
            g[f"{T.chain_key(n, l)}__out"], g[f"{T.chain_key(n, l)}__stash"] = T.bits(out), T.bits(stash)
    assert sorted(g) == sorted(T.all_keys())
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    np.savez_compressed(dst, **g)
    print(f"{dst}: {len(g)} arrays, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
