#!/usr/bin/env python
"""Generate tests/golden/sort_adversary.npz: key sequences that drive libstdc++'s std::sort into its heap-sort fallback, and the
order the GENUINE std::sort (oracle/libsort_probe.so, oracle/sort_probe.cpp) leaves them in.

Run where the probe library is built (make -C oracle oracle):  python tests/golden/make_sort_adversary.py
The fixture travels with the repo, so the GPU tests need neither the probe nor a C++ compiler.

A case is (n, k, mirror): the adversary's values val (a permutation of 0..n-1) coarsened by the divisor k into ceil(n / k) distinct keys,
  mirror = 0   key = 3 + (n - 1 - val) / k   the lopsided partitions' big part is the right one (introsort recurses into it)
  mirror = 1   key = 3 + val / k             the big part is the left one (introsort loops on it; the chain a top-4 selection follows)
Cases:
  * n in SMALL with k = 1
  * n in MID and n in LARGE with the smallest k that leaves <= 68 distinct keys, with k + 1 and with 2 k
  * (511, 10): with (100, 2) and (257, 5), which the rule above gives already, the coarsened cases first seen to reach the fallback
  * a basecall holds its quality in 6 bits, so a pileup can carry keys 3..63 only: every n also gets the smallest k that leaves
    <= 61 distinct keys (where the list above lacks it) -- the cases the device tests can use are those with max(key) <= 63
  * the mirrored form of every case with n <= 511 and max(key) <= 63
Arrays: n, k, mirror [cases]; off [cases + 1] into keys / perm (uint16 each)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import pyoracle  # noqa: E402

SMALL = [17, 33, 36, 37, 40, 48, 64, 68]
MID = [69, 100, 129, 200, 257, 300, 400, 511]
LARGE = [512, 600, 1023, 1100, 2000]
MAX_DISTINCT = 68   # the divisors the cases are defined by
MAX_DISTINCT_Q = 61  # qualities 3..63: what 6 bits hold


def case_list():
    cases = []
    for n in SMALL:
        cases.append((n, 1, 0))
    for n in MID + LARGE:
        k0 = -(-n // MAX_DISTINCT)
        cases += [(n, k0, 0), (n, k0 + 1, 0), (n, 2 * k0, 0)]
    cases.append((511, 10, 0))
    for n in SMALL + MID + LARGE:
        c = (n, -(-n // MAX_DISTINCT_Q), 0)
        if c not in cases:
            cases.append(c)
    cases += [(n, k, 1) for n, k, _ in cases if n <= 511 and 3 + (n - 1) // k <= 63]
    return cases


def main():
    assert pyoracle.sort_probe() is not None, "oracle/libsort_probe.so missing: make -C oracle oracle"
    cases = case_list()
    keys, perms = [], []
    for n, k, mirror in cases:
        key = pyoracle.sort_adversary_keys(n, k, bool(mirror))
        assert len(np.unique(key)) == -(-n // k)
        keys.append(key)
        perms.append(pyoracle.std_sort_idx_by_key_desc(key).astype(np.uint16))
    off = np.zeros(len(cases) + 1, np.int64)
    np.cumsum([len(x) for x in keys], out=off[1:])
    arr = np.array(cases, np.int32)
    path = os.path.join(HERE, "sort_adversary.npz")
    np.savez_compressed(path, n=arr[:, 0], k=arr[:, 1], mirror=arr[:, 2], off=off, keys=np.concatenate(keys), perm=np.concatenate(perms))
    print("%s: %d cases, %d keys, %d bytes" % (path, len(cases), int(off[-1]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
