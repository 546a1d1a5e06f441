"""Recorded result bits of the training GEMM's entry points (needs an MI355X and a built
libpntf.so).

    python tests/golden/make_gemm_goldens.py [--out tests/golden/gemm_bits.json]

Writes gemm_bits.json: the device name, its CU count and, per case of tests/test_gemm_bits.py,
the sha256 of the bytes that the library in the tree gives.  It calls the public ABI through
pntf._lib alone, so it runs unchanged on any commit that has that ABI.  Run it at the commit
whose bits are to be kept (it was run once, at the last commit before pntf_gemm.hip's build
variants were removed and its host launch code rewritten) and never to make a failing test
pass.  Every case runs twice; one whose bits differ between the two runs stops the script.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "p-ntfields_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import torch  # noqa: E402

import test_gemm_bits as T  # noqa: E402
from pntf import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.FIXTURE)
    args = ap.parse_args()
    lib, cus = _lib.load(), T.cus_of_device()
    digests = {}
    for family in T.FAMILIES:
        first = T.run_family(lib, family, cus)
        second = T.run_family(lib, family, cus)
        unstable = sorted(k for k in first if first[k] != second[k])
        assert not unstable, ("bits differ between two runs", unstable)
        digests.update(first)
        print("%s: %d cases, stable over two runs" % (family, len(first)), flush=True)
    assert sorted(digests) == sorted(T.all_ids(cus))
    with open(args.out, "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "cus": cus, "digests": digests}, fh,
                  indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d digests, %s, %d CUs" % (args.out, len(digests),
                                                 torch.cuda.get_device_name(0), cus))


if __name__ == "__main__":
    main()
