"""Writes tests/golden/dm_fused_parent_bits.npz: the SHA-256 of every output (each plane of dZ2, dpred, b2part) of the four forms of the fused
scorer dgrad (csrc/dm_fused.hip) at the cases of tests/dm_fused_schedule_cases.py, and the outputs themselves at the smallest case, so that a
mismatch can be located.  Needs a GPU.  Run it with the build whose bits are to be kept - the fixture in the tree comes from the build before
the tile loop's loads moved in front of the products - and only again when a change is MEANT to alter the kernel's results.

    python scripts/make_dm_fused_parent_bits.py [--out PATH]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from chameleon_recsys_amd import _lib
from tests import dm_fused_schedule_cases as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=S.FIXTURE)
    args = ap.parse_args()
    lib = _lib.load()
    gpu = torch.device("cuda:0")
    digests, stored = {}, {}
    for case in S.CASES:
        cid = S.case_id(case)
        digests["inputs/" + cid] = S.inputs_digest(S.inputs(*case))
        for form in S.FORMS:
            out = S.run_form(gpu, lib, form, case)
            for k, v in out.items():
                digests["%s/%s/%s" % (form, cid, k)] = S.digest(v)
                if case == S.STORED:
                    stored["out/%s/%s" % (form, k)] = v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, digests=np.array(json.dumps(digests, sort_keys=True)), **stored)
    print("%d digests, %d stored arrays -> %s (%d bytes)" % (len(digests), len(stored), args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
