#!/usr/bin/env python
"""Record the state blob format (tests/golden/state_blob_format.json): for each of the CASES of tests/test_gpu_state_copy.py, after that
case's scripted rollout, mcr_state_blob_bytes, the four header words and the SHA-256 of every env's get_state_blob(e).  The test
test_blobs_reproduce_the_recorded_format holds both snapshot paths (get_state_blob, save_states) to these figures: whoever changes the
format on purpose bumps BLOB_MAGIC and records them again.  Needs the MI355X.

    python tools/make_state_blob_golden.py                  # writes the file
    python tools/make_state_blob_golden.py --check          # compares a fresh recording with the file: exit status 1 where they differ"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "state_blob_format.json")


def record():
    import numpy as np
    import torch
    from tests.test_gpu_state_copy import CASES, scripted_rollout
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {}
    for case in CASES:
        env = scripted_rollout(torch, case)
        hdr = np.zeros(4, np.uint32)
        assert env.L.mcr_state_blob_header(env.h, hdr.ctypes.data) == 0
        out[case] = dict(blob_bytes=int(env.L.mcr_state_blob_bytes(env.h)), header=[int(w) for w in hdr],
                         sha256=[hashlib.sha256(env.get_state_blob(e).tobytes()).hexdigest() for e in range(env.B)])
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with --out instead of writing it")
    args = ap.parse_args()
    got = record()
    if args.check:
        with open(args.out) as f:
            want = json.load(f)
        bad = [case for case in got if got[case] != want.get(case)]
        print("differs: " + ", ".join(bad) if bad else "identical")
        return 1 if bad else 0
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1)
        f.write("\n")
    print(json.dumps(got, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
